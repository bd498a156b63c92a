// body of per_add_kernel and of its group form: leaves of rows [p.start, p.start + p.n) mod p.capacity = mp (max_p as read by this launch),
// ancestors recomputed level by level.  `p` is the PerAdd record (its scalars; member 0's in a group), `tree` the tree written.
    // the range as at most two runs of consecutive leaves: [a0, b0) and, behind the wrap, [0, b1)
    const long long a0 = p.start, b0 = p.start + p.n < p.capacity ? p.start + p.n : p.capacity, b1 = p.start + p.n - b0;
    for (long long i = a0 + threadIdx.x; i < b0; i += PER_ADD_THREADS) tree[p.P + i] = mp;
    for (long long i = threadIdx.x; i < b1; i += PER_ADD_THREADS) tree[p.P + i] = mp;
    // level k: the parents of what level k - 1 wrote.  The two runs may meet in the upper levels: both then store the same sum of the
    // same two children, which the barrier below the level has made final.
    for (long long lo0 = p.P + a0, hi0 = p.P + b0 - 1, lo1 = p.P, hi1 = p.P + b1 - 1, w = p.P; w > 1; w >>= 1) {
        __syncthreads();
        lo0 >>= 1; hi0 >>= 1; lo1 >>= 1; hi1 >>= 1;
        for (long long nd = lo0 + threadIdx.x; nd <= hi0; nd += PER_ADD_THREADS) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);
        if (b1 > 0)
            for (long long nd = lo1 + threadIdx.x; nd <= hi1; nd += PER_ADD_THREADS) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);
    }
