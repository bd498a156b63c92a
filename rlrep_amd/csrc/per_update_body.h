// body of per_update_kernel and of its group form: leaves at idx[j] <- max over the duplicates of (td_j + eps)^alpha, max_p follows,
// ancestors level by level, by ONE workgroup of PER_THREADS.  P and B are the record's sizes; `tree`, `scal`, `idx`, `td` are the
// agent's or the member's; `sh` is float[4] of LDS.
    const float alpha = scal[1], eps = scal[3];
    unsigned* leaves = reinterpret_cast<unsigned*>(tree + P);
    // (an index outside the tree is skipped in every phase: the callers check theirs, nothing is ever written outside the tree)
    auto inside = [&](int j) { const long long ix = idx[j]; return ix >= 0 && ix < P; };
    for (int j = threadIdx.x; j < B; j += PER_THREADS) if (inside(j)) leaves[idx[j]] = 0u;
    __syncthreads();
    // stratified sampling hits a heavy leaf many times: the maximum of the duplicates, whatever order they arrive in (the bit patterns of
    // non-negative floats order as the floats do)
    float mx = 0.f;
    for (int j = threadIdx.x; j < B; j += PER_THREADS) {
        if (!inside(j)) continue;
        float nw = alpha == 0.f ? 1.0f : powf(__fadd_rn(td[j], eps), alpha);
        // a priority that is not positive (td = 0 with eps = 0) or not a number (a NaN td) becomes PER_MIN_PRIORITY: a touched row keeps a
        // positive leaf, so it stays in the tree and a later update can raise it again
        nw = nw > PER_MIN_PRIORITY ? nw : PER_MIN_PRIORITY;
        atomicMax(leaves + idx[j], __float_as_uint(nw));
        mx = fmaxf(mx, nw);
    }
    mx = per_block_max(mx, sh);          // (its barrier is also the one between the maxima and the first level)
    if (threadIdx.x == 0) scal[0] = fmaxf(scal[0], mx);
    // the leaves were written by atomics, which live in the L2: the first level reads them past this CU's L1
    for (int j = threadIdx.x; j < B; j += PER_THREADS) {
        const long long nd = (P + idx[j]) >> 1;
        if (nd >= 1 && inside(j)) {
            const float l = __hip_atomic_load(tree + 2 * nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float r = __hip_atomic_load(tree + 2 * nd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tree[nd] = __fadd_rn(l, r);
        }
    }
    for (long long wd = P >> 1, k = 2; wd > 1; wd >>= 1, ++k) {
        __syncthreads();
        for (int j = threadIdx.x; j < B; j += PER_THREADS) {
            const long long nd = (P + idx[j]) >> k;
            if (inside(j)) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);      // (duplicates store identical values)
        }
    }
