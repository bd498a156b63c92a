// body of the samplers -- per_sample_kernel, its group form, and workgroup 0 of the fused sample + gather launches: B stratified draws (or
// B given indices) and their importance weights normalised by the batch maximum, by ONE workgroup of PER_THREADS.  `p` is the PerSample
// record (its scalars; member 0's in a group) and P, B its sizes; `tree`, `idx`, `w`, `beta`, `seed` are the agent's or the member's; `md`
// is the byte offset of the member's step counter (0 for a single agent); `sh` is float[4] of LDS.
    float pmin = __builtin_inff();
    if (!p.given) {
        // the stream offset and the total are read here, inside the branch: in front of it they cost per_sample_kernel nine instructions.
        // A fused launch has read them in front of its role branch, for its gatherers too, and says so (PER_SAMPLE_HAS_STREAM).
#ifndef PER_SAMPLE_HAS_STREAM
        const unsigned long long off = per_stream(p.offset, p.step_dev, md);
        const float total = tree[1], seg = __fdiv_rn(total, (float)B);
#endif
        for (int j = threadIdx.x; j < B; j += PER_THREADS) {
            float val;
            idx[j] = per_descend(tree, P, seed, j, off, total, seg, val);
            w[j] = val;                        // (the leaf, until the batch minimum is known)
            pmin = fminf(pmin, val);
        }
    } else {
        for (int j = threadIdx.x; j < B; j += PER_THREADS) {
            const long long ix = idx[j];
            const float val = (ix >= 0 && ix < P) ? tree[P + ix] : 0.f;       // (the caller checks given indices; never read outside the tree)
            w[j] = val;
            pmin = fminf(pmin, val);
        }
    }
    pmin = per_block_min(pmin, sh);
    for (int j = threadIdx.x; j < B; j += PER_THREADS) {       // (each thread reads back what it wrote itself)
        const float pj = w[j];
        w[j] = (pj == pmin || beta == 0.f) ? 1.0f : powf(__fdiv_rn(pmin, pj), beta);
    }
