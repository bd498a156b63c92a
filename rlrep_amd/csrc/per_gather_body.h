// body of a gathering workgroup of the fused sample + gather launches (per_sample_fill_kernel and its group form): samples [lo, lo + n) of
// the batch.  It repeats THEIR descents (one per thread, a single pass), keeps their indices in LDS (rows: int[PER_FILL_ROWS]) and copies
// their ring rows.  `pf` is the PerSampleFill record and `p` its PerSample (scalars; member 0's in a group); `tree`, `idx`, `seed` are
// the agent's or the member's; `off`, `total`, `seg` as per_sample_body.h reads them; GRP and `md` as slot_put takes them; `m`, `rstride` the member
// and the rings' stride (both unused by a single agent).
    const int lo = (blockIdx.x - 1) * pf.rows, n = B - lo < pf.rows ? B - lo : pf.rows;
    if ((int)threadIdx.x < n) {
        float val;
        long long ix = p.given ? (long long)idx[lo + threadIdx.x] : (long long)per_descend(tree, P, seed, lo + threadIdx.x, off, total, seg, val);
        // a drawn leaf carries mass, so its row is one the ring holds; a given index is the caller's to check.  Whatever it is, nothing is
        // read outside the ring
        ix = ix < 0 ? 0 : ix >= pf.capacity ? pf.capacity - 1 : ix;
        rows[threadIdx.x] = (int)ix;
    }
    __syncthreads();
    const int row_w = 2 * pf.f.S + pf.f.A + 2, SA = pf.f.S + pf.f.A;
    const int count = n * row_w;                    // (about PER_FILL_ELEMS * 256 elements, or one row)
    const float* ring = rl_mv<GRP>(pf.f.ring, (long long)m * rstride);          // (the product here, behind the barrier, as the group form had it)
    // PER_FILL_ELEMS loads at a time into registers, then their stores: written as one loop, every load waits for the stores in front of it
    // (the slot arrays might alias the ring, for all the compiler knows), and a thread's elements cost a memory latency EACH
    for (int base = 0; base < count; base += PER_FILL_ELEMS * PER_THREADS) {
        float v[PER_FILL_ELEMS]; int kk[PER_FILL_ELEMS], cc[PER_FILL_ELEMS];
#pragma unroll
        for (int u = 0; u < PER_FILL_ELEMS; ++u) {
            const int e = base + u * PER_THREADS + threadIdx.x;
            kk[u] = e / row_w; cc[u] = e - kk[u] * row_w;
            v[u] = e < count ? ring[(size_t)rows[kk[u]] * row_w + cc[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PER_FILL_ELEMS; ++u) {
            if (base + u * PER_THREADS + (int)threadIdx.x >= count) continue;
            slot_put<GRP>(pf.f, md, SA, lo + kk[u], cc[u], v[u]);
        }
    }
