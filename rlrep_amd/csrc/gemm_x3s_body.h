// body of the 64-wide bf16x3 tile (gemm_x3s_kernel) and of its group form (group.h), included inside both kernels: GRP (compile time) and dm -- the member's
// byte offset, 0 in the single-agent kernel -- are declared by the kernel; every pointer the body loads from its task
// record is moved by dm where it is loaded (rl_mv), the record itself stays in the kernel-argument segment
    const int gdir[GEMM_MAX_TASKS] = {d0, d1, d2, d3, d4, d5, d6, d7};
    constexpr int BT = 64;
    constexpr int AIMG = LA == LD_ROW ? X3S_RIMGB : X3S_TIMGB, BIMG = LB == LD_ROW ? X3S_RIMGB : X3S_TIMGB;
    constexpr int EPB = 4 * 32 * 36 * 4;                         // epilogue patches [32][36] per wave, bytes
    constexpr int STB = 3 * AIMG + 3 * BIMG;
    static_assert(EPB <= STB, "the epilogue patches live in stage 0");
    // TWO LDS stages (two arrays: the compiler then knows that the fragment reads of one and the staging writes of the other do not alias), ONE
    // barrier per slice: slice kt is multiplied out of one stage while slice kt + 1 is split into the other.
    __shared__ __attribute__((aligned(16))) float lds[STB / 4], lds1[STB / 4];
    unsigned char* const L0 = reinterpret_cast<unsigned char*>(lds);
    unsigned char* const L1 = reinterpret_cast<unsigned char*>(lds1);
    const unsigned Lb0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)L0;
    const unsigned Lb1 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)L1;

    const int bid = blockIdx.x;
    int ti = 0;
#pragma unroll
    for (int q = 1; q < GEMM_MAX_TASKS; ++q) if (bid >= gdir[q]) ti = q;          // (preloaded directory: first tiles, INT_MAX beyond the last task)
    const GemmTask& t = gb.t[ti];
    const float* const pA = rl_mv<GRP>(t.A, dm); const float* const pB = rl_mv<GRP>(t.B, dm);
    const int lda = t.lda, ldb = t.ldb, R = t.R, Cn = t.Cn, K = t.K;
    const int tiles_c = t.tiles_c, splits = t.splits, kchunk = t.kchunk;
    const int tiles_r = (R + BT - 1) / BT;
    const int local = gl_xcd_remap(bid - t.tile_base, t.ntiles);
    const int per_split = tiles_r * tiles_c;
    const int split = local / per_split, rem = local - split * per_split;
    const int tc = rem / tiles_r, tr = rem - tc * tiles_r;
    const int r0 = tr * BT, c0 = tc * BT;
    const int kbeg = split * kchunk, kend = min(K, kbeg + kchunk);
    const int nk = (kend - kbeg + GL_BK - 1) / GL_BK;

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = w >> 1, wc = w & 1;
    const int r32 = lane & 31, hh = lane >> 5, g1 = (lane >> 4) & 1;
    const bool want_bias = LA == LD_COL && t.epi == EPI_DW && (t.flags & FLAG_BIASGRAD) && tc == 0;

    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    f32x4 rs = {0.f, 0.f, 0.f, 0.f};

    // TWO sets of staging registers, loads two slices ahead of their split: set z holds the slices of parity z.  (One set, loaded behind the barrier
    // and split before the next one, left a load's whole latency in every slice wherever fewer than four workgroups share a CU.)
    f32x4 ear[2][2], ebr[2][2];
    f32x4 eac[2][2], ebc[2][2];
#define X3S_LOAD(Z, KS)                                                                                                       \
    {                                                                                                                         \
        const int kz_ = kbeg + GL_BK * (KS);                                                                                  \
        if constexpr (LA == LD_ROW) x3s_load_row<VEC, 0>(pA, lda, r0, R, kz_, kend, ear[Z]); else x3s_load_col<VEC, 0>(pA, lda, r0, R, kz_, kend, eac[Z]); \
        if constexpr (LB == LD_ROW) x3s_load_row<VEC, 0>(pB, ldb, c0, Cn, kz_, kend, ebr[Z]); else x3s_load_col<VEC, 0>(pB, ldb, c0, Cn, kz_, kend, ebc[Z]); \
    }
    // what depends on the loaded values (K tail / edge zero fill, unaligned shift), then split set Z = slice KS into the stage at LW
#define X3S_SPLIT(Z, KS, LW)                                                                                                  \
    {                                                                                                                         \
        const int kz_ = kbeg + GL_BK * (KS);                                                                                  \
        if constexpr (LA == LD_ROW) x3s_load_row<VEC, 1>(pA, lda, r0, R, kz_, kend, ear[Z]); else x3s_load_col<VEC, 1>(pA, lda, r0, R, kz_, kend, eac[Z]); \
        if constexpr (LB == LD_ROW) x3s_load_row<VEC, 1>(pB, ldb, c0, Cn, kz_, kend, ebr[Z]); else x3s_load_col<VEC, 1>(pB, ldb, c0, Cn, kz_, kend, ebc[Z]); \
        if (want_bias) rs += eac[Z][0] + eac[Z][1];                                                                           \
        if constexpr (LA == LD_ROW) x3s_write_row(LW, ear[Z]); else x3s_write_col(LW, eac[Z]);                                \
        if constexpr (LB == LD_ROW) x3s_write_row((LW) + 3 * AIMG, ebr[Z]); else x3s_write_col((LW) + 3 * AIMG, ebc[Z]);      \
    }
    X3S_LOAD(0, 0) X3S_LOAD(1, 1)
    X3S_SPLIT(0, 0, L0)
    X3S_LOAD(0, 2)

    const int foA = x3r_off(wr * 32 + r32, hh), foB = 3 * AIMG + x3r_off(wc * 32 + r32, hh);
    const int fsw = x3r_off(r32, 2 + hh) - x3r_off(r32, hh);            // block 1 relative to block 0 (swizzled chunks)
    const unsigned tA0 = x3s_taddr(0, 8 * hh, wr * 4 + 2 * g1), tA1 = x3s_taddr(0, 8 * hh + 4, wr * 4 + 2 * g1);
    const unsigned tB0 = x3s_taddr(3 * AIMG, 8 * hh, wc * 4 + 2 * g1), tB1 = x3s_taddr(3 * AIMG, 8 * hh + 4, wc * 4 + 2 * g1);

#define X3S_BLOCK(C, LR, LBR)                                                                                                 \
        {                                                                                                                     \
            bf16x8 a[3], b[3];                                                                                                \
            if constexpr (LA == LD_ROW) {                                                                                     \
                _Pragma("unroll") for (int m = 0; m < 3; ++m) a[m] = *reinterpret_cast<const bf16x8*>((LR) + foA + m * X3S_RIMGB + fsw * (C)); \
            } else {                                                                                                          \
                a[0] = x3t_frag<(C) * 2048>((LBR) + tA0, (LBR) + tA1); a[1] = x3t_frag<(C) * 2048 + X3S_TIMGB>((LBR) + tA0, (LBR) + tA1); \
                a[2] = x3t_frag<(C) * 2048 + 2 * X3S_TIMGB>((LBR) + tA0, (LBR) + tA1);                                         \
            }                                                                                                                 \
            if constexpr (LB == LD_ROW) {                                                                                     \
                _Pragma("unroll") for (int m = 0; m < 3; ++m) b[m] = *reinterpret_cast<const bf16x8*>((LR) + foB + m * X3S_RIMGB + fsw * (C)); \
            } else {                                                                                                          \
                b[0] = x3t_frag<(C) * 2048>((LBR) + tB0, (LBR) + tB1); b[1] = x3t_frag<(C) * 2048 + X3S_TIMGB>((LBR) + tB0, (LBR) + tB1); \
                b[2] = x3t_frag<(C) * 2048 + 2 * X3S_TIMGB>((LBR) + tB0, (LBR) + tB1);                                         \
            }                                                                                                                 \
            f32x16 v = acc;                                                                                                   \
            v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], v, 0, 0, 0);                                              \
            v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], v, 0, 0, 0);                                              \
            v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], v, 0, 0, 0);                                              \
            v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], v, 0, 0, 0);                                              \
            v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], v, 0, 0, 0);                                              \
            v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], v, 0, 0, 0);                                              \
            acc = v;                                                                                                          \
        }
    // one slice: multiply slice KT out of the stage LR while set Z (slice KT + 1) is split into LW and refilled with slice KT + 3
#define X3S_ITER(Z, KT, LR, LBR, LW)                                                                                          \
    {                                                                                                                         \
        __syncthreads();                                                                                                      \
        X3S_SPLIT(Z, (KT) + 1, LW)                                                                                            \
        X3S_LOAD(Z, (KT) + 3)                                                                                                 \
        X3S_BLOCK(0, LR, LBR) X3S_BLOCK(1, LR, LBR)                                                                           \
    }
    // (ONE basic block per pair of slices: with a branch between the two the compiler's wait-count pass waited with vmcnt(0) in the second -- for the
    // loads the first had just issued.  A slice past the end of an odd chunk multiplies the zeros its own K-tail fill produces.)
    for (int kt = 0; kt < nk; kt += 2) {
        X3S_ITER(1, kt, L0, Lb0, L1)
        X3S_ITER(0, kt + 1, L1, Lb1, L0)
    }
#undef X3S_ITER
#undef X3S_BLOCK
#undef X3S_SPLIT
#undef X3S_LOAD
    __syncthreads();                                             // (the epilogue's patches and the bias sums reuse stage 0)

    // split-K without a finishing launch (FLAG_FIN_INLINE): every split workgroup writes its partial tile THROUGH to memory (the XCDs' L2s are
    // not coherent with each other inside a launch), takes a ticket on the tile's counter, and the LAST one to arrive sums the slabs IN SPLIT ORDER
    // (its own included, from memory: the arithmetic of gemm_lds_fin_kernel, bit for bit) and runs the epilogue.  The counters sit behind the
    // task's slabs, zero between launches (the last arrival resets its own).
    const bool inl = splits > 1 && (t.flags & FLAG_FIN_INLINE);
    const int C4p = (Cn + 3) & ~3;
    if (want_bias) {       // row sums of the k-major A: this thread holds rows 4 (tid % 16) .. over its 16 k slots
        float* part = lds;                                   // [64 rows][16 k slots]
        const int c4 = (int)(threadIdx.x & 15) * 4, ks = (int)(threadIdx.x >> 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) part[(c4 + q) * 16 + ks] = rs[q];
        __syncthreads();
        if (threadIdx.x < 64) {
            const float* q = part + threadIdx.x * 16;
            float s0 = 0.f;
#pragma unroll
            for (int z = 0; z < 16; ++z) s0 += q[z];
            const int r = r0 + threadIdx.x;
            if (r < R) { if (inl) dp_store1(rl_mv<GRP>(t.bslab, dm) + (size_t)split * R + r, s0); else if (splits > 1) rl_mv<GRP>(t.bslab, dm)[(size_t)split * R + r] = s0; else rl_mv<GRP>(t.out2, dm)[r] = s0; }
        }
        __syncthreads();
    }

    // accumulator (32x32 C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) -> LDS patch -> row segments
    float* E = lds + w * (32 * 36);
#pragma unroll
    for (int q = 0; q < 16; ++q) E[((q & 3) + 8 * (q >> 2) + 4 * hh) * 36 + r32] = acc[q];
    const f32x4 bpre = splits > 1 ? (f32x4){0.f, 0.f, 0.f, 0.f} : gl_bias4<GRP>(t, c0 + wc * 32 + (lane & 7) * 4, dm);       // (this lane's columns: the same in every iteration)
#pragma unroll 4
    for (int it = 0; it < 4; ++it) {
        const int rr = it * 8 + (lane >> 3), cc = (lane & 7) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(E + rr * 36 + cc);
        const int r = r0 + wr * 32 + rr, c = c0 + wc * 32 + cc;
        if (r < R && c < Cn) {
            if (inl) dp_store4(rl_mv<GRP>(t.slab, dm) + ((size_t)split * R + r) * C4p + c, v);
            else if (splits > 1) st4(rl_mv<GRP>(t.slab, dm) + ((size_t)split * R + r) * C4p + c, v);
            else gl_epilogue4<GRP>(t, r, c, v, &bpre, dm);
        }
    }
    if (!inl) return;
    __builtin_amdgcn_s_waitcnt(0x0F70);                          // vmcnt(0): this thread's write-through stores have reached memory
    __syncthreads();
    int* const tick = reinterpret_cast<int*>(rl_mv<GRP>(t.slab, dm) + (size_t)splits * R * C4p) + rem;
    if (threadIdx.x == 0) {
        const int old = atomicAdd(tick, 1);
        const int last = old == splits - 1;
        if (last) atomicExch(tick, 0);
        reinterpret_cast<volatile int*>(lds)[0] = last;          // (stage 0 is free: the patches above were consumed before the barrier)
    }
    __syncthreads();
    if (reinterpret_cast<volatile int*>(lds)[0] == 0) return;
#pragma unroll 2
    for (int it = 0; it < 4; ++it) {
        const int rr = it * 8 + (lane >> 3), cc = (lane & 7) * 4;
        const int r = r0 + wr * 32 + rr, c = c0 + wc * 32 + cc;
        if (r < R && c < Cn) {
            const float* p = rl_mv<GRP>(t.slab, dm) + (size_t)r * C4p + c;
            const size_t stride = (size_t)R * C4p;
            f32x4 v = dp_load4(p);
            for (int s = 1; s < splits; ++s) v += dp_load4(p + s * stride);
            gl_epilogue4<GRP>(t, r, c, v, nullptr, dm);
        }
    }
    if (want_bias && threadIdx.x < 64) {
        const int r = r0 + threadIdx.x;
        if (r < R) {
            float s0 = dp_load1(rl_mv<GRP>(t.bslab, dm) + r);
            for (int q = 1; q < splits; ++q) s0 += dp_load1(rl_mv<GRP>(t.bslab, dm) + (size_t)q * R + r);
            rl_mv<GRP>(t.out2, dm)[r] = s0;
        }
    }
