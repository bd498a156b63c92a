// body of the 32 x 32 bf16x3 tile whose waves split K (gemm_x3q_kernel) and of its group form (group.h), included inside both kernels: GRP (compile time) and dm -- the member's
// byte offset, 0 in the single-agent kernel -- are declared by the kernel; every pointer the body loads from its task
// record is moved by dm where it is loaded (rl_mv), the record itself stays in the kernel-argument segment
    const int gdir[GEMM_MAX_TASKS] = {d0, d1, d2, d3, d4, d5, d6, d7};
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * X3Q_WAVE];          // 48 KB: a 12 KB patch per wave; the epilogue's [4][32][36] floats afterwards
    const int bid = blockIdx.x;
    int ti = 0;
#pragma unroll
    for (int q = 1; q < GEMM_MAX_TASKS; ++q) if (bid >= gdir[q]) ti = q;
    const GemmTask& t = gb.t[ti];
    const float* const pA = rl_mv<GRP>(t.A, dm); const float* const pB = rl_mv<GRP>(t.B, dm);
    const int lda = t.lda, ldb = t.ldb, R = t.R, Cn = t.Cn, K = t.K;
    const int tiles_r = (R + 31) >> 5;
    const int local = gl_xcd_remap(bid - t.tile_base, t.ntiles);
    const int tc = local / tiles_r, tr = local - tc * tiles_r;         // (neighbours share the 32 weight rows / columns of B)
    const int r0 = tr * 32, c0 = tc * 32;

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int kq = (((K + 3) >> 2) + 31) & ~31;                      // this wave's quarter of K, whole 32-deep slices
    const int kbeg = min(w * kq, K), kend = min(K, kbeg + kq);
    const int nk = (kend - kbeg + 31) >> 5;
    unsigned char* const Lw = lds + w * X3Q_WAVE;

    // staging roles
    const int srow = lane >> 1, skh = lane & 1;                      // row-major: (row, k half)
    const int skp = lane >> 2, scg = lane & 3;                       // k-major: (k pair, column group)
    const float* const pa = pA + (size_t)min(r0 + srow, R - 1) * lda;
    const float* const pb = LB == LD_ROW ? pB + (size_t)min(c0 + srow, Cn - 1) * ldb : pB + min(c0 + 8 * scg, Cn - 8);
    // fragment roles (32x32x16: lane = (row | column r32, k half hh))
    const int r32 = lane & 31, hh = lane >> 5;
    const int fo = x3r_off(r32, hh), fsw = x3r_off(r32, 2 + hh) - x3r_off(r32, hh);

    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc0[q] = 0.f; acc1[q] = 0.f; }
    f32x4 ea[2][4], eb[2][4];
#define X3Q_LOAD(Z, KS)                                                                                                       \
    {                                                                                                                         \
        const int kz_ = kbeg + 32 * (KS);                                                                                     \
        x3q_load_row<0>(pa, kz_, kend, K, skh, ea[Z]);                                                                        \
        if constexpr (LB == LD_ROW) x3q_load_row<0>(pb, kz_, kend, K, skh, eb[Z]); else x3q_load_col<0>(pb, ldb, kz_, kend, K, skp, eb[Z]); \
    }
#define X3Q_SPLIT(Z, KS)                                                                                                      \
    {                                                                                                                         \
        const int kz_ = kbeg + 32 * (KS);                                                                                     \
        x3q_load_row<1>(pa, kz_, kend, K, skh, ea[Z]);                                                                        \
        if constexpr (LB == LD_ROW) x3q_load_row<1>(pb, kz_, kend, K, skh, eb[Z]); else x3q_load_col<1>(pb, ldb, kz_, kend, K, skp, eb[Z]); \
        x3q_write_row(Lw, srow, skh, ea[Z]);                                                                                  \
        if constexpr (LB == LD_ROW) x3q_write_row(Lw + 3 * X3Q_IMG, srow, skh, eb[Z]); else x3q_write_col(Lw + 3 * X3Q_IMG, skp, scg, eb[Z]); \
    }
    // one slice: its twelve fragments out of the patch, the loads of slice KT + 2 into the set it frees, the MFMAs, and -- under them -- the split of
    // slice KT + 1 into the same patch (the fragment reads above have been issued: same-wave LDS operations execute in order)
#define X3Q_ITER(Z, KT)                                                                                                       \
    {                                                                                                                         \
        bf16x8 a[2][3], b[2][3];                                                                                              \
        _Pragma("unroll") for (int c = 0; c < 2; ++c) {                                                                       \
            _Pragma("unroll") for (int m = 0; m < 3; ++m) {                                                                   \
                a[c][m] = *reinterpret_cast<const bf16x8*>(Lw + m * X3Q_IMG + fo + fsw * c);                                  \
                b[c][m] = *reinterpret_cast<const bf16x8*>(Lw + (3 + m) * X3Q_IMG + fo + fsw * c);                            \
            }                                                                                                                 \
        }                                                                                                                     \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                                \
        X3Q_LOAD(Z, (KT) + 2)                                                                                                 \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][0], b[0][2], acc0, 0, 0, 0);                                      \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][0], b[1][2], acc1, 0, 0, 0);                                      \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][2], b[0][0], acc0, 0, 0, 0);                                      \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][2], b[1][0], acc1, 0, 0, 0);                                      \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][1], b[0][1], acc0, 0, 0, 0);                                      \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][1], b[1][1], acc1, 0, 0, 0);                                      \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][0], b[0][1], acc0, 0, 0, 0);                                      \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][0], b[1][1], acc1, 0, 0, 0);                                      \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][1], b[0][0], acc0, 0, 0, 0);                                      \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][1], b[1][0], acc1, 0, 0, 0);                                      \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][0], b[0][0], acc0, 0, 0, 0);                                      \
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][0], b[1][0], acc1, 0, 0, 0);                                      \
        X3Q_SPLIT((Z) ^ 1, (KT) + 1)                                                                                          \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                                \
    }
    if (nk > 0) {
        X3Q_LOAD(0, 0) X3Q_LOAD(1, 1)
        X3Q_SPLIT(0, 0)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        // (pairs of slices: one basic block per pair, static register sets; a slice past the end of an odd quarter multiplies the zeros of its own fill)
        for (int kt = 0; kt < nk; kt += 2) {
            X3Q_ITER(0, kt)
            X3Q_ITER(1, kt + 1)
        }
    }
#undef X3Q_ITER
#undef X3Q_SPLIT
#undef X3Q_LOAD
    __syncthreads();                                                 // every wave is done with its patch: the partial tiles meet in LDS

    // accumulator (32x32 C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) -> this wave's [32][36] patch
    float* const E = reinterpret_cast<float*>(lds) + w * (32 * 36);
#pragma unroll
    for (int q = 0; q < 16; ++q) E[((q & 3) + 8 * (q >> 2) + 4 * hh) * 36 + r32] = acc0[q] + acc1[q];
    __syncthreads();
    // wave w finishes rows 8 w .. 8 w + 7 of the tile: the four quarters in order, then the epilogue
    const int rr = 8 * w + (lane >> 3), cc = (lane & 7) * 4;
    const float* const E0 = reinterpret_cast<const float*>(lds) + rr * 36 + cc;
    f32x4 v = *reinterpret_cast<const f32x4*>(E0);
#pragma unroll
    for (int p = 1; p < 4; ++p) v += *reinterpret_cast<const f32x4*>(E0 + p * (32 * 36));
    const int r = r0 + rr, c = c0 + cc;
    if (r < R && c < Cn) gl_epilogue4<GRP>(t, r, c, v, nullptr, dm);
