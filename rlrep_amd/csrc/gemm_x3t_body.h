// body of the 128-wide bf16x3 dX / dW tile (gemm_x3t_kernel) and of its group form (group.h), included inside both kernels: GRP (compile time) and dm -- the member's
// byte offset, 0 in the single-agent kernel -- are declared by the kernel; every pointer the body loads from its task
// record is moved by dm where it is loaded (rl_mv), the record itself stays in the kernel-argument segment
    const int gdir[GEMM_MAX_TASKS] = {d0, d1, d2, d3, d4, d5, d6, d7};
    constexpr int BT = 128;
    constexpr int EPB = 8 * 32 * 68 * 4;                         // epilogue patches [32][68] per wave, bytes
    constexpr int AIMG = LA == LD_ROW ? X3_IMGB : X3T_IMGB;      // bytes per A image
    constexpr int STB = 3 * AIMG + 3 * X3T_IMGB;                 // six images
    constexpr int LDSB = EPB > STB ? EPB : STB;
    __shared__ __attribute__((aligned(16))) float lds[LDSB / 4];
    unsigned char* const L = reinterpret_cast<unsigned char*>(lds);
    const unsigned Lb = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)L;

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

    f32x16 acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;
    f32x4 rs = {0.f, 0.f, 0.f, 0.f};

    f32x4 ea[2], eb[2];
    float ear[8];                                               // (row-major A: gemm_x3_kernel's staging registers)
    if constexpr (LA == LD_ROW) x3_stage_load<LD_ROW>(pA, lda, r0, R, kbeg, kend, ear);
    else x3t_stage_load(pA, lda, r0, R, kbeg, kend, ea);
    x3t_stage_load(pB, ldb, c0, Cn, kbeg, kend, eb);
    if (X3_STAGGER && ((blockIdx.x >> 8) & 1)) __builtin_amdgcn_s_sleep(X3_STAGGER);        // (anti-phase start of a CU's two workgroups: gemm_x3_kernel)

    // transposed-read addresses: k-block h of this lane's k group (k = 8 hh + 4 h within a 16-deep block c; c and the image by immediate offset)
    const unsigned aA0 = x3t_addr(Lb, 8 * hh, wr * 4 + 2 * g1), aA1 = x3t_addr(Lb, 8 * hh + 4, wr * 4 + 2 * g1);
    const unsigned aB00 = x3t_addr(Lb + 3 * AIMG, 8 * hh, wc * 8 + 2 * g1), aB01 = x3t_addr(Lb + 3 * AIMG, 8 * hh + 4, wc * 8 + 2 * g1);
    const unsigned aB10 = x3t_addr(Lb + 3 * AIMG, 8 * hh, wc * 8 + 4 + 2 * g1), aB11 = x3t_addr(Lb + 3 * AIMG, 8 * hh + 4, wc * 8 + 4 + 2 * g1);
    const unsigned char* const far = L + x3r_off(wr * 32 + r32, hh);                       // row-major A fragments (ds_read_b128; swizzled chunks: x3r_off)
    const int fsw = x3r_off(r32, 2 + hh) - x3r_off(r32, hh);

    for (int kt = 0; kt < nk; ++kt) {
        if (want_bias) rs += ea[0] + ea[1];
        if constexpr (LA == LD_ROW) x3_stage_write<LD_ROW>(L, ear);
        else x3t_stage_write(L, ea);
        x3t_stage_write(L + 3 * AIMG, eb);
        __syncthreads();
        const int kn = kbeg + GL_BK * (kt + 1);
        if constexpr (LA == LD_ROW) x3_stage_load<LD_ROW>(pA, lda, r0, R, kn, kend, ear);
        else x3t_stage_load(pA, lda, r0, R, kn, kend, ea);
        x3t_stage_load(pB, ldb, c0, Cn, kn, kend, eb);
#define X3T_BLOCK(C)                                                                                                          \
        {                                                                                                                     \
            bf16x8 a[3], b[2][3];                                                                                             \
            if constexpr (LA == LD_ROW) {                                                                                     \
                _Pragma("unroll") for (int m = 0; m < 3; ++m) a[m] = *reinterpret_cast<const bf16x8*>(far + m * X3_IMGB + fsw * (C)); \
            } else {                                                                                                          \
                a[0] = x3t_frag<(C) * 4096>(aA0, aA1); a[1] = x3t_frag<(C) * 4096 + X3T_IMGB>(aA0, aA1);                       \
                a[2] = x3t_frag<(C) * 4096 + 2 * X3T_IMGB>(aA0, aA1);                                                         \
            }                                                                                                                 \
            b[0][0] = x3t_frag<(C) * 4096>(aB00, aB01); b[0][1] = x3t_frag<(C) * 4096 + X3T_IMGB>(aB00, aB01);                 \
            b[0][2] = x3t_frag<(C) * 4096 + 2 * X3T_IMGB>(aB00, aB01);                                                        \
            b[1][0] = x3t_frag<(C) * 4096>(aB10, aB11); b[1][1] = x3t_frag<(C) * 4096 + X3T_IMGB>(aB10, aB11);                 \
            b[1][2] = x3t_frag<(C) * 4096 + 2 * X3T_IMGB>(aB10, aB11);                                                        \
            _Pragma("unroll") for (int y = 0; y < 2; ++y) {                                                                   \
                f32x16 v = acc[y];                                                                                            \
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[y][2], v, 0, 0, 0);                                       \
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[y][0], v, 0, 0, 0);                                       \
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[y][1], v, 0, 0, 0);                                       \
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[y][1], v, 0, 0, 0);                                       \
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[y][0], v, 0, 0, 0);                                       \
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[y][0], v, 0, 0, 0);                                       \
                acc[y] = v;                                                                                                   \
            }                                                                                                                 \
        }
        X3T_BLOCK(0) X3T_BLOCK(1)
#undef X3T_BLOCK
        __syncthreads();
    }

    // bias gradient = row sums of operand A: this thread holds four rows (4 (tid % 32) ..) over its k slots -> LDS -> fixed-order sum over the 16 slots
    if (want_bias) {
        float* part = lds;                                   // [128 rows][16 k slots]
        const int c4 = (int)(threadIdx.x & 31) * 4, ks = (int)(threadIdx.x >> 5);
#pragma unroll
        for (int q = 0; q < 4; ++q) part[(c4 + q) * 16 + ks] = rs[q];
        __syncthreads();
        if (threadIdx.x < 128) {
            const float* q = part + threadIdx.x * 16;
            float s0 = 0.f;
#pragma unroll
            for (int z = 0; z < 16; ++z) s0 += q[z];
            const int r = r0 + threadIdx.x;
            if (r < R) { if (splits > 1) rl_mv<GRP>(t.bslab, dm)[(size_t)split * R + r] = s0; else rl_mv<GRP>(t.out2, dm)[r] = s0; }
        }
        __syncthreads();
    }

    // accumulators (32x32 C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) -> LDS patch -> row segments
    float* E = lds + w * (32 * 68);
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int q = 0; q < 16; ++q) E[((q & 3) + 8 * (q >> 2) + 4 * hh) * 68 + y * 32 + r32] = acc[y][q];
    const f32x4 bpre = splits > 1 ? (f32x4){0.f, 0.f, 0.f, 0.f} : gl_bias4<GRP>(t, c0 + wc * 64 + (lane & 15) * 4, dm);      // (this lane's columns: the same in every iteration)
#pragma unroll 4
    for (int it = 0; it < 8; ++it) {
        const int rr = it * 4 + (lane >> 4), cc = (lane & 15) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(E + rr * 68 + cc);
        const int r = r0 + wr * 32 + rr, c = c0 + wc * 64 + cc;
        if (r < R && c < Cn) {
            if (splits > 1) st4(rl_mv<GRP>(t.slab, dm) + ((size_t)split * R + r) * ((Cn + 3) & ~3) + c, v);
            else gl_epilogue4<GRP>(t, r, c, v, &bpre, dm);
        }
    }
