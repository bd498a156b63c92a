// body of the 128-wide bf16x3 forward tile (gemm_x3_kernel) and of its group form (group.h), included inside both kernels: GRP (compile time) and dm -- the member's
// byte offset, 0 in the single-agent kernel -- are declared by the kernel; every pointer the body loads from its task
// record is moved by dm where it is loaded (rl_mv), the record itself stays in the kernel-argument segment
    const int gdir[GEMM_MAX_TASKS] = {d0, d1, d2, d3, d4, d5, d6, d7};
    constexpr int BT = 128;
    constexpr int EPB = 8 * 32 * 68 * 4;                         // epilogue patches [32][68] per wave, bytes
    constexpr int STB = 6 * X3_IMGB;                             // six images
    constexpr int LDSB = EPB > STB ? EPB : STB;
    __shared__ __attribute__((aligned(16))) float lds[LDSB / 4];
    unsigned char* const L = reinterpret_cast<unsigned char*>(lds);

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
    const int r32 = lane & 31, hh = lane >> 5;
    const bool want_bias = (LA == LD_COL) && t.epi == EPI_DW && (t.flags & FLAG_BIASGRAD) && tc == 0;

    f32x16 acc[2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[b][q] = 0.f;
    float rs = 0.f;

    float ea[8], eb[8];
    x3_stage_load<LA>(pA, lda, r0, R, kbeg, kend, ea);
    x3_stage_load<LB>(pB, ldb, c0, Cn, kbeg, kend, eb);

    // The two workgroups of a CU alternate a VALU phase (split + LDS write) and a matrix phase; started together they
    // stay in step.  Workgroups are dealt one per CU before any CU gets its second (observed, speed only), so delaying
    // every second group of 256 by about one VALU phase starts the pair in anti-phase.
    if (X3_STAGGER && ((blockIdx.x >> 8) & 1)) __builtin_amdgcn_s_sleep(X3_STAGGER);

    // fragment of 16-deep block c: chunk 2 c + hh of this lane's row -- the swizzle term (row >> 2) & 3 is the same for rows r32, 32 + r32, ...
    const unsigned char* const fa = L + x3r_off(wr * 32 + r32, hh);
    const unsigned char* const fb = L + 3 * X3_IMGB + x3r_off(wc * 64 + r32, hh);
    const int fsw = x3r_off(r32, 2 + hh) - x3r_off(r32, hh);            // block 1 relative to block 0: +32 or -32 bytes

    for (int kt = 0; kt < nk; ++kt) {
        if (want_bias) rs += ((ea[0] + ea[1]) + (ea[2] + ea[3])) + ((ea[4] + ea[5]) + (ea[6] + ea[7]));
        x3_stage_write<LA>(L, ea);
        x3_stage_write<LB>(L + 3 * X3_IMGB, eb);
        __syncthreads();
        const int kn = kbeg + GL_BK * (kt + 1);
        x3_stage_load<LA>(pA, lda, r0, R, kn, kend, ea);
        x3_stage_load<LB>(pB, ldb, c0, Cn, kn, kend, eb);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            bf16x8 a[3], b[2][3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                a[m] = *reinterpret_cast<const bf16x8*>(fa + m * X3_IMGB + fsw * c);
                b[0][m] = *reinterpret_cast<const bf16x8*>(fb + m * X3_IMGB + fsw * c);
                b[1][m] = *reinterpret_cast<const bf16x8*>(fb + 32 * X3_RSB + m * X3_IMGB + fsw * c);
            }
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                f32x16 v = acc[y];
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[y][2], v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[y][0], v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[y][1], v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[y][1], v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[y][0], v, 0, 0, 0);
                v = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[y][0], v, 0, 0, 0);
                acc[y] = v;
            }
        }
        __syncthreads();
    }

    // bias gradient: this thread's row (k-major A: row tid & 127, one of four k groups) -> LDS -> fixed-order sum
    if (want_bias) {
        float* part = lds;                                   // [128][4]
        part[(threadIdx.x & 127) * 4 + (threadIdx.x >> 7)] = rs;
        __syncthreads();
        if (threadIdx.x < 128) {
            const float* q = part + threadIdx.x * 4;
            const float s = (q[0] + q[1]) + (q[2] + q[3]);
            const int r = r0 + threadIdx.x;
            if (r < R) { if (splits > 1) rl_mv<GRP>(t.bslab, dm)[(size_t)split * R + r] = s; else rl_mv<GRP>(t.out2, dm)[r] = s; }
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
