// body of the fp32-MFMA BT x BT tile (gemm_lds_kernel) and of its group form (group.h), included inside both kernels: GRP (compile time) and dm -- the member's
// byte offset, 0 in the single-agent kernel -- are declared by the kernel; every pointer the body loads from its task
// record is moved by dm where it is loaded (rl_mv), the record itself stays in the kernel-argument segment
    const int gdir[GEMM_MAX_TASKS] = {d0, d1, d2, d3, d4, d5, d6, d7};
    constexpr int WT = BT / 2, TT = WT / 16;
    constexpr int SA = GlTile<BT, LA>::FLOATS, SB = GlTile<BT, LB>::FLOATS;
    constexpr int EPF = 4 * WT * (WT + 4);
    constexpr int LDSF = (2 * (SA + SB) > EPF) ? 2 * (SA + SB) : EPF;
    __shared__ __attribute__((aligned(16))) float lds[LDSF];

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
    const int i = lane & 15, kq = lane >> 4;

    f32x4 acc[TT][TT];
#pragma unroll
    for (int a = 0; a < TT; ++a)
#pragma unroll
        for (int b = 0; b < TT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float asum[TT];
#pragma unroll
    for (int a = 0; a < TT; ++a) asum[a] = 0.f;

    const bool vecA = !(t.flags & FLAG_SCALAR_A), vecB = !(t.flags & FLAG_SCALAR_B);
    f32x4 va[BT / 32], vb[BT / 32];
    gl_stage_load<BT, LA>(pA, lda, r0, R, kbeg, kend, vecA, va);
    gl_stage_load<BT, LB>(pB, ldb, c0, Cn, kbeg, kend, vecB, vb);
    gl_stage_write<BT, LA>(lds, va);
    gl_stage_write<BT, LB>(lds + SA, vb);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        // slice kt+1 (past the end: a clamped, zeroed re-read that nobody consumes) -- issued before the MFMAs of slice kt
        const int kn = kbeg + GL_BK * (kt + 1);
        gl_stage_load<BT, LA>(pA, lda, r0, R, kn, kend, vecA, va);
        gl_stage_load<BT, LB>(pB, ldb, c0, Cn, kn, kend, vecB, vb);
        const float* As = lds + cur * (SA + SB);
        const float* Bs = As + SA;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float fa[TT][2], fb[TT][2];
            gl_frag<BT, LA, TT>(As, wr * WT, i, kq, j, fa);
            gl_frag<BT, LB, TT>(Bs, wc * WT, i, kq, j, fb);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int a = 0; a < TT; ++a)
#pragma unroll
                    for (int b = 0; b < TT; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a][e], fb[b][e], acc[a][b], 0, 0, 0);
            if (LA == LD_COL) {
#pragma unroll
                for (int a = 0; a < TT; ++a) asum[a] += fa[a][0] + fa[a][1];
            }
        }
        float* Sn = lds + (cur ^ 1) * (SA + SB);
        gl_stage_write<BT, LA>(Sn, va);
        gl_stage_write<BT, LB>(Sn + SA, vb);
        __syncthreads();
    }

    const size_t C4w = (size_t)((Cn + 3) & ~3);
    // bias gradient (EPI_DW): row sums of operand A, taken from the fragments the column-0 waves of column-tile 0 consumed
    const bool has_bias = LA == LD_COL && t.epi == EPI_DW && (t.flags & FLAG_BIASGRAD) && tc == 0;
    if (has_bias && wc == 0) {
#pragma unroll
        for (int a = 0; a < TT; ++a) {
            float s = asum[a];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            const int r = r0 + wr * WT + a * 16 + lane;
            if (lane < 16 && r < R) {
                if (splits > 1) rl_mv<GRP>(t.bslab, dm)[(size_t)split * R + r] = s;
                else rl_mv<GRP>(t.out2, dm)[r] = s;
            }
        }
    }

    // accumulators -> this wave's LDS patch -> 16-byte row segments (coalesced stores, vector epilogue operands)
    float* E = lds + w * (WT * (WT + 4));
#pragma unroll
    for (int a = 0; a < TT; ++a)
#pragma unroll
        for (int b = 0; b < TT; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) E[(a * 16 + 4 * kq + q) * (WT + 4) + b * 16 + i] = acc[a][b][q];
    constexpr int LPR = WT / 4, RPI = 64 / LPR;
    const f32x4 bpre = splits > 1 ? (f32x4){0.f, 0.f, 0.f, 0.f} : gl_bias4<GRP>(t, c0 + wc * WT + (lane % LPR) * 4, dm);      // (this lane's columns: the same in every iteration)
#pragma unroll 4
    for (int it = 0; it < WT / RPI; ++it) {
        const int rr = it * RPI + lane / LPR, cc = (lane % LPR) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(E + rr * (WT + 4) + cc);
        const int r = r0 + wr * WT + rr, c = c0 + wc * WT + cc;
        if (r < R && c < Cn) {
            if (splits > 1) st4(rl_mv<GRP>(t.slab, dm) + ((size_t)split * R + r) * C4w + c, v);       // partial tile: the finishing blocks add the slabs in split order
            else gl_epilogue4<GRP>(t, r, c, v, &bpre, dm);
        }
    }
