// body of nc_fwd_kernel and of its K-chunked form nc_fwd_chunk_kernel (noisecritic.hip), included inside both kernels: G2, NW are the kernels'
// template parameters, CHUNK (compile time) is declared by the kernel
    const int bid = blockIdx.x;
    NCT(0); NCT(4);
    int ti = 0;
#pragma unroll
    for (int q = 1; q < NC_MAX_TASKS; ++q) if (q < nb.ntasks && bid >= nb.t[q].tile_base) ti = q;
    const NcFwdTask& t = nb.t[ti];
    const int local = bid - t.tile_base;
    const int tb = local / t.tiles_h, th = local - tb * t.tiles_h;
    const int RB = 4 * G2;
    const int b0 = tb * RB, n0 = th * (16 * NW);
    const int F = t.F, H = t.H, N = t.N;
    const int Fp = (F + 15) & ~15;
    const int LDS_LD = CHUNK ? NC_CW + 16 : Fp + 16;
    float* mu_s = nc_smem;                     // [RB][LDS_LD]
    float* sg_s = mu_s + RB * LDS_LD;          // [RB][LDS_LD]
    float* nz_s = sg_s + RB * LDS_LD;          // [N][LDS_LD]

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m16 = lane & 15, kq = lane >> 4;
    const int bp = m16 >> 2, nn = m16 & 3;
    const int col = n0 + 16 * w + m16;
    const bool colok = col < H;
    const bool vecW = ((F & 3) == 0) && ((((uintptr_t)t.W) & 15) == 0);
    const float* wrow = t.W + (size_t)(colok ? col : 0) * F;

    // first W fragment is in flight while the tables are staged
    float wv[4], wn[4];
    {
        const int k0 = 4 * kq;
        const int valid = colok ? max(0, min(4, F - k0)) : 0;
        ld4(wrow + k0, vecW, valid, wv);
    }
    // Table staging: one wave-wide 16-byte load moves a whole 256-float row; every wave issues ALL of its
    // row loads back to back (fixed trip count, fully unrolled) so their L2 latencies overlap instead of
    // serialising (the element-wise loop this replaces cost 7.7 us of a 40 us launch).
    // (CHUNK: only the first chunk here; the later ones are staged between the K loops below)
    {
        constexpr int NROWS = 2 * RB + 4 * NC_NF;          // mean rows, sigma rows, noise rows (N = 20)
        constexpr int SLOTS = (NROWS + NW - 1) / NW;
        const int stage_end = CHUNK ? min(Fp, NC_CW) : Fp;
        for (int cb = 0; cb < stage_end; cb += 256) {
#include "nc_fwd_stage_body.h"
        }
    }
    __syncthreads();
    NCT(1);

    f32x4 acc[G2][NC_NF];
#pragma unroll
    for (int g = 0; g < G2; ++g)
#pragma unroll
        for (int f = 0; f < NC_NF; ++f) acc[g][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // (A variant with two named register sets, which issued the LDS table reads and the W fragment of chunk c+1 before the MFMAs
    // of chunk c, measured the same 47.8k cycles per workgroup for this loop -- tools/exp/nc_timeline.py: staging 4.9k, loop
    // 48.2k, epilogue 3.6k cycles at 2.1 GHz.  The loop runs at 85 % of 32 cycles per MFMA, the rate tools/exp/mfma_peak.hip
    // measures for four waves per SIMD: 126 of 157 TF.)
    if constexpr (!CHUNK) {
        constexpr int cb = 0;
        for (int kb = 0; kb < Fp; kb += 16) {
#include "nc_fwd_kstep_body.h"
        }
    } else {
        constexpr int NROWS = 2 * RB + 4 * NC_NF;
        constexpr int SLOTS = (NROWS + NW - 1) / NW;
        for (int cb = 0;;) {
            const int kend = min(cb + NC_CW, Fp);
            for (int kb = cb; kb < kend; kb += 16) {
#include "nc_fwd_kstep_body.h"
            }
            cb += NC_CW;
            if (cb >= Fp) break;
            __syncthreads();                            // every wave is done with this chunk's table
            {
#include "nc_fwd_stage_body.h"
            }
            __syncthreads();
        }
    }

    NCT(2);
    if (!colok) return;
    const float bj = t.bias[col];
    const float invN = 1.0f / (float)N;
#pragma unroll
    for (int g = 0; g < G2; ++g) {
        const int b = b0 + 4 * g + (lane >> 4);
        if (b >= t.B) continue;
        float sum = 0.f;
#pragma unroll
        for (int f = 0; f < NC_NF; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float y = elu_fast(acc[g][f][r] + bj);
                sum += y;
#ifndef RL_NC_NOU
                if (t.U) t.U[((size_t)b * N + 4 * f + r) * H + col] = y;
#endif
            }
        t.Hm[(size_t)b * H + col] = sum * invN;
    }
    NCT(3); NCT(5);
