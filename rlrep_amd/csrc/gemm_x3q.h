// gemm_x3q_kernel: the bf16x3 tile for products with FEW ROWS and a LONG inner dimension -- ctrlsac's M = 256 layers at main.py's dimensions
// (256 x {1024, 2048} x {1024, 2048}: agent/ctrlsac/ctrlsac_agent.py:54-102, 213-251), diffsrsac's at HalfCheetah dims.  (Included by gemm_lds.hip.)
//
// On the 64 x 64 tile (gemm_x3s_kernel) such a product has 64 - 128 output tiles for 256 CUs, so it was cut along K into slabs: 256 - 512
// workgroups of ONE wave per SIMD each, whose slice is the serial split -> barrier -> 12 MFMAs -> barrier of a lone workgroup, plus a finishing launch
// that adds the slabs (19 - 32 us per layer; the finishers alone were 13 % of ctrlsac's GPU time: profiles/r05_ctrlsac_*_kernel_stats.csv;
// VERDICT r05 item 2).  Here the output tile is 32 x 32 -- 256 / 512 workgroups WITHOUT slabs -- and the K split moves INSIDE the workgroup:
//
//   * 4 waves = 4 quarters of K.  A wave is a workgroup of its own for the whole main loop: it stages ITS 32 x 32 slices of A and B (64 lanes x
//     4 16-byte loads per operand), splits them three ways and passes them through a PRIVATE 12 KB patch of LDS into MFMA fragments -- no
//     __syncthreads in the loop, so the four waves of a workgroup (one per SIMD) and the two or three workgroups of a CU drift apart and cover
//     each other's load / split / multiply phases;
//   * LDS is only the transposition buffer: a slice's twelve fragments are read into registers at once, the next slice is split into the same
//     patch while the MFMAs of this one run (same-wave LDS operations execute in order); loads run two slices ahead in two register sets
//     (three sets, loads three slices ahead, were measured: 12.6 us against 10.7 for 256 x 1024 x 1024 -- 216 VGPRs, a ninth slice of zeros per
//     quarter of eight -- and ctrlsac 850 against 873 train()/s: docs/history/r06.md);
//   * two accumulators (k-block 0 / k-block 1 of every slice) halve the dependent-MFMA chain;
//   * at the end the four partial tiles meet in LDS, every wave adds its 8 rows of them IN QUARTER ORDER and runs the epilogue (gl_epilogue4: the
//     forward / dX epilogues of the engine) -- deterministic, no slab, no finishing launch.
//
// A is row-major [R, K]; B is row-major [Cn, K] (forward) or k-major [K, Cn] (dX).  Needs K % 16 == 0, 16-byte-regular operands, and Cn % 8 == 0 for
// the k-major B (rl_gemm_lds_route sends everything else to the 64-wide tile as before).
#pragma once

#define X3Q_IMG (32 * X3_RSB)              /* one bf16 image of a 32-row slice: 32 rows x 64 bytes (x3r_off swizzle) */
#define X3Q_WAVE (6 * X3Q_IMG)             /* per wave: three images of A, three of B */

// 16 consecutive k of one row (lane = (row, k half)): raw loads (PHASE 0) / zero fill past the wave's K range (PHASE 1), as in x3s_load_row
template <int PHASE>
__device__ __forceinline__ void x3q_load_row(const float* __restrict__ p, int k0, int kend, int Klim, int kh, f32x4 (&e)[4]) {
    const int k = k0 + 16 * kh;
    if constexpr (PHASE == 0) {
        const float* q = p + min(k, Klim - 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = *reinterpret_cast<const f32x4*>(q + 4 * j);
    } else {
        const bool ok = k < kend;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = ok ? e[j] : zero;
    }
}
// k-major operand: two consecutive k (lane = (k pair, group of 8 columns)): e[0..1] = row k, e[2..3] = row k + 1
template <int PHASE>
__device__ __forceinline__ void x3q_load_col(const float* __restrict__ p, int ld, int k0, int kend, int Klim, int kp, f32x4 (&e)[4]) {
    const int k = k0 + 2 * kp;
    if constexpr (PHASE == 0) {
        const float* q = p + (size_t)min(k, Klim - 2) * ld;
        e[0] = *reinterpret_cast<const f32x4*>(q); e[1] = *reinterpret_cast<const f32x4*>(q + 4);
        e[2] = *reinterpret_cast<const f32x4*>(q + ld); e[3] = *reinterpret_cast<const f32x4*>(q + ld + 4);
    } else {
        const bool ok = k < kend;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = ok ? e[j] : zero;
    }
}
// split 16 consecutive k of row `row` into the three images at img (chunks 2 kh, 2 kh + 1 of the row: two 16-byte writes per image)
__device__ __forceinline__ void x3q_write_row(unsigned char* __restrict__ img, int row, int kh, const f32x4 (&e)[4]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        u32x4 hi, mid, lo;
        unsigned h, m, l;
        x3_split2(e[2 * j][0], e[2 * j][1], h, m, l); hi[0] = h; mid[0] = m; lo[0] = l;
        x3_split2(e[2 * j][2], e[2 * j][3], h, m, l); hi[1] = h; mid[1] = m; lo[1] = l;
        x3_split2(e[2 * j + 1][0], e[2 * j + 1][1], h, m, l); hi[2] = h; mid[2] = m; lo[2] = l;
        x3_split2(e[2 * j + 1][2], e[2 * j + 1][3], h, m, l); hi[3] = h; mid[3] = m; lo[3] = l;
        unsigned char* p = img + x3r_off(row, 2 * kh + j);
        *reinterpret_cast<u32x4*>(p) = hi;
        *reinterpret_cast<u32x4*>(p + X3Q_IMG) = mid;
        *reinterpret_cast<u32x4*>(p + 2 * X3Q_IMG) = lo;
    }
}
// k-major: (k, k + 1) of eight columns -> one packed pair per column, transposed into the row-major image (image row = column)
__device__ __forceinline__ void x3q_write_col(unsigned char* __restrict__ img, int kp, int cg, const f32x4 (&e)[4]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned h, m, l;
        x3_split2(e[j >> 2][j & 3], e[2 + (j >> 2)][j & 3], h, m, l);
        unsigned char* p = img + x3r_off(8 * cg + j, kp >> 2) + 4 * (kp & 3);
        *reinterpret_cast<unsigned*>(p) = h;
        *reinterpret_cast<unsigned*>(p + X3Q_IMG) = m;
        *reinterpret_cast<unsigned*>(p + 2 * X3Q_IMG) = l;
    }
}

template <int LB>
__global__ __launch_bounds__(256, 2) void gemm_x3q_kernel(GL_DIR_PARAMS, GemmBatch gb) {
    constexpr bool GRP = false; constexpr long long dm = 0;
#include "gemm_x3q_body.h"
}
// group form (group.h): member = blockIdx.y
template <int LB>
__global__ __launch_bounds__(256, 2) void gemm_x3q_kernel_grp(GL_DIR_PARAMS, GemmBatch gb, long long mstride, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    constexpr bool GRP = true; const long long dm = (long long)member * mstride;
#include "gemm_x3q_body.h"
}
