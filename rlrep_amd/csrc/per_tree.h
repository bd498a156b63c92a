// Prioritized replay on the device, what its kernels share.  per.hip (a single agent) and per_group.hip (seed groups) are
// kernels that say where a tree, its scalars and its draw buffers lie and then run ONE body: a group member's arithmetic is a standalone
// agent's by construction, not by a restatement that only the tests hold equal.
//   here                    the sizes, the block minimum / maximum, the descent, the stream offset, the row-to-slot scatter
//   per_add_body.h          the add            per_update_body.h       the update
//   per_sample_body.h       the sampler        per_gather_body.h       a gathering workgroup of the fused sample + gather launches
//   qhead_critic_w_body.h   the weighted sac critic head
// The *_body.h files are #included into the kernels, as group.h says of the large bodies: called as forceinline functions, add, sample and
// update came out with other operand orders and compares than the kernels they replace, and with __restrict__ on the functions'
// parameters per_update grew by an eighth (clang honours it there and ignores it on a kernel's local variables).  What is a function here
// compiles to the same instructions either way (docs/history/per_kernels_one_body.md has the comparison, kernel by kernel).
//
// Tree: float32[2P], P = the smallest power of two >= the ring's rows; node n has children 2n, 2n + 1; row i's leaf is tree[P + i]; an
// internal node is ONE fp32 add of its children; leaves of rows never written hold 0.  scal: float32[4] = {max_p, alpha, beta, eps}.
// Every operation whose order DESIGN.md 6f fixes is written with __fadd_rn / __fmul_rn / __fdiv_rn, so that the fp32 restatement of the
// tests (tests/per_reference.py) reproduces it bit for bit (hipcc contracts a * b + c otherwise).
#pragma once
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "group.h"

#define PER_ADD_THREADS 1024
#define PER_THREADS 256
#define PER_MIN_PRIORITY 1.17549435e-38f       // the smallest normal float32: the floor of an updated leaf (per_update_body)
#define PER_FILL_ROWS 256       // most samples per gathering workgroup of the fused launch: one descent per thread
#define PER_FILL_ELEMS 4        // elements a thread of a gathering workgroup copies, about (per_fill_rows)

// `rows` of the fused sample + gather launches: whole rows, about PER_FILL_ELEMS elements per thread (rl_launch_per_sample_fill says why)
static inline int per_fill_rows(const SlotFill& f) {
    const int rows = PER_FILL_ELEMS * PER_THREADS / (2 * f.S + f.A + 2);
    return rows < 1 ? 1 : rows > PER_FILL_ROWS ? PER_FILL_ROWS : rows;
}

#ifdef __HIPCC__
// the minimum / maximum over a workgroup of PER_THREADS; sh: float[4] of LDS.  The barrier inside is one the callers rely on.
__device__ __forceinline__ float per_block_min(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}
__device__ __forceinline__ float per_block_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// draw j of the stratified sampler: the leaf it lands on and that leaf's value.  A function of (j, the tree, the Philox word) alone.
__device__ __forceinline__ int per_descend(const float* tree, long long P, unsigned long long seed, int j, unsigned long long off, float total, float seg,
                                           float& val) {
    const long long q = j >> 2;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t word = (j & 3) == 0 ? c[0] : (j & 3) == 1 ? c[1] : (j & 3) == 2 ? c[2] : c[3];
    const float u = __fmul_rn(__fadd_rn((float)(word >> 8), 0.5f), 1.0f / 16777216.0f);
    float m = __fmul_rn(__fadd_rn((float)j, u), seg);
    // one aligned 8-byte load per level (both children), log2 P <= 20 dependent loads for a ring of 10^6 rows; the chosen child's value at
    // the last level is the leaf itself.  Never into a zero-mass subtree: left needs m < l (so l > 0) or r == 0 (so l = the parent's mass).
    long long n = 1; val = total;
    while (n < P) {
        const float2 lr = *reinterpret_cast<const float2*>(tree + 2 * n);
        if (lr.y == 0.f || m < lr.x) { n = 2 * n; val = lr.x; }
        else { m = __fsub_rn(m, lr.x); n = 2 * n + 1; val = lr.y; }
    }
    return (int)(n - P);
}
// the stream offset of a launch: the host's, plus the device step counter where there is one (md: the member's byte offset, 0 for a
// single agent)
__device__ __forceinline__ unsigned long long per_stream(unsigned long long offset, const int* step_dev, long long md) {
    return offset + (step_dev ? (unsigned long long)(unsigned)*rl_mv<true>(step_dev, md) : 0ull);
}

// the gather: element c of a ring row -> sample b of the slot arrays, laid out as fill_slot_body (elementwise.hip) lays them out; SA = f.S + f.A,
// which the caller's loop keeps.
// GRP: the record stays in the kernel-argument segment and every pointer is moved by md bytes where it is loaded (rl_mv: no local copy, no
// scratch).  A record that is already the member's (rl_rebase) or a single agent's: GRP = false.
template <bool GRP> __device__ __forceinline__ void slot_put(const SlotFill& f, long long md, int SA, int b, int c, float v) {
    if (c < f.S) {
        rl_mv<GRP>(f.XE, md)[(size_t)b * (SA + f.S) + c] = v;
        rl_mv<GRP>(f.XF, md)[(size_t)b * SA + c] = v;
        rl_mv<GRP>(f.XFpi, md)[(size_t)b * SA + c] = v;
    } else if (c < SA) {
        rl_mv<GRP>(f.XE, md)[(size_t)b * (SA + f.S) + c] = v;
        rl_mv<GRP>(f.XF, md)[(size_t)b * SA + c] = v;
    } else if (c < SA + f.S) {
        rl_mv<GRP>(f.XE, md)[(size_t)b * (SA + f.S) + c] = v;
        rl_mv<GRP>(f.XF2, md)[(size_t)b * SA + (c - SA)] = v;
    } else if (c == SA + f.S) {
        rl_mv<GRP>(f.R, md)[b] = v;
    } else {
        rl_mv<GRP>(f.D, md)[b] = v;
    }
}

#endif
