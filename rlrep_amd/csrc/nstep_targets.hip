// N-step CRITIC targets for the representation agents (vlsac, ctrlsac, spedersac, diffsrsac): the replay gather that follows each sampled
// row's trajectory forward through the ring, as nstep.hip does for sac, and overwrites ONLY what the critic and actor steps read of the
// chain.  Their feature step models one-step dynamics from the same minibatch the critic reuses, so the plain gather's rows stay where it
// reads them (XE, XF, R) and the critic heads read a reward array of their own (Slot::Rn).  DESIGN.md 6h.
//
// The walk is nstep.hip's, restated here so that that unit's code object stays what it was: for base row i0 of a ring of `capacity` rows
// [s | a | s' | r | d], fill level size, successor distance `stride`:
//   g = 1, R = r[i0], last = i0;  for k = 1 .. n - 1:  j = (last + stride) mod capacity; the chain continues iff d[last] == 0, j < size and
//   the S words of s[j] equal the S words of s'[last] bit for bit;  then g = g * gamma, R = R + g * r[j], last = j.
// Written:  XF2[b, 0:S] = s'[last]  (leading dimension S + A; columns [S, S + A) are the policy's action on s', not touched),
//           Rn[b] = R,  D[b] = 1 - g (1 - d[last]).   Left alone: XE, XF, XFpi, R.
// Every operation is one correctly rounded fp32 operation (contraction off in the three helpers: __fmul_rn / __fadd_rn are the plain
// operators in this ROCm and were fused, docs/history/nstep.md), so tests/nstep_targets_reference.py reproduces the kernel bit for bit.
//
// One wave per sample, four per workgroup; per hop the lanes stride over the S compare words, r[j] and d[j] are loaded beside them, a
// wave-wide ballot decides and the accumulation is lane-uniform.  No LDS, no scratch, no atomics.  Every ring address is formed from a row
// index in [0, capacity); an index outside the ring reads nothing and writes zeros.
#include "common.h"
#include "kparams.h"
#include "launchers.h"

#define NSTEP_T_THREADS 256

__device__ __forceinline__ float nstept_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float nstept_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float nstept_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__global__ __launch_bounds__(NSTEP_T_THREADS) void nstep_targets_kernel(NStepTargets p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = p.S, SA = p.S + p.A, row_w = 2 * p.S + p.A + 2;
    const long long cap = p.capacity, size = *p.size_dev;
    const float gamma = p.gamma;
    const float* __restrict__ ring = p.ring;
    const unsigned* __restrict__ ringw = reinterpret_cast<const unsigned*>(p.ring);
    for (int b = blockIdx.x * 4 + wv; b < p.B; b += gridDim.x * 4) {
        const long long i0 = p.idx[b];
        const bool inside = i0 >= 0 && i0 < cap;
        long long last = inside ? i0 : 0;
        float R = inside ? ring[(size_t)last * row_w + SA + S] : 0.f;
        float dl = inside ? ring[(size_t)last * row_w + SA + S + 1] : 1.f;          // (outside: no hop is taken)
        float g = 1.f;
        for (int k = 1; k < p.n; ++k) {
            if (!(dl == 0.f)) break;
            unsigned ju = (unsigned)last + (unsigned)p.stride;           // (last < cap < 2^31 and stride < 2^31: no wrap of the 32-bit sum)
            if (ju >= (unsigned)cap) ju %= (unsigned)cap;
            const long long j = ju;
            if (j >= size) break;
            const unsigned* __restrict__ sj = ringw + (size_t)j * row_w;                 // s[j]
            const unsigned* __restrict__ s2l = ringw + (size_t)last * row_w + SA;        // s'[last]
            const float rj = ring[(size_t)j * row_w + SA + S], dj = ring[(size_t)j * row_w + SA + S + 1];
            unsigned diff = 0u;
            for (int c = lane; c < S; c += 64) diff |= sj[c] ^ s2l[c];
            if (__ballot(diff != 0u) != 0ull) break;
            g = nstept_mul(g, gamma);
            R = nstept_add(R, nstept_mul(g, rj));
            dl = dj;
            last = j;
        }
        const float D = inside ? nstept_sub(1.f, nstept_mul(g, nstept_sub(1.f, dl))) : 0.f;
        const float* __restrict__ s2 = ring + (size_t)last * row_w + SA;                 // s' of the chain's last row
        for (int c = lane; c < S; c += 64) p.XF2[(size_t)b * SA + c] = inside ? s2[c] : 0.f;
        if (lane == 0) { p.Rn[b] = R; p.D[b] = D; }
    }
}

extern "C" int rl_launch_nstep_targets(const NStepTargets* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;          // (built for one agent: a seed group has no form of it)
    int grid = (p->B + 3) / 4;
    grid = grid < 1 ? 1 : grid > 2048 ? 2048 : grid;
    hipLaunchKernelGGL(nstep_targets_kernel, dim3(grid), dim3(NSTEP_T_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
