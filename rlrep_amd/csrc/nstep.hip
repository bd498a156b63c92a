// N-step returns on the device, for sac: the replay gather that follows each sampled row's trajectory forward through the ring and leaves
// the n-step batch in the minibatch slot, laid out as fill_slot_kernel (elementwise.hip) leaves the one-step batch.  DESIGN.md 6h.
//
// For a sampled base row i0 of a ring of `capacity` rows [s | a | s' | r | d], fill level size, successor distance `stride`:
//   g = 1, R = r[i0], last = i0;  for k = 1 .. n - 1:  j = (last + stride) mod capacity; the chain continues iff d[last] == 0, j < size and
//   the S words of s[j] equal the S words of s'[last] BIT FOR BIT (ring rows carry no truncation flag: "row j is the step after row last"
//   is a property of the rows themselves);  then g = g * gamma, R = R + g * r[j], last = j.
//   Output row: s, a of i0; s' = s'[last]; reward R; done D' = 1 - g (1 - d[last]), so that the unchanged critic heads' y = R + (1 - D') gamma tv
//   is R + gamma^m (1 - d) tv.
// Every operation is one correctly rounded fp32 operation, so that the NumPy restatement of the tests (tests/nstep_reference.py) reproduces
// the kernel bit for bit: nstep_mul / nstep_add / nstep_sub below.  hipcc contracts a * b + c, and __fmul_rn / __fadd_rn do not stop it --
// in this ROCm they are the plain operators, so R + g * r written with them became one fused multiply-add (1 .. 3 ulps off the restatement,
// docs/history/nstep.md); the three helpers switch contraction off for their own operation.
//
// One wave per sample, four per workgroup.  The chain is a dependent walk (at most n - 1 hops); per hop the lanes stride over the S words of
// the compare (S may exceed 64), r[j] and d[j] are loaded WITH the compare words, not behind the vote, a wave-wide ballot decides, and the
// accumulation is lane-uniform.  No LDS, no scratch, no atomics.  Every ring address is formed from a row index in [0, capacity).
#include "common.h"
#include "kparams.h"
#include "launchers.h"

#define NSTEP_THREADS 256

__device__ __forceinline__ float nstep_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float nstep_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float nstep_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// the waves of this workgroup (blocks x of the grid cooperate on the B samples): f's pointers are the agent's own, or a member's already rebased
__device__ __forceinline__ void nstep_gather_body(const NStepGather& p, const SlotFill& f, const long long size, const float gamma) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int S = f.S, A = f.A, SA = S + A, row_w = 2 * S + A + 2;
    const long long cap = p.capacity;
    const unsigned* __restrict__ ringw = reinterpret_cast<const unsigned*>(f.ring);
    for (int b = blockIdx.x * 4 + wv; b < f.B; b += gridDim.x * 4) {
        const long long i0 = f.idx[b];
        const bool inside = i0 >= 0 && i0 < cap;                // (an index outside the ring reads nothing: the row becomes zeros)
        long long last = inside ? i0 : 0;
        float R = inside ? f.ring[(size_t)last * row_w + SA + S] : 0.f;
        float dl = inside ? f.ring[(size_t)last * row_w + SA + S + 1] : 1.f;
        float g = 1.f;
        for (int k = 1; k < p.n; ++k) {
            if (!(dl == 0.f)) break;
            unsigned ju = (unsigned)last + (unsigned)p.stride;           // (last < cap < 2^31 and stride < 2^31: no wrap of the 32-bit sum)
            if (ju >= (unsigned)cap) ju %= (unsigned)cap;
            const long long j = ju;
            if (j >= size) break;
            const unsigned* __restrict__ sj = ringw + (size_t)j * row_w;                 // s[j]
            const unsigned* __restrict__ s2l = ringw + (size_t)last * row_w + SA;        // s'[last]
            const float rj = f.ring[(size_t)j * row_w + SA + S], dj = f.ring[(size_t)j * row_w + SA + S + 1];
            unsigned diff = 0u;
            for (int c = lane; c < S; c += 64) diff |= sj[c] ^ s2l[c];
            if (__ballot(diff != 0u) != 0ull) break;
            g = nstep_mul(g, gamma);
            R = nstep_add(R, nstep_mul(g, rj));
            dl = dj;
            last = j;
        }
        const float D = inside ? nstep_sub(1.f, nstep_mul(g, nstep_sub(1.f, dl))) : 0.f;
        // the row, as fill_slot_body lays it out: [s, a] of i0, s' of the chain's last row
        const float* __restrict__ r0 = f.ring + (size_t)(inside ? i0 : 0) * row_w;
        const float* __restrict__ rl = f.ring + (size_t)last * row_w;
        for (int c = lane; c < SA + S; c += 64) {
            const float v = !inside ? 0.f : c < SA ? r0[c] : rl[c];
            f.XE[(size_t)b * (SA + S) + c] = v;
            if (c < S) {
                f.XF[(size_t)b * SA + c] = v;
                f.XFpi[(size_t)b * SA + c] = v;
            } else if (c < SA) {
                f.XF[(size_t)b * SA + c] = v;
            } else {
                f.XF2[(size_t)b * SA + (c - SA)] = v;
            }
        }
        if (lane == 0) { f.R[b] = R; f.D[b] = D; }
    }
}

__global__ __launch_bounds__(NSTEP_THREADS) void nstep_gather_kernel(NStepGather p) {
    nstep_gather_body(p, p.fill, *p.size_dev, p.gamma);
}

// A sac seed group, grid (x, R): member m's ring (rstride bytes further per member), its fill level size_dev[m], its slot buffers (mstride
// bytes further per member) and ITS discount, read from the member's hyper record at every replay (rlrep_group_set_member_hyper holds at the
// next one).  idx_rows == 0: the indices lie in member 0's block -- the pool the group train prologue wrote -- and move by the member
// stride; otherwise idx is int32[R, idx_rows] (a prioritized buffer group's draw buffers).
__global__ __launch_bounds__(NSTEP_THREADS) void nstep_gather_kernel_grp(NStepGather p, int idx_rows, long long mstride, long long rstride,
                                                                         const MemberHyper* __restrict__ hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    SlotFill f = p.fill;
    const int* idx0 = f.idx;
    rl_rebase(f, (long long)m * mstride, (long long)m * rstride);
    if (idx_rows) f.idx = idx0 + (long long)m * idx_rows;
    nstep_gather_body(p, f, p.size_dev[m], rl_mv<true>(hyp, (long long)m * mstride)->gamma);
}

extern "C" int rl_launch_nstep_gather(const NStepGather* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;          // (a seed group takes rl_launch_nstep_gather_grp)
    int grid = (p->fill.B + 3) / 4;
    grid = grid < 1 ? 1 : grid > 2048 ? 2048 : grid;
    hipLaunchKernelGGL(nstep_gather_kernel, dim3(grid), dim3(NSTEP_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
// needs an active group (the entry point opens a GrpScope): its member stride, ring stride, hyper records, live table and grid y
extern "C" int rl_launch_nstep_gather_grp(const NStepGather* p, int idx_rows, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    int grid = (p->fill.B + 3) / 4;
    grid = grid < 1 ? 1 : grid > 2048 ? 2048 : grid;
    hipLaunchKernelGGL(nstep_gather_kernel_grp, dim3(grid, gr->grid_y), dim3(NSTEP_THREADS), 0, st, *p, idx_rows, gr->stride, gr->ring_stride, gr->hyp, gr->live);
    return (int)hipGetLastError();
}
