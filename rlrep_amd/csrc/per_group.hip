// Prioritized replay for sac SEED GROUPS: the group forms of per.hip's kernels.  Every member has a sum tree and a scalar
// block of its own, owned by the buffer group:
//   trees float32[R, 2P]   (member stride 2P floats)        scal float32[R, 4] = {max_p, alpha, beta, eps} per member
//   idx   int32[R, B], w float32[R, B]  (the draw buffers)  td = the member's |TD| buffer in its workspace (member stride of the group)
// One launch per step of prioritized replay covers all members: grid (x, R), one workgroup per member for the three tree kernels.  The
// arithmetic of member m is per.hip's on the member's slices -- the bodies are RESTATED here, per.hip's kernels are untouched (group.h: the
// group forms are separate kernels; docs/history/per_group.md says why they are not shared through *_body.h) -- so member m is bit for bit
// what a standalone agent with a PrioritizedReplayBuffer of its own computes.  No member reads another member's words.
//
// per_gather_grp copies the rows per_sample_grp drew into the members' minibatch slot 0 (a group has no stand-alone gather): a launch of its
// own on grid (blocks, R), as the single agent's sample is followed by fill_slot_kernel.
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "group.h"
#include "launchers.h"

#define PER_ADD_THREADS 1024
#define PER_THREADS 256
#define PER_MIN_PRIORITY 1.17549435e-38f       // the smallest normal float32: the floor of an updated leaf (per.hip)

// ------------------------------------------------------------------------------------------------
// per_add_grp: every member's leaves of rows [start, start + n) mod capacity = that member's max_p, ancestors recomputed.  No live table:
// the ring writers (ReplayBufferGroup.flush / add_device) write the rings of ALL members, retired ones included, and the tree follows the ring.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PER_ADD_THREADS) void per_add_grp_kernel(PerAdd p) {
    const long long m = blockIdx.y;
    float* __restrict__ tree = p.tree + m * 2 * p.P;
    const float mp = p.scal[4 * m];
    const long long a0 = p.start, b0 = p.start + p.n < p.capacity ? p.start + p.n : p.capacity, b1 = p.start + p.n - b0;
    for (long long i = a0 + threadIdx.x; i < b0; i += PER_ADD_THREADS) tree[p.P + i] = mp;
    for (long long i = threadIdx.x; i < b1; i += PER_ADD_THREADS) tree[p.P + i] = mp;
    for (long long lo0 = p.P + a0, hi0 = p.P + b0 - 1, lo1 = p.P, hi1 = p.P + b1 - 1, w = p.P; w > 1; w >>= 1) {
        __syncthreads();
        lo0 >>= 1; hi0 >>= 1; lo1 >>= 1; hi1 >>= 1;
        for (long long nd = lo0 + threadIdx.x; nd <= hi0; nd += PER_ADD_THREADS) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);
        if (b1 > 0)
            for (long long nd = lo1 + threadIdx.x; nd <= hi1; nd += PER_ADD_THREADS) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);
    }
}

// ------------------------------------------------------------------------------------------------
// per_sample_grp: member m's B stratified draws (or its B given indices) and their importance weights; per_gather_grp: the drawn rows
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float per_grp_block_min(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}
__device__ __forceinline__ float per_grp_block_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// p0: member 0's record.  The tree, the scalars and the draw buffers move by their own strides (2P, 4 and B elements), the step counter by
// the group's member stride; the Philox key is the member's seed.
__global__ __launch_bounds__(PER_THREADS) void per_sample_grp_kernel(PerSample p0, long long mstride, const unsigned long long* __restrict__ seeds,
                                                                     const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    __shared__ float sh[4];
    const long long P = p0.P;
    const int B = p0.B;
    const float* __restrict__ tree = p0.tree + (long long)m * 2 * P;
    int* idx = p0.idx + (long long)m * B;
    float* w = p0.w + (long long)m * B;
    const float beta = p0.scal[4 * m + 2];
    float pmin = __builtin_inff();
    if (!p0.given) {
        const int* step_dev = p0.step_dev;
        rl_rb(step_dev, (long long)m * mstride);
        const unsigned long long seed = seeds[m];
        const unsigned long long off = p0.offset + (step_dev ? (unsigned long long)(unsigned)*step_dev : 0ull);
        const float total = tree[1], seg = __fdiv_rn(total, (float)B);
        for (int j = threadIdx.x; j < B; j += PER_THREADS) {
            const long long q = j >> 2;
            uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
            philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
            const uint32_t word = (j & 3) == 0 ? c[0] : (j & 3) == 1 ? c[1] : (j & 3) == 2 ? c[2] : c[3];
            const float u = __fmul_rn(__fadd_rn((float)(word >> 8), 0.5f), 1.0f / 16777216.0f);
            float mm = __fmul_rn(__fadd_rn((float)j, u), seg);
            long long n = 1; float val = total;
            while (n < P) {
                const float2 lr = *reinterpret_cast<const float2*>(tree + 2 * n);
                if (lr.y == 0.f || mm < lr.x) { n = 2 * n; val = lr.x; }
                else { mm = __fsub_rn(mm, lr.x); n = 2 * n + 1; val = lr.y; }
            }
            idx[j] = (int)(n - P);
            w[j] = val;                        // (the leaf, until the batch minimum is known)
            pmin = fminf(pmin, val);
        }
    } else {
        for (int j = threadIdx.x; j < B; j += PER_THREADS) {
            const long long ix = idx[j];
            const float val = (ix >= 0 && ix < P) ? tree[P + ix] : 0.f;       // (the caller checks given indices; never read outside the tree)
            w[j] = val;
            pmin = fminf(pmin, val);
        }
    }
    pmin = per_grp_block_min(pmin, sh);
    for (int j = threadIdx.x; j < B; j += PER_THREADS) {       // (each thread reads back what it wrote itself)
        const float pj = w[j];
        w[j] = (pj == pmin || beta == 0.f) ? 1.0f : powf(__fdiv_rn(pmin, pj), beta);
    }
}

// the gather of a group (a group has no stand-alone fill_slot): fill_slot_kernel's copy (elementwise.hip) -- ring row idx[m][b] of member m's
// ring -> the member's slot buffers -- on grid (blocks, R).  A launch of its own behind per_sample_grp: folded into the sampler's one
// workgroup per member it took 30 us at B = 256, S = 17 (docs/history/per_group.md).
__global__ __launch_bounds__(256) void per_gather_grp_kernel(SlotFill f0, const int* __restrict__ idx0, long long ring_rows, long long mstride, long long rstride,
                                                             const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    SlotFill f = f0;
    rl_rebase(f, (long long)m * mstride, (long long)m * rstride);
    const int* __restrict__ idx = idx0 + (long long)m * f.B;
    const int S = f.S, A = f.A, SA = S + A, row_w = 2 * S + A + 2;
    const int total_e = f.B * row_w;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total_e; e += gridDim.x * 256) {
        const int b = e / row_w, c = e - b * row_w;
        const long long src = idx[b];
        const float v = (src >= 0 && src < ring_rows) ? f.ring[(size_t)src * row_w + c] : 0.f;      // (an index outside the ring reads nothing)
        if (c < S) {
            f.XE[(size_t)b * (SA + S) + c] = v;
            f.XF[(size_t)b * SA + c] = v;
            f.XFpi[(size_t)b * SA + c] = v;
        } else if (c < SA) {
            f.XE[(size_t)b * (SA + S) + c] = v;
            f.XF[(size_t)b * SA + c] = v;
        } else if (c < SA + S) {
            f.XE[(size_t)b * (SA + S) + c] = v;
            f.XF2[(size_t)b * SA + (c - SA)] = v;
        } else if (c == SA + S) {
            f.R[b] = v;
        } else {
            f.D[b] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// per_update_grp: member m's leaves at idx[j] <- max over the duplicates of (td_j + eps)^alpha, its max_p follows, ancestors level by level
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PER_THREADS) void per_update_grp_kernel(PerUpdate p0, long long mstride, long long td_stride, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    __shared__ float sh[4];
    const long long P = p0.P;
    const int B = p0.B;
    float* tree = p0.tree + (long long)m * 2 * P;
    float* scal = p0.scal + 4 * m;
    const int* __restrict__ idx = p0.idx + (long long)m * B;
    // td_stride < 0: the members' |TD| buffers in their workspaces (member stride of the group); otherwise a caller's [R, td_stride] floats
    const float* __restrict__ td = td_stride < 0 ? rl_mv<true>(p0.td, (long long)m * mstride) : p0.td + (long long)m * td_stride;
    const float alpha = scal[1], eps = scal[3];
    unsigned* leaves = reinterpret_cast<unsigned*>(tree + P);
    auto inside = [&](int j) { const long long ix = idx[j]; return ix >= 0 && ix < P; };
    for (int j = threadIdx.x; j < B; j += PER_THREADS) if (inside(j)) leaves[idx[j]] = 0u;
    __syncthreads();
    float mx = 0.f;
    for (int j = threadIdx.x; j < B; j += PER_THREADS) {
        if (!inside(j)) continue;
        float nw = alpha == 0.f ? 1.0f : powf(__fadd_rn(td[j], eps), alpha);
        nw = nw > PER_MIN_PRIORITY ? nw : PER_MIN_PRIORITY;
        atomicMax(leaves + idx[j], __float_as_uint(nw));
        mx = fmaxf(mx, nw);
    }
    mx = per_grp_block_max(mx, sh);          // (its barrier is also the one between the maxima and the first level)
    if (threadIdx.x == 0) scal[0] = fmaxf(scal[0], mx);
    // the leaves were written by atomics, which live in the L2: the first level reads them past this CU's L1
    for (int j = threadIdx.x; j < B; j += PER_THREADS) {
        const long long nd = (P + idx[j]) >> 1;
        if (nd >= 1 && inside(j)) {
            const float l = __hip_atomic_load(tree + 2 * nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float r = __hip_atomic_load(tree + 2 * nd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tree[nd] = __fadd_rn(l, r);
        }
    }
    for (long long wd = P >> 1, k = 2; wd > 1; wd >>= 1, ++k) {
        __syncthreads();
        for (int j = threadIdx.x; j < B; j += PER_THREADS) {
            const long long nd = (P + idx[j]) >> k;
            if (inside(j)) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);      // (duplicates store identical values)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the weighted sac critic head of a group: qhead_critic_w_kernel (per.hip) restated behind the member's rebase, as qhead_critic_kernel_grp
// (elementwise.hip) stands to qhead_critic_kernel.  w: [R, B] (the buffer group's draw buffer), td: the member's workspace.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qhead_critic_w_kernel_grp(QHeadCriticW pw0, long long mstride, const MemberHyper* __restrict__ hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    QHeadCritic p = pw0.q;
    rl_rebase(p, (long long)member * mstride);
    p.gamma = rl_mv<true>(hyp, (long long)member * mstride)->gamma;
    const float* __restrict__ pw_w = pw0.w + (long long)member * p.B;
    float* __restrict__ pw_td = rl_mv<true>(pw0.td, (long long)member * mstride);
    __shared__ float shp[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float alpha = (float)exp(p.alpha_state[0]);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = blockIdx.x * 4 + w; b < p.B; b += gridDim.x * 4) {
        const size_t ro = (size_t)b * (p.ldE ? p.ldE : p.H);
        const float bt0 = p.bt[0][0], bt1 = p.bt[1][0], bc0 = p.bc[0][0], bc1 = p.bc[1][0], lpb = p.logp[b], Rb = p.R[b], Db = p.D[b], wb = pw_w[b];
        __builtin_amdgcn_sched_barrier(0);
        float dd0 = 0.f, dd1 = 0.f, dd2 = 0.f, dd3 = 0.f;
#pragma unroll 4
        for (int k = lane; k < p.H; k += 64) {
            const float e0 = p.Et[0][ro + k], e1 = p.Et[1][ro + k], e2 = p.Ec[0][ro + k], e3 = p.Ec[1][ro + k];
            const float w0 = p.wt[0][k], w1 = p.wt[1][k], w2 = p.wc[0][k], w3 = p.wc[1][k];
            dd0 = fmaf(e0, w0, dd0); dd1 = fmaf(e1, w1, dd1); dd2 = fmaf(e2, w2, dd2); dd3 = fmaf(e3, w3, dd3);
        }
        const float tq1 = wave_sum(dd0) + bt0;
        const float tq2 = wave_sum(dd1) + bt1;
        const float q1 = wave_sum(dd2) + bc0;
        const float q2 = wave_sum(dd3) + bc1;
        const float tv = fminf(tq1, tq2) - alpha * lpb;
        const float y = Rb + (1.f - Db) * p.gamma * tv;
        const float d1 = q1 - y, d2 = q2 - y;
        const float g1 = __fmul_rn(2.f * d1 * p.inv_batch, wb), g2 = __fmul_rn(2.f * d2 * p.inv_batch, wb);
        if (p.train) {
            for (int k = lane; k < p.H; k += 64) {
                p.GE[0][ro + k] = g1 * p.wc[0][k] * elu_grad_from_out(p.Ec[0][ro + k]);
                p.GE[1][ro + k] = g2 * p.wc[1][k] * elu_grad_from_out(p.Ec[1][ro + k]);
            }
            if (lane == 0) { p.dq[b] = g1; p.dq[p.B + b] = g2; }
        }
        if (lane == 0) pw_td[b] = __fmul_rn(0.5f, __fadd_rn(fabsf(d1), fabsf(d2)));
        acc[0] = fmaf(__fmul_rn(wb, d1), d1, acc[0]); acc[1] = fmaf(__fmul_rn(wb, d2), d2, acc[1]); acc[2] += q1; acc[3] += q2;
    }
    if (lane == 0) { for (int i = 0; i < 4; ++i) shp[w][i] = acc[i]; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int i = threadIdx.x;
        p.partial[4 * blockIdx.x + i] = ((shp[0][i] + shp[1][i]) + shp[2][i]) + shp[3][i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.step) bump_group(p.step);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
extern "C" int rl_launch_per_add_grp(const PerAdd* p, int members, hipStream_t st) {
    hipLaunchKernelGGL(per_add_grp_kernel, dim3(1, members), dim3(PER_ADD_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
// both need an active group (the entry points open a GrpScope): its member stride, seeds, live table and grid y
extern "C" int rl_launch_per_sample_grp(const PerSample* p, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(per_sample_grp_kernel, dim3(1, gr->grid_y), dim3(PER_THREADS), 0, st, *p, gr->stride, gr->seeds, gr->live);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_per_gather_grp(const SlotFill* fill, const int* idx, long long ring_rows, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    const long long total = (long long)fill->B * (2 * fill->S + fill->A + 2);
    if (total >= (1ll << 31)) return -5;
    long long g = (total + 255) / 256;
    g = g < 1 ? 1 : g > 2048 ? 2048 : g;            // (the grid of rl_launch_fill_slot)
    hipLaunchKernelGGL(per_gather_grp_kernel, dim3((unsigned)g, gr->grid_y), dim3(256), 0, st, *fill, idx, ring_rows, gr->stride, gr->ring_stride, gr->live);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_per_update_grp(const PerUpdate* p, long long td_stride, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(per_update_grp_kernel, dim3(1, gr->grid_y), dim3(PER_THREADS), 0, st, *p, gr->stride, td_stride, gr->live);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_qhead_critic_w_grp(const QHeadCriticW* p, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(qhead_critic_w_kernel_grp, dim3(p->q.nblk, gr->grid_y), dim3(256), 0, st, *p, gr->stride, gr->hyp, gr->live);
    return (int)hipGetLastError();
}
