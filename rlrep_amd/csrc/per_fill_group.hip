// Prioritized replay of the critic's minibatch for ctrlsac SEED GROUPS: the group forms of per_fill.hip's fused launch and
// of the weighted critic head whose |TD| array belongs to the buffer group.  Every member has a sum tree, a scalar block and draw buffers
// of its own, owned by the buffer group (utils/buffer_group.py CriticPrioritizedReplayBufferGroup):
//   trees float32[R, 2P]    scal float32[R, 4] = {max_p, alpha, beta, eps}    idx int32[R, B], w float32[R, B], td float32[R, B]
// group.h: the group forms are SEPARATE kernels and the bodies are RESTATED here -- per_fill.hip, per.hip, per_group.hip and elementwise.hip
// keep the code objects every other train() runs -- so member m is bit for bit what a standalone ctrlsac agent with a
// CriticPrioritizedReplayBuffer of its own computes.  No member reads another member's words.
//
// per_sample_fill_grp_kernel, grid (1 + G, grid_y): y is a slot of the live table, x the role inside the member.  Workgroup x = 0 is the
// member's sampler (all B draws, the batch minimum, idx[m] and w[m]); workgroups 1 .. G repeat the descents of THEIR `rows` samples (one per
// thread) and copy whole ring rows into the member's slot 0.  A draw is a function of (j, the tree, the Philox word) alone and the trees are
// read-only inside the launch, so there is no hand-off between workgroups (the per-XCD L2s are not coherent inside a launch).  The record stays
// in the kernel-argument segment: every pointer is moved where it is loaded (rl_mv<true>), no local copy, no scratch.
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "group.h"
#include "launchers.h"

#define PSFG_THREADS 256
#define PSFG_ROWS 256           // most samples per gathering workgroup: one descent per thread
#define PSFG_ELEMS 4            // elements a thread of a gathering workgroup copies, about (the launcher's choice of `rows`)

// draw j of the stratified sampler (psf_descend of per_fill.hip, operation for operation) on member m's tree with member m's seed
__device__ __forceinline__ int psfg_descend(const float* __restrict__ tree, long long P, unsigned long long seed, int j, unsigned long long off, float total,
                                            float seg, float& val) {
    const long long q = j >> 2;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t word = (j & 3) == 0 ? c[0] : (j & 3) == 1 ? c[1] : (j & 3) == 2 ? c[2] : c[3];
    const float u = __fmul_rn(__fadd_rn((float)(word >> 8), 0.5f), 1.0f / 16777216.0f);
    float m = __fmul_rn(__fadd_rn((float)j, u), seg);
    // one aligned 8-byte load per level (both children); never into a zero-mass subtree: left needs m < l (so l > 0) or r == 0
    long long n = 1; val = total;
    while (n < P) {
        const float2 lr = *reinterpret_cast<const float2*>(tree + 2 * n);
        if (lr.y == 0.f || m < lr.x) { n = 2 * n; val = lr.x; }
        else { m = __fsub_rn(m, lr.x); n = 2 * n + 1; val = lr.y; }
    }
    return (int)(n - P);
}

__device__ __forceinline__ float psfg_block_min(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}

// pf: member 0's record.  The tree, the scalars and the draw buffers move by their own strides (2P, 4 and B elements), the step counter and
// the six slot arrays by the group's member stride, the ring by the rings' stride; the Philox key is the member's seed.
__global__ __launch_bounds__(PSFG_THREADS) void per_sample_fill_grp_kernel(PerSampleFill pf, long long mstride, long long rstride,
                                                                           const unsigned long long* __restrict__ seeds, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    __shared__ float sh[4];
    __shared__ int rows[PSFG_ROWS];
    const long long P = pf.s.P, md = (long long)m * mstride;
    const int B = pf.s.B;
    const float* __restrict__ tree = pf.s.tree + (long long)m * 2 * P;
    int* idx = pf.s.idx + (long long)m * B;
    const unsigned long long seed = seeds[m];
    // (the device step counter, read as per_sample_fill_kernel reads it: the member's own)
    const unsigned long long off = pf.s.offset + (pf.s.step_dev ? (unsigned long long)(unsigned)*rl_mv<true>(pf.s.step_dev, md) : 0ull);
    const float total = tree[1], seg = __fdiv_rn(total, (float)B);
    if (blockIdx.x == 0) {
        // ---- the member's sampler: idx[m][B] and w[m][B] ----
        float* w = pf.s.w + (long long)m * B;
        const float beta = pf.s.scal[4 * m + 2];
        float pmin = __builtin_inff();
        if (!pf.s.given) {
            for (int j = threadIdx.x; j < B; j += PSFG_THREADS) {
                float val;
                idx[j] = psfg_descend(tree, P, seed, j, off, total, seg, val);
                w[j] = val;                        // (the leaf, until the batch minimum is known)
                pmin = fminf(pmin, val);
            }
        } else {
            for (int j = threadIdx.x; j < B; j += PSFG_THREADS) {
                const long long ix = idx[j];
                const float val = (ix >= 0 && ix < P) ? tree[P + ix] : 0.f;       // (the caller checks given indices; never read outside the tree)
                w[j] = val;
                pmin = fminf(pmin, val);
            }
        }
        pmin = psfg_block_min(pmin, sh);
        for (int j = threadIdx.x; j < B; j += PSFG_THREADS) {       // (each thread reads back what it wrote itself)
            const float pj = w[j];
            w[j] = (pj == pmin || beta == 0.f) ? 1.0f : powf(__fdiv_rn(pmin, pj), beta);
        }
        return;
    }
    // ---- a gatherer of member m: samples [lo, lo + n) ----
    const int lo = (blockIdx.x - 1) * pf.rows, n = B - lo < pf.rows ? B - lo : pf.rows;
    if ((int)threadIdx.x < n) {
        float val;
        long long ix = pf.s.given ? (long long)idx[lo + threadIdx.x] : (long long)psfg_descend(tree, P, seed, lo + threadIdx.x, off, total, seg, val);
        // a drawn leaf carries mass, so its row is one the ring holds; a given index is the caller's to check.  Whatever it is, nothing is
        // read outside the member's ring
        ix = ix < 0 ? 0 : ix >= pf.capacity ? pf.capacity - 1 : ix;
        rows[threadIdx.x] = (int)ix;
    }
    __syncthreads();
    const int S = pf.f.S, A = pf.f.A, row_w = 2 * S + A + 2, SA = S + A;
    const int count = n * row_w;                    // (about PSFG_ELEMS * 256 elements, or one row)
    const float* __restrict__ ring = rl_mv<true>(pf.f.ring, (long long)m * rstride);
    // PSFG_ELEMS loads at a time into registers, then their stores (per_fill.hip says why)
    for (int base = 0; base < count; base += PSFG_ELEMS * PSFG_THREADS) {
        float v[PSFG_ELEMS]; int kk[PSFG_ELEMS], cc[PSFG_ELEMS];
#pragma unroll
        for (int u = 0; u < PSFG_ELEMS; ++u) {
            const int e = base + u * PSFG_THREADS + threadIdx.x;
            kk[u] = e / row_w; cc[u] = e - kk[u] * row_w;
            v[u] = e < count ? ring[(size_t)rows[kk[u]] * row_w + cc[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PSFG_ELEMS; ++u) {
            if (base + u * PSFG_THREADS + (int)threadIdx.x >= count) continue;
            const int c = cc[u], b = lo + kk[u];
            if (c < S) {
                rl_mv<true>(pf.f.XE, md)[(size_t)b * (SA + S) + c] = v[u];
                rl_mv<true>(pf.f.XF, md)[(size_t)b * SA + c] = v[u];
                rl_mv<true>(pf.f.XFpi, md)[(size_t)b * SA + c] = v[u];
            } else if (c < SA) {
                rl_mv<true>(pf.f.XE, md)[(size_t)b * (SA + S) + c] = v[u];
                rl_mv<true>(pf.f.XF, md)[(size_t)b * SA + c] = v[u];
            } else if (c < SA + S) {
                rl_mv<true>(pf.f.XE, md)[(size_t)b * (SA + S) + c] = v[u];
                rl_mv<true>(pf.f.XF2, md)[(size_t)b * SA + (c - SA)] = v[u];
            } else if (c == SA + S) {
                rl_mv<true>(pf.f.R, md)[b] = v[u];
            } else {
                rl_mv<true>(pf.f.D, md)[b] = v[u];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the weighted critic head of a ctrlsac group: qhead_critic_w_kernel (per.hip) restated behind the member's rebase, as
// qhead_critic_w_kernel_grp (per_group.hip) restates it for sac -- but w AND td are the buffer group's [R, B] arrays, B elements per member
// (sac's td lies in the member's workspace and moves by the member stride; the ctrlsac builder reserves no such array)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qhead_critic_wtd_kernel_grp(QHeadCriticW pw0, long long mstride, const MemberHyper* __restrict__ hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    QHeadCritic p = pw0.q;
    rl_rebase(p, (long long)member * mstride);
    p.gamma = rl_mv<true>(hyp, (long long)member * mstride)->gamma;
    const float* __restrict__ pw_w = pw0.w + (long long)member * p.B;
    float* __restrict__ pw_td = pw0.td + (long long)member * p.B;
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
// launchers: both need an active group (the entry points open a GrpScope): its member stride, ring stride, seeds, live table and grid y
// ------------------------------------------------------------------------------------------------
// `rows` follows rl_launch_per_sample_fill (per_fill.hip): whole rows, about PSFG_ELEMS elements per thread of a gathering workgroup
extern "C" int rl_launch_per_sample_fill_grp(PerSampleFill* p, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    const int row_w = 2 * p->f.S + p->f.A + 2;
    int rows = PSFG_ELEMS * PSFG_THREADS / row_w;
    rows = rows < 1 ? 1 : rows > PSFG_ROWS ? PSFG_ROWS : rows;
    p->rows = rows;
    hipLaunchKernelGGL(per_sample_fill_grp_kernel, dim3(1 + (p->s.B + rows - 1) / rows, gr->grid_y), dim3(PSFG_THREADS), 0, st, *p, gr->stride, gr->ring_stride,
                       gr->seeds, gr->live);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_qhead_critic_wtd_grp(const QHeadCriticW* p, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(qhead_critic_wtd_kernel_grp, dim3(p->q.nblk, gr->grid_y), dim3(256), 0, st, *p, gr->stride, gr->hyp, gr->live);
    return (int)hipGetLastError();
}
