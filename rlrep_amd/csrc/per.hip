// Prioritized experience replay (Schaul et al. 2016) on the device, for sac: a sum tree beside the replay ring, a stratified sampler that
// reads it inside the captured train(), the sac critic head with per-sample weights, and the TD errors written back as priorities.
//
// Tree: float32[2P], P = the smallest power of two >= the ring's rows; node n has children 2n, 2n + 1; row i's leaf is tree[P + i]; an
// internal node is ONE fp32 add of its children; leaves of rows never written hold 0.  scal: float32[4] = {max_p, alpha, beta, eps}.
// Every operation whose order DESIGN.md 6f fixes is written with __fadd_rn / __fmul_rn / __fdiv_rn, so that the fp32 restatement of the
// tests (tests/per_reference.py) reproduces it bit for bit (hipcc contracts a * b + c otherwise).
//
// per_add / per_sample / per_update are ONE workgroup each: the levels of the tree are dependent, a workgroup barrier between two levels
// is all the ordering they need (the per-XCD L2s are not coherent inside a launch: a multi-workgroup form needs a release / acquire per
// hand-off), and the touched part of the tree is small beside the launches they follow (profiles/per_replay.txt).
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "launchers.h"

#define PER_ADD_THREADS 1024
#define PER_THREADS 256
#define PER_MIN_PRIORITY 1.17549435e-38f       // the smallest normal float32: the floor of an updated leaf (per_update_kernel)

// ------------------------------------------------------------------------------------------------
// per_add: leaves of rows [start, start + n) mod capacity = max_p (as read by this launch), ancestors recomputed level by level
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PER_ADD_THREADS) void per_add_kernel(PerAdd p) {
    const float mp = p.scal[0];
    // the range as at most two runs of consecutive leaves: [a0, b0) and, behind the wrap, [0, b1)
    const long long a0 = p.start, b0 = p.start + p.n < p.capacity ? p.start + p.n : p.capacity, b1 = p.start + p.n - b0;
    for (long long i = a0 + threadIdx.x; i < b0; i += PER_ADD_THREADS) p.tree[p.P + i] = mp;
    for (long long i = threadIdx.x; i < b1; i += PER_ADD_THREADS) p.tree[p.P + i] = mp;
    // level k: the parents of what level k - 1 wrote.  The two runs may meet in the upper levels: both then store the same sum of the
    // same two children, which the barrier below the level has made final.
    for (long long lo0 = p.P + a0, hi0 = p.P + b0 - 1, lo1 = p.P, hi1 = p.P + b1 - 1, w = p.P; w > 1; w >>= 1) {
        __syncthreads();
        lo0 >>= 1; hi0 >>= 1; lo1 >>= 1; hi1 >>= 1;
        for (long long nd = lo0 + threadIdx.x; nd <= hi0; nd += PER_ADD_THREADS) p.tree[nd] = __fadd_rn(p.tree[2 * nd], p.tree[2 * nd + 1]);
        if (b1 > 0)
            for (long long nd = lo1 + threadIdx.x; nd <= hi1; nd += PER_ADD_THREADS) p.tree[nd] = __fadd_rn(p.tree[2 * nd], p.tree[2 * nd + 1]);
    }
}

// the whole tree from its leaves (restore): every level, all nodes
__global__ __launch_bounds__(PER_ADD_THREADS) void per_rebuild_kernel(float* __restrict__ tree, long long P) {
    for (long long w = P >> 1; w >= 1; w >>= 1) {
        for (long long nd = w + threadIdx.x; nd < 2 * w; nd += PER_ADD_THREADS) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// per_sample: B stratified draws (or B given indices), their importance weights normalised by the batch maximum
// ------------------------------------------------------------------------------------------------
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

__global__ __launch_bounds__(PER_THREADS) void per_sample_kernel(PerSample p) {
    __shared__ float sh[4];
    const float beta = p.scal[2];
    float pmin = __builtin_inff();
    if (!p.given) {
        const unsigned long long off = p.offset + (p.step_dev ? (unsigned long long)(unsigned)*p.step_dev : 0ull);
        const float total = p.tree[1], seg = __fdiv_rn(total, (float)p.B);
        for (int j = threadIdx.x; j < p.B; j += PER_THREADS) {
            const long long q = j >> 2;
            uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
            philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
            const uint32_t word = (j & 3) == 0 ? c[0] : (j & 3) == 1 ? c[1] : (j & 3) == 2 ? c[2] : c[3];
            const float u = __fmul_rn(__fadd_rn((float)(word >> 8), 0.5f), 1.0f / 16777216.0f);
            float m = __fmul_rn(__fadd_rn((float)j, u), seg);
            // one 8-byte load per level (both children), log2 P <= 20 dependent loads for a ring of 10^6 rows; the chosen child's value at the
            // last level is the leaf itself.  Never into a zero-mass subtree: left needs m < l (so l > 0) or r == 0 (so l = the parent's mass).
            long long n = 1; float val = total;
            while (n < p.P) {
                const float2 lr = *reinterpret_cast<const float2*>(p.tree + 2 * n);
                if (lr.y == 0.f || m < lr.x) { n = 2 * n; val = lr.x; }
                else { m = __fsub_rn(m, lr.x); n = 2 * n + 1; val = lr.y; }
            }
            p.idx[j] = (int)(n - p.P);
            p.w[j] = val;                      // (the leaf, until the batch minimum is known)
            pmin = fminf(pmin, val);
        }
    } else {
        for (int j = threadIdx.x; j < p.B; j += PER_THREADS) {
            const long long ix = p.idx[j];
            const float val = (ix >= 0 && ix < p.P) ? p.tree[p.P + ix] : 0.f;       // (the caller checks given indices; never read outside the tree)
            p.w[j] = val;
            pmin = fminf(pmin, val);
        }
    }
    pmin = per_block_min(pmin, sh);
    for (int j = threadIdx.x; j < p.B; j += PER_THREADS) {       // (each thread reads back what it wrote itself)
        const float pj = p.w[j];
        p.w[j] = (pj == pmin || beta == 0.f) ? 1.0f : powf(__fdiv_rn(pmin, pj), beta);
    }
}

// ------------------------------------------------------------------------------------------------
// per_update: leaves at idx[j] <- max over the duplicates of (td_j + eps)^alpha, max_p follows, ancestors level by level
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PER_THREADS) void per_update_kernel(PerUpdate p) {
    __shared__ float sh[4];
    const float alpha = p.scal[1], eps = p.scal[3];
    unsigned* leaves = reinterpret_cast<unsigned*>(p.tree + p.P);
    // (an index outside the tree is skipped in every phase: the callers check theirs, nothing is ever written outside the tree)
    auto inside = [&](int j) { const long long ix = p.idx[j]; return ix >= 0 && ix < p.P; };
    for (int j = threadIdx.x; j < p.B; j += PER_THREADS) if (inside(j)) leaves[p.idx[j]] = 0u;
    __syncthreads();
    // stratified sampling hits a heavy leaf many times: the maximum of the duplicates, whatever order they arrive in (the bit patterns of
    // non-negative floats order as the floats do)
    float mx = 0.f;
    for (int j = threadIdx.x; j < p.B; j += PER_THREADS) {
        if (!inside(j)) continue;
        float nw = alpha == 0.f ? 1.0f : powf(__fadd_rn(p.td[j], eps), alpha);
        // a priority that is not positive (td = 0 with eps = 0) or not a number (a NaN td) becomes PER_MIN_PRIORITY: a touched row keeps a
        // positive leaf, so it stays in the tree and a later update can raise it again
        nw = nw > PER_MIN_PRIORITY ? nw : PER_MIN_PRIORITY;
        atomicMax(leaves + p.idx[j], __float_as_uint(nw));
        mx = fmaxf(mx, nw);
    }
    mx = per_block_max(mx, sh);          // (its barrier is also the one between the maxima and the first level)
    if (threadIdx.x == 0) p.scal[0] = fmaxf(p.scal[0], mx);
    // the leaves were written by atomics, which live in the L2: the first level reads them past this CU's L1
    for (int j = threadIdx.x; j < p.B; j += PER_THREADS) {
        const long long nd = (p.P + p.idx[j]) >> 1;
        if (nd >= 1 && inside(j)) {
            const float l = __hip_atomic_load(p.tree + 2 * nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float r = __hip_atomic_load(p.tree + 2 * nd + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            p.tree[nd] = __fadd_rn(l, r);
        }
    }
    for (long long w = p.P >> 1, k = 2; w > 1; w >>= 1, ++k) {
        __syncthreads();
        for (int j = threadIdx.x; j < p.B; j += PER_THREADS) {
            const long long nd = (p.P + p.idx[j]) >> k;
            if (inside(j)) p.tree[nd] = __fadd_rn(p.tree[2 * nd], p.tree[2 * nd + 1]);      // (duplicates store identical values)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// the sac critic head with per-sample weights: qhead_critic_kernel (elementwise.hip, qhead_critic_body.h) restated -- included under a
// switch, the body would have to change in the kernels every unweighted train() runs.  With d_h = q_h - y:
//   g_h = (2 d_h inv_batch) w   (in this order: w = 1 is the identity),  loss partials w d_h^2,  td = 0.5 (|d_1| + |d_2|)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qhead_critic_w_kernel(QHeadCriticW pw) {
    const QHeadCritic& p = pw.q;
    __shared__ float shp[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float alpha = (float)exp(p.alpha_state[0]);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = blockIdx.x * 4 + w; b < p.B; b += gridDim.x * 4) {
        const size_t ro = (size_t)b * (p.ldE ? p.ldE : p.H);
        const float bt0 = p.bt[0][0], bt1 = p.bt[1][0], bc0 = p.bc[0][0], bc1 = p.bc[1][0], lpb = p.logp[b], Rb = p.R[b], Db = p.D[b], wb = pw.w[b];
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
        if (lane == 0) pw.td[b] = __fmul_rn(0.5f, __fadd_rn(fabsf(d1), fabsf(d2)));
        // (the unweighted kernel's acc += d * d is one fused multiply-add: with w = 1 this is the same operation on the same operands)
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
extern "C" int rl_launch_per_add(const PerAdd* p, hipStream_t st) {
    hipLaunchKernelGGL(per_add_kernel, dim3(1), dim3(PER_ADD_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_per_rebuild(float* tree, long long P, hipStream_t st) {
    hipLaunchKernelGGL(per_rebuild_kernel, dim3(1), dim3(PER_ADD_THREADS), 0, st, tree, P);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_per_sample(const PerSample* p, hipStream_t st) {
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(PER_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_per_update(const PerUpdate* p, hipStream_t st) {
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(PER_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_qhead_critic_w(const QHeadCriticW* p, hipStream_t st) {
    if (rl_grp_active()) return rl_launch_qhead_critic_w_grp(p, st);          // (a sac seed group: per_group.hip)
    hipLaunchKernelGGL(qhead_critic_w_kernel, dim3(p->q.nblk), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
