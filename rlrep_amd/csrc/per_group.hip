// Prioritized replay for SEED GROUPS: the group forms of per.hip's kernels.  Every member has a sum tree, a scalar
// block and draw buffers of its own, owned by the buffer group:
//   trees float32[R, 2P]   (member stride 2P floats)        scal float32[R, 4] = {max_p, alpha, beta, eps} per member
//   idx   int32[R, B], w float32[R, B]  (the draw buffers)  td: sac, the member's |TD| buffer in its workspace (member stride of the group);
//                                                               ctrlsac, the buffer group's float32[R, B]
// One launch per step of prioritized replay covers all members: grid (x, R), y a slot of the live table.  A kernel here says where member
// m's tree, scalars, draw buffers, seed, counter and td lie, then runs the body a single agent's kernel runs (per_tree.h,
// qhead_critic_w_body.h; group.h: the group forms are separate kernels around the same device bodies), so member m is bit for bit what a
// standalone agent with a prioritized buffer of its own computes.  No member reads another member's words.
#include "per_tree.h"
#include "launchers.h"

// No live table: the ring writers (ReplayBufferGroup.flush / add_device) write the rings of ALL members, retired ones included, and the tree
// follows the ring.
__global__ __launch_bounds__(PER_ADD_THREADS) void per_add_grp_kernel(PerAdd p) {
    const long long m = blockIdx.y;
    float* tree = p.tree + m * 2 * p.P;
    const float mp = p.scal[4 * m];
#include "per_add_body.h"
}

// p / pf: member 0's record.  The tree, the scalars and the draw buffers move by their own strides (2P, 4 and B elements), the step counter
// and the slot arrays by the group's member stride, the ring by the rings' stride; the Philox key is the member's seed.
__global__ __launch_bounds__(PER_THREADS) void per_sample_grp_kernel(PerSample p, long long mstride, const unsigned long long* __restrict__ seeds,
                                                                     const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    __shared__ float sh[4];
    const long long P = p.P;
    const int B = p.B;
    const float* tree = p.tree + (long long)m * 2 * P;
    int* idx = p.idx + (long long)m * B;
    float* w = p.w + (long long)m * B;
    const float beta = p.scal[4 * m + 2];
    const unsigned long long seed = seeds[m];
    const long long md = (long long)m * mstride;
#include "per_sample_body.h"
}

// the gather of a sac group (a group has no stand-alone fill_slot): fill_slot_kernel's copy (elementwise.hip) -- ring row idx[m][b] of member
// m's ring -> the member's slot buffers -- on grid (blocks, R).  A launch of its own behind per_sample_grp: folded into the sampler's one
// workgroup per member it took 30 us at B = 256, S = 17 (docs/history/per_group.md).
__global__ __launch_bounds__(256) void per_gather_grp_kernel(SlotFill f0, const int* __restrict__ idx0, long long ring_rows, long long mstride, long long rstride,
                                                             const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    SlotFill f = f0;
    rl_rebase(f, (long long)m * mstride, (long long)m * rstride);
    const int* __restrict__ idx = idx0 + (long long)m * f.B;
    const int SA = f.S + f.A, row_w = 2 * f.S + f.A + 2;
    const int total_e = f.B * row_w;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < total_e; e += gridDim.x * 256) {
        const int b = e / row_w, c = e - b * row_w;
        const long long src = idx[b];
        slot_put<false>(f, 0, SA, b, c, (src >= 0 && src < ring_rows) ? f.ring[(size_t)src * row_w + c] : 0.f);      // (an index outside the ring reads nothing)
    }
}

// td_stride < 0: the members' |TD| buffers in their workspaces (member stride of the group); otherwise a caller's [R, td_stride] floats
__global__ __launch_bounds__(PER_THREADS) void per_update_grp_kernel(PerUpdate p, long long mstride, long long td_stride, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    __shared__ float sh[4];
    const long long P = p.P;
    const int B = p.B;
    float* tree = p.tree + (long long)m * 2 * P;
    float* scal = p.scal + 4 * m;
    const int* idx = p.idx + (long long)m * B;
    const float* td = td_stride < 0 ? rl_mv<true>(p.td, (long long)m * mstride) : p.td + (long long)m * td_stride;
#include "per_update_body.h"
}

// per_sample_fill_kernel (per.hip) for a ctrlsac group, grid (1 + G, grid_y): x is the role inside the member.  Workgroup x = 0 is the
// member's sampler (idx[m] and w[m]); workgroups 1 .. G copy whole ring rows into the member's slot 0.
__global__ __launch_bounds__(PER_THREADS) void per_sample_fill_grp_kernel(PerSampleFill pf, long long mstride, long long rstride,
                                                                          const unsigned long long* __restrict__ seeds, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    const PerSample& p = pf.s;
    __shared__ float sh[4];
    __shared__ int rows[PER_FILL_ROWS];
    const long long P = p.P, md = (long long)m * mstride;
    const int B = p.B;
    const float* tree = p.tree + (long long)m * 2 * P;
    int* idx = p.idx + (long long)m * B;
    const unsigned long long seed = seeds[m];
    const unsigned long long off = per_stream(p.offset, p.step_dev, md);
    const float total = tree[1], seg = __fdiv_rn(total, (float)B);
    if (blockIdx.x == 0) {
        float* w = p.w + (long long)m * B;
        const float beta = p.scal[4 * m + 2];
#define PER_SAMPLE_HAS_STREAM
#include "per_sample_body.h"
#undef PER_SAMPLE_HAS_STREAM
        return;
    }
    constexpr bool GRP = true;
#include "per_gather_body.h"
}

// the weighted sac critic head of a group, as qhead_critic_kernel_grp (elementwise.hip) stands to qhead_critic_kernel.  w: [R, B] (the buffer
// group's draw buffer); td: the member's workspace for sac, the buffer group's [R, B] array for ctrlsac (qhead_critic_wtd: its builder
// reserves no such array in the workspace).  Two kernels, not a stride argument: no branch on the critic chain.
__global__ __launch_bounds__(256) void qhead_critic_w_kernel_grp(QHeadCriticW pw0, long long mstride, const MemberHyper* __restrict__ hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    QHeadCritic p = pw0.q;
    rl_rebase(p, (long long)member * mstride);
    p.gamma = rl_mv<true>(hyp, (long long)member * mstride)->gamma;
    const float* __restrict__ pw_w = pw0.w + (long long)member * p.B;
    float* __restrict__ pw_td = rl_mv<true>(pw0.td, (long long)member * mstride);
#include "qhead_critic_w_body.h"
}
__global__ __launch_bounds__(256) void qhead_critic_wtd_kernel_grp(QHeadCriticW pw0, long long mstride, const MemberHyper* __restrict__ hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    QHeadCritic p = pw0.q;
    rl_rebase(p, (long long)member * mstride);
    p.gamma = rl_mv<true>(hyp, (long long)member * mstride)->gamma;
    const float* __restrict__ pw_w = pw0.w + (long long)member * p.B;
    float* __restrict__ pw_td = pw0.td + (long long)member * p.B;
#include "qhead_critic_w_body.h"
}

// ------------------------------------------------------------------------------------------------
// launchers: all but per_add need an active group (the entry points open a GrpScope): its member stride, ring stride, seeds, live table, grid y
// ------------------------------------------------------------------------------------------------
extern "C" int rl_launch_per_add_grp(const PerAdd* p, int members, hipStream_t st) {
    hipLaunchKernelGGL(per_add_grp_kernel, dim3(1, members), dim3(PER_ADD_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
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
// `rows` as rl_launch_per_sample_fill (per.hip) chooses it
extern "C" int rl_launch_per_sample_fill_grp(PerSampleFill* p, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    p->rows = per_fill_rows(p->f);
    hipLaunchKernelGGL(per_sample_fill_grp_kernel, dim3(1 + (p->s.B + p->rows - 1) / p->rows, gr->grid_y), dim3(PER_THREADS), 0, st, *p, gr->stride, gr->ring_stride,
                       gr->seeds, gr->live);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_qhead_critic_wtd_grp(const QHeadCriticW* p, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(qhead_critic_wtd_kernel_grp, dim3(p->q.nblk, gr->grid_y), dim3(256), 0, st, *p, gr->stride, gr->hyp, gr->live);
    return (int)hipGetLastError();
}
