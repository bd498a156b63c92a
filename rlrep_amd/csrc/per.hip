// Prioritized experience replay (Schaul et al. 2016) on the device, for a single agent: a sum tree beside the replay ring, a stratified
// sampler that reads it inside the captured train(), the sac critic head with per-sample weights, and the TD errors written back as
// priorities; for vlsac / ctrlsac / spedersac / diffsrsac the sampler and the slot gather as ONE launch.
// The arithmetic is in per_tree.h and the *_body.h files it lists; the seed groups' kernels (per_group.hip) stand around the same bodies.
// A kernel here names what its body reads: P and B by REFERENCE (the record's words are loaded where the body uses them, as these kernels
// always did; copied first, per_sample_fill_kernel came out two instructions shorter and no longer its measured self), md = 0.
//
// per_add / per_sample / per_update are ONE workgroup each: the levels of the tree are dependent, a workgroup barrier between two levels
// is all the ordering they need (the per-XCD L2s are not coherent inside a launch: a multi-workgroup form needs a release / acquire per
// hand-off), and the touched part of the tree is small beside the launches they follow (profiles/per_replay.txt).
#include "per_tree.h"
#include "launchers.h"

__global__ __launch_bounds__(PER_ADD_THREADS) void per_add_kernel(PerAdd p) {
    float* tree = p.tree;
    const float mp = p.scal[0];
#include "per_add_body.h"
}

// the whole tree from its leaves (restore): every level, all nodes
__global__ __launch_bounds__(PER_ADD_THREADS) void per_rebuild_kernel(float* __restrict__ tree, long long P) {
    for (long long w = P >> 1; w >= 1; w >>= 1) {
        for (long long nd = w + threadIdx.x; nd < 2 * w; nd += PER_ADD_THREADS) tree[nd] = __fadd_rn(tree[2 * nd], tree[2 * nd + 1]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(PER_THREADS) void per_sample_kernel(PerSample p) {
    __shared__ float sh[4];
    const long long& P = p.P;
    const int& B = p.B;
    const float* tree = p.tree;
    int* idx = p.idx;
    float* w = p.w;
    const float beta = p.scal[2];
    const unsigned long long seed = p.seed;
    const long long md = 0;
#include "per_sample_body.h"
}

__global__ __launch_bounds__(PER_THREADS) void per_update_kernel(PerUpdate p) {
    __shared__ float sh[4];
    const long long& P = p.P;
    const int& B = p.B;
    float* tree = p.tree;
    float* scal = p.scal;
    const int* idx = p.idx;
    const float* td = p.td;
#include "per_update_body.h"
}

// The sampler and the slot gather of elementwise.hip as ONE launch.  Workgroup 0 is the sampler: per_sample_kernel's body -- all B draws,
// the batch minimum, idx[B] and w[B].  Workgroups 1 .. G gather: workgroup g owns the `rows` consecutive samples from (g - 1) rows on.  A
// draw is a function of (j, the tree, the Philox word) alone and the tree is read-only inside the launch, so the gatherers reach the indices
// workgroup 0 writes without any hand-off between workgroups -- the per-XCD L2s are not coherent inside a launch, a hand-off would need a
// release / acquire pair per workgroup.  A gatherer needs neither the weights nor the batch minimum, so only workgroup 0 runs all B descents:
// every draw is descended twice in the launch, whatever the grid.  LDS holds PER_FILL_ROWS indices, whatever B is.
__global__ __launch_bounds__(PER_THREADS) void per_sample_fill_kernel(PerSampleFill pf) {
    const PerSample& p = pf.s;
    __shared__ float sh[4];
    __shared__ int rows[PER_FILL_ROWS];
    const long long& P = p.P;
    const int& B = p.B;
    const float* tree = p.tree;
    int* idx = p.idx;
    const unsigned long long seed = p.seed;
    const long long md = 0, m = 0, rstride = 0;          // (a single agent: nothing moves)
    const unsigned long long off = per_stream(p.offset, p.step_dev, md);
    const float total = tree[1], seg = __fdiv_rn(total, (float)B);
    if (blockIdx.x == 0) {
        float* w = p.w;
        const float beta = p.scal[2];
#define PER_SAMPLE_HAS_STREAM
#include "per_sample_body.h"
#undef PER_SAMPLE_HAS_STREAM
        return;
    }
    constexpr bool GRP = false;
#include "per_gather_body.h"
}

__global__ __launch_bounds__(256) void qhead_critic_w_kernel(QHeadCriticW pw) {
    const QHeadCritic& p = pw.q;
    const float* pw_w = pw.w;
    float* pw_td = pw.td;
#include "qhead_critic_w_body.h"
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
// Grid: rl_launch_fill_slot gives every element of the B rows a thread of its own (up to 2048 workgroups).  Here a gathering workgroup first
// pays a descent of log2 P dependent loads (20 for 10^6 rows) in as many lanes as it owns samples, so it takes WHOLE rows -- a row cut in two
// would be descended once more -- and enough of them that a thread then copies about PER_FILL_ELEMS = 4 elements, loaded together: the copy
// adds about one more memory latency to the ~20 of the descent, while the number of descents in the launch stays 2 B whatever the grid.
// rows = clamp(4 * 256 / row width, 1, 256): 24 rows at (S, A) = (17, 6) -- 1 + 11 workgroups at B = 256 -- and 1 row at (376, 17),
// 1 + 256 workgroups.  Measured (profiles/per_critic.txt, its last section): with 8 elements a thread, copied one after the other, the
// launch lost to per_sample + fill_slot at (17, 6) B = 256 (9.5 against 7.5 us); this form wins in all eight cases measured.
extern "C" int rl_launch_per_sample_fill(PerSampleFill* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    p->rows = per_fill_rows(p->f);
    hipLaunchKernelGGL(per_sample_fill_kernel, dim3(1 + (p->s.B + p->rows - 1) / p->rows), dim3(PER_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
