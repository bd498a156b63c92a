// Environments of a seed group ON THE DEVICE (include/rlrep.h rlrep_group_env_*): acting, exploring, stepping the dynamics and writing the
// replay-ring row of every live member are ONE launch (group_env_step_kernel), captured in front of the group's train() graph, and one
// evaluation of every live member is ONE launch (group_env_eval_kernel) instead of members x episodes x (up to the time limit) host round trips.
//
// The kernels are templates over the kind (group_env.h: EnvPendulum, EnvMountainCar -- S, the row width, the time limit, start state,
// observation and dynamics).  The dynamics are the public gym specifications as rlrep_amd/envs/pendulum.py and envs/mountain_car.py restate
// them, computed in fp64 by ONE lane in the operation order of those files, with contraction off (NumPy does not fuse): observation, reward and
// (for the kinds that keep an fp32 state) the state are rounded to fp32 where the host environment rounds them.  What differs from the host is
// libm: sin / cos / fmod are the device library's.
//
// Shape: grid (1, members) resp. (episodes, members), 1024 threads, RL_GRP_MEMBER first (group.h): the workgroups of a retired member return
// before they read or write anything.  The actor forward is select_action_body.h, the body of select_action_kernel(_grp): same tiles, same
// summation order, same Philox draw -- the action is bit for bit what rlrep_group_select_action returns for the same observation, seed and
// offset.  All stores are ordinary per-lane stores from lane 0.
#include <hip/hip_runtime.h>
#include "common.h"
#include "kparams.h"
#include "group.h"
#include "philox.h"
#include "group_env.h"
#include "launchers.h"

// an episode's start state of kind Env from one Philox block
template <class Env>
__device__ __forceinline__ void env_start(unsigned long long seed, unsigned long long counter, uint32_t word2, uint32_t stream, double& x0, double& x1) {
    uint32_t c[4] = {(uint32_t)counter, (uint32_t)(counter >> 32), word2, stream};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    Env::start(c, x0, x1);
}

// rlrep_group_env_reset: every member's record starts a fresh episode (all members, whatever the live table says: a reset is the caller's
// explicit act, like rlrep_group_clone_members); ring cursors, counters and the returns ring are zeroed, and so is the group's EnvCtl.
template <class Env>
__global__ __launch_bounds__(64) void group_env_reset_kernel(EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl, const unsigned long long* __restrict__ seeds) {
    if (threadIdx.x != 0) return;
    const int m = blockIdx.y;
    EnvRecord* rec = recs + m;
    double th, thd;
    env_start<Env>(seeds[m], 0ull, 1u, RL_STREAM_ENV, th, thd);
    rec->theta = th; rec->theta_dot = thd; rec->episode_return = 0.0; rec->ring_ptr = 0; rec->nsteps = 0;
    rec->t = 0; rec->ring_size = 0; rec->episodes_done = 0; rec->force = 0; rec->force_action = 0.f; rec->act = 0.f;
    Env::observe(th, thd, rec->obs);
    for (int q = Env::S; q < 4; ++q) rec->obs[q] = 0.f;
    for (int q = 0; q < RL_ENV_RETURNS; ++q) rec->returns[q] = 0.0;
    for (int q = 0; q < 6; ++q) rec->pad_[q] = 0.0;
    if (m == 0) { ctl->t_global = 0; ctl->calls = 0ull; ctl->ticket = 0; ctl->pad_ = 0; }
}

// One environment step of every live member.  p0: member 0's actor (obs / act unset); ring: member 0's replay ring, member m's lies
// ring_stride floats further and holds `capacity` rows [s | a | s' | r | done_bool] (replay_add_kernel_grp's layout).
template <class Env>
__global__ __launch_bounds__(1024) void group_env_step_kernel(SelectAct p0, long long mstride, const unsigned long long* __restrict__ seeds,
                                                              const int* __restrict__ live, EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl,
                                                              float* __restrict__ ring, long long ring_stride, long long capacity,
                                                              int* __restrict__ size_dev, float eps_greedy, long long start_timesteps) {
    RL_GRP_MEMBER(m, live);
    const int n_live = live[0];
    EnvRecord* const rec = recs + m;
    // the group's counters as they stand before this launch: whoever finishes last advances them (below), after every workgroup has read them
    const long long t_global = ctl->t_global;
    const unsigned long long calls = ctl->calls;
    const bool warm = t_global < start_timesteps;
    const long long dm = (long long)m * mstride;
    SelectAct p = p0;
    p.obs = rec->obs; p.act = &rec->act;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
    p.explore = 1; p.offset = (calls + 1ull) << 20;                 // SeedBatchMixin.select_action(explore=True): `_ctr += 1`, offset `_ctr << 20`
#include "select_action_body.h"
    if (threadIdx.x != 0) return;
    // ---- one lane from here on (it wrote rec->act itself: A = 1) ----
    float a = rec->act;
    const unsigned long long n = (unsigned long long)rec->nsteps;
    {
        uint32_t c[4] = {(uint32_t)n, (uint32_t)(n >> 32), 0u, RL_STREAM_ENV};
        philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
        if (warm || env_u01f(c[0]) < eps_greedy) a = fminf(fmaxf(p.lo + (p.hi - p.lo) * env_u01f(c[1]), p.lo), p.hi);
    }
    if (rec->force) { a = rec->force_action; rec->force = 0; }
    double th = rec->theta, thd = rec->theta_dot;
    float s[Env::S], nx[Env::S];
#pragma unroll
    for (int q = 0; q < Env::S; ++q) s[q] = rec->obs[q];
    bool goal;
    const float r32 = Env::dynamics(th, thd, a, goal);
    Env::observe(th, thd, nx);
    long long ptr = rec->ring_ptr;
    if (ptr < 0 || ptr >= capacity) ptr = 0;                        // (a cursor written by the host: never leave the ring)
    float* row = ring + (long long)m * ring_stride + ptr * Env::ROW;
#pragma unroll
    for (int q = 0; q < Env::S; ++q) { row[q] = s[q]; row[Env::S + 1 + q] = nx[q]; }
    row[Env::S] = a; row[2 * Env::S + 1] = r32;
    const int t = rec->t + 1;
    // done_bool is the host loop's rule (main.py): an end by the time limit does not count, and neither does a goal reached on the limit's step
    row[2 * Env::S + 2] = (Env::TERMINATES && goal && t < Env::LIMIT) ? 1.f : 0.f;
    rec->ring_ptr = ptr + 1 >= capacity ? 0 : ptr + 1;
    const int fill = (int)min((long long)rec->ring_size + 1, capacity);
    rec->ring_size = fill;
    size_dev[m] = fill;
    rec->act = a;
    rec->nsteps = (long long)(n + 1);
    const double ret = rec->episode_return + (double)r32;
    if ((Env::TERMINATES && goal) || t >= Env::LIMIT) {
        const int done = rec->episodes_done;
        rec->returns[done & (RL_ENV_RETURNS - 1)] = ret;
        rec->episodes_done = done + 1;
        rec->episode_return = 0.0; rec->t = 0;
        env_start<Env>(p.seed, n + 1, 1u, RL_STREAM_ENV, th, thd);
        Env::observe(th, thd, nx);
    } else {
        rec->episode_return = ret; rec->t = t;
    }
    rec->theta = th; rec->theta_dot = thd;
#pragma unroll
    for (int q = 0; q < Env::S; ++q) rec->obs[q] = nx[q];
    // "last workgroup advances the counters": every workgroup read them before its own ticket, so the last ticket follows every read
    __threadfence();
    if (atomicAdd(&ctl->ticket, 1) == n_live - 1) {
        ctl->ticket = 0;
        ctl->t_global = t_global + 1;
        if (!warm) ctl->calls = calls + 1ull;
    }
}

// One evaluation: workgroup (e, slot) rolls out one whole episode of its member with the MEAN action (select_action(explore=False)) from the
// start state Philox(seed, RL_STREAM_EVAL, counter0 + e) gives, and writes the fp64 sum of the fp32 rewards to out[m * episodes + e] and the
// start state to starts[(m * episodes + e) * 2 ..].  The observation and the action live in LDS behind the body's buffers; the weights are
// read from L2 every step (the three layers do not fit in LDS).
// A kind whose episodes can end before the limit leaves the loop WORKGROUP-UNIFORMLY: lane 0 alone decides (it holds the state) and writes a
// flag word in LDS, and every lane reads that word behind the barrier at the head of the next iteration -- the barrier that follows the
// dynamics anyway -- so all 1024 lanes see one value and break in the same iteration; no lane waits at a barrier the others have left.  The
// flag is written again only behind the body's barriers, after every lane has read it.  The trip count is bounded by the constant Env::LIMIT.
template <class Env>
__global__ __launch_bounds__(1024) void group_env_eval_kernel(SelectAct p0, long long mstride, const unsigned long long* __restrict__ seeds,
                                                              const int* __restrict__ live, unsigned long long counter0, int episodes,
                                                              double* __restrict__ out, double* __restrict__ starts) {
    RL_GRP_MEMBER(m, live);
    extern __shared__ float sm[];
    // behind the body's buffers (8-byte aligned): x0 | x1 | return (fp64: kept out of the registers the body needs), then obs[S] | act[A]
    // (| the end flag of a kind that terminates)
    double* const st = (double*)(sm + ((p0.S + 2 * p0.Ha + 2 * p0.A + 1) & ~1));
    float* const slot = (float*)(st + 3);
    const int e = blockIdx.x;
    const long long dm = (long long)m * mstride;
    SelectAct p = p0;
    p.obs = slot; p.act = slot + p0.S;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
    p.explore = 0; p.offset = 0ull;
    if (threadIdx.x == 0) {
        double th, thd;
        env_start<Env>(p.seed, counter0 + (unsigned long long)e, 0u, RL_STREAM_EVAL, th, thd);
        double* first = starts + ((long long)m * episodes + e) * 2;
        first[0] = th; first[1] = thd;
        st[0] = th; st[1] = thd; st[2] = 0.0;
        Env::observe(th, thd, slot);
        if constexpr (Env::TERMINATES) slot[p0.S + p0.A] = 0.f;
    }
    for (int step = 0; step < Env::LIMIT; ++step) {
        __syncthreads();
        if constexpr (Env::TERMINATES) {
            if (slot[p0.S + p0.A] != 0.f) break;                    // uniform: one LDS word, read by all lanes behind the barrier
        }
        {
#include "select_action_body.h"
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double th = st[0], thd = st[1];
            bool goal;
            st[2] += (double)Env::dynamics(th, thd, slot[p0.S], goal);
            st[0] = th; st[1] = thd;
            Env::observe(th, thd, slot);
            if constexpr (Env::TERMINATES) { if (goal) slot[p0.S + p0.A] = 1.f; }
        }
    }
    if (threadIdx.x == 0) out[(long long)m * episodes + e] = st[2];
}

static size_t env_lds(const SelectAct* p, bool slot, bool flag) {
    return sizeof(float) * ((size_t)p->S + 2 * (size_t)p->Ha + 2 * (size_t)p->A + (slot ? 1 + 6 + (size_t)p->S + (size_t)p->A + (flag ? 1 : 0) : 0));      // (eval: alignment slack, three doubles, obs, act, end flag)
}
template <class Env>
static int env_launch_step(const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y, EnvRecord* recs, EnvCtl* ctl,
                           float* ring, long long ring_stride, long long capacity, int* size_dev, float eps_greedy, long long start_timesteps, hipStream_t st) {
    const size_t lds = env_lds(p, false, false);
    if (lds > 60 * 1024 || p->S != Env::S || p->A != Env::A || grid_y < 1 || grid_y > RLREP_GROUP_MAX_MEMBERS) return -7;
    hipLaunchKernelGGL(group_env_step_kernel<Env>, dim3(1, grid_y), dim3(1024), lds, st, *p, mstride, seeds, live, recs, ctl, ring, ring_stride, capacity, size_dev,
                       eps_greedy, start_timesteps);
    return (int)hipGetLastError();
}
template <class Env>
static int env_launch_eval(const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y, unsigned long long counter0,
                           int episodes, double* out, double* starts, hipStream_t st) {
    const size_t lds = env_lds(p, true, Env::TERMINATES);
    if (lds > 60 * 1024 || p->S != Env::S || p->A != Env::A || grid_y < 1 || grid_y > RLREP_GROUP_MAX_MEMBERS || episodes < 1 || episodes > RL_ENV_MAX_EPISODES) return -7;
    hipLaunchKernelGGL(group_env_eval_kernel<Env>, dim3(episodes, grid_y), dim3(1024), lds, st, *p, mstride, seeds, live, counter0, episodes, out, starts);
    return (int)hipGetLastError();
}
// the launchers dispatch on the kind (an unknown one is -7: rlrep_group_env_create refuses it long before)
extern "C" int rl_launch_group_env_reset(int kind, EnvRecord* recs, EnvCtl* ctl, const unsigned long long* seeds, int members, hipStream_t st) {
    if (members < 1 || members > RLREP_GROUP_MAX_MEMBERS) return -7;
    switch (kind) {
    case EnvPendulum::KIND: hipLaunchKernelGGL(group_env_reset_kernel<EnvPendulum>, dim3(1, members), dim3(64), 0, st, recs, ctl, seeds); break;
    case EnvMountainCar::KIND: hipLaunchKernelGGL(group_env_reset_kernel<EnvMountainCar>, dim3(1, members), dim3(64), 0, st, recs, ctl, seeds); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
extern "C" int rl_launch_group_env_step(int kind, const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y,
                                        EnvRecord* recs, EnvCtl* ctl, float* ring, long long ring_stride, long long capacity, int* size_dev, float eps_greedy,
                                        long long start_timesteps, hipStream_t st) {
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_step<EnvPendulum>(p, mstride, seeds, live, grid_y, recs, ctl, ring, ring_stride, capacity, size_dev, eps_greedy, start_timesteps, st);
    case EnvMountainCar::KIND: return env_launch_step<EnvMountainCar>(p, mstride, seeds, live, grid_y, recs, ctl, ring, ring_stride, capacity, size_dev, eps_greedy, start_timesteps, st);
    default: return -7;
    }
}
extern "C" int rl_launch_group_env_eval(int kind, const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y,
                                        unsigned long long counter0, int episodes, double* out, double* starts, hipStream_t st) {
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_eval<EnvPendulum>(p, mstride, seeds, live, grid_y, counter0, episodes, out, starts, st);
    case EnvMountainCar::KIND: return env_launch_eval<EnvMountainCar>(p, mstride, seeds, live, grid_y, counter0, episodes, out, starts, st);
    default: return -7;
    }
}
