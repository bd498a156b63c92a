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
//
// A SINGLE agent (any of the five algorithms: they share the actor trunk; rlrep_env_*) has forms of its own -- env_reset_kernel,
// env_step_kernel, env_eval_kernel: grid (1, 1) resp. (episodes, 1), no member stride, no live table, the seed by value in SelectAct::seed.
// What a record's step and an episode's rollout ARE is written once, in env_step_body.h and env_eval_body.h, and included into both forms.
//
// SEVERAL environments per member / agent (rlrep_group_env_create_n, rlrep_env_create_n; E = num_envs in [1, 64]) are the `_n` forms of the
// reset and step kernels: grid (E, members) resp. (E, 1), workgroup (e, slot) runs record m * E + e with the same body.  No workgroup waits on
// another: every record carries its own ring cursor, E rows apart from its neighbours' (group_env.h has the table), and the counters advance
// by E behind the same ticket.  A handle with E = 1 launches the one-environment kernels, which are instruction for instruction what they were.
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

// record e of its agent starts a fresh episode (start state at counter 0): counters and the returns ring are zeroed, the ring cursor is row e
template <class Env>
__device__ __forceinline__ void env_reset_record(EnvRecord* rec, unsigned long long seed, uint32_t e) {
    double th, thd;
    env_start<Env>(seed, 0ull, 2u * e + 1u, RL_STREAM_ENV, th, thd);
    rec->theta = th; rec->theta_dot = thd; rec->episode_return = 0.0; rec->ring_ptr = (long long)e; rec->nsteps = 0;
    rec->t = 0; rec->ring_size = 0; rec->episodes_done = 0; rec->force = 0; rec->force_action = 0.f; rec->act = 0.f;
    Env::observe(th, thd, rec->obs);
    for (int q = Env::S; q < 4; ++q) rec->obs[q] = 0.f;
    for (int q = 0; q < RL_ENV_RETURNS; ++q) rec->returns[q] = 0.0;
    for (int q = 0; q < 6; ++q) rec->pad_[q] = 0.0;
}
__device__ __forceinline__ void env_reset_ctl(EnvCtl* ctl) { ctl->t_global = 0; ctl->calls = 0ull; ctl->ticket = 0; ctl->pad_ = 0; }

// rlrep_group_env_reset: every member's record starts a fresh episode (all members, whatever the live table says: a reset is the caller's
// explicit act, like rlrep_group_clone_members); ring cursors, counters and the returns ring are zeroed, and so is the group's EnvCtl.
template <class Env>
__global__ __launch_bounds__(64) void group_env_reset_kernel(EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl, const unsigned long long* __restrict__ seeds) {
    if (threadIdx.x != 0) return;
    const int m = blockIdx.y;
    env_reset_record<Env>(recs + m, seeds[m], 0u);
    if (m == 0) env_reset_ctl(ctl);
}
// rlrep_env_reset: the single agent's form -- one record, the seed by value
template <class Env>
__global__ __launch_bounds__(64) void env_reset_kernel(EnvRecord* __restrict__ rec, EnvCtl* __restrict__ ctl, unsigned long long seed) {
    if (threadIdx.x != 0) return;
    env_reset_record<Env>(rec, seed, 0u);
    env_reset_ctl(ctl);
}
// the forms for E environments: grid (E, members) resp. (E, 1), record (m, e) at index m * E + e
template <class Env>
__global__ __launch_bounds__(64) void group_env_reset_kernel_n(EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl, const unsigned long long* __restrict__ seeds) {
    if (threadIdx.x != 0) return;
    const int m = blockIdx.y, e = blockIdx.x;
    env_reset_record<Env>(recs + (long long)m * gridDim.x + e, seeds[m], (uint32_t)e);
    if (m == 0 && e == 0) env_reset_ctl(ctl);
}
template <class Env>
__global__ __launch_bounds__(64) void env_reset_kernel_n(EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl, unsigned long long seed) {
    if (threadIdx.x != 0) return;
    const int e = blockIdx.x;
    env_reset_record<Env>(recs + e, seed, (uint32_t)e);
    if (e == 0) env_reset_ctl(ctl);
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
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
#define ENV_RING (ring + (long long)m * ring_stride)
#define ENV_SIZE_WORD size_dev[m]
#define ENV_INDEX 0
#define ENV_STRIDE 1
#include "env_step_body.h"
#undef ENV_RING
#undef ENV_SIZE_WORD
#undef ENV_INDEX
#undef ENV_STRIDE
    // "last workgroup advances the counters": every workgroup read them before its own ticket, so the last ticket follows every read
    __threadfence();
    if (atomicAdd(&ctl->ticket, 1) == n_live - 1) {
        ctl->ticket = 0;
        ctl->t_global = t_global + 1;
        if (!warm) ctl->calls = calls + 1ull;
    }
}

// rlrep_env_step: the single agent's form of the step -- one workgroup, one record, no member stride, no live table; the seed rides by value
// in SelectAct::seed, as select_action_kernel takes it.  p0: the agent's actor (obs / act unset).  The body is the group's (env_step_body.h);
// one workgroup needs no ticket: lane 0 advances the counters it read at the head.
template <class Env>
__global__ __launch_bounds__(1024) void env_step_kernel(SelectAct p0, EnvRecord* __restrict__ rec, EnvCtl* __restrict__ ctl, float* __restrict__ ring,
                                                        long long capacity, int* __restrict__ size_dev, float eps_greedy, long long start_timesteps) {
    const long long t_global = ctl->t_global;
    const unsigned long long calls = ctl->calls;
    const bool warm = t_global < start_timesteps;
    SelectAct p = p0;
#define ENV_RING ring
#define ENV_SIZE_WORD size_dev[0]
#define ENV_INDEX 0
#define ENV_STRIDE 1
#include "env_step_body.h"
#undef ENV_RING
#undef ENV_SIZE_WORD
#undef ENV_INDEX
#undef ENV_STRIDE
    ctl->t_global = t_global + 1;
    if (!warm) ctl->calls = calls + 1ull;
}

// The step with E = gridDim.x environments per member: workgroup (e, slot) steps record (m, e) = recs[m * E + e] with the member's actor and
// seed.  Nothing here waits: the record's own cursor names its row ((ptr + e) mod capacity of the step that starts at ptr), environment 0
// publishes the fill level (the same number in all E records), and the counters the workgroups read at the head are advanced by E by whoever
// takes the last of the n_live * E tickets -- which follows every read, as in the one-environment form.  A miscount could leave wrong
// counters behind, never a workgroup waiting.
template <class Env>
__global__ __launch_bounds__(1024) void group_env_step_kernel_n(SelectAct p0, long long mstride, const unsigned long long* __restrict__ seeds,
                                                                const int* __restrict__ live, EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl,
                                                                float* __restrict__ ring, long long ring_stride, long long capacity,
                                                                int* __restrict__ size_dev, float eps_greedy, long long start_timesteps) {
    RL_GRP_MEMBER(m, live);
    const int n_live = live[0];
    const int env_i = blockIdx.x, env_n = gridDim.x;
    EnvRecord* const rec = recs + ((long long)m * env_n + env_i);
    const long long t_global = ctl->t_global;
    const unsigned long long calls = ctl->calls;
    const bool warm = t_global < start_timesteps;                   // (decided once per launch: the caller keeps start_timesteps a multiple of E)
    const long long dm = (long long)m * mstride;
    SelectAct p = p0;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
#define ENV_RING (ring + (long long)m * ring_stride)
#define ENV_SIZE_WORD size_dev[m]
#define ENV_INDEX env_i
#define ENV_STRIDE env_n
#include "env_step_body.h"
#undef ENV_RING
#undef ENV_SIZE_WORD
#undef ENV_INDEX
#undef ENV_STRIDE
    __threadfence();
    if (atomicAdd(&ctl->ticket, 1) == n_live * env_n - 1) {
        ctl->ticket = 0;
        ctl->t_global = t_global + env_n;
        if (!warm) ctl->calls = calls + (unsigned long long)env_n;
    }
}
// the single agent's form: grid (E, 1), record e = recs[e]; E workgroups, so the ticket of the group form with E arrivals
template <class Env>
__global__ __launch_bounds__(1024) void env_step_kernel_n(SelectAct p0, EnvRecord* __restrict__ recs, EnvCtl* __restrict__ ctl, float* __restrict__ ring,
                                                          long long capacity, int* __restrict__ size_dev, float eps_greedy, long long start_timesteps) {
    const int env_i = blockIdx.x, env_n = gridDim.x;
    EnvRecord* const rec = recs + env_i;
    const long long t_global = ctl->t_global;
    const unsigned long long calls = ctl->calls;
    const bool warm = t_global < start_timesteps;
    SelectAct p = p0;
#define ENV_RING ring
#define ENV_SIZE_WORD size_dev[0]
#define ENV_INDEX env_i
#define ENV_STRIDE env_n
#include "env_step_body.h"
#undef ENV_RING
#undef ENV_SIZE_WORD
#undef ENV_INDEX
#undef ENV_STRIDE
    __threadfence();
    if (atomicAdd(&ctl->ticket, 1) == env_n - 1) {
        ctl->ticket = 0;
        ctl->t_global = t_global + env_n;
        if (!warm) ctl->calls = calls + (unsigned long long)env_n;
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
// (the member's actor and seed: spelled where the body takes its parameter block)
#define ENV_EVAL_ACTOR \
    const long long dm = (long long)m * mstride; \
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm); \
    p.seed = seeds[m];
#define ENV_EVAL_FIRST (starts + ((long long)m * episodes + e) * 2)
#define ENV_EVAL_SCORE out[(long long)m * episodes + e]
#include "env_eval_body.h"
#undef ENV_EVAL_FIRST
#undef ENV_EVAL_SCORE
#undef ENV_EVAL_ACTOR
}

// rlrep_env_evaluate: the single agent's form -- workgroup e rolls out episode e (env_eval_body.h), out[e] and starts[2 e ..]
template <class Env>
__global__ __launch_bounds__(1024) void env_eval_kernel(SelectAct p0, unsigned long long counter0, double* __restrict__ out, double* __restrict__ starts) {
#define ENV_EVAL_ACTOR
#define ENV_EVAL_FIRST (starts + (long long)e * 2)
#define ENV_EVAL_SCORE out[e]
#include "env_eval_body.h"
#undef ENV_EVAL_FIRST
#undef ENV_EVAL_SCORE
#undef ENV_EVAL_ACTOR
}

static size_t env_lds(const SelectAct* p, bool slot, bool flag) {
    return sizeof(float) * ((size_t)p->S + 2 * (size_t)p->Ha + 2 * (size_t)p->A + (slot ? 1 + 6 + (size_t)p->S + (size_t)p->A + (flag ? 1 : 0) : 0));      // (eval: alignment slack, three doubles, obs, act, end flag)
}
template <class Env>
static int env_launch_step(const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y, int num_envs, EnvRecord* recs, EnvCtl* ctl,
                           float* ring, long long ring_stride, long long capacity, int* size_dev, float eps_greedy, long long start_timesteps, hipStream_t st) {
    const size_t lds = env_lds(p, false, false);
    if (lds > 60 * 1024 || p->S != Env::S || p->A != Env::A || grid_y < 1 || grid_y > RLREP_GROUP_MAX_MEMBERS) return -7;
    if (num_envs < 1 || num_envs > RL_ENV_MAX_ENVS || capacity < num_envs) return -7;
    if (num_envs == 1)
        hipLaunchKernelGGL(group_env_step_kernel<Env>, dim3(1, grid_y), dim3(1024), lds, st, *p, mstride, seeds, live, recs, ctl, ring, ring_stride, capacity, size_dev,
                           eps_greedy, start_timesteps);
    else
        hipLaunchKernelGGL(group_env_step_kernel_n<Env>, dim3(num_envs, grid_y), dim3(1024), lds, st, *p, mstride, seeds, live, recs, ctl, ring, ring_stride, capacity,
                           size_dev, eps_greedy, start_timesteps);
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
template <class Env>
static int env_launch_reset(EnvRecord* recs, EnvCtl* ctl, const unsigned long long* seeds, int members, int num_envs, hipStream_t st) {
    if (num_envs == 1) hipLaunchKernelGGL(group_env_reset_kernel<Env>, dim3(1, members), dim3(64), 0, st, recs, ctl, seeds);
    else hipLaunchKernelGGL(group_env_reset_kernel_n<Env>, dim3(num_envs, members), dim3(64), 0, st, recs, ctl, seeds);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_group_env_reset(int kind, EnvRecord* recs, EnvCtl* ctl, const unsigned long long* seeds, int members, int num_envs, hipStream_t st) {
    if (members < 1 || members > RLREP_GROUP_MAX_MEMBERS || num_envs < 1 || num_envs > RL_ENV_MAX_ENVS) return -7;
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_reset<EnvPendulum>(recs, ctl, seeds, members, num_envs, st);
    case EnvMountainCar::KIND: return env_launch_reset<EnvMountainCar>(recs, ctl, seeds, members, num_envs, st);
    default: return -7;
    }
}
extern "C" int rl_launch_group_env_step(int kind, const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y,
                                        int num_envs, EnvRecord* recs, EnvCtl* ctl, float* ring, long long ring_stride, long long capacity, int* size_dev, float eps_greedy,
                                        long long start_timesteps, hipStream_t st) {
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_step<EnvPendulum>(p, mstride, seeds, live, grid_y, num_envs, recs, ctl, ring, ring_stride, capacity, size_dev, eps_greedy, start_timesteps, st);
    case EnvMountainCar::KIND: return env_launch_step<EnvMountainCar>(p, mstride, seeds, live, grid_y, num_envs, recs, ctl, ring, ring_stride, capacity, size_dev, eps_greedy, start_timesteps, st);
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
// ---- the single agent's forms (rlrep_env_*): the seed rides in p->seed ----
template <class Env>
static int env_launch_step1(const SelectAct* p, int num_envs, EnvRecord* rec, EnvCtl* ctl, float* ring, long long capacity, int* size_dev, float eps_greedy, long long start_timesteps, hipStream_t st) {
    const size_t lds = env_lds(p, false, false);
    if (lds > 60 * 1024 || p->S != Env::S || p->A != Env::A || capacity < 1) return -7;
    if (num_envs < 1 || num_envs > RL_ENV_MAX_ENVS || capacity < num_envs) return -7;
    if (num_envs == 1) hipLaunchKernelGGL(env_step_kernel<Env>, dim3(1, 1), dim3(1024), lds, st, *p, rec, ctl, ring, capacity, size_dev, eps_greedy, start_timesteps);
    else hipLaunchKernelGGL(env_step_kernel_n<Env>, dim3(num_envs, 1), dim3(1024), lds, st, *p, rec, ctl, ring, capacity, size_dev, eps_greedy, start_timesteps);
    return (int)hipGetLastError();
}
template <class Env>
static int env_launch_eval1(const SelectAct* p, unsigned long long counter0, int episodes, double* out, double* starts, hipStream_t st) {
    const size_t lds = env_lds(p, true, Env::TERMINATES);
    if (lds > 60 * 1024 || p->S != Env::S || p->A != Env::A || episodes < 1 || episodes > RL_ENV_MAX_EPISODES) return -7;
    hipLaunchKernelGGL(env_eval_kernel<Env>, dim3(episodes, 1), dim3(1024), lds, st, *p, counter0, out, starts);
    return (int)hipGetLastError();
}
template <class Env>
static int env_launch_reset1(EnvRecord* rec, EnvCtl* ctl, unsigned long long seed, int num_envs, hipStream_t st) {
    if (num_envs == 1) hipLaunchKernelGGL(env_reset_kernel<Env>, dim3(1, 1), dim3(64), 0, st, rec, ctl, seed);
    else hipLaunchKernelGGL(env_reset_kernel_n<Env>, dim3(num_envs, 1), dim3(64), 0, st, rec, ctl, seed);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_env_reset(int kind, EnvRecord* rec, EnvCtl* ctl, unsigned long long seed, int num_envs, hipStream_t st) {
    if (num_envs < 1 || num_envs > RL_ENV_MAX_ENVS) return -7;
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_reset1<EnvPendulum>(rec, ctl, seed, num_envs, st);
    case EnvMountainCar::KIND: return env_launch_reset1<EnvMountainCar>(rec, ctl, seed, num_envs, st);
    default: return -7;
    }
}
extern "C" int rl_launch_env_step(int kind, const SelectAct* p, int num_envs, EnvRecord* rec, EnvCtl* ctl, float* ring, long long capacity, int* size_dev, float eps_greedy,
                                  long long start_timesteps, hipStream_t st) {
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_step1<EnvPendulum>(p, num_envs, rec, ctl, ring, capacity, size_dev, eps_greedy, start_timesteps, st);
    case EnvMountainCar::KIND: return env_launch_step1<EnvMountainCar>(p, num_envs, rec, ctl, ring, capacity, size_dev, eps_greedy, start_timesteps, st);
    default: return -7;
    }
}
extern "C" int rl_launch_env_eval(int kind, const SelectAct* p, unsigned long long counter0, int episodes, double* out, double* starts, hipStream_t st) {
    switch (kind) {
    case EnvPendulum::KIND: return env_launch_eval1<EnvPendulum>(p, counter0, episodes, out, starts, st);
    case EnvMountainCar::KIND: return env_launch_eval1<EnvMountainCar>(p, counter0, episodes, out, starts, st);
    default: return -7;
    }
}
