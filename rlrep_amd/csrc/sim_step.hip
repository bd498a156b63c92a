// Fused simulators for the one-graph simulator loop (include/rlrep.h rlrep_sim_*; DESIGN.md 6i "Fused simulators"; rlrep_amd/envs/fused_sim.py):
// N environments of one kind (group_env.h: EnvPendulum, EnvMountainCar, unchanged) stepped by ONE launch, one thread per environment, 256
// threads per workgroup, grid ceil(N / 256); no LDS, no scratch.  The state is caller-owned device memory, structure of arrays (kparams.h
// SimState): consecutive lanes read consecutive words of every array, and a wave's [N, S] rows (S = 2 or 3) are one contiguous span.
//
// Three forms, templates over the kind as group_env.hip's kernels are:
//   sim_start_kernel       every environment begins a new episode from its next start state
//   sim_step_kernel        dynamics, observation, reward, done, the running return, the end of an episode and the restart (or the freeze)
//   sim_step_kernel_ctl    the step, and the transition packed into replay-ring row (ctl[START] + e) mod capacity; ONE thread does what
//                          replay_add_cols_kernel_ctl's one thread does.  The loop record is read through a wave-uniform address (scalar
//                          loads): every workgroup reads START, one thread reads SIZE and WARM and writes ITER, T and CALLS -- words no
//                          workgroup of this launch reads (kparams.h, the loop record's rule).
// The `s` column of a ring row is obs[e] as it stood before the step: the thread that overwrites it has read it first, so no copy is needed.
//
// Start state k of environment e under seed sigma is Env::start of the Philox4x32-10 block with key sigma and counter
// {k lo, k hi, e, RL_STREAM_SIM_START}: word 2 is the environment, so neither e nor k bounds the other.
//
// The dynamics are fp64 in the operation order of the host environments (group_env.h); sin / cos / fmod are the device library's, a few
// hundred fp64 operations per environment and step, which at one thread per environment is far below the launch's own latency.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "group.h"
#include "group_env.h"
#include "launchers.h"

// the start state `k` of environment `e` (group_env.h RL_STREAM_SIM_START)
template <class Env>
__device__ __forceinline__ void sim_start_state(unsigned long long seed, unsigned long long k, uint32_t e, double& x0, double& x1) {
    uint32_t c[4] = {(uint32_t)k, (uint32_t)(k >> 32), e, RL_STREAM_SIM_START};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    Env::start(c, x0, x1);
}

// environment e draws its next start state and stands at step 0 of a new episode; returns the state, writes t, ep_return and starts
template <class Env>
__device__ __forceinline__ void sim_restart(const SimState& s, int e, double& x0, double& x1) {
    const long long k = s.starts[e];
    sim_start_state<Env>(s.seed, (unsigned long long)k, (uint32_t)e, x0, x1);
    s.starts[e] = k + 1;
    s.t[e] = 0;
    s.ep_return[e] = 0.0;
}

template <class Env>
__global__ __launch_bounds__(256) void sim_start_kernel(SimState s) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n) return;
    double x0, x1;
    sim_restart<Env>(s, e, x0, x1);
    s.x0[e] = x0; s.x1[e] = x1;
    float o[Env::S];
    Env::observe(x0, x1, o);
#pragma unroll
    for (int q = 0; q < Env::S; ++q) s.obs[(long long)e * Env::S + q] = o[q];
}

// One step of environment e.  cur: the observation before the step, nx: s', r32: the reward, done: done_bool (env_step_body.h's rule).  A
// frozen environment (t = -1: it ended under auto_restart = 0) gives nx = cur, r = 0, done = 0 and changes nothing.
template <class Env>
__device__ __forceinline__ void sim_step_one(const SimState& s, int e, float action, float* cur, float* nx, float& r32, float& done) {
#pragma unroll
    for (int q = 0; q < Env::S; ++q) cur[q] = s.obs[(long long)e * Env::S + q];
    const int t0 = s.t[e];
    if (t0 < 0) {
#pragma unroll
        for (int q = 0; q < Env::S; ++q) nx[q] = cur[q];
        r32 = 0.f; done = 0.f;
        return;
    }
    double x0 = s.x0[e], x1 = s.x1[e];
    bool goal;
    r32 = Env::dynamics(x0, x1, action, goal);
    Env::observe(x0, x1, nx);
    const int t = t0 + 1;
    // done_bool is the host loop's rule (main.py): an end by the time limit does not count, and neither does a goal reached on the limit's step
    done = (Env::TERMINATES && goal && t < Env::LIMIT) ? 1.f : 0.f;
    const double ret = s.ep_return[e] + (double)r32;
    float o[Env::S];
#pragma unroll
    for (int q = 0; q < Env::S; ++q) o[q] = nx[q];
    if ((Env::TERMINATES && goal) || t >= Env::LIMIT) {
        s.last_return[e] = ret;
        s.episodes[e] += 1;
        if (s.auto_restart) {
            sim_restart<Env>(s, e, x0, x1);
            Env::observe(x0, x1, o);
        } else {                                        // frozen where it ended: the state and the return stay as the last step left them
            s.t[e] = -1;
            s.ep_return[e] = ret;
        }
    } else {
        s.t[e] = t;
        s.ep_return[e] = ret;
    }
    s.x0[e] = x0; s.x1[e] = x1;
#pragma unroll
    for (int q = 0; q < Env::S; ++q) s.obs[(long long)e * Env::S + q] = o[q];
}

template <class Env>
__global__ __launch_bounds__(256) void sim_step_kernel(SimState s, const float* __restrict__ act, long long ld_act, float* __restrict__ next_obs,
                                                       float* __restrict__ reward, float* __restrict__ done) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n) return;
    float cur[Env::S], nx[Env::S], r32, d;
    sim_step_one<Env>(s, e, act[(long long)e * ld_act], cur, nx, r32, d);
#pragma unroll
    for (int q = 0; q < Env::S; ++q) next_obs[(long long)e * Env::S + q] = nx[q];
    reward[e] = r32; done[e] = d;
}

// step-and-append: ring row (START + e) mod capacity = [obs before the step | the action as given | s' | r | done]
template <class Env>
__global__ __launch_bounds__(256) void sim_step_kernel_ctl(SimState s, const float* __restrict__ act, long long ld_act, float* __restrict__ ring,
                                                           long long capacity, int* __restrict__ size_dev, long long* __restrict__ ctl) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    long long st = ctl[RL_CTL_START];
    if (st < 0 || st >= capacity) st = 0;                                  // (a cursor written by the host: never leave the ring)
    if (e < s.n) {
        const float a = act[(long long)e * ld_act];
        float cur[Env::S], nx[Env::S], r32, d;
        sim_step_one<Env>(s, e, a, cur, nx, r32, d);
        long long dst = st + e; if (dst >= capacity) dst -= capacity;      // (the launcher holds n <= capacity)
        float* row = ring + dst * Env::ROW;
#pragma unroll
        for (int q = 0; q < Env::S; ++q) { row[q] = cur[q]; row[Env::S + Env::A + q] = nx[q]; }
        row[Env::S] = a; row[2 * Env::S + Env::A] = r32; row[2 * Env::S + Env::A + 1] = d;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (size_dev) *size_dev = (int)min(max(ctl[RL_CTL_SIZE], 0ll), capacity);
        ctl[RL_CTL_ITER] += 1;
        ctl[RL_CTL_T] += s.n;
        if (!ctl[RL_CTL_WARM]) ctl[RL_CTL_CALLS] += s.n;
    }
}

// ---- group forms (include/rlrep.h rlrep_group_sim_*): R x n environments, grid (ceil(n / 256), slot) ----
// Every array of the state is [members, n] planes (obs [members, n, S]) and member m's start states are keyed by sim_seeds[m]: its plane is the
// single simulator with that seed, word for word -- sim_step_one and sim_restart run unchanged on a SimState rebased to the plane, so `e` is
// the environment's index within the member.  s0.seed is ignored.
template <class Env>
__device__ __forceinline__ SimState sim_member(const SimState& s0, int m, const unsigned long long* __restrict__ seeds) {
    SimState s = s0;
    const long long d = (long long)m * s0.n;
    s.x0 += d; s.x1 += d; s.ep_return += d; s.last_return += d; s.t += d; s.episodes += d; s.starts += d; s.obs += d * Env::S;
    s.seed = seeds[m];
    return s;
}
// a reset of the whole group: grid y is the member, the live table is not consulted
template <class Env>
__global__ __launch_bounds__(256) void sim_start_kernel_grp(SimState s0, const unsigned long long* __restrict__ seeds) {
    const SimState s = sim_member<Env>(s0, (int)blockIdx.y, seeds);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n) return;
    double x0, x1;
    sim_restart<Env>(s, e, x0, x1);
    s.x0[e] = x0; s.x1[e] = x1;
    float o[Env::S];
    Env::observe(x0, x1, o);
#pragma unroll
    for (int q = 0; q < Env::S; ++q) s.obs[(long long)e * Env::S + q] = o[q];
}
// act, next_obs, reward, done: member m's plane lies n rows behind member m - 1's.  A retired member's planes are neither read nor written.
template <class Env>
__global__ __launch_bounds__(256) void sim_step_kernel_grp(SimState s0, const unsigned long long* __restrict__ seeds, const int* __restrict__ live,
                                                           const float* __restrict__ act, long long ld_act, float* __restrict__ next_obs,
                                                           float* __restrict__ reward, float* __restrict__ done) {
    RL_GRP_MEMBER(m, live);
    const SimState s = sim_member<Env>(s0, m, seeds);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n) return;
    const long long g = (long long)m * s.n + e;
    float cur[Env::S], nx[Env::S], r32, d;
    sim_step_one<Env>(s, e, act[g * ld_act], cur, nx, r32, d);
#pragma unroll
    for (int q = 0; q < Env::S; ++q) next_obs[g * Env::S + q] = nx[q];
    reward[g] = r32; done[g] = d;
}
// step-and-append of a group (kparams.h "the loop record of a GROUP"): member m's rows go into its ring (ring + m * ring_stride) from ITS
// start row; thread 0 of workgroup (0, slot) publishes its fill level, the one of slot 0 advances the group's ITER, T and CALLS once
template <class Env>
__global__ __launch_bounds__(256) void sim_step_kernel_ctl_grp(SimState s0, const unsigned long long* __restrict__ seeds, const int* __restrict__ live,
                                                               const float* __restrict__ act, long long ld_act, float* __restrict__ ring,
                                                               long long ring_stride, long long capacity, int* __restrict__ size_dev,
                                                               long long* __restrict__ ctl) {
    RL_GRP_MEMBER(m, live);
    const SimState s = sim_member<Env>(s0, m, seeds);
    const long long* cm = ctl + (long long)m * RL_LOOP_CTL_WORDS;
    const int e = blockIdx.x * 256 + threadIdx.x;
    long long st = cm[RL_CTL_START];
    if (st < 0 || st >= capacity) st = 0;                                  // (a cursor written by the host: never leave the ring)
    if (e < s.n) {
        const float a = act[((long long)m * s.n + e) * ld_act];
        float cur[Env::S], nx[Env::S], r32, d;
        sim_step_one<Env>(s, e, a, cur, nx, r32, d);
        long long dst = st + e; if (dst >= capacity) dst -= capacity;      // (the launcher holds n <= capacity)
        float* row = ring + (long long)m * ring_stride + dst * Env::ROW;
#pragma unroll
        for (int q = 0; q < Env::S; ++q) { row[q] = cur[q]; row[Env::S + Env::A + q] = nx[q]; }
        row[Env::S] = a; row[2 * Env::S + Env::A] = r32; row[2 * Env::S + Env::A + 1] = d;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (size_dev) size_dev[m] = (int)min(max(cm[RL_CTL_SIZE], 0ll), capacity);
        if (blockIdx.y == 0) {
            ctl[RL_CTL_ITER] += 1;
            ctl[RL_CTL_T] += s.n;
            if (!ctl[RL_CTL_WARM]) ctl[RL_CTL_CALLS] += s.n;
        }
    }
}

// ---- launchers: grid ceil(n / 256); the caller (engine.hip rlrep_sim_*) has checked the arguments; an unknown kind is -7 ----
static inline dim3 sim_grid(const SimState* s) { return dim3((unsigned)((s->n + 255) / 256)); }
extern "C" int rl_launch_sim_start(const SimState* s, hipStream_t st) {
    if (s->n < 1 || s->n > RL_SIM_MAX_ENVS) return -7;
    switch (s->kind) {
    case EnvPendulum::KIND: hipLaunchKernelGGL(sim_start_kernel<EnvPendulum>, sim_grid(s), dim3(256), 0, st, *s); break;
    case EnvMountainCar::KIND: hipLaunchKernelGGL(sim_start_kernel<EnvMountainCar>, sim_grid(s), dim3(256), 0, st, *s); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
extern "C" int rl_launch_sim_step(const SimState* s, const float* act, long long ld_act, float* next_obs, float* reward, float* done, hipStream_t st) {
    if (s->n < 1 || s->n > RL_SIM_MAX_ENVS) return -7;
    switch (s->kind) {
    case EnvPendulum::KIND: hipLaunchKernelGGL(sim_step_kernel<EnvPendulum>, sim_grid(s), dim3(256), 0, st, *s, act, ld_act, next_obs, reward, done); break;
    case EnvMountainCar::KIND: hipLaunchKernelGGL(sim_step_kernel<EnvMountainCar>, sim_grid(s), dim3(256), 0, st, *s, act, ld_act, next_obs, reward, done); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
extern "C" int rl_launch_sim_step_ctl(const SimState* s, const float* act, long long ld_act, float* ring, long long capacity, int* size_dev, long long* ctl,
                                      hipStream_t st) {
    if (s->n < 1 || s->n > RL_SIM_MAX_ENVS || capacity < s->n) return -7;
    switch (s->kind) {
    case EnvPendulum::KIND: hipLaunchKernelGGL(sim_step_kernel_ctl<EnvPendulum>, sim_grid(s), dim3(256), 0, st, *s, act, ld_act, ring, capacity, size_dev, ctl); break;
    case EnvMountainCar::KIND: hipLaunchKernelGGL(sim_step_kernel_ctl<EnvMountainCar>, sim_grid(s), dim3(256), 0, st, *s, act, ld_act, ring, capacity, size_dev, ctl); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
// the group's: grid (ceil(n / 256), y); the caller (group_api.hip rlrep_group_sim_*) holds the group active and has checked the arguments
extern "C" int rl_launch_sim_start_grp(const SimState* s, const unsigned long long* seeds, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr) return RL_GRP_UNSUPPORTED;
    if (s->n < 1 || s->n > RL_SIM_MAX_ENVS) return -7;
    const dim3 grid(sim_grid(s).x, (unsigned)gr->members);                  // (a reset of every member: not the live table's grid)
    switch (s->kind) {
    case EnvPendulum::KIND: hipLaunchKernelGGL(sim_start_kernel_grp<EnvPendulum>, grid, dim3(256), 0, st, *s, seeds); break;
    case EnvMountainCar::KIND: hipLaunchKernelGGL(sim_start_kernel_grp<EnvMountainCar>, grid, dim3(256), 0, st, *s, seeds); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
extern "C" int rl_launch_sim_step_grp(const SimState* s, const unsigned long long* seeds, const float* act, long long ld_act, float* next_obs, float* reward,
                                      float* done, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr || !gr->live) return RL_GRP_UNSUPPORTED;
    if (s->n < 1 || s->n > RL_SIM_MAX_ENVS) return -7;
    const dim3 grid(sim_grid(s).x, (unsigned)gr->grid_y);
    switch (s->kind) {
    case EnvPendulum::KIND: hipLaunchKernelGGL(sim_step_kernel_grp<EnvPendulum>, grid, dim3(256), 0, st, *s, seeds, gr->live, act, ld_act, next_obs, reward, done); break;
    case EnvMountainCar::KIND: hipLaunchKernelGGL(sim_step_kernel_grp<EnvMountainCar>, grid, dim3(256), 0, st, *s, seeds, gr->live, act, ld_act, next_obs, reward, done); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
extern "C" int rl_launch_sim_step_ctl_grp(const SimState* s, const unsigned long long* seeds, const float* act, long long ld_act, float* ring,
                                          long long ring_stride, long long capacity, int* size_dev, long long* ctl, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr || !gr->live) return RL_GRP_UNSUPPORTED;
    if (s->n < 1 || s->n > RL_SIM_MAX_ENVS || capacity < s->n) return -7;
    const dim3 grid(sim_grid(s).x, (unsigned)gr->grid_y);
    switch (s->kind) {
    case EnvPendulum::KIND:
        hipLaunchKernelGGL(sim_step_kernel_ctl_grp<EnvPendulum>, grid, dim3(256), 0, st, *s, seeds, gr->live, act, ld_act, ring, ring_stride, capacity, size_dev, ctl); break;
    case EnvMountainCar::KIND:
        hipLaunchKernelGGL(sim_step_kernel_ctl_grp<EnvMountainCar>, grid, dim3(256), 0, st, *s, seeds, gr->live, act, ld_act, ring, ring_stride, capacity, size_dev, ctl); break;
    default: return -7;
    }
    return (int)hipGetLastError();
}
