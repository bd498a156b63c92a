// Fused simulators over a kind given as TEXT (include/rlrep.h rlrep_sim_kind_*, rlrep_simx_*; envs/fused_sim.py CustomFusedSim).
// This file is self-contained: it is compiled at build time by sim_jit_check.hip (with the two example kinds of envs/kinds/) and, as text
// carried in the library, at run time by sim_jit.hip in front of a user's struct.  It restates the three kernels of sim_step.hip over a
// general kind and shares nothing with that file.
//
// A kind is one struct:
//   struct MyKind {
//       static constexpr int NX = 4, S = 4, A = 2, LIMIT = 100;      // state doubles 1..8, observations 1..16, actions 1..8, time limit >= 1
//       static constexpr bool TERMINATES = true;                     // can a state END the episode (a goal)?
//       static __device__ void start(const uint32_t* c, double* x);          // x[NX] from the 4 * ceil(NX / 2) Philox words c
//       static __device__ void observe(const double* x, float* obs);         // obs[S], fp32 as a host environment would return it
//       static __device__ float dynamics(double* x, const float* a, bool& goal);   // one step in place; the RAW actions a[A]; returns the reward
//   };
// Block q of start state k of environment e under seed sigma is the Philox4x32-10 block with key sigma and counter
// {k lo, k hi, e, SIMX_STREAM_SIM_START + q}; words 4q .. 4q + 3 of c.  Block 0 is the block the built-in kinds draw.
//
// State: structure of arrays in caller-owned device memory (SimxState = include/rlrep.h rlrep_simx_state): x float64 [NX, n] -- word i of
// environment e at x[i * n + e], so consecutive lanes read consecutive words -- and ep_return, last_return, t, episodes, starts, obs [n, S] as
// kparams.h SimState has them.  One thread per environment, 256 threads per workgroup, grid ceil(n / 256), no LDS; S, A and NX are
// compile-time, so the state, the observation and the ring row live in registers and the row packing unrolls.
//
// The rules are sim_step.hip sim_step_one's: done = TERMINATES && goal && t + 1 < LIMIT; an episode that ended (the goal, or the limit)
// files its return and restarts from its next start state, or, with auto_restart = 0, is frozen (t = -1); a frozen environment's step gives
// s' = s, r = 0, done = 0 and changes nothing.  The _ctl form keeps to the loop record's rule (kparams.h RL_CTL_*): every workgroup reads
// START through a wave-uniform address, one thread reads SIZE and WARM and writes ITER, T and CALLS.
#ifndef RL_SIM_JIT_H
#define RL_SIM_JIT_H
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#else
typedef __hip_internal::uint32_t uint32_t;     // (the run-time compiler's own header keeps its fixed-width names in a namespace)
#endif

#define SIMX_STREAM_SIM_START 0xE3000000u       // csrc/group_env.h RL_STREAM_SIM_START
#define SIMX_PI 3.141592653589793
enum { SIMX_CTL_CALLS = 0, SIMX_CTL_T = 1, SIMX_CTL_ITER = 2, SIMX_CTL_START = 4, SIMX_CTL_SIZE = 5, SIMX_CTL_WARM = 6 };   // kparams.h RL_CTL_*

struct SimxState {
    double* x;                             // [NX, n]
    double *ep_return, *last_return;       // [n]
    int* t;                                // [n] step in the episode; -1: ended and frozen
    long long *episodes, *starts;          // [n]
    float* obs;                            // [n, S]
    int n, auto_restart;
    unsigned long long seed;
};

// (0, 1) from two Philox words, 53 bits: group_env.h env_u01d
__device__ __forceinline__ double simx_u01d(uint32_t hi, uint32_t lo) {
    return ((double)((((unsigned long long)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ void simx_philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

template <class K>
struct SimxCheck {
    static_assert(K::NX >= 1 && K::NX <= 8, "a kind has 1 to 8 state doubles (NX)");
    static_assert(K::S >= 1 && K::S <= 16, "a kind has 1 to 16 observations (S)");
    static_assert(K::A >= 1 && K::A <= 8, "a kind has 1 to 8 actions (A)");
    static_assert(K::LIMIT >= 1, "a kind's time limit (LIMIT) is at least 1");
    static constexpr int ROW = 2 * K::S + K::A + 2, BLOCKS = (K::NX + 1) / 2;
};

// environment e draws its next start state into x[NX] and stands at step 0 of a new episode: writes t, ep_return and starts
template <class K>
__device__ __forceinline__ void simx_restart(const SimxState& s, int e, double* x) {
    constexpr int NB = SimxCheck<K>::BLOCKS;
    const unsigned long long k = (unsigned long long)s.starts[e];
    uint32_t c[4 * NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        uint32_t b[4] = {(uint32_t)k, (uint32_t)(k >> 32), (uint32_t)e, SIMX_STREAM_SIM_START + (uint32_t)q};
        simx_philox4x32_10(b, (uint32_t)s.seed, (uint32_t)(s.seed >> 32));
        c[4 * q] = b[0]; c[4 * q + 1] = b[1]; c[4 * q + 2] = b[2]; c[4 * q + 3] = b[3];
    }
    K::start(c, x);
    s.starts[e] = (long long)k + 1;
    s.t[e] = 0;
    s.ep_return[e] = 0.0;
}

template <class K>
__device__ __forceinline__ void simx_start_body(const SimxState& s) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n) return;
    double x[K::NX];
    simx_restart<K>(s, e, x);
#pragma unroll
    for (int i = 0; i < K::NX; ++i) s.x[(long long)i * s.n + e] = x[i];
    float o[K::S];
    K::observe(x, o);
#pragma unroll
    for (int q = 0; q < K::S; ++q) s.obs[(long long)e * K::S + q] = o[q];
}

// One step of environment e.  cur: the observation before the step, nx: s', r32: the reward, done: done_bool
template <class K>
__device__ __forceinline__ void simx_step_one(const SimxState& s, int e, const float* a, float* cur, float* nx, float& r32, float& done) {
#pragma unroll
    for (int q = 0; q < K::S; ++q) cur[q] = s.obs[(long long)e * K::S + q];
    const int t0 = s.t[e];
    if (t0 < 0) {                                       // frozen
#pragma unroll
        for (int q = 0; q < K::S; ++q) nx[q] = cur[q];
        r32 = 0.f; done = 0.f;
        return;
    }
    double x[K::NX];
#pragma unroll
    for (int i = 0; i < K::NX; ++i) x[i] = s.x[(long long)i * s.n + e];
    bool goal = false;
    r32 = K::dynamics(x, a, goal);
    K::observe(x, nx);
    const int t = t0 + 1;
    done = (K::TERMINATES && goal && t < K::LIMIT) ? 1.f : 0.f;        // an end by the time limit, or a goal on the limit's step, does not count
    const double ret = s.ep_return[e] + (double)r32;
    float o[K::S];
#pragma unroll
    for (int q = 0; q < K::S; ++q) o[q] = nx[q];
    if ((K::TERMINATES && goal) || t >= K::LIMIT) {
        s.last_return[e] = ret;
        s.episodes[e] += 1;
        if (s.auto_restart) {
            simx_restart<K>(s, e, x);
            K::observe(x, o);
        } else {                                        // frozen where it ended
            s.t[e] = -1;
            s.ep_return[e] = ret;
        }
    } else {
        s.t[e] = t;
        s.ep_return[e] = ret;
    }
#pragma unroll
    for (int i = 0; i < K::NX; ++i) s.x[(long long)i * s.n + e] = x[i];
#pragma unroll
    for (int q = 0; q < K::S; ++q) s.obs[(long long)e * K::S + q] = o[q];
}

template <class K>
__device__ __forceinline__ void simx_step_body(const SimxState& s, const float* __restrict__ act, long long ld_act, float* __restrict__ next_obs,
                                               float* __restrict__ reward, float* __restrict__ done) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= s.n) return;
    float a[K::A], cur[K::S], nx[K::S], r32, d;
#pragma unroll
    for (int j = 0; j < K::A; ++j) a[j] = act[(long long)e * ld_act + j];
    simx_step_one<K>(s, e, a, cur, nx, r32, d);
#pragma unroll
    for (int q = 0; q < K::S; ++q) next_obs[(long long)e * K::S + q] = nx[q];
    reward[e] = r32; done[e] = d;
}

// step-and-append: ring row (START + e) mod capacity = [obs before the step | the actions as given | s' | r | done]
template <class K>
__device__ __forceinline__ void simx_step_ctl_body(const SimxState& s, const float* __restrict__ act, long long ld_act, float* __restrict__ ring,
                                                   long long capacity, int* __restrict__ size_dev, long long* __restrict__ ctl) {
    constexpr int S = K::S, A = K::A, ROW = SimxCheck<K>::ROW;
    const int e = blockIdx.x * 256 + threadIdx.x;
    long long st = ctl[SIMX_CTL_START];
    if (st < 0 || st >= capacity) st = 0;                                  // (a cursor written by the host: never leave the ring)
    if (e < s.n) {
        float a[A], cur[S], nx[S], r32, d;
#pragma unroll
        for (int j = 0; j < A; ++j) a[j] = act[(long long)e * ld_act + j];
        simx_step_one<K>(s, e, a, cur, nx, r32, d);
        long long dst = st + e; if (dst >= capacity) dst -= capacity;      // (the entry point holds n <= capacity)
        float* row = ring + dst * ROW;
#pragma unroll
        for (int q = 0; q < S; ++q) { row[q] = cur[q]; row[S + A + q] = nx[q]; }
#pragma unroll
        for (int j = 0; j < A; ++j) row[S + j] = a[j];
        row[2 * S + A] = r32; row[2 * S + A + 1] = d;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (size_dev) {
            long long sz = ctl[SIMX_CTL_SIZE];
            sz = sz < 0 ? 0 : (sz > capacity ? capacity : sz);
            *size_dev = (int)sz;
        }
        ctl[SIMX_CTL_ITER] += 1;
        ctl[SIMX_CTL_T] += s.n;
        if (!ctl[SIMX_CTL_WARM]) ctl[SIMX_CTL_CALLS] += s.n;
    }
}

// the three kernels of kind K under the C names simx_start_<tag>, simx_step_<tag>, simx_step_ctl_<tag> (the run-time compile's tag is `jit`)
#define RL_SIMX_KERNELS(K, tag)                                                                                                                  \
    extern "C" __global__ __launch_bounds__(256) void simx_start_##tag(SimxState s) { simx_start_body<K>(s); }                                   \
    extern "C" __global__ __launch_bounds__(256) void simx_step_##tag(SimxState s, const float* act, long long ld_act, float* next_obs,          \
                                                                      float* reward, float* done) {                                              \
        simx_step_body<K>(s, act, ld_act, next_obs, reward, done);                                                                               \
    }                                                                                                                                            \
    extern "C" __global__ __launch_bounds__(256) void simx_step_ctl_##tag(SimxState s, const float* act, long long ld_act, float* ring,          \
                                                                          long long capacity, int* size_dev, long long* ctl) {                   \
        simx_step_ctl_body<K>(s, act, ld_act, ring, capacity, size_dev, ctl);                                                                    \
    }
#endif  // RL_SIM_JIT_H
