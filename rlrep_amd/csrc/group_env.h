// Device environments of a seed group (group_env.hip; include/rlrep.h rlrep_group_env_*): what the kernels and the host entry points share.
// One EnvRecord per member and environment ([members][num_envs], record (m, e) at index m * num_envs + e) in an allocation of its own (as grp_seeds and the live table are): the member stride, the clone segments and the
// checkpoint device records of a group do not know it.  rlrep_amd/envs/device.py reads the same layout (RECORD_DTYPE): keep them in step.
#pragma once
#include <stdint.h>

#define RL_ENV_RETURNS 16                 // finished-episode returns a record keeps (a ring: entry episodes_done % 16 is written next)
#define RL_ENV_MAX_EPISODES 64            // grid x of one evaluation launch at the most
#define RL_ENV_MAX_ENVS 64                // environments per member / agent (num_envs): grid x of one step launch at the most
// Philox stream ids (XORed into counter word 3, as PhiloxFill::stream_id is).  Every draw of train() and select_action uses stream 0 with
// offsets below 2^49, so word 3 stays below 2^17 there: these two words are used by nothing else.
#define RL_STREAM_ENV 0xE0000000u         // collection: word 2 = 0 the exploration draws of a step, 1 an episode's start state; counter = the member's nsteps
#define RL_STREAM_EVAL 0xE1000000u        // evaluation start states: counter = eval_index * episodes + episode
#define RL_STREAM_SIM 0xE2000000u         // the exploration mix of a simulator loop (actor_tile_kernel_ctl): counter = the loop's iteration, word 2 = row e,
                                          // word 3 = RL_STREAM_SIM + block q; the pick is word 0 of block 0, u_j word (1 + j) & 3 of block (1 + j) >> 2
#define RL_STREAM_SIM_START 0xE3000000u   // start states of a fused simulator (sim_step.hip): counter = the environment's count of start states drawn, word 2 = environment e
// With E = num_envs environments per member (rlrep_group_env_create_n / rlrep_env_create_n), environment e of a member draws
//   key            the member's / agent's seed                      (as before)
//   counter        record (m, e)'s own nsteps                       (as before)
//   word 3         RL_STREAM_ENV                                    (as before)
//   word 2         2 e       the exploration draws of a step        (e = 0: 0, the single environment's)
//                  2 e + 1   an episode's start state               (e = 0: 1, the single environment's)
//   actor noise    stream 0 at offset (calls + 1 + e) << 20: select_action(explore=True) at call counter calls + 1 + e -- E calls, in
//                  environment order; the launch then counts E calls
// so environment 0 is the single environment draw for draw, and word 2 stays below 128.  RL_STREAM_EVAL does not know E: evaluation is
// per member.
// Ring rows of a step: record (m, e)'s cursor is (ptr + e) mod capacity where the member's next free row is ptr (reset: ptr = 0;
// set_cursor(ptr)); a step writes there and advances the cursor by E mod capacity and ring_size by E (capped), so the E rows of one step lie
// in environment order behind ptr, wrapping inside the step where capacity is no multiple of E.  Record (m, 0)'s cursor is the next free row.

struct EnvRecord {                        // 256 bytes
    double theta, theta_dot;              //   0: the state, fp64 as the host environment keeps it (MountainCarContinuous-v0: position p and velocity v,
                                          //      fp32-representable values: that environment rounds its state where gym's float32 array does)
    double episode_return;                //  16: fp64 sum of the fp32 rewards of the running episode
    long long ring_ptr;                   //  24: the row of the member's replay ring the next step writes
    long long nsteps;                     //  32: steps since rlrep_group_env_reset (the counter of the member's RL_STREAM_ENV draws)
    int t;                                //  40: step in the episode
    int ring_size;                        //  44: rows of the ring that are filled (published to size_dev[member] by every step)
    int episodes_done;                    //  48
    int force;                            //  52: 1 = the next step takes force_action instead of the policy's / the exploration draw (one shot)
    float force_action;                   //  56
    float act;                            //  60: the last action taken
    float obs[4];                         //  64: the current observation, fp32 as the host environment returns it: obs[0..S-1] of the kind, (cos, sin,
                                          //      theta_dot) resp. (p, v); the rest is 0
    double returns[RL_ENV_RETURNS];       //  80: returns of finished episodes
    double pad_[6];                       // 208
};
static_assert(sizeof(EnvRecord) == 256, "EnvRecord layout (rlrep_amd/envs/device.py RECORD_DTYPE)");

// group-wide counters, advanced by the last workgroup of a step launch (of n_live * num_envs; the single agent's: of num_envs)
struct EnvCtl {
    long long t_global;                   // steps per member taken since reset (a launch adds num_envs): a launch with t_global < start_timesteps draws uniform actions (warm-up)
    unsigned long long calls;             // the select_action call counter: a step past warm-up draws at offset (calls + 1 + e) << 20 and the launch counts num_envs calls
    int ticket, pad_;
};
static_assert(sizeof(EnvCtl) == 24, "EnvCtl layout");

// ---- the kinds (include/rlrep.h RLREP_ENV_*) -------------------------------------------------------------------------------------------------
// Everything a kind is, in ONE place: a row of rl_env_kinds for the host entry points, and a traits struct for the kernels of group_env.hip,
// which are templates over it -- S, the ring row 2S + A + 2, the time limit, whether a state can END the episode (a kind that cannot pays
// nothing for the test: `if constexpr`), and three functions:
//   start(c, x0, x1)             an episode's start state from the four words of one Philox block
//   observe(x0, x1, obs)         obs[0..S-1], fp32 as the host environment returns it
//   dynamics(x0, x1, a, goal)    one step in fp64, operation for operation the host file's, contraction off; returns the fp32 reward and sets
//                                `goal` where the new state is terminal.  (x0, x1) leave as the host environment holds them afterwards.
// A further kind is one more struct, one more row and one more case in the three launchers' switch.
struct EnvKindInfo { int kind; const char* name; int S, A, row, limit; float lo, hi; };           // lo, hi: the environment's own action range
static const EnvKindInfo rl_env_kinds[] = {
    {0, "Pendulum-v1", 3, 1, 9, 200, -2.f, 2.f},
    {2, "MountainCarContinuous-v0", 2, 1, 7, 999, -1.f, 1.f},
};
static inline const EnvKindInfo* rl_env_kind(int kind) {
    for (const EnvKindInfo& k : rl_env_kinds) if (k.kind == kind) return &k;
    return nullptr;
}

#ifdef __HIPCC__
#define RL_PI 3.141592653589793
__device__ __forceinline__ float env_u01f(uint32_t w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }          // (0, 1), 24 bits
__device__ __forceinline__ double env_u01d(uint32_t hi, uint32_t lo) {                                                   // (0, 1), 53 bits
    return ((double)((((unsigned long long)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// Pendulum-v1 (rlrep_amd/envs/pendulum.py): g = 10, m = l = 1, dt = 0.05, torque clipped to +-2, speed to +-8, reward from the wrapped angle,
// 200-step time limit and no other end, reset theta ~ U(-pi, pi), theta_dot ~ U(-1, 1).  The state stays fp64.
struct EnvPendulum {
    static constexpr int KIND = 0, S = 3, A = 1, ROW = 9, LIMIT = 200;
    static constexpr bool TERMINATES = false;
    static __device__ __forceinline__ void start(const uint32_t* c, double& th, double& thd) {
        th = -RL_PI + 2.0 * RL_PI * env_u01d(c[0], c[1]);
        thd = -1.0 + 2.0 * env_u01d(c[2], c[3]);
    }
    static __device__ __forceinline__ void observe(double th, double thd, float* obs) {
        obs[0] = (float)cos(th); obs[1] = (float)sin(th); obs[2] = (float)thd;
    }
    // PendulumEnv.step (envs/pendulum.py:46-56), operation for operation
    static __device__ __forceinline__ float dynamics(double& th, double& thd, float action, bool& goal) {
#pragma clang fp contract(off)
        const double u = fmin(fmax((double)action, -2.0), 2.0);
        double wrapped = fmod(th + RL_PI, 2.0 * RL_PI);                 // Python's float %: the sign of the divisor
        if (wrapped < 0.0) wrapped += 2.0 * RL_PI;
        wrapped -= RL_PI;
        const double cost = (wrapped * wrapped + 0.1 * (thd * thd)) + 0.001 * (u * u);
        double v = thd + (15.0 * sin(th) + 3.0 * u) * 0.05;
        v = fmin(fmax(v, -8.0), 8.0);
        th = th + v * 0.05;
        thd = v;
        goal = false;
        return (float)(-cost);
    }
};

// MountainCarContinuous-v0 (rlrep_amd/envs/mountain_car.py): power 0.0015, speed clipped to +-0.07, position to [-1.2, 0.6], an inelastic left
// wall, the goal p >= 0.45 with v >= 0 ends the episode with +100, reward -0.1 a^2 of the RAW action, 999-step time limit, reset
// p ~ U(-0.6, -0.4), v = 0.  (p, v) are rounded to fp32 at reset and at the end of every step, as gym's float32 state array does; the goal is
// decided on the fp64 values before that rounding.
struct EnvMountainCar {
    static constexpr int KIND = 2, S = 2, A = 1, ROW = 7, LIMIT = 999;
    static constexpr bool TERMINATES = true;
    static __device__ __forceinline__ void start(const uint32_t* c, double& p, double& v) {
#pragma clang fp contract(off)
        p = (double)(float)(-0.6 + 0.2 * env_u01d(c[0], c[1]));
        v = 0.0;
    }
    static __device__ __forceinline__ void observe(double p, double v, float* obs) { obs[0] = (float)p; obs[1] = (float)v; }
    // MountainCarContinuousEnv.step, operation for operation
    static __device__ __forceinline__ float dynamics(double& p_, double& v_, float action, bool& goal) {
#pragma clang fp contract(off)
        const double a = (double)action;
        const double force = fmin(fmax(a, -1.0), 1.0);
        double v = v_ + (force * 0.0015 - 0.0025 * cos(3.0 * p_));
        v = fmin(fmax(v, -0.07), 0.07);
        double p = p_ + v;
        p = fmin(fmax(p, -1.2), 0.6);
        if (p == -1.2 && v < 0.0) v = 0.0;
        goal = p >= 0.45 && v >= 0.0;
        const double r = (goal ? 100.0 : 0.0) - 0.1 * (a * a);
        p_ = (double)(float)p; v_ = (double)(float)v;
        return (float)r;
    }
};
#endif
