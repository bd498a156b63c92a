// Device environments of a seed group (group_env.hip; include/rlrep.h rlrep_group_env_*): what the kernels and the host entry points share.
// One EnvRecord per member in an allocation of its own (as grp_seeds and the live table are): the member stride, the clone segments and the
// checkpoint device records of a group do not know it.  rlrep_amd/envs/device.py reads the same layout (RECORD_DTYPE): keep them in step.
#pragma once
#include <stdint.h>

#define RL_ENV_RETURNS 16                 // finished-episode returns a record keeps (a ring: entry episodes_done % 16 is written next)
#define RL_ENV_MAX_EPISODES 64            // grid x of one evaluation launch at the most
#define RL_ENV_EPISODE_STEPS 200          // Pendulum-v1's time limit
// Philox stream ids (XORed into counter word 3, as PhiloxFill::stream_id is).  Every draw of train() and select_action uses stream 0 with
// offsets below 2^49, so word 3 stays below 2^17 there: these two words are used by nothing else.
#define RL_STREAM_ENV 0xE0000000u         // collection: word 2 = 0 the exploration draws of a step, 1 an episode's start state; counter = the member's nsteps
#define RL_STREAM_EVAL 0xE1000000u        // evaluation start states: counter = eval_index * episodes + episode

struct EnvRecord {                        // 256 bytes
    double theta, theta_dot;              //   0: the state, fp64 as the host environment keeps it
    double episode_return;                //  16: fp64 sum of the fp32 rewards of the running episode
    long long ring_ptr;                   //  24: the row of the member's replay ring the next step writes
    long long nsteps;                     //  32: steps since rlrep_group_env_reset (the counter of the member's RL_STREAM_ENV draws)
    int t;                                //  40: step in the episode
    int ring_size;                        //  44: rows of the ring that are filled (published to size_dev[member] by every step)
    int episodes_done;                    //  48
    int force;                            //  52: 1 = the next step takes force_action instead of the policy's / the exploration draw (one shot)
    float force_action;                   //  56
    float act;                            //  60: the last action taken
    float obs[4];                         //  64: the current observation (cos, sin, theta_dot), fp32 as the host environment returns it
    double returns[RL_ENV_RETURNS];       //  80: returns of finished episodes
    double pad_[6];                       // 208
};
static_assert(sizeof(EnvRecord) == 256, "EnvRecord layout (rlrep_amd/envs/device.py RECORD_DTYPE)");

// group-wide counters, advanced by the last live member's workgroup of a step launch
struct EnvCtl {
    long long t_global;                   // steps taken since reset: a step with t_global < start_timesteps draws a uniform action (warm-up)
    unsigned long long calls;             // the select_action call counter: a step past warm-up draws at offset (calls + 1) << 20 and counts one call
    int ticket, pad_;
};
static_assert(sizeof(EnvCtl) == 24, "EnvCtl layout");
