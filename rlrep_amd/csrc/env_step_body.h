// body of the device environment's step kernels (group_env.hip: group_env_step_kernel, env_step_kernel), one record's work.  The kernel
// has set up: `p` (SelectAct: the actor's weights, dimensions, action range and seed of THIS record's agent), `rec` (its EnvRecord), `calls`
// and `warm` (from the EnvCtl as it stood before the launch), `capacity` and `eps_greedy`, and two macros evaluated by lane 0 where they are used: ENV_RING (its ring)
// and ENV_SIZE_WORD (the word its fill level is published in).  All lanes run the actor forward; lane 0 alone goes on behind it.
    p.obs = rec->obs; p.act = &rec->act;
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
    float* row = ENV_RING + ptr * Env::ROW;
#pragma unroll
    for (int q = 0; q < Env::S; ++q) { row[q] = s[q]; row[Env::S + 1 + q] = nx[q]; }
    row[Env::S] = a; row[2 * Env::S + 1] = r32;
    const int t = rec->t + 1;
    // done_bool is the host loop's rule (main.py): an end by the time limit does not count, and neither does a goal reached on the limit's step
    row[2 * Env::S + 2] = (Env::TERMINATES && goal && t < Env::LIMIT) ? 1.f : 0.f;
    rec->ring_ptr = ptr + 1 >= capacity ? 0 : ptr + 1;
    const int fill = (int)min((long long)rec->ring_size + 1, capacity);
    rec->ring_size = fill;
    ENV_SIZE_WORD = fill;
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
