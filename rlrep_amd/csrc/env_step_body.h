// body of the device environment's step kernels (group_env.hip: group_env_step_kernel(_n), env_step_kernel(_n)), one record's work.  The kernel
// has set up: `p` (SelectAct: the actor's weights, dimensions, action range and seed of THIS record's agent), `rec` (its EnvRecord), `calls`
// and `warm` (from the EnvCtl as it stood before the launch), `capacity` and `eps_greedy`, and four macros evaluated where they are used:
// ENV_RING (its ring), ENV_SIZE_WORD (the word its fill level is published in), ENV_INDEX (which of its agent's environments the record is:
// word 2 of its Philox blocks, its place in the action offsets, and only index 0 publishes the fill level) and ENV_STRIDE (how many
// environments the agent has: the rows a cursor advances by).  The one-environment forms pass the literals 0 and 1, which fold away.
// All lanes run the actor forward; lane 0 alone goes on behind it.
    p.obs = rec->obs; p.act = &rec->act;
    p.explore = 1; p.offset = (calls + 1ull + (unsigned long long)(ENV_INDEX)) << 20;      // select_action(explore=True), one call per environment in their order: `_ctr += 1`, offset `_ctr << 20`
#include "select_action_body.h"
    if (threadIdx.x != 0) return;
    // ---- one lane from here on (it wrote rec->act itself: A = 1) ----
    float a = rec->act;
    const unsigned long long n = (unsigned long long)rec->nsteps;
    {
        uint32_t c[4] = {(uint32_t)n, (uint32_t)(n >> 32), 2u * (uint32_t)(ENV_INDEX), RL_STREAM_ENV};
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
    if (ptr < 0 || ptr >= capacity) ptr = (ENV_INDEX);                      // (a cursor written by the host: never leave the ring)
    float* row = ENV_RING + ptr * Env::ROW;
#pragma unroll
    for (int q = 0; q < Env::S; ++q) { row[q] = s[q]; row[Env::S + 1 + q] = nx[q]; }
    row[Env::S] = a; row[2 * Env::S + 1] = r32;
    const int t = rec->t + 1;
    // done_bool is the host loop's rule (main.py): an end by the time limit does not count, and neither does a goal reached on the limit's step
    row[2 * Env::S + 2] = (Env::TERMINATES && goal && t < Env::LIMIT) ? 1.f : 0.f;
    // the cursor advances by ENV_STRIDE rows modulo capacity (the launcher holds ENV_STRIDE <= capacity); a stride of one wraps to row 0, spelled
    // so that the one-environment forms keep the instructions they had
    const long long nxt = ptr + (ENV_STRIDE);
    rec->ring_ptr = nxt < capacity ? nxt : ((ENV_STRIDE) == 1 ? 0ll : nxt - capacity);
    const int fill = (int)min((long long)rec->ring_size + (ENV_STRIDE), capacity);
    rec->ring_size = fill;
    if ((ENV_INDEX) == 0) ENV_SIZE_WORD = fill;                     // (the value is the same in every environment of the agent: they step together)
    rec->act = a;
    rec->nsteps = (long long)(n + 1);
    const double ret = rec->episode_return + (double)r32;
    if ((Env::TERMINATES && goal) || t >= Env::LIMIT) {
        const int done = rec->episodes_done;
        rec->returns[done & (RL_ENV_RETURNS - 1)] = ret;
        rec->episodes_done = done + 1;
        rec->episode_return = 0.0; rec->t = 0;
        env_start<Env>(p.seed, n + 1, 2u * (uint32_t)(ENV_INDEX) + 1u, RL_STREAM_ENV, th, thd);
        Env::observe(th, thd, nx);
    } else {
        rec->episode_return = ret; rec->t = t;
    }
    rec->theta = th; rec->theta_dot = thd;
#pragma unroll
    for (int q = 0; q < Env::S; ++q) rec->obs[q] = nx[q];
