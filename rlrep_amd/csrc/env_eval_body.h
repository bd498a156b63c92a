// body of the device environment's evaluation kernels (group_env.hip: group_env_eval_kernel, env_eval_kernel): one workgroup, one episode.
// The kernel's parameter block is `p0` (SelectAct: the actor's weights, dimensions, action range and -- single form -- seed).  Macros the kernel
// defines: ENV_EVAL_ACTOR (statements that make the copy `p` THIS workgroup's agent: the group form moves the weights to the member and takes
// its seed, the single form needs none), and, evaluated by lane 0 where they are used, ENV_EVAL_FIRST (where the episode's start state goes)
// and ENV_EVAL_SCORE (the word its return goes to).  `counter0` is the Philox counter of episode 0.
    extern __shared__ float sm[];
    // behind the body's buffers (8-byte aligned): x0 | x1 | return (fp64: kept out of the registers the body needs), then obs[S] | act[A]
    // (| the end flag of a kind that terminates)
    double* const st = (double*)(sm + ((p0.S + 2 * p0.Ha + 2 * p0.A + 1) & ~1));
    float* const slot = (float*)(st + 3);
    const int e = blockIdx.x;
    SelectAct p = p0;
    p.obs = slot; p.act = slot + p0.S;
    ENV_EVAL_ACTOR
    p.explore = 0; p.offset = 0ull;
    if (threadIdx.x == 0) {
        double th, thd;
        env_start<Env>(p.seed, counter0 + (unsigned long long)e, 0u, RL_STREAM_EVAL, th, thd);
        double* first = ENV_EVAL_FIRST;
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
    if (threadIdx.x == 0) ENV_EVAL_SCORE = st[2];
