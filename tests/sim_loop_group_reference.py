"""The NumPy restatement of the loop record of a seed group (csrc/kparams.h "the loop record of a GROUP"; csrc/actor_tile.hip
actor_tile_kernel_ctl_grp, csrc/elementwise.hip replay_add_cols_kernel_ctl_grp, csrc/sim_step.hip sim_step_kernel_ctl_grp).  A plain module,
imported like sim_loop_reference.py, whose exploration mix member r applies with its own seed.

The record is int64[R, 8].  CALLS (word 0), T (1), ITER (2) and WARM (6) are the group's and live in row 0; NEXT (3), START (4) and SIZE (5)
are member r's cursor into its own ring and live in row r.  The two launches of an iteration run the live members only:

    act launch      every live member r: START = clamp(NEXT), NEXT = (START + N) mod capacity, SIZE = min(max(SIZE, 0) + N, capacity);
                    once (the first live member's thread): WARM = T < start_timesteps
    append launch   every live member r: rows START .. START + N - 1 (wrapping) of ring r are written, size word r = clamp(SIZE);
                    once: ITER += 1, T += N, CALLS += N unless WARM

With nobody live nothing runs and nothing advances.  A retired member's row stands still."""
import numpy as np

import sim_loop_reference as single

WORDS = 8
CALLS, T, ITER, NEXT, START, SIZE, WARM = range(7)
mix = single.mix                # member r: mix(actions[r], seeds[r], ITER, WARM, eps_greedy, lo, hi)


def new_record(members, ptr=0, sizes=None, capacity=None):
    """the record as SimLoopGroup.set_cursor leaves it: every member's cursor at `ptr`, its own fill level"""
    w = np.zeros((members, WORDS), np.int64)
    w[:, NEXT] = w[:, START] = ptr % capacity if capacity else ptr
    w[:, SIZE] = 0 if sizes is None else np.asarray(sizes, np.int64)
    return w


def act(w, live, n, capacity, start_timesteps):
    """the act launch's bookkeeping, in place; returns (warm, calls, it): what the workgroups read"""
    calls, t, it = int(w[0, CALLS]), int(w[0, T]), int(w[0, ITER])
    warm = t < start_timesteps
    members = [r for r in range(len(w)) if live[r]]
    for r in members:
        ptr = int(w[r, NEXT])
        if ptr < 0 or ptr >= capacity:
            ptr = 0
        nxt = ptr + n
        w[r, START] = ptr
        w[r, NEXT] = nxt if nxt < capacity else nxt - capacity
        w[r, SIZE] = min(max(int(w[r, SIZE]), 0) + n, capacity)
    if members:
        w[0, WARM] = int(warm)
    return warm, calls, it


def append(w, live, n, capacity):
    """the append launch's bookkeeping, in place; returns {member: (ring rows written, published fill level)}"""
    out = {}
    members = [r for r in range(len(w)) if live[r]]
    for r in members:
        st = int(w[r, START])
        if st < 0 or st >= capacity:
            st = 0
        out[r] = ((st + np.arange(n)) % capacity, min(max(int(w[r, SIZE]), 0), capacity))
    if members:
        w[0, ITER] += 1
        w[0, T] += n
        if not w[0, WARM]:
            w[0, CALLS] += n
    return out


def iteration(w, live, n, capacity, start_timesteps):
    """one iteration: (warm, rows written per live member)"""
    warm, _, _ = act(w, live, n, capacity, start_timesteps)
    return warm, append(w, live, n, capacity)
