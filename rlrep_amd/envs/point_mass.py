"""The host twin of the example simulator kind rlrep_amd/envs/kinds/point_mass.h, NumPy float64, operation for operation:
a point mass in the plane, x = (px, py, vx, vy), two actions (the force, clipped to +-1 per component), semi-implicit Euler with dt = 0.1,
speeds clamped to +-1, positions to +-2, reward (-d - 0.01 |f|^2) + (10 inside the goal radius 0.1), where d is the distance from the origin
after the step; the goal ends the episode, the time limit is 100 steps; start position uniform in (-1, 1)^2, speed 0.

`step(x, a)` is vectorised over environments and keeps no state; `start_state` restates the Philox draw of the device (block 0 gives px, block
1 gives py); `step_sim` adds the fused simulators' episode rules (csrc/sim_jit.h simx_step_one): done_bool, the end of an episode, the freeze.
Only + - * /, compares and sqrt, all IEEE-exact, so the device reproduces every bit."""
import numpy as np

from rlrep_amd.utils import philox_host

NX, S, A, LIMIT, TERMINATES = 4, 4, 2, 100, True
DT, F_MAX, V_MAX, P_MAX, GOAL_RADIUS, GOAL_BONUS, ACTION_COST = 0.1, 1.0, 1.0, 2.0, 0.1, 10.0, 0.01
STREAM_SIM_START = 0xE3000000                               # csrc/group_env.h RL_STREAM_SIM_START
ACTION_RANGE = (-1.0, 1.0)


def _clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def observe(x):
    """x float64 [NX, N] -> obs float32 [N, S]"""
    return np.ascontiguousarray(np.asarray(x, np.float64).T).astype(np.float32)


def step(x, a):
    """x float64 [NX, N], a float32 [N, A] (raw) -> (x' float64 [NX, N], reward float32 [N], goal bool [N], wall bool [N]: a position clamp bit)"""
    x = np.asarray(x, np.float64)
    a = np.asarray(a, np.float32).astype(np.float64)
    fx, fy = _clamp(a[:, 0], -F_MAX, F_MAX), _clamp(a[:, 1], -F_MAX, F_MAX)
    vx, vy = _clamp(x[2] + fx * DT, -V_MAX, V_MAX), _clamp(x[3] + fy * DT, -V_MAX, V_MAX)
    qx, qy = x[0] + vx * DT, x[1] + vy * DT
    px, py = _clamp(qx, -P_MAX, P_MAX), _clamp(qy, -P_MAX, P_MAX)
    d = np.sqrt(px * px + py * py)
    goal = d < GOAL_RADIUS
    r = (-d - ACTION_COST * (fx * fx + fy * fy)) + np.where(goal, GOAL_BONUS, 0.0)
    return np.stack([px, py, vx, vy]), r.astype(np.float32), goal, (px != qx) | (py != qy)


def _u01d(hi, lo):
    return (float(((int(hi) << 32) | int(lo)) >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def start_block(seed, e, k, q=0):
    """uint32[4]: Philox block q of start state k of environment e -- key seed, counter {k lo, k hi, e, STREAM_SIM_START + q}"""
    off = ((STREAM_SIM_START + int(q)) << 32) | int(e)
    return philox_host.raw_stream(4 * (int(k) + 1), seed, off)[4 * int(k):]


def start_state(seed, e, k):
    """float64[NX]: start state k of environment e"""
    c0, c1 = start_block(seed, e, k, 0), start_block(seed, e, k, 1)
    return np.array([-1.0 + 2.0 * _u01d(c0[0], c0[1]), -1.0 + 2.0 * _u01d(c1[0], c1[1]), 0.0, 0.0])


def step_sim(x, t, a, auto_restart=True):
    """the fused simulator's rules around step(): x [NX, N], t int [N] (-1 = frozen), a [N, A] ->
    dict(x, t, next_obs, reward, done, ended, goal, wall); an ended environment's x is left as the step gave it and its t is 0 (auto_restart: the
    caller puts the start state in) or -1 (frozen)"""
    x, t = np.array(x, np.float64), np.array(t, np.int64)
    live = t >= 0
    x2, r, goal, wall = step(x, a)
    t2 = t + 1
    done = (goal & (t2 < LIMIT) & live).astype(np.float32)
    ended = live & (goal | (t2 >= LIMIT))
    x2 = np.where(live, x2, x)
    return dict(x=x2, t=np.where(live, np.where(ended, 0 if auto_restart else -1, t2), t), next_obs=observe(x2), reward=np.where(live, r, np.float32(0)),
                done=done, ended=ended, goal=goal & live, wall=wall & live)
