"""The host restatement of the fused simulators (DESIGN.md 6i "Fused simulators"; csrc/sim_step.hip), built on rlrep_amd/utils/philox_host.py
and the host environments.  A plain module, imported like sim_loop_reference.py.

Start state k of environment e under seed sigma: the Philox4x32-10 block with key sigma and counter {k lo, k hi, e, STREAM_SIM_START}, i.e.
block k of philox_host.raw_stream at offset (STREAM_SIM_START << 32) | e, handed to the kind's start (csrc/group_env.h):
  Pendulum-v1               theta = -pi + 2 pi u(c0, c1), theta_dot = -1 + 2 u(c2, c3)
  MountainCarContinuous-v0  p = fp32(-0.6 + 0.2 u(c0, c1)), v = 0
with u(hi, lo) = (((hi << 32 | lo) >> 11) + 0.5) / 2^53.  One step is the host environment's own step() from the given state."""
import numpy as np

from rlrep_amd.utils import philox_host

STREAM_SIM_START = 0xE3000000
PENDULUM, MOUNTAIN_CAR = 0, 2                       # include/rlrep.h RLREP_ENV_*
LIMIT = {PENDULUM: 200, MOUNTAIN_CAR: 999}
S = {PENDULUM: 3, MOUNTAIN_CAR: 2}


def start_block(seed, e, k):
    """uint32[4]: the Philox block of start state k of environment e"""
    off = (STREAM_SIM_START << 32) | int(e)
    return philox_host.raw_stream(4 * (int(k) + 1), seed, off)[4 * int(k):]


def u01d(hi, lo):
    """env_u01d: 53 bits of two words, in (0, 1)"""
    return (float(((int(hi) << 32) | int(lo)) >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def start_state(kind, seed, e, k):
    """(x0, x1) float64: start state k of environment e"""
    c = start_block(seed, e, k)
    if kind == PENDULUM:
        return -np.pi + 2.0 * np.pi * u01d(c[0], c[1]), -1.0 + 2.0 * u01d(c[2], c[3])
    return float(np.float32(-0.6 + 0.2 * u01d(c[0], c[1]))), 0.0


def observe(kind, x0, x1):
    """float32[S]: the observation of state (x0, x1) as the host environment returns it"""
    if kind == PENDULUM:
        return np.array([np.cos(x0), np.sin(x0), x1], np.float32)
    return np.array([x0, x1], np.float32)


def host_step(kind, x0, x1, a, t):
    """the host environment's step() from state (x0, x1) at episode step t with the raw action a -> dict(obs float32[S], reward float32,
    done_bool float (main.py's rule: a goal before the limit's step), ended bool (the goal or the time limit), state (x0', x1'))"""
    if kind == PENDULUM:
        from rlrep_amd.envs.pendulum import PendulumEnv
        env = PendulumEnv()
        env._th, env._thd, env._t = float(x0), float(x1), int(t)
        obs, rew, done, _ = env.step(np.asarray([a], np.float32))
        return dict(obs=obs, reward=np.float32(rew), done_bool=0.0, ended=bool(done), state=(float(env._th), float(env._thd)))
    from rlrep_amd.envs.mountain_car import MountainCarContinuousEnv
    env = MountainCarContinuousEnv()
    env._p, env._v, env._t = float(x0), float(x1), int(t)
    obs, rew, done, _ = env.step(np.asarray([a], np.float32))
    goal = bool(env._unrounded[0] >= 0.45 and env._unrounded[1] >= 0.0)
    return dict(obs=obs, reward=np.float32(rew), done_bool=float(goal and t + 1 < LIMIT[kind]), ended=bool(done), state=(float(env._p), float(env._v)))
