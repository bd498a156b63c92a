"""MountainCarContinuous-v0, host side: the NumPy environment (rlrep_amd/envs/mountain_car.py) against fixed cases of the public
specification, the cases tests/test_device_env_mountaincar.py compares the device step with, the launcher's refusals and the ABI of the
second device-environment kind.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from seed_group_util import run_launcher

F32 = lambda x: float(np.float32(x))  # noqa: E731


def _at(p, v, t=0):
    from rlrep_amd.envs.mountain_car import MountainCarContinuousEnv
    env = MountainCarContinuousEnv()
    env._p, env._v, env._t = F32(p), F32(v), t
    return env


def _rollout(env, policy):
    """(steps, return, last reward) of one episode of `policy(obs)` from where env stands"""
    obs, total, n = env._obs(), 0.0, 0
    while True:
        obs, r, done, _ = env.step(np.array([policy(obs)], np.float32))
        total, n = total + r, n + 1
        if done:
            return n, total, r


def test_make_builds_the_environment_without_gym():
    from rlrep_amd import envs
    env = envs.make('MountainCarContinuous-v0')
    assert type(env).__name__ == 'MountainCarContinuousEnv' and env._max_episode_steps == 999
    assert env.observation_space.shape == (2,) and env.action_space.shape == (1,)
    assert env.action_space.low.tolist() == [-1.0] and env.action_space.high.tolist() == [1.0]
    assert env.seed(5) == [5]
    a = env.reset()
    env.seed(5)
    b = env.reset()
    assert a.dtype == np.float32 and a.shape == (2,) and np.array_equal(a, b) and -0.6 <= a[0] <= -0.4 and a[1] == 0.0
    assert -1.0 <= env.action_space.sample()[0] <= 1.0
    assert type(envs.make('Pendulum-v1')).__name__ == 'PendulumEnv'
    try:
        import gym  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match='Pendulum-v1 and MountainCarContinuous-v0 are built in'):
            envs.make('HalfCheetah-v4')


def test_fixed_steps_of_the_specification():
    env = _at(0.44, 0.05)
    obs, r, done, info = env.step(np.array([1.0], np.float32))
    assert done and r == 100.0 - 0.1 and info == {} and obs.dtype == np.float32 and obs[0] >= 0.45 and obs[1] > 0
    env = _at(-1.2, -0.01)
    obs, r, done, _ = env.step(np.array([-1.0], np.float32))
    assert obs.tolist() == [np.float32(-1.2), 0.0] and not done and r == -0.1 and (env._p, env._v) == (F32(-1.2), 0.0)
    # the state is what the observation shows
    env = _at(-0.5, 0.0)
    obs, _, _, _ = env.step(np.array([0.3], np.float32))
    assert (env._p, env._v) == (float(obs[0]), float(obs[1])) and env._unrounded != (env._p, env._v)
    # the reward takes the RAW action, the dynamics the clipped one
    a, b = _at(-0.5, 0.0), _at(-0.5, 0.0)
    oa, ra, _, _ = a.step(np.array([3.0], np.float32))
    ob, rb, _, _ = b.step(np.array([1.0], np.float32))
    assert np.array_equal(oa, ob) and ra == -0.1 * 9.0 and rb == -0.1
    # the time limit is a `done` of its own
    env = _at(-0.5, 0.0, t=998)
    assert env.step(np.array([0.0], np.float32))[2] is True
    env = _at(-0.5, 0.0, t=997)
    assert env.step(np.array([0.0], np.float32))[2] is False


def test_pushing_right_never_arrives_and_chasing_the_velocity_does():
    n, total, last = _rollout(_at(-0.5, 0.0), lambda obs: 1.0)
    assert n == 999 and last == -0.1 and abs(total + 99.9) < 1e-9
    for p0 in np.linspace(-0.6, -0.4, 21):
        n, total, last = _rollout(_at(p0, 0.0), lambda obs: 1.0 if obs[1] > 0 else -1.0)
        assert 70 <= n <= 90 and last == 100.0 - 0.1 and abs(total - (100.0 - 0.1 * n)) < 1e-9 and 91.0 <= total <= 93.0, (p0, n, total)


def test_the_gpu_tests_cases_hit_every_branch_and_stay_clear_of_the_goal_line():
    """What tests/test_device_env_mountaincar.py compares the device step with.  No case may lie where a last-bit difference of the two
    libms' cos could flip `goal`: the fp64 position the goal is decided on is further than 1e-9 from 0.45, and near the goal the velocity is
    further than 1e-9 from 0."""
    import test_device_env_mountaincar as T
    cases = T.mountaincar_dynamics_cases()
    assert 200 <= len(cases) <= 1000
    hit = dict(speed_hi=0, speed_lo=0, wall=0, right=0, action=0, goal=0, goal_on_limit=0, limit=0)
    for p, v, a, t in cases:
        assert p == F32(p) and v == F32(v) and a == F32(a) and 0 <= t < 999
        obs, r, done, goal, done_bool, (pu, vu) = T.host_step(p, v, a, t)
        assert np.all(np.isfinite(obs)) and np.isfinite(r)
        assert abs(pu - 0.45) > 1e-9 and (pu < 0.44 or abs(vu) > 1e-9), (p, v, a, t, pu, vu)
        assert done == (goal or t == 998) and done_bool == (1.0 if goal and t < 998 else 0.0)
        hit['speed_hi'] += vu == 0.07
        hit['speed_lo'] += vu == -0.07
        hit['wall'] += pu == -1.2 and vu == 0.0 and v < 0
        hit['right'] += pu == 0.6
        hit['action'] += abs(a) > 1.0
        hit['goal'] += goal and t < 998
        hit['goal_on_limit'] += goal and t == 998
        hit['limit'] += (not goal) and t == 998
    assert all(n >= 3 for n in hit.values()), hit


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------
def test_launcher_refusals():
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'MountainCarContinuous-v0', '--device-env'])
    assert '--device-env' in str(e.value) and 'seed group' in str(e.value) and '--seeds' in str(e.value)
    with pytest.raises(SystemExit, match='sac and ctrlsac only'):
        run_launcher(['--alg', 'vlsac', '--env', 'MountainCarContinuous-v0', '--seeds', '0,1', '--device-env'])
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'HalfCheetah-v4', '--seeds', '0,1', '--device-env'])
    assert 'only Pendulum-v1' in str(e.value) and 'MountainCarContinuous-v0' in str(e.value) and 'HalfCheetah-v4' in str(e.value)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------
def test_kind_two_is_built_and_the_abi_is_unchanged():
    import re
    from rlrep_amd import _lib
    from rlrep_amd.envs import device
    lib = _lib.lib
    out = C.c_void_p()
    assert lib.rlrep_group_env_create(None, 2, C.byref(out)) == -1
    msg = lib.rlrep_last_error().decode()
    assert 'null' in msg and 'not built' not in msg and not out.value                  # refused for the null agent, not for the kind
    assert lib.rlrep_group_env_create(None, 1, C.byref(out)) == -1 and 'kind 1 is not built' in lib.rlrep_last_error().decode()
    assert lib.rlrep_abi_version() == 4
    assert re.search(r'#define\s+RLREP_ENV_MOUNTAIN_CAR_CONTINUOUS\s+2\b', open(_lib.HEADER_PATH).read())
    assert device.KIND_MOUNTAIN_CAR_CONTINUOUS == 2 and device.KIND_PENDULUM == 0
    assert issubclass(device.DeviceMountainCarGroup, device.DeviceEnvGroup) and issubclass(device.DevicePendulumGroup, device.DeviceEnvGroup)
    assert device.DeviceMountainCarGroup.max_episode_steps == 999 and device.DevicePendulumGroup.max_episode_steps == 200
    assert device.device_class('MountainCarContinuous-v0') is device.DeviceMountainCarGroup and device.device_class('HalfCheetah-v4') is None
    assert device.RECORD_DTYPE == np.dtype([('theta', '<f8'), ('theta_dot', '<f8'), ('episode_return', '<f8'), ('ring_ptr', '<i8'), ('nsteps', '<i8'),
                                            ('t', '<i4'), ('ring_size', '<i4'), ('episodes_done', '<i4'), ('force', '<i4'), ('force_action', '<f4'),
                                            ('act', '<f4'), ('obs', '<f4', (4,)), ('returns', '<f8', (16,)), ('pad', '<f8', (6,))])
