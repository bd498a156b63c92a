"""Several device environments per member / agent (num_envs), host side: the create_n / num_envs entry points are declared, bound and exported
with the signatures include/rlrep.h states and refuse what they cannot build before they touch a device, the Python constructors take
`num_envs` and check it without a GPU, main.py checks --num-envs before the GPU, and `start_state` / `explore_words` restate the stream table of
csrc/group_env.h in NumPy on oracle/philox.py (tests/test_device_env_vec.py compares the device with them).  No GPU."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

from seed_group_util import run_launcher
from test_device_env_cpu import CTYPE, _header_prototype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import philox  # noqa: E402

ENTRY_POINTS = {
    'rlrep_group_env_create_n': ('int32_t', ['rlrep_agent*', 'int32_t', 'int32_t', 'rlrep_group_env**']),
    'rlrep_group_env_num_envs': ('int32_t', ['rlrep_group_env*']),
    'rlrep_env_create_n': ('int32_t', ['rlrep_agent*', 'int32_t', 'uint64_t', 'int32_t', 'rlrep_env**']),
    'rlrep_env_num_envs': ('int32_t', ['rlrep_env*']),
}
RL_STREAM_ENV = 0xE0000000              # csrc/group_env.h


# ---- the stream table of csrc/group_env.h, in NumPy ---------------------------------------------------------------------------------------------
def _block(seed, counter, word2):
    """the four words of Philox block (counter, word 2, RL_STREAM_ENV) under key `seed`"""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    ctr = np.array([counter & 0xFFFFFFFF, counter >> 32, word2, RL_STREAM_ENV], np.uint32)
    return [int(w) for w in philox.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))]


def _u01d(hi, lo):
    """env_u01d: (0, 1) from 53 bits of two words"""
    return (float(((hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def start_state(kind, seed, counter, e=0):
    """(x0, x1): the start state of the episode environment `e` of the agent with `seed` begins at step counter `counter` (0: the reset) --
    Env::start of block (seed, counter, word 2 = 2 e + 1, RL_STREAM_ENV).  kind 0: Pendulum-v1 (theta, theta_dot), 2: MountainCarContinuous-v0
    (p, v)."""
    c = _block(seed, counter, 2 * int(e) + 1)
    if kind == 0:
        return -np.pi + 2.0 * np.pi * _u01d(c[0], c[1]), -1.0 + 2.0 * _u01d(c[2], c[3])
    if kind == 2:
        return float(np.float32(-0.6 + 0.2 * _u01d(c[0], c[1]))), 0.0
    raise ValueError(kind)


def start_obs(kind, x0, x1):
    """the fp32 observation of state (x0, x1), as the host environments return it"""
    if kind == 0:
        return np.array([np.cos(x0), np.sin(x0), x1], np.float32)
    return np.array([x0, x1], np.float32)


def explore_words(seed, counter, e=0):
    """(word 0, word 1) of the exploration block of environment `e` at step counter `counter`: word 2 = 2 e"""
    c = _block(seed, counter, 2 * int(e))
    return c[0], c[1]


def test_stream_table_environment_0_is_the_single_environment_and_the_others_differ():
    for kind in (0, 2):
        for seed in (0, 5, 2 ** 40 + 3):
            for counter in (0, 199, 2 ** 33):
                # environment 0: words 0 (exploration) and 1 (start state) of the record's counter, as one environment draws them
                c = _block(seed, counter, 1)
                want = ((-np.pi + 2.0 * np.pi * _u01d(c[0], c[1]), -1.0 + 2.0 * _u01d(c[2], c[3])) if kind == 0
                        else (float(np.float32(-0.6 + 0.2 * _u01d(c[0], c[1]))), 0.0))
                assert start_state(kind, seed, counter, 0) == want == start_state(kind, seed, counter)
                assert explore_words(seed, counter, 0) == tuple(_block(seed, counter, 0)[:2])
                starts = [start_state(kind, seed, counter, e) for e in range(64)]
                assert len({s[0] for s in starts}) == 64                    # pairwise different
                assert len({explore_words(seed, counter, e) for e in range(64)}) == 64
                for x0, x1 in starts:
                    if kind == 0:
                        assert -np.pi < x0 < np.pi and -1.0 < x1 < 1.0
                    else:
                        assert float(np.float32(-0.6)) <= x0 <= float(np.float32(-0.4)) and x1 == 0.0 and x0 == float(np.float32(x0))
    # word 2 of the 64 environments' draws stays in [0, 128): nothing else in stream RL_STREAM_ENV
    assert sorted({2 * e + k for e in range(64) for k in (0, 1)}) == list(range(128))
    # the same block through the oracle's stream layout: offset = word 2 | (word 3 ^ stream) << 32, block q = counter
    assert _block(7, 3, 5) == [int(w) for w in philox.raw_stream(16, 7, 5, RL_STREAM_ENV)[12:16]]


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported_with_the_stated_signatures():
    from rlrep_amd import _lib
    declared = set(_lib.declared_symbols())
    for name, (res, params) in ENTRY_POINTS.items():
        assert name in declared and name in _lib.SIGNATURES, name
        assert _header_prototype(name) == (res, params), name
        fn = getattr(_lib.lib, name)                                        # exported
        bres, bargs = _lib.SIGNATURES[name]
        assert bres is CTYPE[res] and fn.restype is bres, name
        assert len(bargs) == len(params) == len(fn.argtypes), name
        for b, prm in zip(bargs, params):
            if prm.endswith('*'):
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, prm)
            else:
                assert b is CTYPE[prm], (name, prm)
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_create_n_refuses_kind_num_envs_and_a_null_agent_before_any_launch():
    from rlrep_amd import _lib
    lib = _lib.lib
    forms = (('group_env_create_n', lambda kind, E, out: lib.rlrep_group_env_create_n(None, kind, E, C.byref(out))),
             ('env_create_n', lambda kind, E, out: lib.rlrep_env_create_n(None, kind, 0, E, C.byref(out))))
    for name, create in forms:
        out = C.c_void_p()
        for kind in (1, -1, 7):
            assert create(kind, 4, out) == -1
            msg = lib.rlrep_last_error().decode()
            assert f'kind {kind} is not built (0 = Pendulum-v1, 2 = MountainCarContinuous-v0)' in msg and msg.startswith(name + ':'), msg
        for E in (0, -1, 65):
            assert create(0, E, out) == -1
            msg = lib.rlrep_last_error().decode()
            assert 'num_envs' in msg and str(E) in msg and msg.startswith(name + ':'), msg
        for E in (1, 4, 64):
            assert create(0, E, out) == -1 and create(2, E, out) == -1
            msg = lib.rlrep_last_error().decode()
            assert 'null' in msg and 'num_envs' not in msg and 'not built' not in msg and msg.startswith(name + ':'), msg
        assert not out.value
    assert lib.rlrep_group_env_num_envs(None) == 0 and lib.rlrep_env_num_envs(None) == 0
    # the one-environment calls keep their own names
    out = C.c_void_p()
    assert lib.rlrep_group_env_create(None, 0, C.byref(out)) == -1 and lib.rlrep_last_error().decode().startswith('group_env_create:')
    assert lib.rlrep_env_create(None, 0, 0, C.byref(out)) == -1 and lib.rlrep_last_error().decode().startswith('env_create:')


# ---- Python surface ---------------------------------------------------------------------------------------------------------------------------
class _Single(object):
    """a stub single agent, as tests/test_device_env_single_cpu.py builds one: enough for the checks that come before the GPU"""
    _seed = 0


def _stub_group():
    g = _Single()
    g.R, g.seeds = 2, [0, 1]
    return g


def test_constructors_take_num_envs_and_check_it_without_a_gpu():
    from rlrep_amd.envs import device
    assert device.RECORD_DTYPE.itemsize == 256 and device.MAX_ENVS == 64
    classes = (device.DeviceEnvGroup, device.DeviceEnv, device.DevicePendulumGroup, device.DeviceMountainCarGroup, device.DevicePendulum,
               device.DeviceMountainCar)
    for cls in classes:
        prm = inspect.signature(cls.__init__).parameters
        assert 'num_envs' in prm and prm['num_envs'].default == 1, cls
        assert list(prm)[-3:] == ['eps_greedy', 'start_timesteps', 'num_envs'], cls
    for cls, agent in ((device.DevicePendulum, _Single()), (device.DeviceMountainCar, _Single()), (device.DevicePendulumGroup, _stub_group()),
                       (device.DeviceMountainCarGroup, _stub_group())):
        with pytest.raises(ValueError, match='start_timesteps 10 is not a multiple of num_envs 4'):
            cls(agent, start_timesteps=10, num_envs=4)
        for E in (0, -1, 65):
            with pytest.raises(ValueError, match='num_envs .* outside'):
                cls(agent, num_envs=E)
    with pytest.raises(ValueError, match='not a multiple'):
        device.DeviceEnv(_Single(), device.KIND_PENDULUM, 0.0, 10, 4)
    with pytest.raises(ValueError, match='not a multiple'):
        device.DeviceEnvGroup(_stub_group(), device.KIND_MOUNTAIN_CAR_CONTINUOUS, 0.0, 6, num_envs=4)


class _StubEnvN(object):
    """what the replay rings need of a device environment with several environments: num_envs, set_cursor with the capacity, state()"""

    def __init__(self, R, E):
        from rlrep_amd.envs.device import RECORD_DTYPE, _DeviceEnvBase
        self.R, self.num_envs = R, E
        self.rec = np.zeros((R, E), RECORD_DTYPE)
        self._base = _DeviceEnvBase

    def _records_shape(self):
        return (self.R, self.num_envs)

    def state(self):
        return self.rec.copy()

    def _block(self, what, arr, write):
        if write:
            self.rec = arr.reshape(self.rec.shape).copy()
        return arr

    def set_cursor(self, ptr, sizes, capacity=None):
        return self._base.set_cursor(self, ptr, sizes, capacity)


def test_the_rings_hand_every_environment_its_cursor_and_take_environment_0s_back():
    from rlrep_amd.utils.buffer import ReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    buf = ReplayBuffer(3, 1, max_size=7, device='cpu')
    for k in range(5):
        buf.add(np.full(3, k), np.full(1, k), np.full(3, k + 1), -float(k), 0.0)
    env = _StubEnvN(1, 4)
    buf.collect_on_device(env)
    assert env.rec['ring_ptr'].tolist() == [[5, 6, 0, 1]] and env.rec['ring_size'].tolist() == [[5, 5, 5, 5]]        # (ptr + e) mod capacity
    env.rec['ring_ptr'], env.rec['ring_size'] = np.array([[2, 3, 4, 5]]), 7                                         # one step of 4 rows later
    buf.adopt_device_cursor()
    assert buf.ptr == 2 and buf.size == 7
    grp = ReplayBufferGroup(2, 3, 1, max_size=7, device='cpu')
    for k in range(6):
        grp.add(np.full((2, 3), k), np.full((2, 1), k), np.full((2, 3), k + 1), np.full(2, -k), np.zeros(2))
    genv = _StubEnvN(2, 3)
    grp.collect_on_device(genv)
    assert genv.rec['ring_ptr'].tolist() == [[6, 0, 1]] * 2 and genv.rec['ring_size'].tolist() == [[6] * 3] * 2
    genv.rec['ring_ptr'], genv.rec['ring_size'] = np.array([[2, 3, 4]] * 2), 7
    grp.adopt_device_cursor()
    assert grp.ptr == 2 and grp.sizes == [7, 7]
    with pytest.raises(ValueError, match='capacity'):
        _StubEnvN(1, 4).set_cursor(0, [0])                                  # several environments need the ring's capacity


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
def test_num_envs_needs_a_device_flag():
    for extra in ([], ['--seeds', '0,1']):
        with pytest.raises(SystemExit) as e:
            run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--num-envs', '4', '--start_timesteps', '160', '--eval_freq', '160'] + extra)
        assert '--num-envs' in str(e.value) and '--device-env' in str(e.value) and '--device-loop' in str(e.value)


@pytest.mark.parametrize('flags', [['--device-loop'], ['--seeds', '0,1', '--device-env']])
def test_num_envs_is_checked_before_the_gpu(flags):
    base = ['--alg', 'sac', '--env', 'Pendulum-v1'] + flags
    for E in ('0', '65'):
        with pytest.raises(SystemExit) as e:
            run_launcher(base + ['--num-envs', E, '--start_timesteps', '0', '--eval_freq', '130'])
        assert f'--num-envs {E}' in str(e.value) and '[1, 64]' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(base + ['--num-envs', '4', '--start_timesteps', '150', '--eval_freq', '160'])
    assert '--num-envs 4' in str(e.value) and '--start_timesteps 150' in str(e.value) and 'multiple' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(base + ['--num-envs', '4', '--start_timesteps', '160', '--eval_freq', '150'])
    assert '--num-envs 4' in str(e.value) and '--eval_freq 150' in str(e.value) and 'multiple' in str(e.value)


def test_help_states_the_update_ratio(capsys):
    with pytest.raises(SystemExit):
        run_launcher(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--num-envs' in text and '1/E updates per transition' in text
