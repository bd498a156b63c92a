"""The device environment of a single agent, host side: the rlrep_env_* entry points are declared, bound and exported with the signatures
include/rlrep.h states, they refuse what they cannot run before they touch a device, main.py checks --device-loop before the GPU and leaves
--device-env as it was, and ReplayBuffer hands its cursor over and takes it back.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from seed_group_util import run_launcher
from test_device_env_cpu import CTYPE, _header_prototype

ENTRY_POINTS = {
    'rlrep_env_create': ('int32_t', ['rlrep_agent*', 'int32_t', 'uint64_t', 'rlrep_env**']),
    'rlrep_env_destroy': ('void', ['rlrep_env*']),
    'rlrep_env_reset': ('int32_t', ['rlrep_env*', 'void*']),
    'rlrep_env_step': ('int32_t', ['rlrep_agent*', 'rlrep_env*', 'float*', 'int64_t', 'int32_t*', 'float', 'float', 'float', 'int64_t', 'void*']),
    'rlrep_env_evaluate': ('int32_t', ['rlrep_agent*', 'rlrep_env*', 'int32_t', 'uint64_t', 'double*', 'void*']),
    'rlrep_env_state': ('int32_t', ['rlrep_env*', 'int32_t', 'void*', 'int64_t', 'int32_t', 'void*']),
}


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
    assert 'rlrep_prepare' in declared and _lib.SIGNATURES['rlrep_prepare'] == (C.c_int32, [C.c_void_p, C.c_int32])
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_create_refuses_an_unknown_kind_and_a_null_agent():
    from rlrep_amd import _lib
    lib = _lib.lib
    out = C.c_void_p()
    for kind in (1, -1, 7):
        assert lib.rlrep_env_create(None, kind, 0, C.byref(out)) == -1
        assert f'kind {kind} is not built' in lib.rlrep_last_error().decode() and 'env_create' in lib.rlrep_last_error().decode()
        assert not out.value
    assert lib.rlrep_env_create(None, 0, 0, C.byref(out)) == -1
    assert 'null' in lib.rlrep_last_error().decode() and lib.rlrep_last_error().decode().startswith('env_create')
    assert not out.value
    lib.rlrep_env_destroy(None)                                             # a no-op


def test_other_entry_points_refuse_null_handles_and_name_themselves():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 4)()
    assert lib.rlrep_env_reset(None, None) == -1 and lib.rlrep_last_error().decode().startswith('env_reset:')
    assert lib.rlrep_env_step(None, None, None, 1, None, -2.0, 2.0, 0.01, 0, None) == -1
    assert lib.rlrep_last_error().decode().startswith('env_step:')
    assert lib.rlrep_env_evaluate(None, None, 4, 0, None, None) == -1 and lib.rlrep_last_error().decode().startswith('env_evaluate:')
    assert lib.rlrep_env_state(None, 0, buf, 32, 0, None) == -1 and lib.rlrep_last_error().decode().startswith('env_state:')
    assert lib.rlrep_prepare(None, 64) == -1 and lib.rlrep_last_error().decode().startswith('prepare:')
    # the group's entry points keep their own names in their messages
    assert lib.rlrep_group_env_state(None, 0, buf, 32, 0, None) == -1 and lib.rlrep_last_error().decode().startswith('group_env_state:')


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra, names', [(['--seeds', '0,1'], '--seeds'), (['--sweep', 'lr=1e-4,3e-4'], '--sweep'),
                                          (['--halving-interval', '300'], '--halving-*'), (['--pbt-interval', '300'], '--pbt-*')])
def test_device_loop_is_the_single_agents(extra, names):
    for alg in ('sac', 'vlsac'):
        with pytest.raises(SystemExit) as e:
            run_launcher(['--alg', alg, '--env', 'Pendulum-v1', '--device-loop'] + extra)
        assert '--device-loop' in str(e.value) and names in str(e.value) and '--device-env' in str(e.value)


@pytest.mark.parametrize('alg', ['sac', 'vlsac', 'ctrlsac', 'spedersac', 'diffsrsac'])
def test_device_loop_is_pendulum_and_mountain_car_only(alg):
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', alg, '--env', 'HalfCheetah-v4', '--device-loop'])
    assert '--device-loop' in str(e.value) and 'only Pendulum-v1 and MountainCarContinuous-v0' in str(e.value) and 'HalfCheetah-v4' in str(e.value)


def test_device_env_still_needs_a_seed_group():
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--device-env'])
    assert '--device-env' in str(e.value) and 'seed group' in str(e.value) and '--seeds' in str(e.value)
    with pytest.raises(SystemExit, match='sac and ctrlsac only'):
        run_launcher(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--device-env'])


def test_classes_have_the_device_surface():
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    from rlrep_amd.agent.spedersac.spedersac_agent import SPEDERSACAgent
    from rlrep_amd.agent.diffsrsac.diffsrsac_agent import DIFFSRSACAgent
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.agent.seed_batch import SeedBatchMixin
    from rlrep_amd.envs import device
    for cls in (VLSACAgent, CTRLSACAgent, SPEDERSACAgent, DIFFSRSACAgent):
        assert cls.iterate is SACAgent.iterate and cls.evaluate is SACAgent.evaluate
    assert SACSeedBatch.iterate is SeedBatchMixin.iterate and SACSeedBatch.evaluate is SeedBatchMixin.evaluate      # a group keeps the mixin's
    for name in ('reset', 'state', 'set_state', 'counters', 'set_counters', 'set_cursor', 'eval_starts', 'returns', 'step', 'evaluate', 'snapshot',
                 'load_snapshot'):
        assert callable(getattr(device.DeviceEnv, name)) and callable(getattr(device.DeviceEnvGroup, name)), name
    assert device.device_class('Pendulum-v1') is device.DevicePendulumGroup and device.device_class('MountainCarContinuous-v0') is device.DeviceMountainCarGroup
    assert device.single_device_class('Pendulum-v1') is device.DevicePendulum
    assert device.single_device_class('MountainCarContinuous-v0') is device.DeviceMountainCar and device.single_device_class('HalfCheetah-v4') is None

    class Plain(object):
        _seed = 0
    with pytest.raises(ValueError, match='needs a seed group'):
        device.DevicePendulumGroup(Plain())
    group = Plain()
    group.R, group.seeds = 2, [0, 1]
    with pytest.raises(ValueError, match='needs a single agent'):
        device.DevicePendulum(group)


# ---- the buffer's cursor ------------------------------------------------------------------------------------------------------------------
class _StubEnv(object):
    """what ReplayBuffer needs of a device environment: set_cursor and state()"""

    def __init__(self):
        from rlrep_amd.envs.device import RECORD_DTYPE
        self.rec = np.zeros(1, RECORD_DTYPE)

    def set_cursor(self, ptr, sizes):
        self.rec['ring_ptr'], self.rec['ring_size'] = int(ptr), np.asarray(sizes, np.int32).reshape(-1)

    def state(self):
        return self.rec.copy()


def _row(k):
    return np.full(3, k), np.full(1, k), np.full(3, k + 1), -float(k), 0.0


def test_replay_buffer_hands_the_cursor_over_and_takes_it_back():
    from rlrep_amd.utils.buffer import ReplayBuffer
    buf = ReplayBuffer(3, 1, max_size=4, device='cpu')
    for k in range(6):
        buf.add(*_row(k))
    buf.adopt_device_cursor()                                               # nothing to adopt: a no-op
    assert buf.ptr == 2 and buf.size == 4
    env = _StubEnv()
    buf.collect_on_device(env)
    assert buf._staged == 0 and buf.ring[0, 0].item() == 4.0 and buf.ring[3, 7].item() == -3.0          # staged rows were flushed
    assert int(env.rec['ring_ptr'][0]) == 2 and int(env.rec['ring_size'][0]) == 4
    buf.collect_on_device(env)                                              # the same environment again: a no-op
    with pytest.raises(RuntimeError, match='another device environment'):
        buf.collect_on_device(_StubEnv())
    with pytest.raises(RuntimeError, match='adopt_device_cursor'):
        buf.add(*_row(9))
    env.rec['ring_ptr'], env.rec['ring_size'] = 3, 4                        # the device wrote one row
    buf.adopt_device_cursor()
    assert buf.ptr == 3 and buf.size == 4
    buf.add(*_row(9))
    buf.flush()
    assert buf.ptr == 0 and buf.ring[3, 0].item() == 9.0 and buf.ring[2, 0].item() == 2.0
    with pytest.raises(ValueError, match='sharded'):
        ReplayBuffer(3, 1, max_size=4, device='cpu', shard=(0, 2)).collect_on_device(_StubEnv())
