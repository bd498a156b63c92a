"""The fused simulators without a GPU (DESIGN.md 6i "Fused simulators"): the entry points of the C ABI are declared, bound and exported and
refuse by name before any launch, the ctypes mirror of rlrep_sim_state has the library's size, FusedSim and main.py --fused-sim refuse what
they cannot run before anything touches the GPU, and the restated start states lie where the kinds reset.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import fused_sim_reference as ref
from seed_group_util import run_launcher
from test_device_env_cpu import CTYPE, _header_prototype

RLREP_ERR_ARG = -1
SIM = 'rlrep_sim_state*'
ENTRY_POINTS = {
    'rlrep_sim_state_bytes': ('int32_t', ['void']),
    'rlrep_sim_start': ('int32_t', [SIM, 'void*']),
    'rlrep_sim_step': ('int32_t', [SIM, 'float*', 'int64_t', 'float*', 'float*', 'float*', 'void*']),
    'rlrep_sim_step_append_ctl': ('int32_t', [SIM, 'float*', 'int64_t', 'float*', 'int64_t', 'int32_t', 'int32_t*', 'int64_t*', 'void*']),
}


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_and_exported():
    from rlrep_amd import _lib
    declared = set(_lib.declared_symbols())
    for name, (res, params) in ENTRY_POINTS.items():
        assert name in declared and name in _lib.SIGNATURES, name
        assert _header_prototype(name) == (res, params), name
        fn = getattr(_lib.lib, name)                                        # exported
        bres, bargs = _lib.SIGNATURES[name]
        assert bres is CTYPE[res] and fn.restype is bres, name
        params = [] if params == ['void'] else params
        assert len(bargs) == len(params) == len(fn.argtypes or ()), name
        for b, prm in zip(bargs, params):
            if prm.endswith('*'):
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, prm)
            else:
                assert b is CTYPE[prm], (name, prm)
    assert 'define RLREP_SIM_MAX_ENVS 65536' in ' '.join(open(_lib.HEADER_PATH).read().split())
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_the_ctypes_mirror_has_the_librarys_size_and_the_headers_fields():
    import re
    from rlrep_amd import _lib
    assert C.sizeof(_lib.SimState) == _lib.lib.rlrep_sim_state_bytes() == 88
    src = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    body = re.search(r'typedef struct rlrep_sim_state \{(.*?)\} rlrep_sim_state;', src, flags=re.S).group(1)
    names = re.findall(r'(\w+)\s*(?=[;,])', body)                          # the identifier in front of every `,` and `;`
    assert names == [n for n, _ in _lib.SimState._fields_], names


def _state(n=4, kind=0, **null):
    """a rlrep_sim_state whose arrays are one host buffer (no refusal may dereference them), and what keeps it alive"""
    from rlrep_amd import _lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    st = _lib.SimState(kind=kind, n=n, seed=1, auto_restart=1, **{k: (None if null.get(k) else p) for k in ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')})
    return st, buf


def test_every_refusal_names_its_entry_point_and_launches_nothing():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    cap = 10
    n0 = lib.rlrep_launch_counter()

    def start(st):
        return lib.rlrep_sim_start(C.byref(st) if st is not None else None, None)

    def step(st, act=p, ld=1, nxt=p, rew=p, done=p):
        return lib.rlrep_sim_step(C.byref(st) if st is not None else None, act, ld, nxt, rew, done, None)

    def app(st, act=p, ld=1, ring=p, max_size=cap, row=None, ctl=p):
        row = {0: 9, 2: 7}.get(st.kind if st is not None else 0, 9) if row is None else row
        return lib.rlrep_sim_step_append_ctl(C.byref(st) if st is not None else None, act, ld, ring, max_size, row, None, ctl, None)

    def refused(rc, who, *words):
        msg = lib.rlrep_last_error().decode()
        assert rc == RLREP_ERR_ARG and msg.startswith(who + ':') and all(w in msg for w in words), (who, rc, msg)

    for who, call in (('sim_start', start), ('sim_step', step), ('sim_step_append_ctl', app)):
        refused(call(None), who, 'null')
        for field in ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs'):
            refused(call(_state(**{field: True})[0]), who, 'null')
        for kind in (1, 3, -1):
            refused(call(_state(kind=kind)[0]), who, f'kind {kind}')
        for n in (0, -1, 65537):
            refused(call(_state(n=n)[0]), who, f'n {n}', '[1, 65536]')
    for kind in (0, 2):
        st = _state(kind=kind)[0]
        for null in ('act', 'nxt', 'rew', 'done'):
            refused(step(st, **{null: None}), 'sim_step', 'null')
        refused(step(st, ld=0), 'sim_step', 'ld_act 0')
        for null in ('act', 'ring', 'ctl'):
            refused(app(st, **{null: None}), 'sim_step_append_ctl', 'null')
        refused(app(st, ld=0), 'sim_step_append_ctl', 'ld_act 0')
        refused(app(_state(n=cap + 1, kind=kind)[0]), 'sim_step_append_ctl', f'n {cap + 1}', 'max_size')
        good = 9 if kind == 0 else 7
        for row in (good - 1, good + 1, 16 - good):
            refused(app(st, row=row), 'sim_step_append_ctl', f'row {row}', '2 S + A + 2')
    assert lib.rlrep_launch_counter() == n0


# ---- Python -----------------------------------------------------------------------------------------------------------------------------------
def test_fused_sim_refuses_before_any_device_allocation(monkeypatch):
    import torch
    from rlrep_amd.envs import fused_sim

    def never(*a, **k):
        raise AssertionError('allocated')
    for name in ('zeros', 'full', 'empty'):
        monkeypatch.setattr(torch, name, never)
    for n in (0, -3, 65537):
        with pytest.raises(ValueError, match=f'num_envs {n} outside'):
            fused_sim.FusedSim('Pendulum-v1', n)
        with pytest.raises(ValueError, match='outside'):
            fused_sim.FusedMountainCar(n)
    for kind in ('HalfCheetah-v4', 1, None):
        with pytest.raises(ValueError, match='Pendulum-v1.*MountainCarContinuous-v0'):
            fused_sim.FusedSim(kind, 8)
    assert fused_sim.sim_kind('Pendulum-v1') == fused_sim.sim_kind(0) == 0 and fused_sim.sim_kind('MountainCarContinuous-v0') == fused_sim.sim_kind(2) == 2
    assert issubclass(fused_sim.FusedPendulum, fused_sim.FusedSim) and issubclass(fused_sim.FusedMountainCar, fused_sim.FusedSim)
    assert fused_sim.FusedSim.step is fused_sim.FusedSim.step_ and callable(fused_sim.FusedSim.step_append_)
    assert not hasattr(fused_sim.FusedSim, 'graph_generators')


def test_sim_loop_takes_fused_append():
    from rlrep_amd.envs.sim_loop import SimLoop
    prm = inspect.signature(SimLoop.__init__).parameters
    assert 'fused_append' in prm and prm['fused_append'].default is True
    assert 'step_append_' in __import__('rlrep_amd.envs.sim_loop', fromlist=['x']).__doc__


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'sac', '--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '320']


def test_fused_sim_launcher_refusals_come_before_the_gpu(monkeypatch):
    from rlrep_amd import main

    def never(*a, **k):
        raise AssertionError('reached the environments')
    monkeypatch.setattr(main.envs, 'make', never)
    monkeypatch.setattr(main, 'build_agent', never)
    for extra in ([], ['--torch-envs', '8'], ['--sim-graph'], ['--device-loop'], ['--host-envs', '4']):
        with pytest.raises(SystemExit) as e:
            run_launcher(BASE + ['--env', 'Pendulum-v1', '--fused-sim'] + extra)
        assert str(e.value).startswith('--fused-sim:') and '--torch-envs N --sim-graph' in str(e.value), (extra, str(e.value))
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--env', 'HalfCheetah-v4', '--torch-envs', '8', '--sim-graph', '--fused-sim'])
    assert str(e.value).startswith('--fused-sim:') and 'Pendulum-v1' in str(e.value) and 'MountainCarContinuous-v0' in str(e.value) and 'HalfCheetah-v4' in str(e.value)
    # without the flag --torch-envs says what it said
    for extra in ([], ['--sim-graph']):
        with pytest.raises(SystemExit) as e:
            run_launcher(BASE + ['--env', 'MountainCarContinuous-v0', '--torch-envs', '8'] + extra)
        assert str(e.value) == '--torch-envs 8: the example simulator is Pendulum-v1 (got --env MountainCarContinuous-v0)'
    # with it --torch-envs keeps its other checks
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'MountainCarContinuous-v0', '--torch-envs', '8', '--sim-graph', '--fused-sim', '--start_timesteps', '150',
                      '--eval_freq', '160'])
    assert '--torch-envs 8' in str(e.value) and '--start_timesteps 150' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--env', 'Pendulum-v1', '--torch-envs', '8', '--sim-graph', '--fused-sim', '--per'])
    assert '--sim-graph' in str(e.value) and '--per' in str(e.value)


def test_fused_sim_takes_its_own_loop(monkeypatch, tmp_path):
    from rlrep_amd import main

    class Reached(Exception):
        pass

    def loop(name):
        def f(*a, **k):
            raise Reached(name)
        return f
    monkeypatch.setattr(main, '_fused_sim_loop', loop('fused'))
    monkeypatch.setattr(main, '_sim_graph_loop', loop('graph'))
    monkeypatch.setattr(main, 'build_agent', lambda *a, **k: None)
    monkeypatch.setattr(main.buffer, 'ReplayBuffer', lambda *a, **k: None)
    for env in ('Pendulum-v1', 'MountainCarContinuous-v0'):
        with pytest.raises(Reached, match='fused'):
            main.run(BASE + ['--env', env, '--torch-envs', '8', '--sim-graph', '--fused-sim', '--log_root', str(tmp_path)])
    with pytest.raises(Reached, match='graph'):
        main.run(BASE + ['--env', 'Pendulum-v1', '--torch-envs', '8', '--sim-graph', '--log_root', str(tmp_path)])


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def test_restated_start_states_lie_in_the_reset_ranges_and_differ():
    f32 = np.float32
    for seed in (0, 5):
        pend = np.array([[ref.start_state(ref.PENDULUM, seed, e, k) for k in range(4)] for e in (0, 1, 255, 256, 65535)])
        assert np.all(np.abs(pend[..., 0]) < np.pi) and np.all(np.abs(pend[..., 1]) < 1.0)
        assert len(np.unique(pend[..., 0])) == pend[..., 0].size and len(np.unique(pend[..., 1])) == pend[..., 1].size       # across e and across k
        car = np.array([[ref.start_state(ref.MOUNTAIN_CAR, seed, e, k) for k in range(4)] for e in (0, 1, 255, 256, 65535)])
        assert np.all(car[..., 0] >= float(f32(-0.6))) and np.all(car[..., 0] <= float(f32(-0.4))) and np.all(car[..., 1] == 0.0)
        assert np.array_equal(car[..., 0], car[..., 0].astype(f32).astype(np.float64))                                        # fp32 values
        assert len(np.unique(car[..., 0])) == car[..., 0].size
    assert ref.start_state(ref.PENDULUM, 0, 3, 2) != ref.start_state(ref.PENDULUM, 5, 3, 2)
    # the block is block k of the stream whose counter words 2-3 are (e, STREAM_SIM_START)
    from rlrep_amd.utils import philox_host
    assert np.array_equal(ref.start_block(7, 9, 3), philox_host.raw_stream(16, 7, (0xE3000000 << 32) | 9)[12:])
    assert ref.u01d(0, 0) == 0.5 / 2 ** 53 and ref.u01d(0xFFFFFFFF, 0xFFFFF7FF) < 1.0
    assert ref.u01d(0xFFFFFFFF, 0xFFFFFFFF) == 1.0                          # (2^53 - 1) + 0.5 rounds to 2^53 in float64, as on the device
    # one step of the restated environments, on a case worked by hand: MountainCar one step from the goal, before and on the limit's step
    one = ref.host_step(ref.MOUNTAIN_CAR, float(f32(0.44)), float(f32(0.05)), 1.0, 10)
    assert one['ended'] and one['done_bool'] == 1.0 and one['reward'] == f32(100.0 - 0.1)
    lim = ref.host_step(ref.MOUNTAIN_CAR, float(f32(0.44)), float(f32(0.05)), 1.0, 998)
    assert lim['ended'] and lim['done_bool'] == 0.0 and lim['reward'] == one['reward']
    out = ref.host_step(ref.PENDULUM, 0.0, 0.0, 0.0, 199)
    assert out['ended'] and out['done_bool'] == 0.0 and out['reward'] == 0.0 and np.array_equal(out['obs'], np.array([1, 0, 0], f32))
