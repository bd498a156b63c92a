"""Simulator kinds compiled at run time, without a GPU (csrc/sim_jit.h, csrc/sim_jit.hip, envs/fused_sim.py SimKind /
CustomFusedSim, envs/point_mass.py, main.py --fused-sim-source): the entry points are declared, bound and exported; every RLREP_ERR_ARG refusal
names its entry point and comes before any GPU call; the launcher refuses the flag without its three companions; the NumPy point mass on
hand-worked steps and in a random rollout; the text the library assembles; both example kinds compiled for gfx950 by the run-time compiler
with no device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import sim_kind_reference as kref
from seed_group_util import run_launcher

RLREP_ERR_ARG, RLREP_ERR_HIP = -1, -2
NEW = ('rlrep_simx_state_bytes', 'rlrep_sim_kind_compile', 'rlrep_sim_kind_destroy', 'rlrep_sim_kind_info', 'rlrep_sim_kind_source', 'rlrep_sim_kind_code',
       'rlrep_simx_start', 'rlrep_simx_step', 'rlrep_simx_step_append_ctl')


def _err():
    from rlrep_amd._lib import lib
    return (lib.rlrep_last_error() or b'').decode()


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_and_exported():
    from rlrep_amd import _lib
    declared = set(_lib.declared_symbols())
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        getattr(_lib.lib, name)
    assert _lib.lib.rlrep_abi_version() == 4                                # additive
    assert C.sizeof(_lib.SimxState) == _lib.lib.rlrep_simx_state_bytes() == 72
    from rlrep_amd.envs import fused_sim
    src = ' '.join(open(_lib.HEADER_PATH).read().split())
    for name, v in (('NX', fused_sim.MAX_NX), ('S', fused_sim.MAX_S), ('A', fused_sim.MAX_A)):
        assert f'define RLREP_SIMX_MAX_{name} {v}' in src
    assert (fused_sim.MAX_NX, fused_sim.MAX_S, fused_sim.MAX_A) == (8, 16, 8)


def test_the_description_is_refused_by_name_before_any_gpu_call():
    from rlrep_amd._lib import lib
    text = kref.source('point_mass')
    out = C.c_void_p()
    cases = [(dict(source=None), 'source text is null or empty'), (dict(source=''), 'source text is null or empty'),
             (dict(S=0), 'S 0 outside [1, 16]'), (dict(S=17), 'S 17 outside [1, 16]'), (dict(A=0), 'A 0 outside [1, 8]'), (dict(A=9), 'A 9 outside [1, 8]'),
             (dict(NX=0), 'NX 0 outside [1, 8]'), (dict(NX=9), 'NX 9 outside [1, 8]'), (dict(limit=0), 'limit 0 below 1'),
             (dict(name=None), 'C identifier'), (dict(name='not a name'), 'C identifier')]
    for over, what in cases:
        d, keep = kref.desc(text, **over)
        assert lib.rlrep_sim_kind_compile(C.byref(d), C.byref(out)) == RLREP_ERR_ARG, over
        assert _err().startswith('sim_kind_compile:') and what in _err(), (over, _err())
        assert lib.rlrep_sim_kind_source(C.byref(d), None, 0) == RLREP_ERR_ARG and _err().startswith('sim_kind_source:')
    assert lib.rlrep_sim_kind_compile(None, C.byref(out)) == RLREP_ERR_ARG and _err().startswith('sim_kind_compile:') and 'null description' in _err()
    d, keep = kref.desc(text)
    assert lib.rlrep_sim_kind_compile(C.byref(d), None) == RLREP_ERR_ARG and _err().startswith('sim_kind_compile:') and 'kind_out' in _err()
    assert lib.rlrep_sim_kind_info(None, None) == RLREP_ERR_ARG and _err().startswith('sim_kind_info:')
    lib.rlrep_sim_kind_destroy(None)                                        # a null kind is nothing to destroy


def _kind(S=4, A=2):
    """a stand-in for a compiled kind: a kind's record begins with its rlrep_sim_kind_info_t (include/rlrep.h), and the refusals read nothing else"""
    from rlrep_amd._lib import SimKindInfo
    rec = (SimKindInfo * 2)()
    rec[0].S, rec[0].A, rec[0].NX, rec[0].limit, rec[0].terminates = S, A, 4, 100, 1
    return C.cast(rec, C.c_void_p), rec


def _state(n=4, **null):
    from rlrep_amd import _lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    names = ('x', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')
    return _lib.SimxState(n=n, seed=1, auto_restart=1, **{k: (None if null.get(k) else p) for k in names}), buf


def test_every_launch_refusal_names_its_entry_point_and_launches_nothing():
    from rlrep_amd._lib import lib
    kind, rec = _kind()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    n0 = lib.rlrep_launch_counter()
    entry = {'simx_start': lambda k, st, **o: lib.rlrep_simx_start(k, C.byref(st) if st is not None else None, None),
             'simx_step': lambda k, st, act=p, ld=2, nxt=p, r=p, d=p: lib.rlrep_simx_step(k, C.byref(st) if st is not None else None, act, ld, nxt, r, d, None),
             'simx_step_append_ctl': lambda k, st, act=p, ld=2, ring=p, cap=95, row=12, ctl=p: lib.rlrep_simx_step_append_ctl(
                 k, C.byref(st) if st is not None else None, act, ld, ring, cap, row, p, ctl, None)}
    for who, call in entry.items():
        st, keep = _state()
        assert call(None, st) == RLREP_ERR_ARG and _err().startswith(who + ':') and 'null kind' in _err(), (who, _err())
        assert call(kind, None) == RLREP_ERR_ARG and _err().startswith(who + ':') and 'null simulator state or array' in _err()
        for name in ('x', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs'):
            st, keep = _state(**{name: True})
            assert call(kind, st) == RLREP_ERR_ARG and _err().startswith(who + ':') and 'null simulator state or array' in _err(), (who, name)
        for n in (0, -3, 65537):
            st, keep = _state(n=n)
            assert call(kind, st) == RLREP_ERR_ARG and _err() == f'{who}: n {n} outside [1, 65536]', (who, n, _err())
    st, keep = _state()
    for who in ('simx_step', 'simx_step_append_ctl'):
        assert entry[who](kind, st, ld=1) == RLREP_ERR_ARG and _err() == f'{who}: ld_act 1 below the kind\'s A 2'
        assert entry[who](kind, st, act=None) == RLREP_ERR_ARG and _err().startswith(who + ':') and 'null actions' in _err()
    for out in ('nxt', 'r', 'd'):
        assert entry['simx_step'](kind, st, **{out: None}) == RLREP_ERR_ARG and _err().startswith('simx_step:') and 'output array' in _err()
    for name in ('ring', 'ctl'):
        assert entry['simx_step_append_ctl'](kind, st, **{name: None}) == RLREP_ERR_ARG and _err().startswith('simx_step_append_ctl:')
    assert entry['simx_step_append_ctl'](kind, st, cap=3) == RLREP_ERR_ARG and _err() == 'simx_step_append_ctl: n 4 outside [1, max_size 3]'
    assert entry['simx_step_append_ctl'](kind, st, cap=0) == RLREP_ERR_ARG and _err().startswith('simx_step_append_ctl: n 4 outside')
    for row in (11, 13, 9):
        assert entry['simx_step_append_ctl'](kind, st, row=row) == RLREP_ERR_ARG
        assert _err() == f'simx_step_append_ctl: row {row} is not 2 S + A + 2 (S 4, A 2)'
    assert lib.rlrep_launch_counter() == n0                                 # nothing was launched


# ---- the assembled text -----------------------------------------------------------------------------------------------------------------------
def test_the_compile_text_holds_the_header_the_struct_and_the_static_asserts():
    import os
    from rlrep_amd.envs import fused_sim
    for which, name, (S, A, NX, LIMIT, TERM) in (('pendulum', 'KindPendulum', (3, 1, 2, 200, 'false')), ('point_mass', 'KindPointMass', (4, 4 - 2, 4, 100, 'true'))):
        text = kref.source(which)
        d, keep = kref.desc(text)
        full = fused_sim.assembled_text(d)
        header = open(os.path.join(os.path.dirname(fused_sim.__file__), '..', 'csrc', 'sim_jit.h')).read()
        assert full.startswith(header) and text in full and full.index(text) > len(header) - 1
        tail = full[full.index(text) + len(text):]
        for const, v in (('S', S), ('A', A), ('NX', NX), ('LIMIT', LIMIT), ('TERMINATES', TERM)):
            assert f'static_assert({name}::{const} == {v},' in tail, (which, const)
        assert tail.rstrip().endswith(f'RL_SIMX_KERNELS({name}, jit)')
        assert 'asm' not in full.replace('assemble', '')                    # no inline assembly in what is compiled
    k = fused_sim.kind_constants(kref.source('point_mass'))
    assert k == dict(name='KindPointMass', S=4, A=2, NX=4, limit=100, terminates=True, action_range=(-1.0, 1.0))
    assert fused_sim.kind_constants(kref.source('pendulum'))['action_range'] == (-2.0, 2.0)
    assert fused_sim.kind_constants('struct K { static constexpr int S = N_OBS; };') == dict(name='K', S=None, A=None, NX=None, limit=None, terminates=None,
                                                                                               action_range=(-1.0, 1.0))


def _code(d):
    from rlrep_amd._lib import lib
    n = C.c_int64()
    rc = lib.rlrep_sim_kind_code(C.byref(d), b'gfx950', None, 0, C.byref(n))
    return rc, n.value


def test_the_run_time_compiler_compiles_both_examples_for_gfx950_without_a_device():
    """hiprtc takes an explicit --offload-arch and needs no device for the compile itself; the load is the GPU tests'"""
    from rlrep_amd._lib import lib
    for which in ('pendulum', 'point_mass'):
        d, keep = kref.desc(kref.source(which))
        rc, n = _code(d)
        assert rc == 0 and n > 1000, (which, rc, _err())
        code = C.create_string_buffer(n)
        m = C.c_int64()
        assert lib.rlrep_sim_kind_code(C.byref(d), b'gfx950', code, n, C.byref(m)) == 0 and m.value == n
        assert code.raw[:4] == b'\x7fELF'
        for sym in (b'simx_start_jit', b'simx_step_jit', b'simx_step_ctl_jit'):
            assert sym in code.raw, (which, sym)


def test_a_compile_failure_carries_the_users_identifier_and_constants_are_held_to_the_description():
    text = kref.source('point_mass')
    bad = text.replace('const double d = sqrt', 'const double d = my_own_missing_term + sqrt')
    assert bad != text
    d, keep = kref.desc(bad)
    rc, _ = _code(d)
    assert rc == RLREP_ERR_HIP and _err().startswith('sim_kind_code:') and 'my_own_missing_term' in _err() and 'error' in _err(), _err()
    for over, const in ((dict(S=5), 'S'), (dict(A=1), 'A'), (dict(NX=3), 'NX'), (dict(limit=99), 'LIMIT'), (dict(terminates=False), 'TERMINATES')):
        d, keep = kref.desc(text, **over)
        rc, _ = _code(d)
        assert rc == RLREP_ERR_HIP and f"the struct's {const} differs from the description" in _err(), (over, _err())


# ---- the NumPy point mass ------------------------------------------------------------------------------------------------------------------------
def test_point_mass_twin_on_hand_worked_steps():
    from rlrep_amd.envs import point_mass as pm
    x = np.array([[1.0], [-0.5], [0.0], [0.25]])
    x2, r, goal, wall = pm.step(x, np.array([[0.5, -3.0]], np.float32))    # fx = 0.5, fy clipped to -1
    vx, vy = 0.0 + 0.5 * 0.1, 0.25 + -1.0 * 0.1
    px, py = 1.0 + vx * 0.1, -0.5 + vy * 0.1
    assert x2[:, 0].tolist() == [px, py, vx, vy] and not goal[0] and not wall[0]
    assert r[0] == np.float32(-np.sqrt(px * px + py * py) - 0.01 * (0.25 + 1.0))
    x2, r, goal, wall = pm.step(np.array([[1.95], [0.0], [1.0], [0.0]]), np.array([[1.0, 0.0]], np.float32))     # speed clamp, then the wall
    assert x2[:, 0].tolist() == [2.0, 0.0, 1.0, 0.0] and wall[0] and r[0] == np.float32(-2.0 - 0.01)
    x2, r, goal, wall = pm.step(np.array([[0.05], [0.0], [0.0], [0.0]]), np.zeros((1, 2), np.float32))             # inside the goal radius
    assert goal[0] and r[0] == np.float32(-0.05 + 10.0) and x2[:, 0].tolist() == [0.05, 0.0, 0.0, 0.0]
    x2, r, goal, wall = pm.step(np.array([[0.1], [0.0], [0.0], [0.0]]), np.zeros((1, 2), np.float32))              # on the radius: not inside
    assert not goal[0] and r[0] == np.float32(-0.1)
    for x, a, t, done, ended in kref.FORCED:
        out = pm.step_sim(np.array(x).reshape(4, 1), np.array([t]), np.array([a], np.float32))
        assert out['done'][0] == done and bool(out['ended'][0]) == ended and out['t'][0] == (0 if ended else t + 1), (x, a, t)
        frozen = pm.step_sim(np.array(x).reshape(4, 1), np.array([t]), np.array([a], np.float32), auto_restart=False)
        assert frozen['t'][0] == (-1 if ended else t + 1)
    still = pm.step_sim(np.array(kref.FORCED[0][0]).reshape(4, 1), np.array([-1]), np.zeros((1, 2), np.float32), auto_restart=False)
    assert still['t'][0] == -1 and still['reward'][0] == 0 and still['done'][0] == 0 and still['x'][:, 0].tolist() == list(kref.FORCED[0][0])
    assert pm.observe(np.array(x).reshape(4, 1)).dtype == np.float32 and pm.observe(np.zeros((4, 3))).shape == (3, 4)


def test_point_mass_start_states_and_a_random_rollout_meet_every_end():
    from rlrep_amd.envs import point_mass as pm
    import fused_sim_reference as fref
    seen = set()
    for e in range(4):
        for k in range(3):
            x = pm.start_state(9, e, k)
            assert -1.0 < x[0] < 1.0 and -1.0 < x[1] < 1.0 and x[2] == x[3] == 0.0 and x[0] != x[1]
            seen.add((x[0], x[1]))
            assert np.array_equal(pm.start_block(9, e, k, 0), fref.start_block(9, e, k))     # block 0 is the block the built-in kinds draw
            assert not np.array_equal(pm.start_block(9, e, k, 1), pm.start_block(9, e, k, 0))
    assert len(seen) == 12
    counts = kref.rollout()
    print('point mass rollout:', counts)
    assert all(v >= 3 for v in counts.values()), counts


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'sac', '--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '320']


def test_launcher_refuses_the_flag_without_its_companions_before_the_gpu(monkeypatch, tmp_path):
    import os
    from rlrep_amd import main
    from rlrep_amd.envs import fused_sim

    def never(*a, **k):
        raise AssertionError('reached the environments')
    monkeypatch.setattr(main.envs, 'make', never)
    monkeypatch.setattr(main, 'build_agent', never)
    path = os.path.join(fused_sim.KINDS_DIR, 'point_mass.h')
    have = {'--torch-envs': ['--torch-envs', '8'], '--sim-graph': ['--sim-graph'], '--fused-sim': ['--fused-sim']}
    for missing in have:
        extra = [w for k, v in have.items() if k != missing for w in v]
        with pytest.raises(SystemExit) as e:
            run_launcher(BASE + ['--fused-sim-source', path] + extra)
        assert str(e.value).startswith('--fused-sim-source:') and missing in str(e.value) and '--torch-envs N --sim-graph --fused-sim' in str(e.value), (missing, str(e.value))
    for extra in ([], ['--device-loop'], ['--host-envs', '4'], ['--seeds', '2']):
        with pytest.raises(SystemExit) as e:
            run_launcher(BASE + ['--fused-sim-source', path] + extra)
        assert str(e.value).startswith('--fused-sim-source:'), (extra, str(e.value))
    everything = [w for v in have.values() for w in v]
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--fused-sim-source', str(tmp_path / 'nothing.h')] + everything)
    assert str(e.value).startswith('--fused-sim-source: cannot read')
    open(tmp_path / 'open.h', 'w').write('struct Open { static constexpr int S = N_OBS, A = 1; };')
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--fused-sim-source', str(tmp_path / 'open.h')] + everything)
    assert str(e.value).startswith('--fused-sim-source:') and 'does not spell S, NX, limit, terminates' in str(e.value), str(e.value)


def test_launcher_builds_the_agent_from_the_kinds_dimensions(monkeypatch, tmp_path):
    import os
    from rlrep_amd import main
    from rlrep_amd.envs import fused_sim

    class Reached(Exception):
        pass
    seen = {}

    def build(args, S, A, space):
        seen.update(S=S, A=A, low=space.low.tolist(), high=space.high.tolist())

    def loop(args, agent, replay, ev):
        raise Reached(args.fused_kind['name'])
    monkeypatch.setattr(main.envs, 'make', lambda *a, **k: (_ for _ in ()).throw(AssertionError('made a host environment')))
    monkeypatch.setattr(main, 'build_agent', build)
    monkeypatch.setattr(main.buffer, 'ReplayBuffer', lambda S, A, **k: seen.update(ring=(S, A)))
    monkeypatch.setattr(main, '_fused_sim_loop', loop)
    with pytest.raises(Reached, match='KindPointMass'):
        main.run(BASE + ['--fused-sim-source', os.path.join(fused_sim.KINDS_DIR, 'point_mass.h'), '--torch-envs', '8', '--sim-graph', '--fused-sim',
                         '--log_root', str(tmp_path)])
    assert seen == dict(S=4, A=2, low=[-1.0, -1.0], high=[1.0, 1.0], ring=(4, 2))
