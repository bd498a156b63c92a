"""The one-graph simulator loop of a seed group without a GPU: the entry points of the C ABI are declared, bound and
exported and refuse by name before any launch (what needs a real handle is in tests/test_sim_loop_group.py), the simulator state's ctypes
mirror is the library's, the NumPy restatement of the group's loop record replays a scripted run, and main.py takes --seeds / --sweep with
--torch-envs N --sim-graph --fused-sim and refuses everything it does not run with before the GPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import sim_loop_group_reference as ref
from seed_group_util import run_launcher
from test_device_env_cpu import CTYPE, _header_prototype

RLREP_ERR_ARG = -1
AG, SIM = 'rlrep_agent*', 'rlrep_sim_state*'
ENTRY_POINTS = {
    'rlrep_group_act_device_ctl': ('int32_t', [AG, 'float*', 'int32_t', 'float', 'float', 'float*', 'int64_t*', 'int64_t', 'float', 'int64_t', 'void*']),
    'rlrep_group_replay_add_cols_ctl': ('int32_t', [AG, 'float*', 'int64_t', 'int32_t', 'int32_t', 'int32_t', 'float*', 'int64_t', 'float*', 'int64_t', 'float*',
                                                    'int64_t', 'float*', 'float*', 'int64_t', 'int64_t', 'int32_t*', 'int64_t*', 'void*']),
    'rlrep_group_sim_start': ('int32_t', [AG, SIM, 'uint64_t*', 'void*']),
    'rlrep_group_sim_step': ('int32_t', [AG, SIM, 'uint64_t*', 'float*', 'int64_t', 'float*', 'float*', 'float*', 'void*']),
    'rlrep_group_sim_step_append_ctl': ('int32_t', [AG, SIM, 'uint64_t*', 'float*', 'int64_t', 'float*', 'int64_t', 'int32_t', 'int64_t', 'int32_t*', 'int64_t*',
                                                    'void*']),
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
        assert len(bargs) == len(params) == len(fn.argtypes), name
        for b, prm in zip(bargs, params):
            if prm.endswith('*'):
                assert b is C.c_void_p or issubclass(b, C._Pointer), (name, prm)
            else:
                assert b is CTYPE[prm], (name, prm)
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_the_group_simulator_takes_the_single_simulators_state_mirror():
    from rlrep_amd import _lib
    assert C.sizeof(_lib.SimState) == _lib.lib.rlrep_sim_state_bytes() == 88
    for name in ('rlrep_group_sim_start', 'rlrep_group_sim_step', 'rlrep_group_sim_step_append_ctl'):
        assert _lib.SIGNATURES[name][1][1] is C.POINTER(_lib.SimState), name


def _state(n=4, kind=0, **null):
    from rlrep_amd import _lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    st = _lib.SimState(kind=kind, n=n, seed=1, auto_restart=1, **{k: (None if null.get(k) else p) for k in ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')})
    return st, buf


def _refused(lib, rc, who, *words):
    msg = lib.rlrep_last_error().decode()
    assert rc == RLREP_ERR_ARG and msg.startswith(who + ':') and all(w in msg for w in words), (who, rc, msg)


def test_the_ctl_forms_refuse_by_name_before_any_launch():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 8)()
    p, fake = C.cast(buf, C.c_void_p), C.c_void_p(8)                       # (`fake`: a non-null handle no refusal here may dereference)
    S, A, cap = 3, 1, 10
    row = 2 * S + A + 2
    n0 = lib.rlrep_launch_counter()

    def act(ag=fake, obs=p, rows=4, out=p, ctl=p, max_size=cap, eps=0.0, start=0):
        return lib.rlrep_group_act_device_ctl(ag, obs, rows, -1.0, 1.0, out, ctl, max_size, eps, start, None)
    for null in ('ag', 'obs', 'out', 'ctl'):
        _refused(lib, act(**{null: None}), 'group_act_device_ctl', 'null')
    for rows in (0, -1, 65537):
        _refused(lib, act(rows=rows), 'group_act_device_ctl', f'rows {rows}', '[1, 65536]')
    _refused(lib, act(rows=cap + 1), 'group_act_device_ctl', f'rows {cap + 1}', 'max_size')
    for eps in (-0.1, 1.5, float('nan')):
        _refused(lib, act(eps=eps), 'group_act_device_ctl', 'eps_greedy')
    _refused(lib, act(start=-1), 'group_act_device_ctl', 'start_timesteps')

    def add(ag=fake, ring=p, s=p, a=p, s2=p, r=p, d=p, ctl=p, n=4, row=row, ld_s=S, ld_a=A, ld_s2=S, stride=cap * row):
        return lib.rlrep_group_replay_add_cols_ctl(ag, ring, cap, row, S, A, s, ld_s, a, ld_a, s2, ld_s2, r, d, n, stride, None, ctl, None)
    for null in ('ag', 'ring', 's', 'a', 's2', 'r', 'd', 'ctl'):
        _refused(lib, add(**{null: None}), 'group_replay_add_cols_ctl', 'null')
    for n in (0, -2, cap + 1):
        _refused(lib, add(n=n), 'group_replay_add_cols_ctl', f'n {n}', 'max_size')
    for bad_row in (row - 1, row + 1):
        _refused(lib, add(row=bad_row, stride=cap * bad_row), 'group_replay_add_cols_ctl', f'row {bad_row}', '2 S + A + 2')
    for key, v in (('ld_s', S - 1), ('ld_a', A - 1), ('ld_s2', S - 1)):
        _refused(lib, add(**{key: v}), 'group_replay_add_cols_ctl', 'stride')
    _refused(lib, add(stride=cap * row - 1), 'group_replay_add_cols_ctl', 'ring stride')
    assert lib.rlrep_launch_counter() == n0


def test_the_group_simulator_forms_refuse_by_name_before_any_launch():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    p, fake = C.cast(buf, C.c_void_p), C.c_void_p(8)
    cap = 10
    n0 = lib.rlrep_launch_counter()

    def ref_(st):
        return C.byref(st) if st is not None else None

    def start(st, ag=fake, seeds=p):
        return lib.rlrep_group_sim_start(ag, ref_(st), seeds, None)

    def step(st, ag=fake, seeds=p, act=p, ld=1, nxt=p, rew=p, done=p):
        return lib.rlrep_group_sim_step(ag, ref_(st), seeds, act, ld, nxt, rew, done, None)

    def app(st, ag=fake, seeds=p, act=p, ld=1, ring=p, max_size=cap, row=None, stride=None, ctl=p):
        row = {0: 9, 2: 7}.get(st.kind if st is not None else 0, 9) if row is None else row
        stride = max_size * row if stride is None else stride
        return lib.rlrep_group_sim_step_append_ctl(ag, ref_(st), seeds, act, ld, ring, max_size, row, stride, None, ctl, None)

    for who, call in (('group_sim_start', start), ('group_sim_step', step), ('group_sim_step_append_ctl', app)):
        _refused(lib, call(None), who, 'null')
        _refused(lib, call(_state()[0], ag=None), who, 'null')
        _refused(lib, call(_state()[0], seeds=None), who, 'null')
        for field in ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs'):
            _refused(lib, call(_state(**{field: True})[0]), who, 'null')
        for kind in (1, 3, -1):
            _refused(lib, call(_state(kind=kind)[0]), who, f'kind {kind}')
        for n in (0, -1, 65537):
            _refused(lib, call(_state(n=n)[0]), who, f'n {n}', '[1, 65536]')
    for kind in (0, 2):
        st = _state(kind=kind)[0]
        for null in ('act', 'nxt', 'rew', 'done'):
            _refused(lib, step(st, **{null: None}), 'group_sim_step', 'null')
        _refused(lib, step(st, ld=0), 'group_sim_step', 'ld_act 0')
        for null in ('act', 'ring', 'ctl'):
            _refused(lib, app(st, **{null: None}), 'group_sim_step_append_ctl', 'null')
        _refused(lib, app(st, ld=0), 'group_sim_step_append_ctl', 'ld_act 0')
        _refused(lib, app(_state(n=cap + 1, kind=kind)[0]), 'group_sim_step_append_ctl', f'n {cap + 1}', 'max_size')
        good = 9 if kind == 0 else 7
        for row in (good - 1, good + 1, 16 - good):
            _refused(lib, app(st, row=row), 'group_sim_step_append_ctl', f'row {row}', '2 S + A + 2')
        _refused(lib, app(st, stride=cap * good - 1), 'group_sim_step_append_ctl', 'ring stride')
    assert lib.rlrep_launch_counter() == n0


# ---- the record -------------------------------------------------------------------------------------------------------------------------------
def test_the_restated_record_replays_warm_up_training_a_retirement_and_a_wrap():
    """R = 3, N = 17, a ring of 95 rows, start_timesteps = 2 N: two warm-up iterations, two training ones, member 1 retired for three,
    revived, and on until every cursor has wrapped.  At every stage the host faces of the product's record (SimLoopGroup on a host tensor:
    set_cursor, set_counters, counters, state -- what ReplayBufferGroup and _iterate read) hold the restated words."""
    import torch
    from rlrep_amd.envs import sim_loop
    R, N, CAP, START = 3, 17, 95, 34
    w = ref.new_record(R, ptr=0, sizes=[0] * R, capacity=CAP)
    w[0, ref.CALLS] = 11
    loop = sim_loop.SimLoopGroup.__new__(sim_loop.SimLoopGroup)            # (the record alone: no simulator, nothing launched)
    loop.R, loop.num_envs, loop.start_timesteps = R, N, START
    loop.ctl = torch.full((R, sim_loop.LOOP_CTL_WORDS), -1, dtype=torch.int64)
    loop._write(np.zeros((R, sim_loop.LOOP_CTL_WORDS), np.int64))
    loop.set_cursor(CAP, [0] * R, CAP)                  # (ptr = capacity wraps to row 0)
    loop.set_counters(0, 11, 0)
    assert np.array_equal(loop._read(), w) and loop.counters() == (0, 11, 0)
    with pytest.raises(ValueError, match='2 fill levels for 3 members'):
        loop.set_cursor(0, [0, 0], CAP)
    live = [True] * R
    warms, rows1 = [], []
    for it in range(10):
        if it == 4:
            live[1] = False
            frozen = w[1].copy()
        if it == 7:
            assert np.array_equal(w[1], frozen)          # the retired member's row stood still, bit for bit
            live[1] = True
        warm, rows = ref.iteration(w, live, N, CAP, START)
        warms.append(warm)
        assert sorted(rows) == [r for r in range(R) if live[r]]
        rows1.append(rows.get(1))
        # the shared words after iteration `it`: one value for the group, advanced once
        assert (w[0, ref.ITER], w[0, ref.T]) == (it + 1, N * (it + 1))
        assert w[0, ref.CALLS] == 11 + N * max(0, it + 1 - 2) and w[0, ref.WARM] == int(warm)
        assert not w[1:, [ref.CALLS, ref.T, ref.ITER, ref.WARM]].any()         # rows 1.. hold cursors only
        # the product's faces of these words: per-member cursors, the group's counters in every record; the host mirrors advance alike
        loop._write(w)
        rec = loop.state()
        assert rec.dtype == sim_loop.STATE_DTYPE and rec.shape == (R,)
        assert rec['ring_ptr'].tolist() == w[:, ref.NEXT].tolist() and rec['ring_size'].tolist() == w[:, ref.SIZE].tolist()
        assert rec['start'].tolist() == w[:, ref.START].tolist() and rec['t_global'].tolist() == [N * (it + 1)] * R and rec['iter'].tolist() == [it + 1] * R
        assert loop.counters() == (N * (it + 1), int(w[0, ref.CALLS]), it + 1)
        assert loop.advance() == warm and (loop.t_global, loop.iter) == (N * (it + 1), it + 1)
    assert warms == [True, True] + [False] * 8
    # members 0 and 2 wrote ten iterations: the sixth wrapped (rows 85 .. 94, 0 .. 6)
    for r in (0, 2):
        assert w[r, ref.NEXT] == (10 * N) % CAP == 75 and w[r, ref.START] == (9 * N) % CAP and w[r, ref.SIZE] == CAP
    # member 1 wrote seven: it lags by 3 N mod 95, its fill level grew by N per iteration it ran and is full only now
    assert w[1, ref.NEXT] == (7 * N) % CAP == 24 and w[1, ref.SIZE] == min(7 * N, CAP) == CAP
    assert (int(w[0, ref.NEXT]) - int(w[1, ref.NEXT])) % CAP == (3 * N) % CAP
    assert rows1[4] is None and rows1[5] is None and rows1[6] is None
    first, level = rows1[7]                              # the revived member's next iteration: N rows at ITS cursor
    assert first.tolist() == [(4 * N + e) % CAP for e in range(N)] and level == 5 * N
    wrapped, level = rows1[8]                            # ... and its wrap comes an iteration later than the others'
    assert wrapped.tolist() == list(range(85, 95)) + list(range(0, 7)) and level == CAP
    # nobody live: nothing advances
    before = w.copy()
    assert ref.iteration(w, [False] * R, N, CAP, START) == (False, {}) and np.array_equal(w, before)
    # a cursor the host left outside the ring is clamped, as in the single form
    w[2, ref.NEXT] = CAP + 3
    ref.act(w, [False, False, True], N, CAP, START)
    assert w[2, ref.START] == 0 and w[2, ref.NEXT] == N


def test_the_python_record_is_the_restated_one():
    from rlrep_amd.envs import sim_loop
    assert (sim_loop.CALLS, sim_loop.T_GLOBAL, sim_loop.ITER, sim_loop.NEXT_PTR, sim_loop.START, sim_loop.SIZE, sim_loop.WARM) == \
        (ref.CALLS, ref.T, ref.ITER, ref.NEXT, ref.START, ref.SIZE, ref.WARM) and sim_loop.LOOP_CTL_WORDS == ref.WORDS
    assert issubclass(sim_loop.SimLoopGroup, sim_loop.SimLoop)
    assert sim_loop.SimLoopGroup.step is sim_loop.SimLoop.step and sim_loop.SimLoopGroup.advance is sim_loop.SimLoop.advance      # shared, not copied
    w = np.arange(24, dtype=np.int64).reshape(3, 8)
    assert sim_loop.SimLoopGroup._shared(w).tolist() == w[0].tolist() and sim_loop.SimLoop._shared(w[1]).tolist() == w[1].tolist()


def test_python_refusals_come_before_the_gpu():
    from rlrep_amd.envs import fused_sim, sim_loop

    class Single(object):
        R, _seed, state_dim, action_dim = None, 0, 3, 1

    class Group(object):
        R, seeds, state_dim, action_dim = 3, [0, 1, 2], 3, 1

    class Sim(object):
        obs = None
    with pytest.raises(ValueError, match='SimLoopGroup: needs a seed group'):
        sim_loop.SimLoopGroup(Single(), Sim())
    with pytest.raises(ValueError, match='SimLoop: needs a single agent.*SimLoopGroup'):
        sim_loop.SimLoop(Group(), Sim())
    with pytest.raises(ValueError, match=r'SimLoopGroup: sim.obs must be a contiguous CUDA float32 tensor \[3, N, 3\]'):
        sim_loop.SimLoopGroup(Group(), Sim())
    for n in (0, 65537):
        with pytest.raises(ValueError, match=f'FusedSimGroup: num_envs {n} outside'):
            fused_sim.FusedSimGroup('Pendulum-v1', 3, n)
    with pytest.raises(ValueError, match='FusedSimGroup: 2 seeds for 3 members'):
        fused_sim.FusedSimGroup('Pendulum-v1', 3, 8, seeds=[0, 1])
    with pytest.raises(ValueError, match='FusedSimGroup: .*HalfCheetah.* is not built'):
        fused_sim.FusedSimGroup('HalfCheetah-v4', 3, 8)
    with pytest.raises(ValueError, match='FusedSimGroup: .* is not built for seed groups.*compiled at run time.*single agents'):
        fused_sim.FusedSimGroup(fused_sim.example_kind('pendulum'), 3, 8)          # (source text is nothing a group takes)
    kind = fused_sim.SimKind.__new__(fused_sim.SimKind)          # (not compiled: the refusal looks at the class)
    kind._h = None
    with pytest.raises(ValueError, match='FusedSimGroup: a kind compiled at run time.*single agents'):
        fused_sim.FusedSimGroup(kind, 3, 8)
    assert fused_sim.FusedSimGroup.step is fused_sim.FusedSimGroup.step_ and callable(fused_sim.FusedSimGroup.step_append_)


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
BASE = ['--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '320']
LOOP = ['--torch-envs', '8', '--sim-graph', '--fused-sim']


class Reached(Exception):
    pass


def _stop(name):
    def f(*a, **k):
        raise Reached(name)
    return f


@pytest.mark.parametrize('alg', ['sac', 'ctrlsac'])
@pytest.mark.parametrize('env', ['Pendulum-v1', 'MountainCarContinuous-v0'])
@pytest.mark.parametrize('who', [['--seeds', '0,1,2,3'], ['--seeds', '0,1', '--sweep', 'lr=1e-4,3e-4'], ['--sweep', 'tau=0.005,0.01']])
def test_the_launcher_builds_the_group_for_the_new_flag_combination(monkeypatch, tmp_path, alg, env, who):
    """past every argument check, to the construction of the group (run_seeds' build_agent)"""
    from rlrep_amd import main
    monkeypatch.setattr(main, '_group_class', _stop('group'))
    monkeypatch.setattr(main, 'build_agent', _stop('single'))
    with pytest.raises(Reached, match='group'):
        main.run(['--alg', alg, '--env', env] + BASE + who + LOOP + ['--log_root', str(tmp_path)])


def test_the_launcher_takes_the_group_loop(monkeypatch, tmp_path):
    from rlrep_amd import main
    from rlrep_amd.utils import buffer_group

    class Agent(object):
        R, live = 2, [True, True]

        def __init__(self, *a, **k):
            pass
    monkeypatch.setattr(main, '_group_class', lambda alg: Agent)
    monkeypatch.setattr(buffer_group, 'ReplayBufferGroup', lambda *a, **k: None)
    monkeypatch.setattr(main, '_fused_sim_group_loop', _stop('group loop'))
    monkeypatch.setattr(main, '_device_loop', _stop('device loop'))
    with pytest.raises(Reached, match='group loop'):
        main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1'] + BASE + LOOP + ['--log_root', str(tmp_path)])


@pytest.mark.parametrize('flags,named', [(['--torch-envs', '8'], '--seeds'), (['--torch-envs', '8', '--sim-graph'], '--seeds'),
                                         (['--torch-envs', '8', '--fused-sim'], '--fused-sim')])
def test_a_group_without_both_flags_is_still_refused(flags, named):
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1'] + BASE + flags)
    assert named in str(e.value) and ('--torch-envs 8' in str(e.value) or '--torch-envs N' in str(e.value)), str(e.value)


@pytest.mark.parametrize('flags,named', [
    (['--pbt-interval', '160'], '--pbt-interval'), (['--halving-interval', '160'], '--halving-interval'), (['--group-per'], '--group-per'),
    (['--group-critic-per'], '--group-critic-per'), (['--device-env'], '--device-env'), (['--host-envs', '4'], '--host-envs'),
    (['--device-env', '--num-envs', '4'], '--device-env')])
def test_the_group_loop_refuses_by_name_before_the_gpu(monkeypatch, flags, named):
    from rlrep_amd import main
    monkeypatch.setattr(main, '_group_class', _stop('group'))
    alg = 'ctrlsac' if named == '--group-critic-per' else 'sac'
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', alg, '--env', 'Pendulum-v1', '--seeds', '0,1,2,3'] + BASE + LOOP + flags)
    assert named in str(e.value), str(e.value)


def test_num_envs_and_the_run_time_kind_are_named_too(tmp_path):
    from rlrep_amd import main
    ns = dict(torch_envs=8, seeds='0,1', sweep=None, device_env=False, device_loop=False, host_envs=1, num_envs=1, env='Pendulum-v1', start_timesteps=160.0,
              eval_freq=160, max_timesteps=1e6, sim_graph=True, fused_sim=True)
    main._check_torch_envs(main.argparse.Namespace(**ns))                   # nothing to refuse (and no newer attribute is needed)
    with pytest.raises(SystemExit) as e:
        main._check_torch_envs(main.argparse.Namespace(**dict(ns, num_envs=4)))
    assert '--torch-envs 8' in str(e.value) and '--num-envs' in str(e.value)
    with pytest.raises(SystemExit) as e:
        main._check_torch_envs(main.argparse.Namespace(**dict(ns, fused_sim_source='x.h')))
    assert '--torch-envs 8' in str(e.value) and '--fused-sim-source' in str(e.value)
    with pytest.raises(SystemExit) as e:
        main._check_torch_envs(main.argparse.Namespace(**dict(ns, sim_graph=False)))
    assert '--torch-envs 8' in str(e.value) and '--seeds' in str(e.value)
    from rlrep_amd.envs import fused_sim
    path = tmp_path / 'kind.h'
    path.write_text(fused_sim.example_kind('pendulum'))
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1'] + BASE + LOOP + ['--fused-sim-source', str(path)])
    assert '--fused-sim-source' in str(e.value) and '--torch-envs 8' in str(e.value)


def test_the_group_loop_keeps_the_checks_of_torch_envs():
    base = ['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1'] + LOOP
    with pytest.raises(SystemExit) as e:                # --start_timesteps, counted per member, a multiple of N
        run_launcher(base + ['--start_timesteps', '150', '--eval_freq', '160'])
    assert '--torch-envs 8' in str(e.value) and '--start_timesteps 150' in str(e.value) and 'multiple' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(base + ['--start_timesteps', '160', '--eval_freq', '150'])
    assert '--torch-envs 8' in str(e.value) and '--eval_freq 150' in str(e.value)
    with pytest.raises(SystemExit) as e:                # N at most the ring's rows
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--torch-envs', '64', '--sim-graph', '--fused-sim', '--start_timesteps', '0',
                      '--eval_freq', '64', '--max_timesteps', '32'])
    assert '--torch-envs 64' in str(e.value) and 'ring' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'HalfCheetah-v4', '--seeds', '0,1'] + LOOP + BASE)
    assert '--fused-sim' in str(e.value) and 'HalfCheetah-v4' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '0,1'] + LOOP + BASE)
    assert '--seeds' in str(e.value) and 'vlsac' in str(e.value)
