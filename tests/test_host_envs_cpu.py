"""Vector host environments, host side: rlrep_select_action_n / rlrep_group_select_action_n are declared, bound and exported with the
signatures include/rlrep.h states and refuse a null argument and a row count outside [1, 256] before anything is launched (the refusals that
need a handle are in tests/test_host_envs.py), `add_batch` equals E `add()` calls on CPU rings, `eval_policy_vec` equals a sequential
evaluation over identically seeded environments episode by episode, and main.py checks --host-envs before the GPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from seed_group_util import run_launcher
from test_device_env_cpu import CTYPE, _header_prototype

ENTRY_POINTS = {
    'rlrep_select_action_n': ('int32_t', ['rlrep_agent*', 'float*', 'int32_t', 'int32_t', 'int32_t', 'uint64_t', 'uint64_t', 'float', 'float', 'float*',
                                          'int32_t', 'void*']),
    'rlrep_group_select_action_n': ('int32_t', ['rlrep_agent*', 'float*', 'int32_t', 'int32_t', 'uint64_t', 'float', 'float', 'float*', 'void*']),
}
RLREP_ERR_ARG = -1


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
    # `rows` follows the observation arguments
    single, one = _lib.SIGNATURES['rlrep_select_action_n'][1], _lib.SIGNATURES['rlrep_select_action'][1]
    assert single[:3] + single[4:] == one and single[3] is C.c_int32
    group, gone = _lib.SIGNATURES['rlrep_group_select_action_n'][1], _lib.SIGNATURES['rlrep_group_select_action'][1]
    assert group[:2] + group[3:] == gone and group[2] is C.c_int32
    assert 'define RLREP_SELECT_MAX_ROWS 256' in ' '.join(open(_lib.HEADER_PATH).read().split())
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_null_arguments_and_row_counts_are_refused_before_any_launch():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 8)()
    ptr, fake = C.cast(buf, C.c_void_p), C.c_void_p(8)                      # (`fake`: a non-null handle no refusal here may dereference)
    forms = (('select_action_n', lambda ag, obs, rows, act: lib.rlrep_select_action_n(ag, obs, 1, rows, 0, 0, 0, -1.0, 1.0, act, 1, None)),
             ('group_select_action_n', lambda ag, obs, rows, act: lib.rlrep_group_select_action_n(ag, obs, rows, 0, 0, -1.0, 1.0, act, None)))
    n0 = lib.rlrep_launch_counter()
    for name, call in forms:
        for ag, obs, act in ((None, ptr, ptr), (fake, None, ptr), (fake, ptr, None)):
            assert call(ag, obs, 4, act) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and 'null' in msg, msg
        for rows in (0, -1, 257, 2 ** 20):
            assert call(fake, ptr, rows, ptr) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and f'rows {rows}' in msg and '[1, 256]' in msg, msg
    assert lib.rlrep_launch_counter() == n0
    # the one-row calls keep their own names
    assert lib.rlrep_select_action(None, ptr, 1, 0, 0, 0, -1.0, 1.0, ptr, 1, None) == RLREP_ERR_ARG
    assert lib.rlrep_last_error().decode().startswith('select_action:')
    assert lib.rlrep_group_select_action(None, ptr, 0, 0, -1.0, 1.0, ptr, None) == RLREP_ERR_ARG
    assert lib.rlrep_last_error().decode().startswith('group_select_action:')


# ---- add_batch --------------------------------------------------------------------------------------------------------------------------------
S, A = 2, 1


def _transitions(rng, n, lead=()):
    shape = tuple(lead) + (n,)
    return (rng.normal(size=shape + (S,)), rng.normal(size=shape + (A,)), rng.normal(size=shape + (S,)), rng.normal(size=shape),
            (rng.uniform(size=shape) < 0.3).astype(np.float64))


def _observables(buf):
    buf.flush()
    ring = buf.rings if hasattr(buf, 'rings') else buf.ring
    return (ring.numpy().tobytes(), buf.ptr, buf.sizes if hasattr(buf, 'sizes') else buf.size, getattr(buf, 'device_epoch', None),
            getattr(buf, '_offered', None))


def _cursor(buf):
    return buf.ptr, buf.sizes if hasattr(buf, 'sizes') else buf.size, buf._staged, buf._stage_start, getattr(buf, 'device_epoch', None)


@pytest.mark.parametrize('case', ['wrap', 'stage', 'shard'])
def test_add_batch_equals_successive_adds_on_a_single_ring(case):
    """wrap: capacity 7, E = 3 over 5 batches -- the third batch wraps the ring.  stage: one batch of 11 rows over a staging buffer of 4 (and a
    ring of 7: it also laps the ring).  shard: rank 1 of 2 keeps the odd transitions."""
    from rlrep_amd.utils.buffer import ReplayBuffer
    kw = {'wrap': {}, 'stage': dict(stage_rows=4), 'shard': dict(shard=(1, 2))}[case]
    one, many = ReplayBuffer(S, A, max_size=7, device='cpu', **kw), ReplayBuffer(S, A, max_size=7, device='cpu', **kw)
    rng = np.random.RandomState(3)
    for E in ([11] if case == 'stage' else [3] * 5):
        s, a, s2, r, d = _transitions(rng, E)
        one.add_batch(s, a, s2, r, d)
        for e in range(E):
            many.add(s[e], a[e], s2[e], r[e], d[e])
        assert _cursor(one) == _cursor(many)                                 # before any flush: ptr, size, staged rows, device_epoch
    assert _observables(one) == _observables(many)
    assert one.size == 7 and many.ring.abs().sum() > 0
    if case == 'shard':
        assert one._offered == 15 and one.ptr == 0                           # 7 of the 15 offered transitions are odd: the ring is full once


@pytest.mark.parametrize('case', ['wrap', 'stage'])
def test_add_batch_equals_successive_adds_on_a_group_of_rings(case):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    R = 2
    kw = dict(stage_rows=4) if case == 'stage' else {}
    one, many = ReplayBufferGroup(R, S, A, max_size=7, device='cpu', **kw), ReplayBufferGroup(R, S, A, max_size=7, device='cpu', **kw)
    rng = np.random.RandomState(4)
    for E in ([11] if case == 'stage' else [3] * 5):
        s, a, s2, r, d = _transitions(rng, E, lead=(R,))
        one.add_batch(s, a, s2, r, d)
        for e in range(E):
            many.add(s[:, e], a[:, e], s2[:, e], r[:, e], d[:, e])
        assert _cursor(one) == _cursor(many)
    assert _observables(one) == _observables(many)
    assert one.sizes == [7, 7] and not np.array_equal(one.rings[0].numpy(), one.rings[1].numpy())


def test_add_batch_refuses_while_a_device_environment_owns_the_cursor():
    from rlrep_amd.utils.buffer import ReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    rng = np.random.RandomState(5)
    buf, grp = ReplayBuffer(S, A, max_size=7, device='cpu'), ReplayBufferGroup(2, S, A, max_size=7, device='cpu')
    buf._device_env = grp._device_env = object()                            # what collect_on_device leaves behind
    for b, lead, name in ((buf, (), 'ReplayBuffer.add_batch'), (grp, (2,), 'ReplayBufferGroup.add_batch')):
        with pytest.raises(RuntimeError, match=name + '.*adopt_device_cursor'):
            b.add_batch(*_transitions(rng, 3, lead=lead))
        assert b.ptr == 0 and b._staged == 0


# ---- eval_policy_vec --------------------------------------------------------------------------------------------------------------------------
class _StubPolicy(object):
    """a stateless function of the observation; `calls`: how often it was asked"""

    def __init__(self, kind):
        self.kind, self.calls, self.rows = kind, 0, 0

    def _one(self, obs):
        if self.kind == 'Pendulum-v1':
            return np.array([2.0 * np.tanh(3.0 * obs[1] + obs[2])], np.float32)
        # MountainCar: push with the velocity once it exceeds 0.004.  Rolling freely from rest at p0 a car reaches about 0.087 |p0 + 0.524|, so the
        # cars that start within 0.046 of the valley floor idle to the time limit and the others swing up to the goal
        v = float(obs[1])
        return np.array([np.sign(v) if abs(v) > 0.004 else 0.0], np.float32)

    def select_action(self, obs):
        self.calls += 1
        return self._one(np.asarray(obs, np.float32).reshape(-1))

    def select_actions(self, obs):
        obs = np.asarray(obs, np.float32)
        assert obs.ndim == 2
        self.calls, self.rows = self.calls + 1, self.rows + len(obs)
        return np.stack([self._one(o) for o in obs])


def _sequential(policy, envs_, episodes):
    """what eval_policy computes, per episode: environment i runs episodes i, i + E, ... one after the other"""
    E = len(envs_)
    returns, lengths = [None] * episodes, [None] * episodes
    for i, env in enumerate(envs_):
        for k in range(i, episodes, E):
            obs, done, ret, n = env.reset(), False, 0.0, 0
            while not done:
                obs, reward, done, _ = env.step(policy.select_action(np.asarray(obs)))
                ret, n = ret + reward, n + 1
            returns[k], lengths[k] = ret, n
    return returns, lengths


@pytest.mark.parametrize('name', ['Pendulum-v1', 'MountainCarContinuous-v0'])
def test_eval_policy_vec_equals_a_sequential_evaluation_per_episode(name, capsys):
    from rlrep_amd import envs
    from rlrep_amd.utils import util
    E, episodes = 3, 7                                                      # dealt unevenly: 3, 2, 2 episodes
    want, lengths = _sequential(_StubPolicy(name), [envs.make(name, seed=20 + i) for i in range(E)], episodes)
    policy = _StubPolicy(name)
    got = util.eval_policy_vec(policy, [envs.make(name, seed=20 + i) for i in range(E)], episodes)
    assert isinstance(got, float) and got.returns == want and float(got) == float(np.mean(want))
    assert policy.rows == sum(lengths) and policy.calls == max(sum(lengths[i::E]) for i in range(E))      # one call per lockstep step
    assert 'Evaluation over 7 episodes' in capsys.readouterr().out
    if name.startswith('MountainCar'):
        assert min(lengths) < 999 and max(lengths) == 999, lengths          # some episodes end at the goal, some at the time limit
    else:
        assert lengths == [200] * episodes


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'sac', '--env', 'Pendulum-v1']


@pytest.mark.parametrize('extra', [[], ['--seeds', '0,1']])
def test_host_envs_is_checked_before_the_gpu(extra):
    base = BASE + extra
    for E in ('0', '-3', '257'):
        with pytest.raises(SystemExit) as e:
            run_launcher(base + ['--host-envs', E, '--start_timesteps', '0', '--eval_freq', '120'])
        assert f'--host-envs {E}' in str(e.value) and '[1, 256]' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(base + ['--host-envs', '4', '--start_timesteps', '150', '--eval_freq', '160'])
    assert '--host-envs 4' in str(e.value) and '--start_timesteps 150' in str(e.value) and 'multiple' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(base + ['--host-envs', '4', '--start_timesteps', '160', '--eval_freq', '150'])
    assert '--host-envs 4' in str(e.value) and '--eval_freq 150' in str(e.value) and 'multiple' in str(e.value)


@pytest.mark.parametrize('flags,named', [(['--device-loop'], '--device-loop'), (['--seeds', '0,1', '--device-env'], '--device-env'),
                                         (['--seeds', '0,1', '--pbt-interval', '160'], '--pbt-interval'),
                                         (['--seeds', '0,1', '--halving-interval', '160'], '--halving-interval')])
def test_host_envs_does_not_go_with_the_device_and_ranking_flags(flags, named):
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + flags + ['--host-envs', '4', '--start_timesteps', '160', '--eval_freq', '160'])
    assert '--host-envs 4' in str(e.value) and named in str(e.value)


def test_num_envs_keeps_its_meaning():
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--num-envs', '4', '--host-envs', '4', '--start_timesteps', '160', '--eval_freq', '160'])
    assert str(e.value).startswith('--num-envs:') and '--device-env' in str(e.value) and '--device-loop' in str(e.value)


def test_one_host_environment_is_the_existing_path(monkeypatch):
    """--host-envs 1 (and no flag at all) reach run()'s own loop / run_seeds' own loop, not the vector loops"""
    from rlrep_amd import main

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    def never(*a, **k):
        raise AssertionError('--host-envs 1 took a vector loop')

    monkeypatch.setattr(main, '_host_envs_loop', never)
    monkeypatch.setattr(main, '_host_envs_group_loop', never)
    monkeypatch.setattr(main, '_check_host_envs', lambda args: seen.append(int(args.host_envs)))
    monkeypatch.setattr(main.envs, 'make', stop)                            # the first thing either existing path does
    for argv in (BASE, BASE + ['--host-envs', '1'], BASE + ['--host-envs', '1', '--start_timesteps', '7', '--eval_freq', '3']):
        seen = []
        with pytest.raises(Reached):
            main.run(argv)
        assert seen == [1]
    monkeypatch.undo()
    main._check_host_envs(main.argparse.Namespace(host_envs=1, start_timesteps=7.0, eval_freq=3, device_env=True, device_loop=True))      # nothing to refuse


def test_help_states_what_an_iteration_is(capsys):
    with pytest.raises(SystemExit):
        run_launcher(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--host-envs' in text and 'E transitions' in text and 'one train()' in text and 'caller' in text
