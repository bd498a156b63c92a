"""Device-resident acting and collection, host side: rlrep_act_device / rlrep_group_act_device / rlrep_replay_add_cols /
rlrep_group_replay_add_cols are declared, bound and exported with the signatures include/rlrep.h states, and refuse what needs no agent before
anything is launched (the refusals that need a handle are in tests/test_act_device.py); `add_device` equals `add_batch` on CPU rings;
TorchPendulum on the CPU equals envs/pendulum.py step for step from the same state; main.py checks --torch-envs before the GPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from seed_group_util import run_launcher
from test_device_env_cpu import CTYPE, _header_prototype

COLS = ['float*', 'int64_t', 'int32_t', 'int64_t', 'int32_t', 'int32_t', 'float*', 'int64_t', 'float*', 'int64_t', 'float*', 'int64_t', 'float*', 'float*',
        'int64_t']
ENTRY_POINTS = {
    'rlrep_act_device': ('int32_t', ['rlrep_agent*', 'float*', 'int64_t', 'int32_t', 'int32_t', 'uint64_t', 'uint64_t', 'float', 'float', 'float*', 'int64_t',
                                     'void*']),
    'rlrep_group_act_device': ('int32_t', ['rlrep_agent*', 'float*', 'int32_t', 'int32_t', 'uint64_t', 'float', 'float', 'float*', 'void*']),
    'rlrep_replay_add_cols': ('int32_t', COLS + ['int32_t*', 'int32_t', 'void*']),
    'rlrep_group_replay_add_cols': ('int32_t', COLS + ['int32_t', 'int64_t', 'int32_t*', 'int32_t', 'void*']),
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
    assert 'define RLREP_ACT_MAX_ROWS 65536' in ' '.join(open(_lib.HEADER_PATH).read().split())
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_act_device_refuses_null_arguments_and_row_counts_before_any_launch():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 8)()
    ptr, fake = C.cast(buf, C.c_void_p), C.c_void_p(8)                      # (`fake`: a non-null handle no refusal here may dereference)
    forms = (('act_device', lambda ag, obs, rows, act: lib.rlrep_act_device(ag, obs, 3, rows, 0, 0, 0, -1.0, 1.0, act, 1, None)),
             ('group_act_device', lambda ag, obs, rows, act: lib.rlrep_group_act_device(ag, obs, rows, 0, 0, -1.0, 1.0, act, None)))
    n0 = lib.rlrep_launch_counter()
    for name, call in forms:
        for ag, obs, act in ((None, ptr, ptr), (fake, None, ptr), (fake, ptr, None)):
            assert call(ag, obs, 4, act) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and 'null' in msg, msg
        for rows in (0, -1, 65537, 2 ** 20):
            assert call(fake, ptr, rows, ptr) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and f'rows {rows}' in msg and '[1, 65536]' in msg, msg
    assert lib.rlrep_launch_counter() == n0


def test_replay_add_cols_refuses_by_name_before_any_launch():
    from rlrep_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    S, A, cap = 3, 1, 10
    row = 2 * S + A + 2

    def single(ring=p, s=p, a=p, s2=p, r=p, d=p, n=4, row=row, start=0):
        return lib.rlrep_replay_add_cols(ring, cap, row, start, S, A, s, S, a, A, s2, S, r, d, n, None, 4, None)

    def group(ring=p, s=p, a=p, s2=p, r=p, d=p, n=4, row=row, start=0):
        return lib.rlrep_group_replay_add_cols(ring, cap, row, start, S, A, s, S, a, A, s2, S, r, d, n, 2, cap * row, None, 4, None)
    n0 = lib.rlrep_launch_counter()
    for name, call in (('replay_add_cols', single), ('group_replay_add_cols', group)):
        for null in ('ring', 's', 'a', 's2', 'r', 'd'):
            assert call(**{null: None}) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and 'null' in msg, msg
        for n in (0, -2, cap + 1):
            assert call(n=n) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and f'n {n}' in msg and 'max_size' in msg, msg
        for bad_row in (row - 1, row + 1):
            assert call(row=bad_row) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and f'row {bad_row}' in msg and '2 S + A + 2' in msg, msg
        for start in (-1, cap):
            assert call(start=start) == RLREP_ERR_ARG
            msg = lib.rlrep_last_error().decode()
            assert msg.startswith(name + ':') and f'start {start}' in msg, msg
    assert lib.rlrep_launch_counter() == n0


# ---- add_device -------------------------------------------------------------------------------------------------------------------------------
S, A = 2, 1


def _transitions(rng, n, lead=()):
    shape = tuple(lead) + (n,)
    return tuple(np.asarray(x, np.float32) for x in (rng.normal(size=shape + (S,)), rng.normal(size=shape + (A,)), rng.normal(size=shape + (S,)),
                                                     rng.normal(size=shape), rng.uniform(size=shape) < 0.3))


def _observables(buf):
    buf.flush()
    ring = buf.rings if hasattr(buf, 'rings') else buf.ring
    return (ring.numpy().tobytes(), buf.ptr, buf.sizes if hasattr(buf, 'sizes') else buf.size, getattr(buf, 'device_epoch', None))


@pytest.mark.parametrize('case', ['wrap', 'staged'])
def test_add_device_equals_add_batch_on_a_single_ring(case):
    """wrap: a ring of 7, N = 3 five times -- the third call wraps it.  staged: two host add() calls wait in the staging buffer in front of
    every add_device, which flushes them first: the ring holds the transitions in call order."""
    from rlrep_amd.utils.buffer import ReplayBuffer
    dev, host = ReplayBuffer(S, A, max_size=7, device='cpu'), ReplayBuffer(S, A, max_size=7, device='cpu')
    rng = np.random.RandomState(3)
    for _ in range(5):
        if case == 'staged':
            for _ in range(2):
                one = [x[0] for x in _transitions(rng, 1)]
                dev.add(*one)
                host.add(*one)
        rows = _transitions(rng, 3)
        dev.add_device(*[torch.from_numpy(x) for x in rows])
        host.add_batch(*rows)
        host.flush()
        assert _observables(dev) == _observables(host)
        assert dev._staged == 0
    assert dev.size == 7 and dev.ring.abs().sum() > 0 and dev.device_epoch == 5
    assert dev.ptr == (5 * (5 if case == 'staged' else 3)) % 7


def test_add_device_equals_add_batch_on_a_group_of_rings():
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    R = 2
    dev, host = ReplayBufferGroup(R, S, A, max_size=7, device='cpu'), ReplayBufferGroup(R, S, A, max_size=7, device='cpu')
    rng = np.random.RandomState(4)
    for it in range(5):
        if it % 2:
            one = [x[:, 0] for x in _transitions(rng, 1, lead=(R,))]
            dev.add(*one)
            host.add(*one)
        rows = _transitions(rng, 3, lead=(R,))
        dev.add_device(*[torch.from_numpy(x) for x in rows])
        host.add_batch(*rows)
        assert _observables(dev) == _observables(host)
    assert dev.sizes == [7, 7] and not np.array_equal(dev.rings[0].numpy(), dev.rings[1].numpy())


def test_add_device_refusals():
    from rlrep_amd.utils.buffer import ReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    rng = np.random.RandomState(5)
    t = lambda n, lead=(): [torch.from_numpy(x) for x in _transitions(rng, n, lead=lead)]  # noqa: E731
    buf, grp = ReplayBuffer(S, A, max_size=7, device='cpu'), ReplayBufferGroup(2, S, A, max_size=7, device='cpu')
    for b, lead in ((buf, ()), (grp, (2,))):
        with pytest.raises(ValueError, match='add_device.*max_size'):
            b.add_device(*t(8, lead))
    with pytest.raises(ValueError, match='add_device.*shard'):
        ReplayBuffer(S, A, max_size=7, device='cpu', shard=(0, 2)).add_device(*t(3))
    buf._device_env = grp._device_env = object()                            # what collect_on_device leaves behind
    for b, lead, name in ((buf, (), 'ReplayBuffer.add_device'), (grp, (2,), 'ReplayBufferGroup.add_device')):
        with pytest.raises(RuntimeError, match=name + '.*adopt_device_cursor'):
            b.add_device(*t(3, lead))
        assert b.ptr == 0 and b._staged == 0


# ---- TorchPendulum ----------------------------------------------------------------------------------------------------------------------------
def test_torch_pendulum_equals_the_numpy_environment_step_for_step():
    """8 environments, 250 steps (the time limit and the reset fall inside): before every step the NumPy environment takes environment i's
    fp64 state, both step with the same fp32 action, and angle, angular velocity (fp64), observation and reward (fp32) must be equal.
    Strong torques drive some environments into the velocity clip; actions beyond +-2 meet the torque clip."""
    from rlrep_amd.envs.pendulum import PendulumEnv
    from rlrep_amd.envs.torch_pendulum import TorchPendulum
    N = 8
    env, ref = TorchPendulum(N, 'cpu', seed=3), PendulumEnv()
    obs = env.reset()
    assert obs.shape == (N, 3) and obs.dtype == torch.float32 and env.th.dtype == torch.float64
    assert float(env.th.abs().max()) <= np.pi and float(env.thd.abs().max()) <= 1.0 and len(set(env.th.tolist())) == N
    rng = np.random.RandomState(6)
    speed_clips = torque_clips = 0
    for step in range(250):
        # environment i < 4 pushes with the swing (reaches |thetadot| = 8); the others act at random, a third of the time beyond the torque range
        act = rng.uniform(-3.0, 3.0, (N, 1)).astype(np.float32)
        act[:4, 0] = np.where(env.thd[:4].numpy() >= 0, 2.5, -2.5)
        th0, thd0, t0 = env.th.clone(), env.thd.clone(), env.t
        cur = env.obs.clone()
        nxt, rew, done = env.step(torch.from_numpy(act))
        assert nxt.dtype == rew.dtype == torch.float32 and done.dtype == torch.bool and not bool(done.any())
        ended = t0 + 1 == 200
        for i in range(N):
            ref._th, ref._thd, ref._t = float(th0[i]), float(thd0[i]), t0
            assert np.array_equal(ref._obs(), cur[i].numpy()), (step, i)
            o, r, d, _ = ref.step(act[i])
            assert np.array_equal(o, nxt[i].numpy()), (step, i, o, nxt[i])
            assert np.float32(r) == rew[i].numpy(), (step, i)
            assert d == ended
            if not ended:
                assert ref._th == float(env.th[i]) and ref._thd == float(env.thd[i]), (step, i)
            speed_clips += abs(ref._thd) == 8.0
            torque_clips += abs(float(act[i, 0])) > 2.0
        if ended:
            assert env.t == 0 and env.episodes == 1 and bool(torch.isfinite(env.last_return).all()) and not torch.equal(env.obs, nxt)
            assert float(env.thd.abs().max()) <= 1.0
        else:
            assert torch.equal(env.obs, nxt) and env.t == (t0 + 1)
    assert speed_clips > 0 and torque_clips > 0 and env.t == 50


def test_torch_pendulum_start_states_follow_the_seed():
    from rlrep_amd.envs.torch_pendulum import TorchPendulum
    a, b, c = TorchPendulum(5, 'cpu', seed=1), TorchPendulum(5, 'cpu', seed=1), TorchPendulum(5, 'cpu', seed=2)
    assert torch.equal(a.reset(), b.reset()) and not torch.equal(a.reset(), c.reset())
    assert not torch.equal(a.reset(), a.obs.clone().zero_())


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'sac', '--env', 'Pendulum-v1']
OK = ['--start_timesteps', '160', '--eval_freq', '160']


def test_torch_envs_is_checked_before_the_gpu():
    for N in ('-3', '65537'):
        with pytest.raises(SystemExit) as e:
            run_launcher(BASE + ['--torch-envs', N, '--start_timesteps', '0', '--eval_freq', '120'])
        assert f'--torch-envs {N}' in str(e.value) and '[1, 65536]' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--torch-envs', '8', '--start_timesteps', '150', '--eval_freq', '160'])
    assert '--torch-envs 8' in str(e.value) and '--start_timesteps 150' in str(e.value) and 'multiple' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + ['--torch-envs', '8', '--start_timesteps', '160', '--eval_freq', '150'])
    assert '--torch-envs 8' in str(e.value) and '--eval_freq 150' in str(e.value) and 'multiple' in str(e.value)
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'sac', '--env', 'HalfCheetah-v4', '--torch-envs', '8'] + OK)
    assert '--torch-envs 8' in str(e.value) and 'Pendulum-v1' in str(e.value)


@pytest.mark.parametrize('flags,named', [(['--seeds', '0,1'], '--seeds'), (['--seeds', '0,1', '--device-env'], '--seeds'), (['--device-loop'], '--device-loop'),
                                         (['--host-envs', '4'], '--host-envs'), (['--device-loop', '--num-envs', '4'], '--device-loop'),
                                         (['--sweep', 'lr=1e-4,3e-4'], '--sweep')])
def test_torch_envs_does_not_go_with_the_other_collection_flags(flags, named):
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + flags + ['--torch-envs', '4'] + OK)
    assert '--torch-envs 4' in str(e.value) and named in str(e.value)


def test_num_envs_and_device_env_are_named_too():
    from rlrep_amd import main
    ns = dict(torch_envs=4, seeds=None, sweep=None, device_env=False, device_loop=False, host_envs=1, num_envs=1, env='Pendulum-v1', start_timesteps=160.0,
              eval_freq=160, max_timesteps=1e6)
    main._check_torch_envs(main.argparse.Namespace(**ns))                   # nothing to refuse
    main._check_torch_envs(main.argparse.Namespace(**dict(ns, torch_envs=0, num_envs=4, device_env=True)))     # off: nothing to say
    for key, value, named in (('num_envs', 4, '--num-envs'), ('device_env', True, '--device-env')):
        with pytest.raises(SystemExit) as e:
            main._check_torch_envs(main.argparse.Namespace(**dict(ns, **{key: value})))
        assert '--torch-envs 4' in str(e.value) and named in str(e.value)


def test_no_torch_envs_is_the_existing_path(monkeypatch):
    from rlrep_amd import main

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()

    def never(*a, **k):
        raise AssertionError('the default took the torch simulator loop')
    monkeypatch.setattr(main, '_torch_envs_loop', never)
    monkeypatch.setattr(main.envs, 'make', stop)                            # the first thing the existing path does
    for argv in (BASE, BASE + ['--torch-envs', '0', '--start_timesteps', '7', '--eval_freq', '3']):
        with pytest.raises(Reached):
            main.run(argv)
