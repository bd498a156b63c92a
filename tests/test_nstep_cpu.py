"""CPU: n-step replay.  The restatement tests/nstep_reference.py on chains worked by hand, the CPU buffers' gather_nstep against
it bit for bit, the keyword validation, the agents' refusals that need no device, and the launcher's checks.  No GPU."""
import argparse

import numpy as np
import pytest
import torch

from nstep_reference import chain, nstep_batch, ring_of, trajectories, f32
from seed_group_util import run_launcher

S, A = 2, 1
SA = S + A


def _ring(rows, max_size):
    """rows: (s, s2, r, d) tuples with S-vectors or scalars; the action is the row number"""
    ring = np.zeros((max_size, 2 * S + A + 2), f32)
    for i, (s, s2, r, d) in enumerate(rows):
        ring[i % max_size] = np.concatenate([np.broadcast_to(f32(s), S), [i], np.broadcast_to(f32(s2), S), [r, d]])
    return ring


# ---- the restatement on hand-computed chains ----------------------------------------------------------------------------------------------
def test_hand_computed_chain():
    # rewards 1, 2, 4 at gamma = 0.5: R = 1 + 0.5 * 2 + 0.25 * 4 = 3, g = 0.25, D' = 1 - 0.25 (1 - 0) = 0.75
    ring = _ring([(0, 1, 1.0, 0), (1, 2, 2.0, 0), (2, 3, 4.0, 0), (3, 4, 8.0, 0)], 8)
    last, m, g, R, D = chain(ring, 0, 4, 3, 1, 0.5, S, A)
    assert (last, m) == (2, 3) and g == 0.25 and R == 3.0 and D == 0.75
    # the head y = R + (1 - D') gamma tv = R + gamma^3 tv
    assert (1.0 - D) * 0.5 == 0.125
    # a terminal last row: D' = 1 - g (1 - 1) = 1
    ring[2, -1] = 1.0
    assert chain(ring, 0, 4, 3, 1, 0.5, S, A)[1:] == (3, f32(0.25), f32(3.0), f32(1.0))
    b = nstep_batch(ring, [0], 4, 3, 1, 0.5, S, A)
    assert np.array_equal(b['state'], [[0, 0]]) and np.array_equal(b['action'], [[0]]) and np.array_equal(b['next_state'], [[3, 3]])


@pytest.mark.parametrize('d', [0.0, 1.0])
def test_a_chain_of_one_is_the_row_itself(d):
    ring = _ring([(0, 1, 1.7, d), (5, 6, 2.0, 0)], 4)           # row 1 does not start where row 0 ended
    for n in (1, 3):
        last, m, g, R, D = chain(ring, 0, 2, n, 1, 0.99, S, A)
        assert (last, m, g) == (0, 1, 1.0) and R == ring[0, -2] and D == f32(d)


def test_where_a_chain_stops():
    rows = [(0, 1, 1.0, 0), (1, 2, 1.0, 0), (2, 3, 1.0, 0), (3, 4, 1.0, 0), (4, 5, 1.0, 0)]
    ring = _ring(rows, 8)
    assert chain(ring, 0, 5, 5, 1, 0.5, S, A)[:2] == (4, 5)
    assert chain(ring, 0, 5, 16, 1, 0.5, S, A)[:2] == (4, 5)                 # j = 5 >= size
    assert chain(ring, 0, 3, 5, 1, 0.5, S, A)[:2] == (2, 3)                  # the fill level
    t = ring.copy(); t[1, -1] = 1.0
    assert chain(t, 0, 5, 5, 1, 0.5, S, A)[:2] == (1, 2)                     # d = 1: the terminal row is the last
    t = ring.copy(); t[2, 0] = np.nextafter(f32(2.0), f32(3.0))
    assert chain(t, 0, 5, 5, 1, 0.5, S, A)[:2] == (1, 2)                     # one bit of s[2] differs from s'[1]
    t = ring.copy(); t[2, 1] = -0.0; t[1, SA + 1] = 0.0
    assert chain(t, 0, 5, 5, 1, 0.5, S, A)[:2] == (1, 2)                     # -0 and +0 are different words
    t = ring.copy(); t[2, :S] = np.nan; t[1, SA:SA + S] = np.nan
    assert chain(t, 0, 5, 5, 1, 0.5, S, A)[:2] == (4, 5)                     # equal NaN words continue


def test_the_head_of_a_full_ring_and_the_wrap():
    # 11 rows of one trajectory into 8: rows 8, 9, 10 overwrote 0, 1, 2; the newest row is 2, the oldest 3
    ring = _ring([(i, i + 1, 1.0, 0) for i in range(11)], 8)
    assert chain(ring, 6, 8, 4, 1, 0.5, S, A)[:2] == (1, 4)                  # 6 -> 7 -> 0 -> 1: across the wrap
    assert chain(ring, 1, 8, 4, 1, 0.5, S, A)[:2] == (2, 2)                  # 2 is the newest: row 3 holds step 3, not step 11
    # two interleaved environments in a ring of 8 (8 % 2 == 0): environment 0 wraps onto its own rows
    rows = trajectories(S, A, 12, 2, 0, p_done=0, p_limit=0)
    ring, ptr, size = ring_of(rows, 8)
    assert (ptr, size) == (4, 8)
    assert chain(ring, 6, 8, 3, 2, 0.5, S, A)[:2] == (2, 3)                  # 6 -> 0 -> 2 (steps 6, 8, 10)
    assert chain(ring, 2, 8, 3, 2, 0.5, S, A)[:2] == (2, 1)                  # the head: row 4 holds step 4
    # ... and in a ring of 9 (9 % 2 != 0) the row behind the wrap belongs to the other environment
    ring, ptr, size = ring_of(trajectories(S, A, 9, 2, 0, p_done=0, p_limit=0), 9)
    assert chain(ring, 6, 9, 3, 2, 0.5, S, A)[:2] == (8, 2) and chain(ring, 7, 9, 3, 2, 0.5, S, A)[:2] == (7, 1)


# ---- the CPU buffers ----------------------------------------------------------------------------------------------------------------------
def _assert_batch(got, want, what):
    for k in ('state', 'action', 'reward', 'next_state', 'done'):
        g = getattr(got, k).numpy()
        assert g.dtype == np.float32 and g.shape == want[k].shape and np.array_equal(g.view(np.uint32), want[k].view(np.uint32)), (what, k)


@pytest.mark.parametrize('stride', [1, 4])
def test_cpu_buffer_equals_the_restatement(stride):
    from rlrep_amd.utils.buffer import ReplayBuffer, PrioritizedReplayBuffer
    S2, A2, cap, gamma = 3, 2, 64, 0.97
    rows = trajectories(S2, A2, 150, stride, 7)
    for cls in (ReplayBuffer, PrioritizedReplayBuffer):
        buf = cls(S2, A2, max_size=cap, device='cpu', stage_rows=16, n_step=4, n_stride=stride)
        assert (buf.n_step, buf.n_stride) == (4, stride)
        n = 0
        for stop in (40, 64, 100, 150):          # partly filled, exactly full, wrapped twice
            if stride == 1 and stop == 40:
                for t in range(n, stop):
                    buf.add(rows[0][t], rows[1][t], rows[2][t], rows[3][t], rows[4][t])
            else:
                for t in range(n, stop, stride):
                    buf.add_batch(*[x[t:min(t + stride, stop)] for x in rows])
            n = stop
            ring, ptr, size = ring_of([x[:n] for x in rows], cap)
            assert (buf.ptr, buf.size) == (ptr, size)
            want = nstep_batch(ring, np.arange(size), size, 4, stride, gamma, S2, A2)
            _assert_batch(buf.gather_nstep(np.arange(size), gamma), want, (cls.__name__, stop))
        assert want['reward'].ravel().tolist() != ring[:, -2].tolist()          # some chains are longer than one row
    # load(), and n_step = 1 is gather()
    buf = ReplayBuffer(S2, A2, max_size=cap, device='cpu', n_step=3, n_stride=stride)
    buf.load(*[x[:50] for x in rows])
    ring, _, size = ring_of([x[:50] for x in rows], cap)
    _assert_batch(buf.gather_nstep(torch.arange(50), gamma), nstep_batch(ring, np.arange(50), 50, 3, stride, gamma, S2, A2), 'load')
    one = ReplayBuffer(S2, A2, max_size=cap, device='cpu')
    one.load(*[x[:50] for x in rows])
    g1, g = one.gather_nstep(torch.arange(50), gamma), one.gather(torch.arange(50))
    for k in g._fields:
        assert torch.equal(getattr(g1, k), getattr(g, k)), k


def test_cpu_buffer_group_equals_the_restatement():
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup, PrioritizedReplayBufferGroup
    S2, A2, cap, R = 3, 1, 32, 2
    rows = [trajectories(S2, A2, 45, 1, 20 + r) for r in range(R)]
    for cls in (ReplayBufferGroup, PrioritizedReplayBufferGroup):
        g = cls(R, S2, A2, max_size=cap, device='cpu', n_step=3, n_stride=1)
        for t in range(45):
            g.add(*[np.stack([rows[r][k][t] for r in range(R)]) for k in range(5)])
        g.flush()
        for r, gamma in enumerate((0.9, 0.99)):
            ring, _, size = ring_of(rows[r], cap)
            _assert_batch(g.gather_nstep(r, np.arange(size), gamma), nstep_batch(ring, np.arange(size), size, 3, 1, gamma, S2, A2), (cls.__name__, r))


def test_keyword_validation():
    from rlrep_amd.utils.buffer import ReplayBuffer, PrioritizedReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup, PrioritizedReplayBufferGroup
    mk = [lambda **kw: ReplayBuffer(S, A, max_size=8, device='cpu', **kw), lambda **kw: PrioritizedReplayBuffer(S, A, max_size=8, device='cpu', **kw),
          lambda **kw: ReplayBufferGroup(2, S, A, max_size=8, device='cpu', **kw), lambda **kw: PrioritizedReplayBufferGroup(2, S, A, max_size=8, device='cpu', **kw)]
    for f in mk:
        b = f()
        assert (b.n_step, b.n_stride) == (1, 1)
        assert f(n_step=16, n_stride=64).nstep_key() == ('nstep', 16, 64)
        for bad in (dict(n_step=0), dict(n_step=17), dict(n_step=2.5), dict(n_step=3, n_stride=0), dict(n_stride=-1), dict(n_step=True)):
            with pytest.raises(ValueError, match='n_step|n_stride'):
                f(**bad)
    with pytest.raises(ValueError, match='shard'):
        ReplayBuffer(S, A, max_size=8, device='cpu', shard=(0, 2), n_step=2)
    assert ReplayBuffer(S, A, max_size=8, device='cpu', shard=(0, 2)).n_step == 1


def test_collect_on_device_needs_the_matching_stride():
    from rlrep_amd.utils.buffer import ReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup

    class Env:
        num_envs = 4

        def set_cursor(self, *a):
            self.cursor = a
    for buf in (ReplayBuffer(S, A, max_size=8, device='cpu', n_step=3, n_stride=1), ReplayBufferGroup(2, S, A, max_size=8, device='cpu', n_step=3)):
        with pytest.raises(ValueError, match='n_stride'):
            buf.collect_on_device(Env())
    ok = ReplayBuffer(S, A, max_size=8, device='cpu', n_step=3, n_stride=4)
    ok.collect_on_device(Env())
    plain = ReplayBuffer(S, A, max_size=8, device='cpu')            # n_step = 1: any number of environments, as before
    plain.collect_on_device(Env())


def test_agents_refuse_by_class_name_and_n_step():
    """SACAgent._check_nstep is what every entry point calls before a launch: the representation agents and data-parallel agents refuse"""
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.utils.buffer import ReplayBuffer
    buf, plain = ReplayBuffer(S, A, max_size=8, device='cpu', n_step=3), ReplayBuffer(S, A, max_size=8, device='cpu')

    class Stub:
        ALG, world_size, _dp = 'vlsac', 1, False
        _nstep = staticmethod(SACAgent._nstep)
    Stub.__name__ = 'VLSACAgent'
    with pytest.raises(RuntimeError, match=r'VLSACAgent\.train: ReplayBuffer\(n_step=3\)'):
        SACAgent._check_nstep(Stub(), buf, 'train')
    SACAgent._check_nstep(Stub(), plain, 'train')
    Stub.ALG, Stub.world_size = 'sac', 2
    with pytest.raises(RuntimeError, match=r'ReplayBuffer\(n_step=3\).*data-parallel'):
        SACAgent._check_nstep(Stub(), buf, 'train')
    Stub.world_size = 1
    SACAgent._check_nstep(Stub(), buf, 'train')
    k1, k3 = SACAgent._graph_cache_key(plain, 64), SACAgent._graph_cache_key(buf, 64)
    assert len(k1) == 4 and k3[-3:] == ('nstep', 3, 1)


# ---- the launcher -------------------------------------------------------------------------------------------------------------------------
BASE = ['--env', 'Pendulum-v1', '--max_timesteps', '10']


@pytest.mark.parametrize('argv,word', [
    (['--alg', 'vlsac', '--n-step', '3'], '--alg sac'),
    (['--alg', 'ctrlsac', '--n-step', '3', '--seeds', '0,1'], '--alg sac'),
    (['--alg', 'spedersac', '--n-step', '2'], '--alg sac'),
    (['--alg', 'diffsrsac', '--n-step', '2'], '--alg sac'),
    (['--alg', 'sac', '--n-step', '0'], '1..16'),
    (['--alg', 'sac', '--n-step', '17'], '1..16'),
    (['--alg', 'sac', '--n-step', '3', '--n-stride', '0'], '--n-stride'),
    (['--alg', 'sac', '--n-stride', '4'], '--n-step'),
    (['--alg', 'sac', '--n-step', '3', '--n-stride', '1', '--device-loop', '--num-envs', '4', '--start_timesteps', '8', '--eval_freq', '8'], '--num-envs 4'),
])
def test_launcher_refuses_before_the_gpu(argv, word, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: (_ for _ in ()).throw(AssertionError('the GPU was touched')))
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + argv)
    assert word in str(e.value), e.value


def test_launcher_defaults_the_stride():
    from rlrep_amd import main
    ns = lambda **kw: argparse.Namespace(**dict(dict(alg='sac', n_step=3, n_stride=None, host_envs=1, torch_envs=0, num_envs=1, device_loop=False,
                                                     device_env=False), **kw))
    assert main._nstep_kw(ns()) == dict(n_step=3, n_stride=1)
    assert main._nstep_kw(ns(host_envs=8)) == dict(n_step=3, n_stride=8)
    assert main._nstep_kw(ns(torch_envs=16)) == dict(n_step=3, n_stride=16)
    assert main._nstep_kw(ns(num_envs=4, device_loop=True)) == dict(n_step=3, n_stride=4)
    assert main._nstep_kw(ns(host_envs=8, n_stride=2)) == dict(n_step=3, n_stride=2)
    assert main._nstep_kw(ns(n_step=1)) == {}
    main._check_nstep(ns(num_envs=4, device_loop=True))
    main._check_nstep(argparse.Namespace(alg='vlsac'))             # a namespace built by hand, without the flags
