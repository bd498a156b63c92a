"""CPU: n-step critic targets for vlsac / ctrlsac / spedersac / diffsrsac.  The restatement tests/nstep_targets_reference.py
and the conditions its kernel cases must meet, the CPU buffer's gather_nstep_targets against it bit for bit, the keyword validation and the
refusals, the cache keys, the launcher's exits, and the oracle composition at n = 1 against oracle.train.  No GPU."""
import argparse

import numpy as np
import pytest
import torch

import nstep_targets_reference as ref
from nstep_reference import nstep_slot, ring_of, trajectories, f32
from seed_group_util import run_launcher

S, A = 2, 1
ALGS = ('vlsac', 'ctrlsac', 'spedersac', 'diffsrsac')


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_targets_are_three_arrays_of_the_full_nstep_gather():
    rows = trajectories(3, 1, 96 + 29, 2, 7)
    ring, _, size = ring_of(rows, 96)
    idx = np.arange(size)
    for n in (1, 3, 16):
        full = nstep_slot(ring, idx, size, n, 2, 0.97, 3, 1)
        t = ref.nstep_targets(ring, idx, size, n, 2, 0.97, 3, 1, total=96 + 29)
        assert np.array_equal(_bits(t['S2']), _bits(full['XF2'][:, :3])) and np.array_equal(_bits(t['Rn']), _bits(full['R']))
        assert np.array_equal(_bits(t['D']), _bits(full['D'])) and np.array_equal(t['m'], full['m'])
        if n == 1:
            assert np.array_equal(t['Rn'], ring[idx, -2]) and np.array_equal(t['D'], ring[idx, -1]) and set(t['cut']) == {''}
    # an index outside the ring: zeros
    t = ref.nstep_targets(ring, [96, -1, 5], size, 3, 2, 0.97, 3, 1)
    assert not t['S2'][:2].any() and not t['Rn'][:2].any() and not t['D'][:2].any() and t['m'][2] >= 1


def test_step_of_rows():
    assert list(ref.step_of_rows(3, 5)) == [0, 1, 2, -1, -1]
    assert list(ref.step_of_rows(7, 5)) == [5, 6, 2, 3, 4]
    assert list(ref.step_of_rows(10, 5)) == [5, 6, 7, 8, 9]


@pytest.mark.parametrize('s,a', ref.SHAPES)
@pytest.mark.parametrize('stride', ref.STRIDES)
def test_kernel_cases_meet_their_conditions(s, a, stride):
    """what tests/test_nstep_critic.py runs on the device: in every (shape, stride, n > 1, fill level) case a quarter of the samples chain, and
    a chain is cut by a terminal row, by a time limit, and by the fill level (partly filled ring) or the wrapped write head (full ring)"""
    for n in ref.NS:
        for total in ref.FILL:
            if n > 1:
                assert ref.kernel_case_ok(s, a, stride, n, total), (s, a, stride, n, total)
    for total in ref.FILL:
        ring, size, idx = ref.kernel_case(s, a, stride, total)
        assert size == min(total, ref.CAP) and len(idx) == ref.BATCH and ref.BATCH % 4 != 0 and ref.CAP % 5 != 0
        assert sum(1 for i in idx if not 0 <= i < ref.CAP) == 1
    ring, size, idx = ref.kernel_case(s, a, stride, ref.FILL[1])
    assert ref.nstep_targets(ring, idx, size, 16, stride, ref.GAMMA, s, a, ref.FILL[1])['m'].max() > 5       # n = 16 walks further than n = 5


# ---- the CPU buffer -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 2, 5])
def test_cpu_buffer_equals_the_restatement(stride):
    from rlrep_amd.utils.buffer import ReplayBuffer
    S2, A2, cap = 3, 1, 96
    rows = trajectories(S2, A2, cap + 29, stride, 40 + stride)
    for total in (50, cap + 29):
        buf = ReplayBuffer(S2, A2, max_size=cap, device='cpu', critic_n_step=3, n_stride=stride)
        for t in range(0, total, stride):
            buf.add_batch(*[x[t:min(t + stride, total)] for x in rows])
        buf.flush()
        ring, ptr, size = ring_of([x[:total] for x in rows], cap)
        assert (buf.ptr, buf.size) == (ptr, size)
        idx = np.arange(size)
        got = buf.gather_nstep_targets(idx, 0.97)
        want = ref.nstep_targets(ring, idx, size, 3, stride, 0.97, S2, A2, total)
        assert np.array_equal(_bits(got.next_state.numpy()), _bits(want['S2']))
        assert np.array_equal(_bits(got.reward.numpy().reshape(-1)), _bits(want['Rn']))
        assert np.array_equal(_bits(got.done.numpy().reshape(-1)), _bits(want['D']))
        assert want['m'].max() == 3
        one = buf.gather(torch.as_tensor(idx))                  # what the feature step keeps: the plain rows
        assert np.array_equal(one.reward.numpy().reshape(-1), ring[idx, -2])
    plain = ReplayBuffer(S2, A2, max_size=cap, device='cpu')
    plain.load(*[x[:50] for x in rows])
    t1, b1 = plain.gather_nstep_targets(np.arange(50), 0.97), plain.gather(torch.arange(50))
    assert torch.equal(t1.next_state, b1.next_state) and torch.equal(t1.reward, b1.reward) and torch.equal(t1.done, b1.done)


def test_keyword_validation():
    from rlrep_amd.utils.buffer import ReplayBuffer, PrioritizedReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup, PrioritizedReplayBufferGroup
    mk = lambda **kw: ReplayBuffer(S, A, max_size=8, device='cpu', **kw)
    assert mk().critic_n_step == 1 and mk(critic_n_step=16, n_stride=64).cnstep_key() == ('cnstep', 16, 64)
    for bad in (dict(critic_n_step=0), dict(critic_n_step=17), dict(critic_n_step=2.5), dict(critic_n_step=True), dict(critic_n_step=3, n_stride=0)):
        with pytest.raises(ValueError, match='critic_n_step|n_stride'):
            mk(**bad)
    with pytest.raises(ValueError, match=r'n_step 3 and critic_n_step 2'):
        mk(n_step=3, critic_n_step=2)
    assert mk(n_step=3, critic_n_step=1).n_step == 3
    with pytest.raises(ValueError, match='shard'):
        mk(shard=(0, 2), critic_n_step=2)
    assert mk(shard=(0, 2)).critic_n_step == 1
    for cls, args in ((PrioritizedReplayBuffer, (S, A)), (ReplayBufferGroup, (2, S, A)), (PrioritizedReplayBufferGroup, (2, S, A))):
        assert cls(*args, max_size=8, device='cpu').critic_n_step == 1
        assert cls(*args, max_size=8, device='cpu', critic_n_step=1, n_step=3).n_step == 3
        with pytest.raises(ValueError, match=cls.__name__ + r': critic_n_step 3 > 1 is not supported'):
            cls(*args, max_size=8, device='cpu', critic_n_step=3)


def test_collect_on_device_needs_the_matching_stride():
    from rlrep_amd.utils.buffer import ReplayBuffer

    class Env:
        num_envs = 4

        def set_cursor(self, *a):
            self.cursor = a
    with pytest.raises(ValueError, match='critic_n_step 3 with n_stride 1'):
        ReplayBuffer(S, A, max_size=8, device='cpu', critic_n_step=3).collect_on_device(Env())
    ReplayBuffer(S, A, max_size=8, device='cpu', critic_n_step=3, n_stride=4).collect_on_device(Env())


def test_agents_refuse_by_class_name_and_critic_n_step():
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.agent.spedersac.spedersac_agent import SPEDERSACAgent
    from rlrep_amd.utils.buffer import ReplayBuffer
    buf, plain, nbuf = (ReplayBuffer(S, A, max_size=8, device='cpu', **kw) for kw in (dict(critic_n_step=3), {}, dict(n_step=3)))

    class Stub:
        ALG, world_size, _dp, SEED_GROUP = 'sac', 1, False, False
        _critic_nstep = staticmethod(SACAgent._critic_nstep)
        _nstep = staticmethod(SACAgent._nstep)
    Stub.__name__ = 'SACAgent'
    check = SACAgent._check_critic_nstep
    with pytest.raises(RuntimeError, match=r'SACAgent\.train: ReplayBuffer\(critic_n_step=3\).*use n_step'):
        check(Stub(), buf, 'train')
    check(Stub(), plain, 'train')
    check(Stub(), nbuf, 'train')
    Stub.ALG, Stub.world_size = 'vlsac', 2
    with pytest.raises(RuntimeError, match=r'ReplayBuffer\(critic_n_step=3\).*data-parallel'):
        check(Stub(), buf, 'iterate')
    Stub.world_size, Stub._dp = 1, True
    with pytest.raises(RuntimeError, match='data-parallel'):
        check(Stub(), buf, 'train')
    Stub._dp = False
    for alg in ALGS:
        Stub.ALG = alg
        check(Stub(), buf, 'train')
        with pytest.raises(RuntimeError, match=r'ReplayBuffer\(n_step=3\)'):          # n_step keeps its meaning for them
            SACAgent._check_nstep(Stub(), nbuf, 'train')
    for grp in (SACSeedBatch, CTRLSACSeedBatch):
        assert grp.SEED_GROUP
        Stub.SEED_GROUP, Stub.ALG = True, grp.ALG
        Stub.__name__ = grp.__name__
        with pytest.raises(RuntimeError, match=grp.__name__ + r'\.train: ReplayBuffer\(critic_n_step=3\).*seed group'):
            check(Stub(), buf, 'train')
    assert not SACAgent.SEED_GROUP
    # the cache keys: a plain buffer's stays 4 long
    k1, kc = SACAgent._graph_cache_key(plain, 64), SACAgent._graph_cache_key(buf, 64)
    assert len(k1) == 4 and len(kc) == 7 and kc[-3:] == ('cnstep', 3, 1) and SACAgent._graph_cache_key(nbuf, 64)[-3:] == ('nstep', 3, 1)
    # the minibatch that gets the launch: the last slot-0 key of the plan
    sp = argparse.Namespace(extra_feature_steps=2, action_dim=1, _feature_iters=lambda: 3)
    sp._plan = lambda B: SPEDERSACAgent._plan(sp, B)
    assert SPEDERSACAgent._critic_key(sp, 8) == 'f2a' and SPEDERSACAgent._plan(sp, 8)[0][-1] == 'f2b'


# ---- the launcher -------------------------------------------------------------------------------------------------------------------------
BASE = ['--env', 'Pendulum-v1', '--max_timesteps', '10']


@pytest.mark.parametrize('argv,word', [
    (['--alg', 'sac', '--critic-n-step', '3'], '--n-step 3'),
    (['--alg', 'vlsac', '--critic-n-step', '0'], '1..16'),
    (['--alg', 'ctrlsac', '--critic-n-step', '17'], '1..16'),
    (['--alg', 'vlsac', '--critic-n-step', '3', '--n-stride', '0'], '--n-stride'),
    (['--alg', 'ctrlsac', '--critic-n-step', '3', '--seeds', '0,1'], '--seeds'),
    (['--alg', 'vlsac', '--critic-n-step', '3', '--per'], 'not with --per'),
    (['--alg', 'vlsac', '--critic-n-step', '3', '--n-step', '3'], '--alg sac'),
    (['--alg', 'vlsac', '--n-stride', '4'], '--n-step'),
    (['--alg', 'diffsrsac', '--critic-n-step', '3', '--n-stride', '1', '--device-loop', '--num-envs', '4', '--start_timesteps', '8', '--eval_freq', '8'],
     '--num-envs 4'),
])
def test_launcher_refuses_before_the_gpu(argv, word, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: (_ for _ in ()).throw(AssertionError('the GPU was touched')))
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + argv)
    assert word in str(e.value), e.value


def test_launcher_keywords_and_hand_built_namespaces():
    from rlrep_amd import main
    ns = lambda **kw: argparse.Namespace(**dict(dict(alg='vlsac', n_step=1, critic_n_step=3, n_stride=None, host_envs=1, torch_envs=0, num_envs=1,
                                                     device_loop=False, device_env=False, seeds=None, sweep=None, per=False, group_per=False), **kw))
    assert main._nstep_kw(ns()) == dict(critic_n_step=3, n_stride=1)
    assert main._nstep_kw(ns(host_envs=8)) == dict(critic_n_step=3, n_stride=8)
    assert main._nstep_kw(ns(num_envs=4, device_loop=True)) == dict(critic_n_step=3, n_stride=4)
    assert main._nstep_kw(ns(torch_envs=16, n_stride=2)) == dict(critic_n_step=3, n_stride=2)
    assert main._nstep_kw(ns(critic_n_step=1)) == {}
    assert main._nstep_kw(ns(alg='sac', critic_n_step=1, n_step=3)) == dict(n_step=3, n_stride=1)
    for a in (ns(), ns(n_stride=2), ns(num_envs=4, device_loop=True), argparse.Namespace(alg='vlsac'), argparse.Namespace(alg='sac')):
        main._check_nstep(a)                                   # hand-built namespaces without the flag still pass
        main._check_critic_nstep(a)


# ---- the oracle composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ALGS)
def test_composition_at_n_1_is_oracle_train(alg):
    """tests/nstep_targets_reference.py oracle_train -- feature_step on the one-step Batch, critic_step / update_actor_and_alpha on the Batch
    with the targets' next_state / reward / done -- reproduces oracle.train exactly when the targets are the one-step ones"""
    from fixture_io import Case
    from oracle import make_oracle
    from oracle.agents import gather_batch
    c = Case(alg + '_tiny')
    torch.set_num_threads(4)
    a, b = make_oracle(alg, c.S, c.A, c.init, **c.kw), make_oracle(alg, c.S, c.A, c.init, **c.kw)
    r = c.replay
    rows = c.meta['replay_n']
    ring = np.concatenate([np.asarray(r[k], f32).reshape(rows, -1) for k in ('state', 'action', 'next_state', 'reward', 'done')], axis=1)
    rs = np.random.RandomState(3)
    for t in range(2):
        idx, eps = ref.injected_draws(rs, alg, a, c.S, c.A, c.B, c.kw.get('feature_dim', 0), rows)
        batches, noise = [gather_batch(r, i) for i in idx], [torch.as_tensor(e) for e in eps]
        want = a.train(batches, noise)
        crit = idx[-2] if alg == 'spedersac' else idx[-1]
        got = ref.oracle_train(b, batches, noise, ref.nstep_targets(ring, crit, rows, 1, 1, a.discount, c.S, c.A))
        assert set(got) == set(want) and all(float(got[k]) == float(want[k]) for k in want), (alg, t)
        assert a.steps == b.steps == t + 1
    pa, pb = a.state(), b.state()
    assert all(torch.equal(pa[k], pb[k]) for k in pa), alg
