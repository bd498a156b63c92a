"""CPU-only: prioritized replay of the critic's minibatch for vlsac / ctrlsac / spedersac / diffsrsac.  The CPU fallback of
CriticPrioritizedReplayBuffer against tests/per_reference.py bit for bit, the constructor's and the agents' refusals, the cache key, which
minibatches of a plan stay uniform, and the launcher's exits before the GPU."""
import argparse

import numpy as np
import pytest
import torch

from per_reference import PER_STREAM, RefTree, f32
from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer, PrioritizedReplayBuffer, ReplayBuffer
from seed_group_util import run_launcher

S, A = 3, 1
ALGS = ('vlsac', 'ctrlsac', 'spedersac', 'diffsrsac')


def _rows(n, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, S)).astype(np.float32), r.normal(size=(n, A)).astype(np.float32), r.normal(size=(n, S)).astype(np.float32),
            r.normal(size=n).astype(np.float32), (r.random(n) < 0.1).astype(np.float32))


def _pow32(td, eps, alpha):
    return np.power(np.asarray(td, f32) + f32(eps), f32(alpha), dtype=f32)


def _cpu(max_size=1000, **kw):
    return CriticPrioritizedReplayBuffer(S, A, max_size=max_size, device='cpu', stage_rows=64, **kw)


# ---- the class ----------------------------------------------------------------------------------------------------------------------------
def test_it_is_the_parents_tree_under_another_contract():
    b = _cpu()
    assert isinstance(b, PrioritizedReplayBuffer) and b.critic_prioritized and not b.prioritized
    assert (b.alpha, b.beta, b.eps) == (float(f32(0.6)), float(f32(0.4)), float(f32(1e-6))) and b.max_priority == 1.0
    assert b.P == 1024 and b.tree.shape == (2048,)
    idx, w, td = b.draw_buffers(64)
    assert (idx.dtype, w.dtype, td.dtype) == (torch.int32, torch.float32, torch.float32) and idx.shape == w.shape == td.shape == (64,)
    assert b.draw_buffers(64)[2] is td                   # one triple per batch size for the life of the buffer
    with pytest.raises(RuntimeError, match='empty'):
        b.draw(8, 1, PER_STREAM)


def test_cpu_fallback_equals_the_reference_through_every_writer_and_save_restore(tmp_path):
    b, t = _cpu(), RefTree(1000)
    s, a, s2, r, d = _rows(1400)

    def same(buf, what):
        assert np.array_equal(buf.tree.numpy(), t.tree), what
        assert buf.max_priority == float(t.max_p), what
        assert np.array_equal(buf.priorities(), t.tree[t.P:t.P + buf.size]), what

    for i in range(150):                     # add(): more than the 64 staging rows, so it flushes on its own
        b.add(s[i], a[i], s2[i], r[i], d[i])
    b.flush()
    t.add(0, 150)
    same(b, 'add')
    b.add_batch(s[150:450], a[150:450], s2[150:450], r[150:450], d[150:450])
    b.flush()
    t.add(150, 300)
    same(b, 'add_batch')
    # draw + update from the buffer's own td array: the next rows enter at the new maximum
    idx, w = b.draw(64, 5, PER_STREAM + 1)
    assert np.array_equal(idx.numpy(), t.sample(64, 5, PER_STREAM + 1))
    wr, exact = t.weights(idx.numpy())
    assert np.all(w.numpy()[exact] == 1.0) and np.allclose(w.numpy(), wr, rtol=1e-6)
    td = (np.random.default_rng(3).random(64) * 5).astype(np.float32)
    b.draw_buffers(64)[2].copy_(torch.from_numpy(td))
    b.update(64)
    t.update(idx.numpy(), _pow32(td, t.eps, t.alpha))
    same(b, 'update from the own td array')
    assert b.max_priority > 1.0
    idx, _ = b.draw(64, 5, PER_STREAM + 2)
    td2 = (np.random.default_rng(4).random(64) * 2).astype(np.float32)
    b.update(64, td=td2)                                 # ... or from the caller's
    t.update(idx.numpy(), _pow32(td2, t.eps, t.alpha))
    same(b, 'update from a given td')
    b.add(s[450], a[450], s2[450], r[450], d[450])      # a staged host row, then add_device: flushed first, in call order
    b.add_device(*[torch.from_numpy(x) for x in (s[451:1100], a[451:1100], s2[451:1100], r[451:1100], d[451:1100])])
    t.add(450, 1); t.add(451, 649)
    same(b, 'add_device across the wrap')
    assert b.size == 1000 and b.ptr == 100
    # save / restore into a fresh buffer of the class
    path = str(tmp_path / 'ring.npz')
    b.save(path)
    c = _cpu()
    c.restore(path)
    same(c, 'restore')
    assert torch.equal(c.ring, b.ring) and (c.ptr, c.size) == (b.ptr, b.size)
    assert np.array_equal(c.draw(50, 9, PER_STREAM + 7)[0].numpy(), t.sample(50, 9, PER_STREAM + 7))
    # load() of fewer rows: the rows it no longer holds lose their leaves
    b.load(s[:700], a[:700], s2[:700], r[:700], d[:700])
    t.clear(); t.add(0, 700)
    same(b, 'load')
    # a plain ReplayBuffer's file: every row is new
    plain = ReplayBuffer(S, A, max_size=1000, device='cpu')
    plain.load(s[:300], a[:300], s2[:300], r[:300], d[:300])
    p2 = str(tmp_path / 'plain.npz')
    plain.save(p2)
    c.restore(p2)
    t2 = RefTree(1000)
    t2.add(0, 300)
    assert np.array_equal(c.tree.numpy(), t2.tree) and c.max_priority == 1.0


def test_alpha_zero_keeps_every_leaf_and_weight_at_one():
    b = _cpu(alpha=0.0)
    b.load(*_rows(700))
    for k in range(3):
        _, w = b.draw(64, 2, PER_STREAM + k)
        assert np.all(w.numpy() == 1.0)
        b.update(64, td=(np.random.default_rng(k).random(64) * 9).astype(np.float32))
    assert np.all(b.priorities() == 1.0) and b.tree.numpy()[1] == 700.0 and b.max_priority == 1.0


def test_constructor_refusals():
    mk = lambda **kw: CriticPrioritizedReplayBuffer(S, A, max_size=8, device='cpu', **kw)
    assert mk().critic_n_step == 1 and mk(n_step=1, n_stride=4).n_stride == 4
    with pytest.raises(ValueError, match=r'CriticPrioritizedReplayBuffer: critic_n_step 3 > 1 is not supported'):
        mk(critic_n_step=3)
    with pytest.raises(ValueError, match=r'CriticPrioritizedReplayBuffer: n_step 3 > 1 is not supported.*PrioritizedReplayBuffer'):
        mk(n_step=3)
    with pytest.raises(ValueError, match=r'CriticPrioritizedReplayBuffer: shard= is not supported'):
        mk(shard=(0, 2))
    with pytest.raises(RuntimeError, match=r'CriticPrioritizedReplayBuffer\.collect_on_device'):
        mk().collect_on_device(object())
    assert PrioritizedReplayBuffer(S, A, max_size=8, device='cpu', n_step=3).n_step == 3           # the parent keeps what it took


# ---- the agents' checks, with a stub in place of an agent -------------------------------------------------------------------------------------
def _stub(alg, name, world_size=1, dp=False, seed_group=False):
    from rlrep_amd.agent.sac.sac_agent import SACAgent

    class Stub:
        ALG, SEED_GROUP, _dp = alg, seed_group, dp
        _per, _cper, _nstep, _critic_nstep = (staticmethod(getattr(SACAgent, k)) for k in ('_per', '_cper', '_nstep', '_critic_nstep'))
        _check_nstep, _check_critic_nstep, _check_critic_per = SACAgent._check_nstep, SACAgent._check_critic_nstep, SACAgent._check_critic_per
    Stub.world_size = world_size
    Stub.__name__ = name
    return Stub()


def test_agents_refuse_by_class_name():
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    buf, plain = _cpu(8), ReplayBuffer(S, A, max_size=8, device='cpu')
    check = SACAgent._check_per
    for alg in ALGS:
        for what in ('train', 'prepare', 'train_injected'):
            check(_stub(alg, alg.upper() + 'Agent'), buf, what)
            check(_stub(alg, alg.upper() + 'Agent'), plain, what)
        for what in ('iterate', 'iterate_sim'):
            with pytest.raises(RuntimeError, match=rf'{alg.upper()}Agent\.{what}: CriticPrioritizedReplayBuffer cannot be written'):
                SACAgent._check_critic_per(_stub(alg, alg.upper() + 'Agent'), buf, what)
        with pytest.raises(RuntimeError, match=r'CriticPrioritizedReplayBuffer cannot be written'):
            check(_stub(alg, alg.upper() + 'Agent'), buf, 'iterate')
    with pytest.raises(RuntimeError, match=r'SACAgent\.train: CriticPrioritizedReplayBuffer.*use PrioritizedReplayBuffer'):
        check(_stub('sac', 'SACAgent'), buf, 'train')
    for name, alg in (('SACSeedBatch', 'sac'), ('CTRLSACSeedBatch', 'ctrlsac')):
        with pytest.raises(RuntimeError, match=name + r'\.train: CriticPrioritizedReplayBuffer does not train a seed group'):
            check(_stub(alg, name, seed_group=True), buf, 'train')
    with pytest.raises(RuntimeError, match=r'CriticPrioritizedReplayBuffer does not train a data-parallel agent'):
        check(_stub('vlsac', 'VLSACAgent', world_size=2), buf, 'train')
    with pytest.raises(RuntimeError, match='data-parallel'):
        check(_stub('vlsac', 'VLSACAgent', dp=True), buf, 'train')


def test_the_existing_class_is_still_refused_with_its_message():
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    old = PrioritizedReplayBuffer(S, A, max_size=8, device='cpu')
    for alg in ALGS:
        with pytest.raises(RuntimeError, match=r'PrioritizedReplayBuffer is built for SACAgent only \(' + alg + r' reuses its last feature minibatch.*'
                                               r'what prioritisation means there is open\): use a plain ReplayBuffer') as e:
            SACAgent._check_per(_stub(alg, 'X'), old, 'train')
        assert 'Critic' not in str(e.value)
    SACAgent._check_per(_stub('sac', 'SACAgent'), old, 'train')


def test_cache_key_tells_the_three_classes_apart():
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    new, old, plain = _cpu(8), PrioritizedReplayBuffer(S, A, max_size=8, device='cpu'), ReplayBuffer(S, A, max_size=8, device='cpu')
    assert new.per_key()[0] == 'critic_per' and old.per_key()[0] == 'per' and new.per_key()[0] != old.per_key()[0]
    assert new.per_key()[1:] == (new.tree.data_ptr(), new._scal.data_ptr())
    k0, k1 = SACAgent._graph_cache_key(plain, 64), SACAgent._graph_cache_key(new, 64)
    assert len(k0) == 4 and len(k1) == 7 and k1[4:] == new.per_key()


# ---- which minibatches stay uniform -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ALGS)
@pytest.mark.parametrize('extra', [0, 3])
def test_only_the_critic_key_leaves_the_plan(alg, extra):
    """_sample_into sends exactly one (key, slot) of a train() to the prioritized launch -- _critic_key(B) in slot 0 -- and _fill_pools takes
    that key, and no other, out of the gathers that ride in optimizer launches; a plain buffer's chain is untouched"""
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from test_default_mode import _cls
    cls = _cls(alg)
    sp = argparse.Namespace(extra_feature_steps=extra, action_dim=A, feature_dim=4, state_dim=S, PREFETCH_CHAIN=cls.PREFETCH_CHAIN,
                            _feature_iters=lambda: extra + 1)
    sp._plan = lambda B: cls._plan(sp, B)
    sp._critic_key = lambda B: cls._critic_key(sp, B)
    sp._prefetch_chain = lambda keys: cls._prefetch_chain(sp, keys)
    keys = sp._plan(8)[0]
    ck = sp._critic_key(8)
    assert ck == (f'f{extra}a' if alg == 'spedersac' else f'f{extra}') and keys.count(ck) == 1
    assert len(keys) == (2 if alg == 'spedersac' else 1) * (extra + 1)
    sent, plain_path = [], []
    sp._cper, sp._per = SACAgent._cper, SACAgent._per
    sp._sample_into_critic_per = lambda buffer, B, key, g: sent.append(key)
    sp._inject, sp._pool, sp._next_key = None, {}, {}
    sp._indices = lambda key, B, hi: plain_path.append(key)
    sp._gather = sp._gather_critic_targets = lambda *a, **k: None
    sp._buf = lambda *a, **k: None
    new, plain = _cpu(64), ReplayBuffer(S, A, max_size=64, device='cpu')
    for buf in (new, plain):
        for key in keys:
            slot = 1 if key.endswith('b') else 0
            SACAgent._sample_into(sp, buf, 8, key, slot, False)
    assert sent == [ck] and plain_path == [k for k in keys if k != ck] + keys
    # the prefetch chain: what _fill_pools drops
    chain = sp._prefetch_chain(keys)
    kept = {k: v for k, v in chain.items() if v != ck}
    assert set(chain) - set(kept) == ({k for k, v in chain.items() if v == ck}) and all(v != ck for v in kept.values())
    assert len(chain) - len(kept) == (1 if extra > 0 else 0)


# ---- the launcher, before the GPU ---------------------------------------------------------------------------------------------------------
BASE = ['--env', 'Pendulum-v1', '--critic-per', '--max_timesteps', '600', '--start_timesteps', '300', '--eval_freq', '300']


@pytest.mark.parametrize('argv,words', [
    (['--alg', 'sac'], ('--critic-per', '--per')),
    (['--alg', 'vlsac', '--seeds', '0,1'], ('--critic-per', '--seeds')),
    (['--alg', 'ctrlsac', '--sweep', 'lr=1e-4,3e-4'], ('--critic-per', '--sweep')),
    (['--alg', 'vlsac', '--device-loop'], ('--critic-per', '--device-loop')),
    (['--alg', 'spedersac', '--torch-envs', '4', '--sim-graph', '--start_timesteps', '300'], ('--critic-per', '--sim-graph')),
    (['--alg', 'diffsrsac', '--critic-n-step', '3'], ('--critic-per', '--critic-n-step')),
    (['--alg', 'vlsac', '--per-beta', '1.5'], ('--critic-per', '--per-beta')),
])
def test_launcher_refuses_before_the_gpu(argv, words, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: (_ for _ in ()).throw(AssertionError('the GPU was touched')))
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + argv)
    assert all(w in str(e.value) for w in words), e.value


def test_launcher_takes_the_class_and_anneals_beta(monkeypatch):
    from rlrep_amd import main
    main._check_critic_per(argparse.Namespace(alg='vlsac'))                 # a namespace built by hand, without the field: nothing to refuse
    main._check_critic_per(argparse.Namespace(alg='sac', critic_per=False))
    args = argparse.Namespace(critic_per=True, per_beta=0.4, max_timesteps=600.0)
    b = _cpu(beta=0.4)
    main._per_anneal(args, b, 300)
    assert b.beta == float(f32(0.7))
    main._per_anneal(args, b, 600)
    assert b.beta == 1.0 and b._scal[2].item() == 1.0

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(main.envs, 'make', stop)                            # the first thing the plain path does
    for alg in ALGS:
        with pytest.raises(Reached):
            main.run(['--alg', alg] + BASE)
        with pytest.raises(Reached):
            main.run(['--alg', alg, '--host-envs', '4', '--start_timesteps', '300'] + BASE)
