"""Prioritized critic replay for ctrlsac seed groups, the part that needs no GPU: the flags and the cache key of
CriticPrioritizedReplayBufferGroup, every refusal by its message, the host draw / weights / update of member r against a
CriticPrioritizedReplayBuffer(device='cpu') with member r's exponents and seed, bit for bit, the launcher's checks of --group-critic-per
(all of which run before anything touches the GPU) and the three new symbols of the C ABI."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from per_reference import PER_STREAM, f32
from seed_group_util import ROOT, run_launcher
from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer
from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup, PrioritizedReplayBufferGroup, ReplayBufferGroup

S, A, R = 3, 1, 3
ALPHA, BETA, EPS = [0.6, 0.0, 0.9], [0.4, 1.0, 0.0], [1e-6, 1e-3, 0.0]          # (member 1: alpha = 0, uniform replay)
SEEDS = [3, 5, 11]


def _rows(n, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, S)).astype(np.float32), r.uniform(-1, 1, size=(n, A)).astype(np.float32), r.normal(size=(n, S)).astype(np.float32),
            r.normal(size=(n,)).astype(np.float32), (r.random(n) < 0.05).astype(np.float32))


def _cpu(max_size=1000, **kw):
    kw = dict(dict(alpha=ALPHA, beta=BETA, eps=EPS), **kw)
    return CriticPrioritizedReplayBufferGroup(R, S, A, max_size=max_size, device='cpu', stage_rows=64, **kw)


def test_class_flags_and_cache_key():
    b = _cpu()
    assert isinstance(b, PrioritizedReplayBufferGroup) and isinstance(b, ReplayBufferGroup)
    assert b.prioritized_group is False and b.critic_prioritized_group is True
    assert not getattr(b, 'prioritized', False) and not getattr(b, 'critic_prioritized', False)
    assert b.per_key()[0] == 'critic_per_group' and b.per_key()[1:] == (b.trees.data_ptr(), b._scal.data_ptr())
    assert PrioritizedReplayBufferGroup(R, S, A, max_size=8, device='cpu').per_key()[0] == 'per_group'
    assert b.P == 1024 and tuple(b.trees.shape) == (R, 2048) and tuple(b._scal.shape) == (R, 4)
    idx, w, td = b.draw_buffers(5)
    assert tuple(idx.shape) == tuple(w.shape) == tuple(td.shape) == (R, 5) and idx.dtype == torch.int32 and td.dtype == torch.float32
    assert b.draw_buffers(5)[2] is td                 # one triple per batch size for the life of the buffer group
    from rlrep_amd.agent.seed_batch import SeedBatchMixin
    plain = ReplayBufferGroup(R, S, A, max_size=8, device='cpu')
    k0, k1 = SeedBatchMixin._graph_cache_key(plain, 64), SeedBatchMixin._graph_cache_key(b, 64)
    assert k1[len(k0):] == b.per_key()


def test_constructor_and_method_refusals():
    mk = lambda **kw: CriticPrioritizedReplayBufferGroup(R, S, A, max_size=8, device='cpu', **kw)
    with pytest.raises(ValueError, match=r'CriticPrioritizedReplayBufferGroup: n_step 3 > 1 is not supported.*PrioritizedReplayBufferGroup'):
        mk(n_step=3)
    with pytest.raises(ValueError, match=r'CriticPrioritizedReplayBufferGroup: critic_n_step 2 > 1 is not supported \(n-step critic targets are '
                                         r'built for one agent, not for a seed group\)'):
        mk(critic_n_step=2)
    with pytest.raises(RuntimeError, match=r'CriticPrioritizedReplayBufferGroup\.collect_on_device'):
        mk().collect_on_device(object())
    with pytest.raises(RuntimeError, match=r'CriticPrioritizedReplayBufferGroup\.draw_fill: a member\'s buffer is empty'):
        mk().draw_fill(None, 4, 0)
    b = mk()
    for m in range(R):
        b.load(m, *_rows(8, m))
    with pytest.raises(ValueError, match=r'CriticPrioritizedReplayBufferGroup\.draw_fill: the fused launch runs for a ctrlsac seed group on the device'):
        b.draw_fill(None, 4, 0)
    with pytest.raises(ValueError, match='alpha'):
        mk(alpha=[0.1, 0.2])


@pytest.mark.parametrize('max_size,fill', [(8, 8), (8, 5), (1000, 700)])
@pytest.mark.parametrize('B', [1, 5, 300])
def test_host_arithmetic_of_member_r_is_the_single_buffers(max_size, fill, B):
    """draw, weights and update of member r == CriticPrioritizedReplayBuffer(device='cpu', alpha_r, beta_r, eps_r) drawn with seed s_r: indices,
    weights, the whole tree and the running maximum, bit for bit, over three rounds (the trees part ways after the first update)"""
    g = _cpu(max_size)
    alone = [CriticPrioritizedReplayBuffer(S, A, max_size=max_size, device='cpu', stage_rows=64, alpha=ALPHA[m], beta=BETA[m], eps=EPS[m]) for m in range(R)]
    for m in range(R):
        rows = _rows(fill, 10 + m)
        g.load(m, *rows)
        alone[m].load(*rows)
        assert torch.equal(g.rings[m], alone[m].ring)
    for k in range(3):
        idx, w = g.draw(B, PER_STREAM + k, seeds=SEEDS)
        td = (np.random.default_rng(100 + k).random((R, B)) * 5).astype(np.float32)
        g.draw_buffers(B)[2].copy_(torch.from_numpy(td))          # (what the weighted head leaves: update() reads the group's own array)
        g.update(B)
        for m in range(R):
            i1, w1 = alone[m].draw(B, SEEDS[m], PER_STREAM + k)
            assert np.array_equal(idx[m].numpy(), i1.numpy()) and idx[m].numpy().max() < fill, (k, m)
            assert np.array_equal(w[m].numpy().view(np.uint32), w1.numpy().view(np.uint32)), (k, m)
            alone[m].update(B, td=td[m])
            assert np.array_equal(g.trees[m].numpy().view(np.uint32), alone[m].tree.numpy().view(np.uint32)), (k, m)
            assert g.max_priority(m) == alone[m].max_priority, (k, m)
    # alpha = 0 (member 1): uniform replay -- every weight and every leaf stays 1
    assert np.all(g.draw_buffers(B)[1][1].numpy() == 1.0) and np.all(g.priorities(1) == 1.0) and g.max_priority(1) == 1.0
    assert g.max_priority(0) > 1.0
    # given indices: only the weights; an explicit td and a live list
    given = np.stack([(np.arange(B) * (3 + m)) % fill for m in range(R)]).astype(np.int32)
    idx2, w2 = g.draw(B, 0, given=given)
    before = g.trees[1].numpy().copy()
    g.update(B, td=np.full((R, B), 3.0, np.float32), live=[0, 2])
    assert np.array_equal(idx2.numpy(), given) and np.array_equal(g.trees[1].numpy(), before)
    for m in (0, 2):
        _, w1 = alone[m].draw(B, 0, 0, given=given[m])
        assert np.array_equal(w2[m].numpy(), w1.numpy())
        alone[m].update(B, td=np.full(B, 3.0, np.float32))
        assert np.array_equal(g.trees[m].numpy(), alone[m].tree.numpy())


# ---- the agents' checks: the real classes without their constructors (nothing touches the GPU) --------------------------------------------------
def _bare(cls, **attrs):
    o = object.__new__(cls)
    o.__dict__.update(dict(world_size=1, _dp=False), **attrs)
    return o


def test_agents_take_and_refuse_the_class_by_name():
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
    new, old, plain = _cpu(8), PrioritizedReplayBufferGroup(R, S, A, max_size=8, device='cpu'), ReplayBufferGroup(R, S, A, max_size=8, device='cpu')
    one = CriticPrioritizedReplayBuffer(S, A, max_size=8, device='cpu')
    cg, sg = _bare(CTRLSACSeedBatch), _bare(SACSeedBatch)
    assert cg._cper(new) and cg._cper(one) and not cg._cper(plain) and not cg._cper(old) and not cg._per(new)
    for what in ('train', 'prepare'):
        cg._check_per(new, what)
        cg._check_per(plain, what)
    for what in ('iterate', 'iterate_sim'):
        with pytest.raises(RuntimeError, match=rf'CTRLSACSeedBatch\.{what}: CriticPrioritizedReplayBufferGroup cannot be written by a device environment'):
            cg._check_critic_per(new, what)
    with pytest.raises(RuntimeError, match=r'CTRLSACSeedBatch\.iterate: CriticPrioritizedReplayBufferGroup cannot be written'):
        cg._check_per(new, 'iterate')
    with pytest.raises(RuntimeError, match=r'CTRLSACSeedBatch\.train_injected: a seed group has no eager train\(\) form.*'
                                           r'CriticPrioritizedReplayBufferGroup\.draw_fill\(given='):
        cg._check_per(new, 'train_injected')
    for what in ('train', 'prepare', 'iterate'):
        with pytest.raises(RuntimeError, match=rf'SACSeedBatch\.{what}: CriticPrioritizedReplayBufferGroup is built for CTRLSACSeedBatch only.*'
                                               r'use PrioritizedReplayBufferGroup'):
            sg._check_per(new, what)
    for cls in (SACAgent, CTRLSACAgent, VLSACAgent):
        for what in ('train', 'prepare', 'iterate', 'train_injected'):
            with pytest.raises(RuntimeError, match=rf'{cls.__name__}\.{what}: CriticPrioritizedReplayBufferGroup is built for CTRLSACSeedBatch\.train '
                                                   r'\(a ctrlsac seed group\); a single agent takes a CriticPrioritizedReplayBuffer'):
                _bare(cls)._check_per(new, what)
        with pytest.raises(RuntimeError, match=r'CriticPrioritizedReplayBufferGroup is built for CTRLSACSeedBatch\.train'):
            _bare(cls)._check_critic_per(new, 'iterate_sim')
    # what was refused before is refused as before, with a pointer to the new class behind the old words
    with pytest.raises(RuntimeError, match=r'CTRLSACSeedBatch\.train: PrioritizedReplayBufferGroup is built for SACSeedBatch only \(ctrlsac reuses its '
                                           r'last feature minibatch for the critic step; what prioritisation means there is open\): use a plain '
                                           r'ReplayBufferGroup.*CriticPrioritizedReplayBufferGroup'):
        cg._check_per(old, 'train')
    for grp, name in ((cg, 'CTRLSACSeedBatch'), (sg, 'SACSeedBatch')):
        with pytest.raises(RuntimeError, match=name + r'\.train: CriticPrioritizedReplayBuffer does not train a seed group'):
            grp._check_per(one, 'train')
    sg._check_per(old, 'train')


# ---- the launcher, before the GPU ---------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--group-critic-per', '--max_timesteps', '600', '--start_timesteps', '300', '--eval_freq', '300']
GROUP = BASE + ['--seeds', '0,1']


@pytest.mark.parametrize('argv,words', [
    (BASE, ('--group-critic-per', '--seeds', '--sweep')),
    (GROUP + ['--per'], ('--group-critic-per', '--per')),
    (GROUP + ['--group-per'], ('--group-critic-per', '--group-per')),
    (GROUP + ['--critic-per'], ('--group-critic-per', '--critic-per')),
    (GROUP + ['--device-env'], ('--group-critic-per', '--device-env')),
    (GROUP + ['--critic-n-step', '3'], ('--critic-n-step',)),
    (['--alg', 'sac'] + GROUP[2:], ('--group-critic-per', '--alg ctrlsac', '--group-per')),
    (['--alg', 'vlsac'] + GROUP[2:], ('--group-critic-per', '--alg ctrlsac')),
    (GROUP + ['--per-beta', '1.5'], ('--group-critic-per', '--per-beta')),
    (GROUP + ['--per-alpha', '-1'], ('--group-critic-per', '--per-alpha')),
])
def test_launcher_refuses_before_the_gpu(argv, words, monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: (_ for _ in ()).throw(AssertionError('the GPU was touched')))
    with pytest.raises(SystemExit) as e:
        run_launcher(argv)
    assert all(w in str(e.value) for w in words), e.value


def test_existing_launcher_refusals_keep_their_texts():
    with pytest.raises(SystemExit) as e:            # --group-per on ctrlsac
        run_launcher(['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--group-per', '--seeds', '0,1'])
    assert '--group-per: prioritized replay of a seed group is built for --alg sac (got --alg ctrlsac' in str(e.value)
    with pytest.raises(SystemExit) as e:            # --critic-per on a group
        run_launcher(['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--critic-per', '--seeds', '0,1'])
    assert '--critic-per: prioritized critic replay trains ONE agent' in str(e.value) and 'it does not go with --seeds' in str(e.value)
    with pytest.raises(SystemExit) as e:            # per_alpha without a prioritized group
        run_launcher(['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--sweep', 'per_alpha=0.4,0.6'])
    assert 'per_alpha' in str(e.value) and 'it needs --group-per' in str(e.value) and '--group-critic-per' in str(e.value)


def test_launcher_reaches_the_environments_and_anneals_beta(monkeypatch):
    from rlrep_amd import main
    main._check_group_critic_per(argparse.Namespace(alg='sac'))                 # a namespace built by hand, without the field: nothing to refuse
    main._check_group_critic_per(argparse.Namespace(alg='sac', group_critic_per=False))
    b = _cpu(8, beta=0.4)
    args = argparse.Namespace(group_critic_per=True, per_beta=0.4, max_timesteps=600.0)
    main._per_anneal(args, b, 300)
    assert b.beta == [float(f32(0.7))] * R
    main._per_anneal(args, b, 600)
    assert b.beta == [1.0] * R and np.all(b._scal.numpy()[:, 2] == 1.0)

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(main.envs, 'make', stop)                # the first thing run_seeds does behind its checks
    for extra in ([], ['--sweep', 'per_alpha=0.4,0.6,0.8', '--halving-interval', '300'], ['--pbt-interval', '300'],
                  ['--host-envs', '4', '--start_timesteps', '300']):
        with pytest.raises(Reached):
            main.run(GROUP + extra)
    with pytest.raises(Reached):
        main.run(BASE + ['--sweep', 'per_alpha=0.4,0.6'])


def test_the_three_symbols_are_declared_and_bound():
    from rlrep_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'rlrep.h')).read()
    for name, nargs in (('rlrep_group_per_sample_fill', 14), ('rlrep_group_critic_weights_arm', 3), ('rlrep_group_per_update_td', 8)):
        m = re.search(r'int32_t ' + name + r'\(([^;]*)\);', header)
        assert m is not None, name
        assert len(m.group(1).split(',')) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(_lib.lib, name), name
    assert _lib.lib.rlrep_abi_version() == 4
