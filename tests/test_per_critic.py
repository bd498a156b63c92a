"""GPU: prioritized replay of the critic's minibatch for vlsac / ctrlsac / spedersac / diffsrsac (csrc/per.hip).  The fused
sample-and-gather launch against tests/per_reference.py and against rlrep_per_sample, which minibatches of a train() are prioritized,
alpha = 0 as uniform replay, the weighted critic step against weighted CPU oracles, the launch counts, a long graph run with save /
restore, the refusals and the launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

import nstep_targets_reference as nref
import seed_group_util as sg
from fixture_io import Case, rel_l2
from per_reference import PER_STREAM, RefTree, f32

pytestmark = pytest.mark.gpu

ALGS = ('vlsac', 'ctrlsac', 'spedersac', 'diffsrsac')
RTOL = 1e-4                     # the repository's bar (tests/test_hip_parity.py)


class _Space:
    def __init__(self, A, bound=1.0):
        self.low, self.high = -bound * np.ones(A, np.float32), bound * np.ones(A, np.float32)


def _agent(c, **extra):
    """the fixture's agent from the fixture's initial parameters; graph=False unless asked otherwise; `extra` overrides the fixture's kwargs"""
    from test_default_mode import _cls
    kw = dict(c.kw)
    if c.meta.get('patch_vae_hidden'):
        kw['vae_hidden_dim'] = c.meta['patch_vae_hidden']
    extra.setdefault('graph', False)
    kw.update(extra)
    agent = _cls(c.alg)(state_dim=c.S, action_dim=c.A, action_space=_Space(c.A, c.meta['bound']), max_batch=c.B, **kw)
    agent.core.load_state(c.init)
    return agent


def _load(buf, c):
    r = c.replay
    buf.load(r['state'], r['action'], r['next_state'], r['reward'], r['done'])
    return buf


def _cper(c, max_size=None, **kw):
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer
    return _load(CriticPrioritizedReplayBuffer(c.S, c.A, max_size=max_size or c.meta['replay_n'], **kw), c)


def _plain(c, max_size=None):
    from rlrep_amd.utils.buffer import ReplayBuffer
    return _load(ReplayBuffer(c.S, c.A, max_size=max_size or c.meta['replay_n']), c)


def _tree(buf):
    torch.cuda.synchronize()
    return buf.tree.cpu().numpy()


def _invariant(tree):
    P = len(tree) // 2
    n = np.arange(1, P)
    return bool(np.array_equal(tree[n], (tree[2 * n] + tree[2 * n + 1]).astype(f32)))


def _slot(core, B, S, A):
    """the six arrays of minibatch slot 0, read back (rlrep_slot_dev 0 .. 5)"""
    torch.cuda.synchronize()
    shapes = dict(XE=(B, 2 * S + A), XF=(B, S + A), XF2=(B, S + A), XFpi=(B, S + A), R=(B,), D=(B,))
    return {k: core.slot_array(0, w, int(np.prod(sh))).cpu().numpy().reshape(sh) for w, (k, sh) in enumerate(shapes.items())}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------
BMAX = 300
_hand = {}


def _hand_set(S, A):
    """per (S, A), once: a ring of 1000 rows (P = 1024) at size 700 with tests/test_per.py's hand-set leaves -- a leaf of 1e6, rows 512 .. 699
    zeroed, so the root's right subtree has no mass -- the restatement of its tree, a small vlsac agent to own the slot, and a sac agent"""
    if (S, A) not in _hand:
        from rlrep_amd.agent.sac.sac_agent import SACAgent
        from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
        from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer
        r = np.random.default_rng(S)
        rows = (r.normal(size=(700, S)).astype(np.float32), r.uniform(-1, 1, size=(700, A)).astype(np.float32),
                r.normal(size=(700, S)).astype(np.float32), r.normal(size=700).astype(np.float32), (r.random(700) < 0.05).astype(np.float32))
        buf, ref = CriticPrioritizedReplayBuffer(S, A, max_size=1000), RefTree(1000)
        buf.load(*rows)
        leaves = (1.0 + np.random.default_rng(4).random(700) * 9.0).astype(np.float32)
        leaves[137] = f32(1e6)
        leaves[512:] = 0
        buf.set_priorities(leaves, 1.0)
        ref.set_leaves(np.arange(700), leaves)
        assert np.array_equal(_tree(buf), ref.tree) and ref.tree[3] == 0
        torch.manual_seed(0)
        v = VLSACAgent(state_dim=S, action_dim=A, action_space=_Space(A), max_batch=BMAX, graph=False, hidden_dim=32, feature_dim=16,
                       extra_feature_steps=0)
        sac = SACAgent(state_dim=S, action_dim=A, action_space=_Space(A), max_batch=BMAX, graph=False, hidden_dim=32)
        for _ in range(3):                                       # a train() counter that is not 0, for the device-counter mode
            v.core.begin_train()
        v.core.update_target()
        assert int(sg.steps_words(v.core)[0]) == 3
        _hand[S, A] = (buf, ref, v, sac, buf.ring.cpu().numpy())
    return _hand[S, A]


@pytest.mark.parametrize('beta', [0.0, 0.4, 1.0])
@pytest.mark.parametrize('batch', [1, 50, 300])
@pytest.mark.parametrize('s,a', [(3, 1), (17, 6)])
def test_fused_launch_equals_the_restatement_and_the_two_launches(s, a, batch, beta):
    from rlrep_amd._lib import lib
    buf, ref, v, sac, ring = _hand_set(s, a)
    buf.beta = beta
    ref.beta = f32(beta)
    worst = 0.0
    buf.draw_fill(v.core, batch, 1, 1)                           # (sizes the slot for this batch: the arrays below are the ones the launches fill)
    step = int(sg.steps_words(v.core)[0])
    shapes = (batch * (2 * s + a), batch * (s + a), batch * (s + a), batch * (s + a), batch, batch)
    given = ((np.arange(batch, dtype=np.int64) * 7 + 3) % 512).astype(np.int32)
    modes = [('host offset', dict(seed=2024, offset=PER_STREAM + 1000 * batch + 1), ref.sample(batch, 2024, PER_STREAM + 1000 * batch + 1)),
             ('device counter', dict(seed=7, offset=PER_STREAM, counter_dev=lib.rlrep_steps_dev(v.core.h)), ref.sample(batch, 7, PER_STREAM + step)),
             ('given indices', dict(seed=0, offset=0, given=given), given)]
    for what, kw, want in modes:
        for k, m in enumerate(shapes):                           # poison the slot: every element must come from this launch
            v.core.slot_array(0, k, m).fill_(-7.25)
        idx, w = buf.draw_fill(v.core, batch, **kw)
        torch.cuda.synchronize()
        idx, w = idx.cpu().numpy().copy(), w.cpu().numpy().copy()
        assert np.array_equal(idx, want), (what, batch)
        assert idx.min() >= 0 and idx.max() < 700 and idx.max() < 512
        wr, exact = ref.weights(want)
        assert np.all(w[exact] == 1.0), what
        if beta == 0.0:
            assert np.all(w == 1.0), what
        err = np.abs(w - wr) / wr
        worst = max(worst, float(err.max()))
        assert np.all(err <= RTOL), (what, err.max())
        got = _slot(v.core, batch, s, a)
        rows = ring[idx]
        sa = s + a
        assert np.array_equal(_bits(got['XE']), _bits(rows[:, :sa + s])), what
        assert np.array_equal(_bits(got['XF']), _bits(rows[:, :sa])), what
        assert np.array_equal(_bits(got['XF2'][:, :s]), _bits(rows[:, sa:sa + s])), what
        assert np.array_equal(_bits(got['XFpi'][:, :s]), _bits(rows[:, :s])), what
        assert np.array_equal(_bits(got['R']), _bits(rows[:, sa + s])) and np.array_equal(_bits(got['D']), _bits(rows[:, sa + s + 1])), what
        # rlrep_per_sample on a sac agent, same seed and stream, into the same draw buffers: bit-equal idx and w
        skw = dict(kw)
        if 'counter_dev' in skw:                                 # (the sac agent's own counter stands at 0: the vlsac agent's value as a host offset)
            skw = dict(seed=7, offset=PER_STREAM + step)
        idx2, w2 = buf.draw(batch, skw['seed'], skw['offset'], core=sac.core, given=skw.get('given'))
        torch.cuda.synchronize()
        assert np.array_equal(idx2.cpu().numpy(), idx) and np.array_equal(_bits(w2.cpu().numpy()), _bits(w)), what
    print(f'per_sample_fill (S, A) = ({s}, {a}) B = {batch} beta = {beta}: largest relative error of w against float64 pow {worst:.3e}')


# ---- 2. only the critic's minibatch is prioritized ----------------------------------------------------------------------------------------
def test_only_the_critics_minibatch_is_prioritized():
    c = Case('vlsac_tiny')
    B, n = c.B, c.meta['replay_n']
    leaves = (1.0 + 99.0 * np.random.default_rng(12).random(n)).astype(np.float32)
    a, twin = (_agent(c, graph=True, pipeline=False, seed=5, extra_feature_steps=3) for _ in range(2))
    buf, plain = _cper(c), _plain(c)
    buf.set_priorities(leaves, 100.0)
    ref = RefTree(n)
    ref.set_leaves(np.arange(n), leaves)
    assert a._plan(B)[0] == ['f0', 'f1', 'f2', 'f3'] and a._critic_key(B) == 'f3'
    a.train(buf, B)
    twin.train(plain, B)
    torch.cuda.synchronize()
    step = int(sg.steps_words(a.core)[0])
    assert step == int(sg.steps_words(twin.core)[0]) == 1
    pa, pt = a._bufs['pool_idx'].cpu().numpy(), twin._bufs['pool_idx'].cpu().numpy()
    assert np.array_equal(pa, pt)                                # the train prologue's uniform draw, all four minibatches of it
    assert np.array_equal(a._bufs['pool_eps'].cpu().numpy(), twin._bufs['pool_eps'].cpu().numpy())
    drawn = buf.draw_buffers(B)[0].cpu().numpy()
    assert np.array_equal(drawn, ref.sample(B, a._seed, PER_STREAM + step))
    assert not np.array_equal(drawn, pa[3 * B:])                 # ... whose last one the critic's minibatch is not
    # the first three feature steps saw the same rows: the feature nets moved as the twin's did up to the last step, so the metrics of
    # the call differ only through it
    got = _slot(a.core, B, c.S, c.A)
    assert np.array_equal(_bits(got['XE']), _bits(buf.ring.cpu().numpy()[drawn][:, :2 * c.S + c.A]))


# ---- 3. alpha = 0 is uniform replay -------------------------------------------------------------------------------------------------------
def _read_back(agent, buf, B):
    """(idx list, eps list) of the graph train() just replayed, in train_injected's order; buf: the CriticPrioritizedReplayBuffer it drew
    its critic minibatch from, or None"""
    torch.cuda.synchronize()
    keys, specs = agent._plan(B)
    pool = agent._bufs['pool_idx'].cpu().numpy().astype(np.int64).reshape(len(keys), B)
    idx = [pool[q].copy() for q in range(len(keys))]
    if buf is not None:
        idx[keys.index(agent._critic_key(B))] = buf.draw_buffers(B)[0].cpu().numpy().astype(np.int64)
    flat, o, pooled = agent._bufs['pool_eps'].cpu().numpy(), 0, {}
    for k, sh in specs:
        m = int(np.prod(sh))
        pooled[k] = flat[o:o + m].reshape(sh).copy()
        o += m
    eps = []
    for i in range(agent._feature_iters()):
        if agent.ALG == 'vlsac':
            eps.append(pooled[f'feat{i}'])
        if agent.ALG == 'diffsrsac':
            eps += [agent._bufs[f'idx_n{i}'].cpu().numpy().astype(np.int64), agent._bufs[f'eps_pert{i}'].cpu().numpy().copy()]
    return idx, eps + [pooled['crit'], pooled['act']]


def _worst(sa, sb):
    w = 0.0
    for k in sa:
        x, y = sa[k].double().cpu().numpy().reshape(-1), sb[k].double().cpu().numpy().reshape(-1)
        if not np.array_equal(x, y):
            w = max(w, float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30)))
    return w


@pytest.mark.parametrize('alg', ALGS)
def test_alpha_zero_is_uniform_replay(alg):
    c = Case(alg + '_tiny')
    B, n = c.B, c.meta['replay_n']

    def run(buf):
        a, twin = _agent(c, graph=True, pipeline=False, seed=11), _agent(c, seed=11)
        plain = _plain(c)
        exact, worst = True, 0.0
        for call in range(5):
            info = a.train(buf, B)
            info = {k: float(info[k]) for k in info.keys()}
            idx, eps = _read_back(a, buf if buf is not plain_ctl else None, B)
            tinfo = twin.train_injected(plain, B, idx, eps)
            tinfo = {k: float(tinfo[k]) for k in tinfo.keys()}
            sa, sb = sg.state(a.core), sg.state(twin.core)
            for st in (sa, sb):
                st.pop('train_steps')                            # (the counter block's mirror word is the graph prologue's own)
            same = all(torch.equal(sa[k], sb[k]) for k in sa) and set(info) == set(tinfo) and all(info[k] == tinfo[k] for k in info)
            exact = exact and same
            worst = max(worst, _worst(sa, sb), max(abs(info[k] - tinfo[k]) / max(abs(tinfo[k]), 1e-2) for k in info))
        return exact, worst

    plain_ctl = _plain(c)
    ctl_exact, ctl_worst = run(plain_ctl)                        # the control: a plain-buffer graph agent against its own injected twin
    per = _cper(c, max_size=n + 36, alpha=0.0, beta=0.4)         # (P = 128 > size: leaves above the fill level)
    exact, worst = run(per)
    print(f'alpha = 0 {alg}: control {"bit-identical" if ctl_exact else f"differs by {ctl_worst:.3e}"}, '
          f'prioritized buffer {"bit-identical" if exact else f"differs by {worst:.3e}"}')
    if ctl_exact:
        assert exact, (alg, worst)
    else:
        assert worst <= RTOL, (alg, worst, ctl_worst)
    t = _tree(per)
    assert np.all(per.draw_buffers(B)[1].cpu().numpy() == 1.0)
    assert np.all(t[per.P:per.P + n] == 1.0) and np.all(t[per.P + n:] == 0) and t[1] == float(n) and per.max_priority == 1.0


@pytest.mark.parametrize('alg', ALGS)
def test_graph_form_equals_the_injected_form_with_real_weights(alg):
    """alpha = 0.6, leaves spread over 1 .. 100: the captured train() -- the weighted head in the critic program that starts behind the early
    policy forwards -- against an eager twin on a buffer of its own, fed the read-back indices (given-indices mode) and noise: state,
    metrics and both trees bit for bit, as the plain control of test_alpha_zero_is_uniform_replay is"""
    c = Case(alg + '_tiny')
    B, n = c.B, c.meta['replay_n']
    leaves = (1.0 + 99.0 * np.random.default_rng(31).random(n)).astype(np.float32)
    a, twin = _agent(c, graph=True, pipeline=False, seed=13), _agent(c, seed=13)
    bufa, bufb = _cper(c, alpha=0.6, beta=0.4), _cper(c, alpha=0.6, beta=0.4)
    for b in (bufa, bufb):
        b.set_priorities(leaves, 100.0)
    for call in range(5):
        info = a.train(bufa, B)
        info = {k: float(info[k]) for k in info.keys()}
        idx, eps = _read_back(a, bufa, B)
        w = bufa.draw_buffers(B)[1].cpu().numpy()
        tinfo = twin.train_injected(bufb, B, idx, eps)
        sg.assert_info_equal(info, {k: float(tinfo[k]) for k in tinfo.keys()}, (alg, call))
        sa, sb = sg.state(a.core), sg.state(twin.core)
        for st in (sa, sb):
            st.pop('train_steps')
        sg.assert_equal(sa, sb, (alg, call))
        assert np.array_equal(_bits(w), _bits(bufb.draw_buffers(B)[1].cpu().numpy())) and not np.all(w == 1.0)
        assert np.array_equal(_bits(bufa.draw_buffers(B)[2].cpu().numpy()), _bits(bufb.draw_buffers(B)[2].cpu().numpy()))
        assert np.array_equal(_tree(bufa), _tree(bufb)) and _invariant(_tree(bufa)), (alg, call)
    assert not np.array_equal(_tree(bufa)[bufa.P:bufa.P + n], leaves)


# ---- 4. the weighted critic step against weighted oracles ---------------------------------------------------------------------------------
def _weighted_oracle(alg, S, A, init, **kw):
    """the oracle of `alg` whose critic_step is restated with the loss (w (q1 - y)^2).mean() + (w (q2 - y)^2).mean(); keeps
    td = 0.5 (|q1 - y| + |q2 - y|) of the step for the priorities (tests/test_per.py WeightedOracleSAC, for the four representation agents)"""
    from oracle import agents as oa
    from oracle import make_oracle
    base = type(make_oracle(alg, S, A, init, **kw))

    class Weighted(base):
        w, td = None, None

        def _targets(self, batch, eps_next):
            """(q1, q2 with gradients, target_q): the first half of the oracle's critic_step, per algorithm"""
            P = self.P
            with torch.no_grad():
                mu, std = oa.actor_mu_std(P, batch.next_state)
                a2, logp = oa.squashed_rsample_logp(mu, std, eps_next)
                if alg == 'vlsac':
                    mean, log_std = oa.gauss_head(P, self.fnet, torch.cat([batch.state, batch.action], -1))
                    nmean, nlog_std = oa.gauss_head(P, self.fnet, torch.cat([batch.next_state, a2], -1))
                    nq1, nq2 = oa.vl_critic(P, 'critic_target', nmean, nlog_std)
                    alpha = self.alpha
                elif alg == 'ctrlsac':
                    fz = 'frozen_phi_target' if self.use_feature_target else 'frozen_phi'
                    z = oa.ctrl_phi(P, fz, batch.state, batch.action)
                    nq1, nq2 = oa.ctrl_critic(P, 'critic_target', oa.ctrl_phi(P, fz, batch.next_state, a2))
                    alpha = self.alpha
                else:
                    z = self.phi(batch.state, batch.action)
                    nq1, nq2 = oa.rff_critic(P, 'critic_target', self.phi(batch.next_state, a2))
                    alpha = self.alpha.detach() if alg == 'diffsrsac' else self.alpha
                target_q = batch.reward + (1. - batch.done) * self.discount * (torch.min(nq1, nq2) - alpha * logp)
            if alg == 'vlsac':
                q1, q2 = oa.vl_critic(P, 'critic', mean, log_std)
            elif alg == 'ctrlsac':
                q1, q2 = oa.ctrl_critic(P, 'critic', z)
            else:
                q1, q2 = oa.rff_critic(P, 'critic', z)
            return q1, q2, target_q

        def critic_step(self, batch, eps_next):
            q1, q2, y = self._targets(batch, eps_next)
            w = self.w.reshape(q1.shape)
            q1_loss, q2_loss = (w * (q1 - y) ** 2).mean(), (w * (q2 - y) ** 2).mean()
            self.td = (0.5 * ((q1 - y).abs() + (q2 - y).abs())).detach().reshape(-1).double().numpy()
            if alg == 'diffsrsac':                               # (quirk Q11: metrics only; lambda = 0 at the fixture's hyper-parameters)
                assert self.reg_lambda == 0
                loss = float((q1_loss + q2_loss).detach())
                return {'q_loss_reg': loss, 'q_loss_noreg': loss, 'q1': q1.mean().item(), 'q2': q1.mean().item()}
            self._apply(self.opt_critic, q1_loss + q2_loss, 'critic')
            return {'q1_loss': q1_loss.item(), 'q2_loss': q2_loss.item(), 'q1': q1.mean().item(), 'q2': q2.mean().item()}

    return Weighted(S, A, init, **{k: v for k, v in kw.items() if k in _oracle_kw(alg, kw)})


def _oracle_kw(alg, kw):
    """the keyword arguments oracle.make_oracle passes on for `alg`"""
    drop = {'hidden_dim', 'alpha', 'phi_hidden_dim', 'mu_hidden_dim', 'critic_and_actor_hidden_dim', 'nabla_mu_hidden_dim', 'num_noises',
            'DARL_noise_a', 'DARL_noise_b', 'action_space', 'state_dim', 'action_dim'}
    if alg not in ('vlsac', 'ctrlsac', 'spedersac'):
        drop.add('use_feature_target')
    if alg != 'diffsrsac':
        drop.add('critic_elu_layer_regularizer_lambda')
    if alg in ('sac', 'vlsac', 'ctrlsac', 'spedersac'):
        drop.add('feature_dim')
    return set(kw) - drop


@pytest.mark.parametrize('alg', ALGS)
def test_weighted_critic_matches_a_weighted_oracle(alg):
    from oracle.agents import gather_batch
    c = Case(alg + '_tiny')
    S, A, B, n = c.S, c.A, c.B, c.meta['replay_n']
    agent, twin = _agent(c), _agent(c)
    buf, plain = _cper(c, alpha=0.6, beta=1.0), _plain(c)
    buf.set_priorities((1.0 + 99.0 * np.random.default_rng(21).random(n)).astype(np.float32), 100.0)       # leaves span 1 .. 100
    o = _weighted_oracle(alg, S, A, c.init, **c.kw)
    torch.set_num_threads(4)
    rs = np.random.RandomState(5)
    P, eps_p, alpha_p = buf.P, float(f32(1e-6)), float(f32(0.6))
    worst = dict(info=0.0, grad=0.0, leaf=0.0, param=0.0)
    for t in range(3):
        idx, eps = nref.injected_draws(rs, alg, o, S, A, B, c.kw.get('feature_dim', 0), n)
        crit = idx[-2] if alg == 'spedersac' else idx[-1]
        leaves = _tree(buf)[P + crit].astype(np.float64)         # the weights from the read-back leaves, beta = 1
        o.w = torch.as_tensor(leaves.min() / leaves, dtype=torch.float32)
        info = agent.train_injected(buf, B, idx, eps)
        info = {k: float(info[k]) for k in info.keys()}
        oinfo = nref.oracle_train(o, [gather_batch(c.replay, i) for i in idx], [torch.as_tensor(e) for e in eps])
        for k, v in oinfo.items():
            err = abs(info[k] - v) / max(abs(v), 1e-2)
            worst['info'] = max(worst['info'], float(err))
            assert err <= RTOL, (alg, t, k, info[k], v)
        for pname, g in o.last_grads.get('critic', {}).items() if alg != 'diffsrsac' else ():
            gerr = rel_l2(agent.core.view(pname, 'grad').cpu().numpy(), g.numpy())
            worst['grad'] = max(worst['grad'], gerr)
            assert gerr < RTOL, (alg, t, pname, gerr)
        # the leaves at the critic's indices: (0.5 (|d1| + |d2|) + eps)^alpha from the oracle, the maximum where an index repeats
        want = np.zeros(n)
        np.maximum.at(want, crit, np.power(o.td + eps_p, alpha_p))
        touched = np.unique(crit)
        tree = _tree(buf)
        lerr = np.abs(tree[P + touched].astype(np.float64) - want[touched]) / want[touched]
        worst['leaf'] = max(worst['leaf'], float(lerr.max()))
        assert np.all(lerr <= RTOL), (alg, t, lerr.max())
        assert _invariant(tree)
        # the feature losses take no weights: a plain agent fed the same indices reports the same feature metrics, bit for bit
        tinfo = twin.train_injected(plain, B, idx, eps)
        assert len(agent.FEATURE_KEYS) >= 1
        for k in agent.FEATURE_KEYS:
            assert info[k] == float(tinfo[k]), (alg, t, k, info[k], float(tinfo[k]))
    st, Pm = agent.core.state(), o.state()
    for k in st:
        if k in Pm and not k.endswith('noise') and k != 'noise_alphabars':
            e = rel_l2(st[k].numpy(), Pm[k].numpy())
            worst['param'] = max(worst['param'], e)
            assert e < RTOL, (alg, k, e)
    print(f'weighted parity {alg}: worst metric {worst["info"]:.2e} critic gradient {worst["grad"]:.2e} updated leaf {worst["leaf"]:.2e} '
          f'parameter {worst["param"]:.2e}')


# ---- 5. launches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [3, 0])
@pytest.mark.parametrize('alg', ['vlsac', 'ctrlsac'])
def test_two_launches_more_and_the_plain_forms_come_back(alg, extra):
    c = Case(alg + '_tiny')
    B = c.B
    buf, plain = _cper(c), _plain(c)
    a, twin = (_agent(c, graph=True, pipeline=False, seed=3, extra_feature_steps=extra) for _ in range(2))
    twin.train(plain, B)
    a.train(buf, B)
    torch.cuda.synchronize()
    print(f'launches in a captured {alg} train(), extra_feature_steps = {extra}: plain {twin._graph_launches}, prioritized critic {a._graph_launches}')
    assert a._graph_launches == twin._graph_launches + 2
    assert a._graph_cache_key(plain, B) != a._graph_cache_key(buf, B)
    a.train(plain, B)                                            # back to a plain buffer: the parent's graph
    torch.cuda.synchronize()
    assert a._graph_launches == twin._graph_launches and a._form() == 'graph'
    # an agent on the two-chain form: the new buffer takes the one-graph form and leaves no pair pending; a plain buffer gets the two chains back
    p, ptwin = (_agent(c, graph=True, pipeline=True, seed=3, extra_feature_steps=extra) for _ in range(2))
    assert p._form() == 'two_chains'
    for _ in range(2):
        ptwin.train(plain, B)
        p.train(plain, B)
    assert p._pending
    p.train(buf, B)
    assert not p._pending and p._graph_launches == twin._graph_launches + 2
    p.train(buf, B)
    assert not p._pending
    p.train(plain, B)
    assert p._pending and p._pipe['launches'] == ptwin._pipe['launches']
    p.flush(); ptwin.flush()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v.float()).all()) for v in sg.state(p.core).values())


# ---- 6. a long graph run, save and restore ------------------------------------------------------------------------------------------------
def test_graph_training_keeps_the_tree_and_survives_save_restore(tmp_path):
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer
    c = Case('vlsac_tiny')
    B, n = c.B, c.meta['replay_n']
    cap = n + 36                                                 # P = 128: leaves above the fill level stay 0
    a, bufa = _agent(c, graph=True, seed=2), _cper(c, max_size=cap, alpha=0.6, beta=0.4)
    for _ in range(200):
        a.train(bufa, B)
    st = sg.state(a.core)
    assert all(bool(torch.isfinite(v.float()).all()) for v in st.values())
    t, P = _tree(bufa), bufa.P
    assert _invariant(t) and np.all(t[P:P + n] > 0) and np.all(t[P + n:] == 0) and bufa.max_priority >= float(t[P:].max())
    assert len(np.unique(t[P:P + n])) > n // 2                   # priorities moved
    b, bufb = _agent(c, graph=True, seed=2), _cper(c, max_size=cap, alpha=0.6, beta=0.4)
    for _ in range(195):
        b.train(bufb, B)
    path = str(tmp_path / 'ring.npz')
    bufb.save(path)
    bufc = CriticPrioritizedReplayBuffer(c.S, c.A, max_size=cap, alpha=0.6, beta=0.4)
    bufc.restore(path)
    for _ in range(5):
        b.train(bufc, B)
    sg.assert_equal(st, sg.state(b.core), 'after restore')
    assert np.array_equal(t, _tree(bufc)) and bufc.max_priority == bufa.max_priority


# ---- 7. refusals on the device ------------------------------------------------------------------------------------------------------------
def test_everything_else_refuses_the_class_by_name():
    import bench
    from rlrep_amd._lib import lib
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer, PrioritizedReplayBuffer
    c, cs = Case('vlsac_tiny'), Case('sac_tiny')
    v, sac = _agent(c, graph=True), _agent(cs)
    buf = _cper(c)
    with pytest.raises(RuntimeError, match=r'SACAgent\.train: CriticPrioritizedReplayBuffer.*use PrioritizedReplayBuffer'):
        sac.train(buf, c.B)
    with pytest.raises(RuntimeError, match=r'SACAgent\.train_injected: CriticPrioritizedReplayBuffer'):
        sac.train_injected(buf, c.B, [], [])
    for G, kw in ((SACSeedBatch, dict(hidden_dim=32)), (CTRLSACSeedBatch, dict(hidden_dim=32, feature_dim=16, extra_feature_steps=0))):
        g = G([0, 1], c.S, c.A, bench.Space(c.A), max_batch=c.B, **kw)
        with pytest.raises(RuntimeError, match=G.__name__ + r'\.train: CriticPrioritizedReplayBuffer does not train a seed group'):
            g.train(buf, c.B)
    for what in ('iterate', 'iterate_sim'):
        with pytest.raises(RuntimeError, match=rf'VLSACAgent\.{what}: CriticPrioritizedReplayBuffer cannot be written'):
            getattr(v, what)(object(), buf, c.B)
    # the old class with a vlsac agent: as before
    with pytest.raises(RuntimeError, match=r'PrioritizedReplayBuffer is built for SACAgent only \(vlsac reuses'):
        v.train(_load(PrioritizedReplayBuffer(c.S, c.A, max_size=c.meta['replay_n']), c), c.B)
    # the two entry points that take an agent, by name
    idx, w, td = buf.draw_buffers(c.B)
    err = lambda: lib.rlrep_last_error().decode()
    p = lambda t: C.c_void_p(t.data_ptr())
    for core, word in ((g.core, 'seed group'), (sac.core, 'use rlrep_per_sample / rlrep_critic_step_weighted')):
        rc = lib.rlrep_per_sample_fill(core.h, p(buf.ring), buf.max_size, p(buf.tree), buf.P, p(buf._scal), p(idx), p(w), c.B, 0, 1, PER_STREAM, None, None)
        assert rc < 0 and word in err() and 'per_sample_fill' in err()
        rc = lib.rlrep_critic_weights_arm(core.h, p(w), p(td))
        assert rc < 0 and word in err() and 'critic_weights_arm' in err()
    assert lib.rlrep_critic_weights_arm(v.core.h, p(w), None) < 0 and 'critic_weights_arm' in err()
    assert lib.rlrep_per_sample_fill(v.core.h, p(buf.ring), buf.P + 1, p(buf.tree), buf.P, p(buf._scal), p(idx), p(w), c.B, 0, 1, PER_STREAM, None, None) < 0
    assert lib.rlrep_per_update_td(p(buf.tree), buf.P, p(buf._scal), p(idx), None, c.B, None) < 0 and 'per_update_td' in err()
    assert lib.rlrep_critic_weights_arm(v.core.h, p(w), p(td)) == 1 and lib.rlrep_critic_weights_arm(v.core.h, None, None) == 0
    v.train(buf, c.B)                                            # ... and the agent it is built for trains
    torch.cuda.synchronize()
    assert _invariant(_tree(buf))


# ---- 8. the launcher ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg,extra', [('vlsac', ['--hidden_dim', '64', '--feature_dim', '64', '--start_timesteps', '300', '--eval_freq', '300',
                                                  '--max_timesteps', '600']),
                                       ('ctrlsac', ['--host-envs', '4', '--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '320']),
                                       ('diffsrsac', ['--torch-envs', '8', '--start_timesteps', '304', '--eval_freq', '304', '--max_timesteps', '608'])])
def test_launcher_runs_with_critic_per(tmp_path, alg, extra):
    import glob
    import json
    from rlrep_amd import main
    agent, evaluations = main.run(['--alg', alg, '--env', 'Pendulum-v1', '--critic-per', '--batch_size', '64', '--eval_episodes', '1',
                                   '--log_root', str(tmp_path)] + extra)
    assert np.all(np.isfinite(np.asarray(evaluations, np.float64))) and len(evaluations) >= 2
    buf = agent._held_buffer
    assert type(buf).__name__ == 'CriticPrioritizedReplayBuffer' and buf.beta == 1.0 and buf._scal[2].item() == 1.0
    assert not agent._pending and agent._graph_key[4] == 'critic_per'
    rows = [json.loads(line) for f in glob.glob(str(tmp_path / '**' / 'metrics.jsonl'), recursive=True) for line in open(f)]
    assert rows and all(np.isfinite(v) for row in rows for v in row.values())
    t = _tree(buf)
    assert _invariant(t) and np.all(t[buf.P:buf.P + buf.size] > 0) and np.all(t[buf.P + buf.size:] == 0)
    assert len(np.unique(t[buf.P:buf.P + buf.size])) > 10        # priorities moved
