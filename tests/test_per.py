"""GPU: prioritized replay for sac (csrc/per.hip).  The three tree kernels against tests/per_reference.py (exact wherever no
powf is involved), alpha = 0 as uniform replay bit for bit, the weighted critic step against a weighted CPU oracle, the graph form, the
refusals and the launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

from per_reference import PER_STREAM, RefTree, f32
from seed_group_util import assert_equal, assert_info_equal, standalone, state

pytestmark = pytest.mark.gpu

S, A, B = 3, 1, 64              # sac Pendulum dims
WL = 'sac_pendulum_b64'
RTOL = 1e-4                     # the repository's bar (tests/test_hip_parity.py)
PLAIN_SAC_LAUNCHES = 18         # kernels in a captured plain sac train() at these dims: must not move


def _prb(max_size=1000, **kw):
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer
    return PrioritizedReplayBuffer(S, A, max_size=max_size, **kw)


def _rows(n, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, S)).astype(np.float32), r.uniform(-1, 1, size=(n, A)).astype(np.float32), r.normal(size=(n, S)).astype(np.float32),
            r.normal(size=n).astype(np.float32), (r.random(n) < 0.05).astype(np.float32))


def _tree(buf):
    torch.cuda.synchronize()
    return buf.tree.cpu().numpy()


def _invariant(tree):
    P = len(tree) // 2
    n = np.arange(1, P)
    return bool(np.array_equal(tree[n], (tree[2 * n] + tree[2 * n + 1]).astype(f32)))


@pytest.fixture(scope='module')
def agent():
    return standalone(WL, 5)


# ---- the kernels against the restatement -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def hand_set():
    """a ring of 1000 rows (P = 1024) at size 700 with leaves set by hand: a heavy leaf, and size < 512 would zero the right subtree -- here
    rows 512 .. 699 are zeroed instead, so the root's right subtree is all zero while size stays 700"""
    buf, ref = _prb(1000), RefTree(1000)
    buf.load(*[x[:700] for x in _rows(700)])
    leaves = (1.0 + np.random.default_rng(4).random(700) * 9.0).astype(np.float32)
    leaves[137] = f32(1e6)
    leaves[512:] = 0
    buf.set_priorities(leaves, 1.0)
    ref.set_leaves(np.arange(700), leaves)
    assert np.array_equal(_tree(buf), ref.tree)
    assert ref.tree[3] == 0
    return buf, ref


@pytest.mark.parametrize('batch', [50, 256])
@pytest.mark.parametrize('beta', [0.0, 0.4, 1.0])
def test_sample_equals_the_reference(agent, hand_set, batch, beta):
    buf, ref = hand_set
    buf.beta = beta
    ref.beta = f32(beta)
    worst = 0.0
    for call in range(3):
        off = PER_STREAM + 1000 * batch + call
        idx, w = buf.draw(batch, 2024, off, core=agent.core)
        torch.cuda.synchronize()
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        want = ref.sample(batch, 2024, off)
        assert np.array_equal(idx, want), (batch, call)
        assert idx.max() < 512
        wr, exact = ref.weights(want)
        assert np.all(w[exact] == 1.0)
        if beta == 0.0:
            assert np.all(w == 1.0)
        err = np.abs(w - wr) / wr
        worst = max(worst, float(err.max()))
        assert np.all(err <= RTOL)
    print(f'per_sample B={batch} beta={beta}: largest relative error of w against float64 pow {worst:.3e}')
    # the given-indices mode: only the weights
    given = (np.arange(batch, dtype=np.int32) * 7) % 512
    idx, w = buf.draw(batch, 0, 0, core=agent.core, given=given)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), given)
    wr, exact = ref.weights(given)
    w = w.cpu().numpy()
    assert np.all(w[exact] == 1.0) and np.all(np.abs(w - wr) / wr <= RTOL)


def test_sample_reads_the_device_counter(agent, hand_set):
    """offset + *counter_dev, as a graph replay draws: the agent's train() counter"""
    from rlrep_amd._lib import lib
    buf, ref = hand_set
    from seed_group_util import steps_words
    step = int(steps_words(agent.core)[0])
    idx, _ = buf.draw(50, 7, PER_STREAM, core=agent.core, counter_dev=lib.rlrep_steps_dev(agent.core.h))
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), ref.sample(50, 7, PER_STREAM + step))


def test_add_ranges_equal_the_reference():
    buf, ref = _prb(1000), RefTree(1000)
    s, a, s2, r, d = _rows(1300)
    buf.add(s[0], a[0], s2[0], r[0], d[0])                       # n = 1
    buf.flush()
    ref.add(0, 1)
    assert np.array_equal(_tree(buf), ref.tree)
    buf.add_batch(s[1:850], a[1:850], s2[1:850], r[1:850], d[1:850])
    buf.flush()
    ref.add(1, 849)
    assert np.array_equal(_tree(buf), ref.tree)
    buf.set_priorities(np.full(850, 2.5, np.float32), 2.5)       # the next rows enter at the maximum the LAUNCH reads
    ref.set_leaves(np.arange(850), 2.5); ref.max_p = f32(2.5)
    buf.add_batch(s[850:1150], a[850:1150], s2[850:1150], r[850:1150], d[850:1150])      # n = 300 across the wrap (850 .. 1149 mod 1000)
    buf.flush()
    ref.add(850, 300)
    t = _tree(buf)
    assert np.array_equal(t, ref.tree) and t[1024 + 149] == 2.5 and t[1024 + 150] == 2.5 and buf.ptr == 150 and _invariant(t)
    # add_device: 3000 rows into a 4096-row ring from row 3500
    big, bref = _prb(4096), RefTree(4096)
    s, a, s2, r, d = _rows(4096, 1)
    big.load(s[:3500], a[:3500], s2[:3500], r[:3500], d[:3500])
    bref.add(0, 3500)
    dev = [torch.from_numpy(x[:3000]).cuda() for x in (s, a, s2, r, d)]
    big.add_device(*dev)
    bref.add(3500, 3000)
    assert np.array_equal(_tree(big), bref.tree) and big.ptr == (3500 + 3000) % 4096 and big.size == 4096
    # load of a full ring
    big.load(s, a, s2, r, d)
    bref.clear(); bref.add(0, 4096)
    t = _tree(big)
    assert np.array_equal(t, bref.tree) and t[1] == 4096.0


def test_load_of_fewer_rows_drops_the_leaves_of_the_rows_it_no_longer_holds(agent):
    """load() resets the ring to its first n rows: leaves of rows >= size are 0 again, and nothing above size is ever drawn"""
    buf, ref = _prb(1000), RefTree(1000)
    s, a, s2, r, d = _rows(1000, 2)
    buf.load(s, a, s2, r, d)                                     # a full ring whose priorities have moved
    buf.set_priorities((1.0 + np.arange(1000) % 7).astype(np.float32), 7.0)
    buf.load(s[:300], a[:300], s2[:300], r[:300], d[:300])
    ref.max_p = f32(7.0)
    ref.add(0, 300)
    t = _tree(buf)
    assert buf.size == 300 and np.all(t[1024 + 300:] == 0) and np.array_equal(t, ref.tree) and t[1] == 2100.0
    for call in range(5):
        idx, _ = buf.draw(256, 3, PER_STREAM + call, core=agent.core)
        torch.cuda.synchronize()
        idx = idx.cpu().numpy()
        assert idx.min() >= 0 and idx.max() < 300 and np.array_equal(idx, ref.sample(256, 3, PER_STREAM + call))


def test_update_takes_the_maximum_of_duplicates(agent):
    buf, ref = _prb(1000), RefTree(1000)
    buf.load(*[x[:700] for x in _rows(700)])
    rng = np.random.default_rng(9)
    batch = 256
    given = rng.integers(0, 700, size=batch).astype(np.int32)
    given[200:] = given[:56]                                     # at least 56 duplicated indices (more by chance)
    assert batch - len(np.unique(given)) >= 40
    buf.draw(batch, 0, 0, core=agent.core, given=given)
    td = (rng.random(batch) * 4).astype(np.float32)
    td_dev = torch.from_numpy(td).cuda()
    buf.update(batch, td=td_dev, core=agent.core)
    t = _tree(buf)
    new = ref.new_priorities(td_dev.cpu().numpy())               # float64 pow of the read-back td
    want = np.zeros(1000)
    np.maximum.at(want, given, new)
    touched = np.unique(given)
    got = t[1024 + touched]
    err = np.abs(got - want[touched]) / want[touched]
    print(f'per_update: largest relative error of a leaf against float64 pow {err.max():.3e}')
    assert np.all(err <= RTOL)
    untouched = np.setdiff1d(np.arange(700), touched)
    assert np.all(t[1024 + untouched] == 1.0) and np.all(t[1024 + 700:] == 0)
    # the tree above the device's own leaves, bit for bit
    ref.tree[1024:] = t[1024:]
    ref.rebuild()
    assert np.array_equal(t, ref.tree)
    assert buf.max_priority == max(1.0, float(got.max()))


def test_an_updated_leaf_stays_positive_on_the_device(agent):
    """a NaN td, or td = 0 with eps = 0: the floor (the smallest normal float32), never 0 -- the row stays in the tree and max_p ignores it"""
    from per_reference import PER_MIN_PRIORITY
    buf = _prb(16, eps=0.0)
    buf.load(*_rows(16))
    buf.draw(4, 0, 0, core=agent.core, given=np.array([2, 5, 5, 9], np.int32))
    buf.update(4, td=torch.tensor([0.0, float('nan'), 1.0, float('nan')], device='cuda'), core=agent.core)
    t = _tree(buf)
    assert t[16 + 2] == PER_MIN_PRIORITY and t[16 + 9] == PER_MIN_PRIORITY and t[16 + 5] == 1.0 and np.all(t[16:] > 0)
    assert _invariant(t) and np.isfinite(t).all() and buf.max_priority == 1.0


# ---- alpha = 0 is uniform replay ---------------------------------------------------------------------------------------------------------
def test_alpha_zero_is_uniform_replay_bit_for_bit():
    from rlrep_amd.utils.buffer import ReplayBuffer
    rows = _rows(700, 3)
    per = _prb(1000, alpha=0.0, beta=0.4)
    per.load(*rows)
    plain = ReplayBuffer(S, A, max_size=1000)
    plain.load(*rows)
    a, twin = standalone(WL, 11), standalone(WL, 11)
    for call in range(10):
        info = a.train(per, B)
        torch.cuda.synchronize()
        idx = per.draw_buffers(B)[0].cpu().numpy().astype(np.int64)
        w = per.draw_buffers(B)[1].cpu().numpy()
        eps = a._bufs['pool_eps'].cpu().numpy().reshape(2, B, A)
        assert np.all(w == 1.0) and idx.min() >= 0 and idx.max() < 700
        tinfo = twin.train_injected(plain, B, [idx], [eps[0].copy(), eps[1].copy()])
        assert_info_equal(dict(info), dict(tinfo), call)
        sa, sb = state(a.core), state(twin.core)
        for st in (sa, sb):
            st.pop('train_steps')           # (the counter block's mirror word is the graph prologue's own; the counter itself: a.steps == twin.steps)
        assert_equal(sa, sb, call)
    t = _tree(per)
    assert np.all(t[1024:1024 + 700] == 1.0) and t[1] == 700.0 and per.max_priority == 1.0


# ---- the weighted critic step against a weighted oracle ----------------------------------------------------------------------------------
def test_weighted_critic_matches_a_weighted_oracle():
    from fixture_io import Case, rel_l2
    from oracle.agents import OracleSAC, gather_batch
    import torch.nn.functional as F
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer

    class WeightedOracleSAC(OracleSAC):
        """OracleSAC whose critic loss is (w (q1 - y)^2).mean() + (w (q2 - y)^2).mean(); keeps |q - y| of the step for the priorities"""
        w = None

        def critic_step(self, batch, eps_next):
            from oracle.agents import actor_mu_std, squashed_rsample_logp
            P = self.P
            with torch.no_grad():
                mu, std = actor_mu_std(P, batch.next_state)
                a2, logp = squashed_rsample_logp(mu, std, eps_next)
                tq1, tq2 = self.q_pair('critic_target', batch.next_state, a2)
                target_q = batch.reward + (1. - batch.done) * self.discount * (torch.min(tq1, tq2) - self.alpha.detach() * logp)
            q1, q2 = self.q_pair('critic', batch.state, batch.action)
            w = self.w.reshape(q1.shape)
            loss = (w * (q1 - target_q) ** 2).mean() + (w * (q2 - target_q) ** 2).mean()
            self.td = (0.5 * ((q1 - target_q).abs() + (q2 - target_q).abs())).detach().reshape(-1).double().numpy()
            self._apply(self.opt_critic, loss, 'critic')
            return {'q_loss': loss.item(), 'q1': q1.mean().item(), 'q2': q1.mean().item()}

    c = Case('sac_tiny')

    class Space:
        low, high = -c.meta['bound'] * np.ones(c.A, np.float32), c.meta['bound'] * np.ones(c.A, np.float32)
    agent = SACAgent(state_dim=c.S, action_dim=c.A, action_space=Space(), max_batch=B, graph=False, **c.kw)
    agent.core.load_state(c.init)
    n = c.meta['replay_n']
    buf = PrioritizedReplayBuffer(c.S, c.A, max_size=n, alpha=0.6, beta=1.0)
    r = c.replay
    buf.load(r['state'], r['action'], r['next_state'], r['reward'], r['done'])
    rng = np.random.default_rng(21)
    buf.set_priorities((1.0 + 99.0 * rng.random(n)).astype(np.float32), 100.0)       # leaves span 1 .. 100
    o = WeightedOracleSAC(c.S, c.A, c.init, **c.kw)
    torch.set_num_threads(4)
    rs = np.random.RandomState(5)
    P, eps_p, alpha_p = buf.P, float(f32(1e-6)), float(f32(0.6))
    worst_grad = 0.0
    for t in range(3):
        idx = rs.randint(0, n, size=B)
        eps = [rs.standard_normal((B, c.A)).astype(np.float32) for _ in range(2)]
        leaves = _tree(buf)[P + idx].astype(np.float64)           # the weights from the read-back leaves, beta = 1
        o.w = torch.as_tensor(leaves.min() / leaves, dtype=torch.float32)
        info = agent.train_injected(buf, B, [idx], eps)
        oinfo = o.train([gather_batch(c.replay, idx)], [torch.as_tensor(e) for e in eps])
        for k, v in oinfo.items():
            assert abs(info[k] - v) <= RTOL * max(abs(v), 1e-2), (t, k, info[k], v)
        for pname, g in o.last_grads['critic'].items():
            gerr = rel_l2(agent.core.view(pname, 'grad').cpu().numpy(), g.numpy())
            worst_grad = max(worst_grad, gerr)
            assert gerr < RTOL, (t, pname, gerr)
        # the leaves at the batch indices: (0.5 (|d1| + |d2|) + eps)^alpha from the oracle, the maximum where an index repeats
        want = np.zeros(n)
        np.maximum.at(want, idx, np.power(o.td + eps_p, alpha_p))
        got = _tree(buf)[P + np.unique(idx)].astype(np.float64)
        err = np.abs(got - want[np.unique(idx)]) / want[np.unique(idx)]
        print(f'weighted parity call {t}: largest relative error of an updated leaf {err.max():.3e}')
        assert np.all(err <= RTOL), (t, err.max())
        assert _invariant(_tree(buf))
    print(f'weighted parity: largest relative L2 error of a critic gradient {worst_grad:.3e}')
    st, Pm = agent.core.state(), o.state()
    for k in st:
        if k in Pm:
            assert rel_l2(st[k].numpy(), Pm[k].numpy()) < RTOL, k


# ---- the graph form ----------------------------------------------------------------------------------------------------------------------
def test_graph_launch_count_is_a_plain_train_plus_three():
    from rlrep_amd.utils.buffer import ReplayBuffer
    rows = _rows(700, 3)
    plain = ReplayBuffer(S, A, max_size=1000)
    plain.load(*rows)
    per = _prb(1000)
    per.load(*rows)
    a, b = standalone(WL, 1), standalone(WL, 1)
    a.train(plain, B)
    b.train(per, B)
    torch.cuda.synchronize()
    print(f'launches in a captured sac train(): plain {a._graph_launches}, prioritized {b._graph_launches}')
    assert b._graph_launches <= a._graph_launches + 3
    assert a._graph_launches == PLAIN_SAC_LAUNCHES
    # one agent, both buffers: the graph cache key tells them apart
    assert a._graph_cache_key(plain, B) != a._graph_cache_key(per, B)
    a.train(per, B)
    a.train(plain, B)
    torch.cuda.synchronize()
    assert a._graph_launches == PLAIN_SAC_LAUNCHES


def test_graph_training_keeps_the_tree_and_survives_save_restore(tmp_path):
    rows = _rows(700, 8)

    def fresh():
        buf = _prb(1000, alpha=0.6, beta=0.4)
        buf.load(*rows)
        return buf
    a, bufa = standalone(WL, 2), fresh()
    for _ in range(200):
        a.train(bufa, B)
    st = state(a.core)
    assert all(bool(torch.isfinite(v.float()).all()) for v in st.values())
    t = _tree(bufa)
    assert _invariant(t) and np.all(t[1024:1024 + 700] > 0) and np.all(t[1024 + 700:] == 0) and bufa.max_priority >= float(t[1024:].max())
    assert len(np.unique(t[1024:1024 + 700])) > 100              # priorities moved
    # the same 195 calls, then save -> restore into a fresh buffer, then 5 more: bit-identical to the uninterrupted run
    b, bufb = standalone(WL, 2), fresh()
    for _ in range(195):
        b.train(bufb, B)
    path = str(tmp_path / 'ring.npz')
    bufb.save(path)
    bufc = _prb(1000, alpha=0.6, beta=0.4)
    bufc.restore(path)
    for _ in range(5):
        b.train(bufc, B)
    assert_equal(st, state(b.core), 'after restore')
    assert np.array_equal(t, _tree(bufc)) and bufc.max_priority == bufa.max_priority


# ---- refusals on the device --------------------------------------------------------------------------------------------------------------
def test_everything_but_one_sac_agent_refuses_the_buffer():
    from fixture_io import Case
    from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.envs.device import DevicePendulum
    import bench
    c = Case('vlsac_tiny')

    class Space:
        low, high = -np.ones(c.A, np.float32), np.ones(c.A, np.float32)
    v = VLSACAgent(state_dim=c.S, action_dim=c.A, action_space=Space(), max_batch=c.B, vae_hidden_dim=c.meta['patch_vae_hidden'], **c.kw)
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer
    vb = PrioritizedReplayBuffer(c.S, c.A, max_size=256)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBuffer'):
        v.train(vb, c.B)
    buf = _prb(1000)
    buf.load(*_rows(300))
    g = SACSeedBatch([0, 1], S, A, bench.Space(A), max_batch=B, hidden_dim=64)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBuffer'):
        g.train(buf, B)
    a = standalone(WL, 3)
    env = DevicePendulum(a)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBuffer'):
        a.iterate(env, buf, B)
    # the C entry points, by name: a seed group's handle and an agent that is not sac
    from rlrep_amd._lib import lib
    idx, w = buf.draw_buffers(B)
    for core, word in ((g.core, 'seed group'), (v.core, 'sac only')):
        rc = lib.rlrep_per_sample(core.h, C.c_void_p(buf.tree.data_ptr()), buf.P, C.c_void_p(buf._scal.data_ptr()), C.c_void_p(idx.data_ptr()),
                                  C.c_void_p(w.data_ptr()), B, 0, 1, PER_STREAM, None, None)
        assert rc < 0 and word in lib.rlrep_last_error().decode() and 'per_sample' in lib.rlrep_last_error().decode()
        rc = lib.rlrep_critic_step_weighted(core.h, C.c_void_p(w.data_ptr()), C.c_void_p(w.data_ptr()), None)
        assert rc < 0 and word in lib.rlrep_last_error().decode()
        rc = lib.rlrep_per_update(core.h, C.c_void_p(buf.tree.data_ptr()), buf.P, C.c_void_p(buf._scal.data_ptr()), C.c_void_p(idx.data_ptr()), None, B, None)
        assert rc < 0 and word in lib.rlrep_last_error().decode()
    torch.cuda.synchronize()


# ---- the launcher ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extra', [[], ['--torch-envs', '8']])
def test_launcher_runs_with_per(tmp_path, extra):
    from rlrep_amd import main
    start = ['--start_timesteps', '304', '--eval_freq', '304', '--max_timesteps', '608'] if extra else \
            ['--start_timesteps', '300', '--eval_freq', '300', '--max_timesteps', '600']
    agent, evaluations = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--per', '--batch_size', '64', '--eval_episodes', '1',
                                   '--log_root', str(tmp_path)] + start + extra)
    assert np.all(np.isfinite(evaluations)) and len(evaluations) >= 2
    buf = agent._held_buffer
    assert type(buf).__name__ == 'PrioritizedReplayBuffer' and buf.beta == 1.0 and buf._scal[2].item() == 1.0
    import glob
    import json
    rows = [json.loads(line) for f in glob.glob(str(tmp_path / '**' / 'metrics.jsonl'), recursive=True) for line in open(f)]
    assert rows and all(np.isfinite(v) for row in rows for v in row.values())
    assert _invariant(_tree(buf))
