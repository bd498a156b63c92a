"""GPU: prioritized critic replay for ctrlsac seed groups (csrc/per_group.hip).  The fused group launch against
tests/per_reference.py, against rlrep_per_sample_fill on a standalone ctrlsac agent and against the members' ring rows; member r of a
CTRLSACSeedBatch training from a CriticPrioritizedReplayBufferGroup against its standalone twin -- CTRLSACAgent(seed=s_r, pipeline=False) on a
CriticPrioritizedReplayBuffer(alpha_r, beta_r) fed the same rows -- bit for bit; which minibatches are prioritized; alpha = 0 as uniform replay;
the launch counts; retire / revive; the refusals and the launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

import bench
import seed_group_util as sg
from per_reference import PER_STREAM, RefTree, f32

pytestmark = pytest.mark.gpu

WL = 'ctrlsac_halfcheetah_f256_b256'
S, A, B = 17, 6, 256
SEEDS = (3, 11, 42)
R = len(SEEDS)
N, P = 1000, 1024               # ring rows of the training tests: P = 1024, 24 padding leaves
RTOL = 1e-4                     # the repository's bar (tests/test_hip_parity.py)
TINY = dict(hidden_dim=16, feature_dim=8)          # the ctrlsac_tiny fixture's network, for the kernel cases
BMAX = 300


def _rows(n, s, a, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, s)).astype(np.float32), r.uniform(-1, 1, size=(n, a)).astype(np.float32), r.normal(size=(n, s)).astype(np.float32),
            r.normal(size=n).astype(np.float32), (r.random(n) < 0.05).astype(np.float32))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _invariant(tree):
    n = np.arange(1, len(tree) // 2)
    return bool(np.array_equal(tree[n], (tree[2 * n] + tree[2 * n + 1]).astype(f32)))


def _trees(gb):
    torch.cuda.synchronize()
    return gb.trees.cpu().numpy()


def _gbuf(s=S, a=A, n=N, **kw):
    from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup
    return CriticPrioritizedReplayBufferGroup(R, s, a, max_size=n, **kw)


def _cbuf(s=S, a=A, n=N, **kw):
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer
    return CriticPrioritizedReplayBuffer(s, a, max_size=n, **kw)


def _member_view(g, t, r):
    """member r's copy of tensor `t` of member 0's block (the train() pools)"""
    torch.cuda.synchronize()
    off = t.data_ptr() - g.core._block.data_ptr() + r * g.core.member_stride
    return g.core._block[off:off + t.numel() * t.element_size()].view(t.dtype).clone()


def _pools(g, r):
    """member r's index pool and noise pool of the last train() (the group keeps them inside the member blocks)"""
    ni, ne = g._pool_sizes(B)
    return _member_view(g, g._buf('pool_idx', (ni,), torch.int32), r), _member_view(g, g._buf('pool_eps', (ne,)), r)


def _member_slot(g, r, batch, s, a):
    """the six arrays of member r's minibatch slot 0, read back (rlrep_slot_dev 0 .. 5 is member 0's; member r's lies r member strides on)"""
    from rlrep_amd._lib import lib
    torch.cuda.synchronize()
    shapes = dict(XE=(batch, 2 * s + a), XF=(batch, s + a), XF2=(batch, s + a), XFpi=(batch, s + a), R=(batch,), D=(batch,))
    out = {}
    for k, (name, sh) in enumerate(shapes.items()):
        off = lib.rlrep_slot_dev(g.core.h, 0, k) - g.core.workspace.data_ptr()
        out[name] = g._members[r].workspace[off:off + 4 * int(np.prod(sh))].view(torch.float32).cpu().numpy().reshape(sh)
    return out


def _poison_slots(g, batch, s, a):
    from rlrep_amd._lib import lib
    for r in range(R):
        for k, n in enumerate((batch * (2 * s + a), batch * (s + a), batch * (s + a), batch * (s + a), batch, batch)):
            off = lib.rlrep_slot_dev(g.core.h, 0, k) - g.core.workspace.data_ptr()
            g._members[r].workspace[off:off + 4 * n].view(torch.float32).fill_(-7.25)


# ---- 1. the fused launch ------------------------------------------------------------------------------------------------------------------
HAND_BETA = (0.0, 0.4, 1.0)
_hand = {}


def _hand_set(s, a):
    """per (S, A), once: a ctrlsac group of three with the ctrlsac_tiny network whose members' train() counters differ; rings of 1000 rows
    (P = 1024) at size 700 with tests/test_per.py's hand-set leaves per member -- a leaf of 1e6 at a different row for each member, rows
    512 .. 699 zeroed (the root's right subtree has no mass), a different random leaf seed and beta per member -- the restatements of the
    trees, and a standalone ctrlsac agent with one CriticPrioritizedReplayBuffer per member holding that member's rows and leaves"""
    if (s, a) not in _hand:
        from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
        from rlrep_amd.utils.buffer_group import ReplayBufferGroup
        g = CTRLSACSeedBatch(list(SEEDS), s, a, bench.Space(a), max_batch=BMAX, extra_feature_steps=0, **TINY)
        # counters that differ: one train() with everybody, one more while member 2 is retired
        warm = ReplayBufferGroup(R, s, a, max_size=64)
        for m in range(R):
            warm.load(m, *_rows(64, s, a, 900 + m))
        g.train(warm, 16)
        g.retire_members([2])
        g.train(warm, 16)
        g.revive_members([2])
        steps = [int(sg.steps_words(g._members[m])[0]) for m in range(R)]
        assert steps == [2, 2, 1]
        gb, refs, alone, rings = _gbuf(s, a, beta=list(HAND_BETA)), [], [], []
        for m in range(R):
            rows = _rows(700, s, a, 10 * s + m)
            gb.load(m, *rows)
            leaves = (1.0 + np.random.default_rng(4 + m).random(700) * 9.0).astype(np.float32)
            leaves[137 + 50 * m] = f32(1e6)
            leaves[512:] = 0
            gb.set_priorities(m, leaves, 1.0)
            ref = RefTree(N, 0.6, HAND_BETA[m])
            ref.set_leaves(np.arange(700), leaves)
            assert ref.tree[3] == 0
            refs.append(ref)
            buf = _cbuf(s, a, beta=HAND_BETA[m])
            buf.load(*rows)
            buf.set_priorities(leaves, 1.0)
            alone.append(buf)
        t = _trees(gb)
        assert all(np.array_equal(t[m], refs[m].tree) for m in range(R))
        torch.manual_seed(0)
        twin = CTRLSACAgent(s, a, bench.Space(a), max_batch=BMAX, graph=False, pipeline=False, extra_feature_steps=0, **TINY)
        _hand[s, a] = (g, gb, refs, twin, alone, gb.rings.cpu().numpy(), steps)
    return _hand[s, a]


@pytest.mark.parametrize('s,a,batch', [(3, 1, 1), (3, 1, 50), (3, 1, 300), (17, 6, 1), (17, 6, 50), (17, 6, 300), (376, 6, 5)])
def test_fused_group_launch_equals_the_restatement_the_single_launch_and_the_rings(s, a, batch):
    """B = 1 / 50 / 300 at rows of 9 and 42 floats: the ragged case, a single gatherer and several; (376, 6) at B = 5: rows of 760 floats (humanoid's
    observations, an action the group's fused policy head takes), one row per gatherer.  The three modes; then member 1 retired."""
    from rlrep_amd._lib import lib, check
    g, gb, refs, twin, alone, rings, steps = _hand_set(s, a)
    check(lib.rlrep_group_prepare(g.core.h, batch), 'group_prepare')
    sa, worst = s + a, 0.0
    given = np.stack([((np.arange(batch, dtype=np.int64) * (7 + m) + 3) % 512) for m in range(R)]).astype(np.int32)
    off = PER_STREAM + 1000 * batch + 1
    modes = [('host offset', dict(offset=off), [refs[m].sample(batch, SEEDS[m], off) for m in range(R)], [dict(seed=SEEDS[m], offset=off) for m in range(R)]),
             ('device counter', dict(offset=PER_STREAM, use_counter=True), [refs[m].sample(batch, SEEDS[m], PER_STREAM + steps[m]) for m in range(R)],
              [dict(seed=SEEDS[m], offset=PER_STREAM + steps[m]) for m in range(R)]),           # (the twin's own counter stands at 0: the member's value as a host offset)
             ('given indices', dict(offset=0, given=given), list(given), [dict(seed=0, offset=0, given=given[m]) for m in range(R)])]
    for what, kw, want, tkw in modes:
        _poison_slots(g, batch, s, a)
        idx, w = gb.draw_fill(g.core, batch, **kw)
        torch.cuda.synchronize()
        idx, w = idx.cpu().numpy().copy(), w.cpu().numpy().copy()
        for m in range(R):
            assert np.array_equal(idx[m], want[m]), (what, batch, m)
            assert idx[m].min() >= 0 and idx[m].max() < 512
            wr, exact = refs[m].weights(want[m])
            assert np.all(w[m][exact] == 1.0), (what, m)
            if HAND_BETA[m] == 0.0:
                assert np.all(w[m] == 1.0), (what, m)
            err = np.abs(w[m] - wr) / wr
            worst = max(worst, float(err.max()))
            assert np.all(err <= RTOL), (what, m, err.max())
            got = _member_slot(g, m, batch, s, a)
            rows = rings[m][idx[m]]
            assert np.array_equal(_bits(got['XE']), _bits(rows[:, :sa + s])), (what, m)
            assert np.array_equal(_bits(got['XF']), _bits(rows[:, :sa])), (what, m)
            assert np.array_equal(_bits(got['XF2'][:, :s]), _bits(rows[:, sa:sa + s])), (what, m)
            assert np.array_equal(_bits(got['XFpi'][:, :s]), _bits(rows[:, :s])), (what, m)
            assert np.array_equal(_bits(got['R']), _bits(rows[:, sa + s])) and np.array_equal(_bits(got['D']), _bits(rows[:, sa + s + 1])), (what, m)
            # rlrep_per_sample_fill on a standalone ctrlsac agent whose buffer holds member m's rows and leaves: bit-equal idx and w
            i1, w1 = alone[m].draw_fill(twin.core, batch, **tkw[m])
            torch.cuda.synchronize()
            assert np.array_equal(i1.cpu().numpy(), idx[m]) and np.array_equal(_bits(w1.cpu().numpy()), _bits(w[m])), (what, m)
    print(f'per_sample_fill_grp (S, A) = ({s}, {a}) B = {batch}: largest relative error of w against float64 pow {worst:.3e}')
    # member 1 retired: its draw rows keep a sentinel, its block stands still; the others draw as before
    ib, wb, _ = gb.draw_buffers(batch)
    ib[1].fill_(-5)
    wb[1].fill_(-3.5)
    g.retire_members([1])
    try:
        before = sg.member_bytes(g, 1)
        _poison_slots(g, batch, s, a)
        poisoned = sg.member_bytes(g, 1)
        idx, w = gb.draw_fill(g.core, batch, off + 7)
        torch.cuda.synchronize()
        assert torch.equal(sg.member_bytes(g, 1), poisoned) and not torch.equal(poisoned, before)
        assert bool((idx[1] == -5).all()) and bool((w[1] == -3.5).all())
        for m in (0, 2):
            assert np.array_equal(idx[m].cpu().numpy(), refs[m].sample(batch, SEEDS[m], off + 7)), m
    finally:
        g.revive_members([1])


# ---- 2. members equal their standalone twins ---------------------------------------------------------------------------------------------
ALPHA, BETA = [0.4, 0.6, 0.8], [0.4, 0.5, 1.0]


def _loaded(alpha, beta, seeds=SEEDS, n=700, twins=True):
    """a buffer group and the twins' buffers, member r loaded with n rows of its own"""
    al, be = np.broadcast_to(np.asarray(alpha, np.float64), (len(seeds),)), np.broadcast_to(np.asarray(beta, np.float64), (len(seeds),))
    from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup
    gb, alone = CriticPrioritizedReplayBufferGroup(len(seeds), S, A, max_size=N, alpha=list(al), beta=list(be)), []
    for r in range(len(seeds)):
        rows = _rows(n, S, A, 100 + r)
        gb.load(r, *rows)
        if twins:
            buf = _cbuf(alpha=float(al[r]), beta=float(be[r]))
            buf.load(*rows)
            alone.append(buf)
    return gb, alone


def _plain_group(n=700, members=R):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    gp = ReplayBufferGroup(members, S, A, max_size=N)
    for r in range(members):
        gp.load(r, *_rows(n, S, A, 100 + r))
    return gp


def _add_one(gb, alone, k):
    """one new transition per member (all members, retired ones included), the same row into the twin's ring"""
    rows = [_rows(1, S, A, 5000 + 37 * k + r) for r in range(gb.members)]
    gb.add(*[np.stack([rows[r][q][0] for r in range(gb.members)]) for q in range(5)])
    gb.flush()
    for r, buf in enumerate(alone):
        if buf is not None:
            buf.add(*[rows[r][q][0] for q in range(5)])
            buf.flush()


def _same_member(g, gb, r, twin, buf, what):
    sg.assert_equal(sg.state(g._members[r]), sg.state(twin.core), (what, r))
    torch.cuda.synchronize()
    assert torch.equal(gb.trees[r], buf.tree), (what, r, 'tree')
    assert gb.max_priority(r) == buf.max_priority, (what, r, 'max_p')
    for k, (x, y) in enumerate(zip(gb.draw_buffers(B), buf.draw_buffers(B))):
        assert torch.equal(x[r], y), (what, r, ('idx', 'w', 'td')[k])


@pytest.mark.parametrize('extra', [{}, dict(use_feature_target=False)], ids=['feature-target', 'no-feature-target'])
def test_members_equal_their_standalone_twins_bit_for_bit(extra):
    g = sg.group(WL, SEEDS, **extra)
    twins = [sg.standalone(WL, s, **extra) for s in SEEDS]
    gb, alone = _loaded(ALPHA, BETA)
    for r in range(R):
        sg.assert_equal(sg.state(g._members[r]), sg.state(twins[r].core), ('init', r))
    for call in range(4):
        infos = g.train(gb, B)
        for r, (twin, buf) in enumerate(zip(twins, alone)):
            tinfo = twin.train(buf, B)
            sg.assert_info_equal(dict(infos[r]), dict(tinfo), (call, r))
            _same_member(g, gb, r, twin, buf, call)
        _add_one(gb, alone, call)                     # per_add and the fill level move during the run
    t = _trees(gb)
    assert all(_invariant(t[r]) for r in range(R)) and gb.sizes == [704] * R
    w = gb.draw_buffers(B)[1].cpu().numpy()
    assert not np.all(w == 1.0) and all(len(np.unique(t[r, P:P + 704])) > 50 for r in range(R))          # real weights, priorities that moved
    assert type(g._held_buffer).__name__ == 'CriticPrioritizedReplayBufferGroup' and g._graph_key[5] == 'critic_per_group'


# ---- 3. only the critic's minibatch is prioritized ---------------------------------------------------------------------------------------
def test_only_the_critics_minibatch_is_prioritized():
    g, gplain = sg.group(WL, SEEDS), sg.group(WL, SEEDS)
    gb, _ = _loaded(ALPHA, BETA, twins=False)
    leaves = [(1.0 + 99.0 * np.random.default_rng(12 + r).random(700)).astype(np.float32) for r in range(R)]
    refs = []
    for r in range(R):
        gb.set_priorities(r, leaves[r], 100.0)
        ref = RefTree(N, ALPHA[r], BETA[r])
        ref.set_leaves(np.arange(700), leaves[r])
        refs.append(ref)
    assert g._plan(B)[0] == ['f0', 'f1', 'f2', 'f3'] and g._critic_key(B) == 'f3'
    g.train(gb, B)
    gplain.train(_plain_group(), B)
    drawn = gb.draw_buffers(B)[0].cpu().numpy()
    rings = gb.rings.cpu().numpy()
    for r in range(R):
        step = int(sg.steps_words(g._members[r])[0])
        assert step == int(sg.steps_words(gplain._members[r])[0]) == 1
        (pa, ea), (pb, eb) = _pools(g, r), _pools(gplain, r)
        pa, pb = pa.cpu().numpy(), pb.cpu().numpy()
        assert len(pa) == 4 * B and np.array_equal(pa, pb), r          # the train prologue's uniform draw, all four minibatches of it
        assert torch.equal(ea, eb) and bool(ea.abs().sum() > 0), r     # ... and all the noise
        assert np.array_equal(drawn[r], refs[r].sample(B, SEEDS[r], PER_STREAM + step)), r
        assert not np.array_equal(drawn[r], pa[3 * B:])              # ... whose last one the critic's minibatch is not
        got = _member_slot(g, r, B, S, A)
        assert np.array_equal(_bits(got['XE']), _bits(rings[r][drawn[r]][:, :2 * S + A])), r


# ---- 4. alpha = 0 is uniform replay ------------------------------------------------------------------------------------------------------
def test_alpha_zero_equals_the_plain_group_where_the_drawn_rows_cannot_matter():
    """The literal comparison with a plain group.  A stratified draw over equal leaves and the prologue's uniform draw pick different rows, so
    every row of a member's ring is the same transition here: whichever rows are drawn, the minibatch is the same, and what is left to differ
    is the arithmetic -- weights of exactly 1 in the weighted head, the update launch.  State and metrics bit for bit over 5 calls."""
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    g, gplain = sg.group(WL, SEEDS), sg.group(WL, SEEDS)
    gb, gp = _gbuf(alpha=0.0, beta=0.4), ReplayBufferGroup(R, S, A, max_size=N)
    for r in range(R):
        one = _rows(1, S, A, 300 + r)
        rows = [np.repeat(x, 700, axis=0) for x in one]
        gb.load(r, *rows)
        gp.load(r, *rows)
    for call in range(5):
        infos, pinfos = g.train(gb, B), gplain.train(gp, B)
        for r in range(R):
            sg.assert_info_equal(dict(infos[r]), dict(pinfos[r]), (call, r))
            sg.assert_equal(sg.state(g._members[r]), sg.state(gplain._members[r]), (call, r))
    t = _trees(gb)
    assert np.all(gb.draw_buffers(B)[1].cpu().numpy() == 1.0)
    assert np.all(t[:, P:P + 700] == 1.0) and np.all(t[:, P + 700:] == 0) and np.all(t[:, 1] == 700.0) and all(gb.max_priority(r) == 1.0 for r in range(R))


def test_alpha_zero_is_uniform_replay_on_real_rings():
    """On rings of distinct rows the plain twin has to be FED what the group drew (as tests/test_per_critic.py feeds the single agent's):
    member r against CTRLSACAgent(seed=s_r).train_injected on a plain ReplayBuffer with the read-back indices and noise, state and metrics
    bit for bit over 5 calls; all weights 1, all touched leaves 1."""
    from rlrep_amd.utils.buffer import ReplayBuffer
    g = sg.group(WL, SEEDS)
    twins = [sg.standalone(WL, s) for s in SEEDS]
    gb, _ = _loaded(0.0, BETA, twins=False)
    plains = []
    for r in range(R):
        buf = ReplayBuffer(S, A, max_size=N)
        buf.load(*_rows(700, S, A, 100 + r))
        plains.append(buf)
    keys, specs = g._plan(B)
    ck = keys.index(g._critic_key(B))
    for call in range(5):
        infos = g.train(gb, B)
        drawn = gb.draw_buffers(B)[0].cpu().numpy().astype(np.int64)
        for r in range(R):
            pool, flat = _pools(g, r)
            pool, flat = pool.cpu().numpy().astype(np.int64).reshape(len(keys), B), flat.cpu().numpy()
            idx = [pool[q].copy() for q in range(len(keys))]
            idx[ck] = drawn[r]
            o, eps = 0, []
            for _, sh in specs:
                n = int(np.prod(sh))
                eps.append(flat[o:o + n].reshape(sh).copy())
                o += n
            tinfo = twins[r].train_injected(plains[r], B, idx, eps)
            sg.assert_info_equal({k: float(infos[r][k]) for k in infos[r].keys()}, {k: float(tinfo[k]) for k in tinfo.keys()}, (call, r))
            sa, sb = sg.state(g._members[r]), sg.state(twins[r].core)
            for st in (sa, sb):
                st.pop('train_steps')                            # (the counter block's mirror word is the graph prologue's own)
            sg.assert_equal(sa, sb, (call, r))
    t = _trees(gb)
    assert np.all(gb.draw_buffers(B)[1].cpu().numpy() == 1.0)
    assert np.all(t[:, P:P + 700] == 1.0) and np.all(t[:, P + 700:] == 0) and all(gb.max_priority(r) == 1.0 for r in range(R))


# ---- 5. the launch counts ------------------------------------------------------------------------------------------------------------------
def test_group_graph_has_its_twins_launch_count_on_either_buffer():
    a = sg.standalone(WL, 3)
    rows = _rows(700, S, A, 100)
    buf, plain = _cbuf(), None
    buf.load(*rows)
    from rlrep_amd.utils.buffer import ReplayBuffer
    plain = ReplayBuffer(S, A, max_size=N)
    plain.load(*rows)
    a.train(plain, B)
    torch.cuda.synchronize()
    n_plain = a._graph_launches
    a.train(buf, B)
    torch.cuda.synchronize()
    n_per = a._graph_launches
    g = sg.group(WL, SEEDS)
    gb, _ = _loaded(ALPHA, BETA, twins=False)
    gp = _plain_group()
    g.train(gp, B)
    torch.cuda.synchronize()
    assert g._graph_launches == n_plain, (g._graph_launches, n_plain)
    assert g._graph_cache_key(gp, B) != g._graph_cache_key(gb, B)
    g.train(gb, B)
    torch.cuda.synchronize()
    print(f'launches in a captured ctrlsac train(): plain {n_plain}, prioritized critic {n_per}; the group: {g._graph_launches}')
    assert g._graph_launches == n_per, (g._graph_launches, n_per)
    assert n_per == n_plain + 2                                  # the fused sample-and-gather and the update; the head launch is the head launch
    g.train(gp, B)                                               # back to a plain group: the parent's graph
    torch.cuda.synchronize()
    assert g._graph_launches == n_plain


# ---- 6. retire / revive --------------------------------------------------------------------------------------------------------------------
def test_a_retired_member_stands_still_and_comes_back_as_its_twin():
    g = sg.group(WL, SEEDS)
    twins = [sg.standalone(WL, s) for s in SEEDS]
    gb, alone = _loaded(ALPHA, BETA)

    def step(live, what):
        infos = g.train(gb, B)
        for r in range(R):
            if r not in live:
                assert infos[r] is None
                continue
            tinfo = twins[r].train(alone[r], B)
            sg.assert_info_equal(dict(infos[r]), dict(tinfo), (what, r))
            _same_member(g, gb, r, twins[r], alone[r], what)

    step((0, 1, 2), 'before')
    g.retire_members([1])
    block = sg.member_bytes(g, 1)
    tree1, mp1 = _trees(gb)[1].copy(), gb.max_priority(1)
    draws1 = [x[1].clone() for x in gb.draw_buffers(B)]
    for call in range(2):
        step((0, 2), ('retired', call))
    assert torch.equal(sg.member_bytes(g, 1), block)
    assert np.array_equal(_trees(gb)[1], tree1) and gb.max_priority(1) == mp1
    assert all(torch.equal(x[1], y) for x, y in zip(gb.draw_buffers(B), draws1))
    g.revive_members([1])
    for call in range(2):                                        # member 1's twin skipped the same two calls
        step((0, 1, 2), ('revived', call))
    t = _trees(gb)
    assert all(_invariant(t[r]) for r in range(R)) and not np.array_equal(t[1], tree1)


# ---- 7. refusals on the device -------------------------------------------------------------------------------------------------------------
def test_everything_else_is_refused_by_name():
    from rlrep_amd._lib import lib
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    Bt = 16
    cg = CTRLSACSeedBatch(list(SEEDS), S, A, bench.Space(A), max_batch=Bt, extra_feature_steps=0, **TINY)
    sacg = SACSeedBatch(list(SEEDS), S, A, bench.Space(A), max_batch=Bt, hidden_dim=32)
    one = CTRLSACAgent(S, A, bench.Space(A), max_batch=Bt, pipeline=False, extra_feature_steps=0, **TINY)
    gb, _ = _loaded(ALPHA, BETA, twins=False)
    with pytest.raises(RuntimeError, match=r'SACSeedBatch\.train: CriticPrioritizedReplayBufferGroup is built for CTRLSACSeedBatch only'):
        sacg.train(gb, Bt)
    with pytest.raises(RuntimeError, match=r'CTRLSACAgent\.train: CriticPrioritizedReplayBufferGroup is built for CTRLSACSeedBatch\.train'):
        one.train(gb, Bt)
    with pytest.raises(RuntimeError, match=r'CTRLSACSeedBatch\.iterate: CriticPrioritizedReplayBufferGroup cannot be written'):
        cg.iterate(object(), gb, Bt)
    with pytest.raises(RuntimeError, match=r'CTRLSACSeedBatch\.train_injected: a seed group has no eager train\(\) form'):
        cg.train_injected(gb, Bt, [], [])
    idx, w, td = gb.draw_buffers(Bt)
    err = lambda: lib.rlrep_last_error().decode()
    p = lambda t: C.c_void_p(t.data_ptr())

    def fill(core, batch=Bt, capacity=None, rings=True):
        return lib.rlrep_group_per_sample_fill(core.h, p(gb.rings) if rings else None, 4 * gb.ring_stride, gb.max_size if capacity is None else capacity,
                                               p(gb.trees), gb.P, p(gb._scal), p(idx), p(w), batch, 0, PER_STREAM, 0, None)

    def update(core, batch=Bt, tdp=True):
        return lib.rlrep_group_per_update_td(core.h, p(gb.trees), gb.P, p(gb._scal), p(idx), p(td) if tdp else None, batch, None)

    cg.prepare(gb, Bt)                                           # (sizes the step programs for Bt: the prepared batch)
    for core, word in ((one.core, 'not a seed group'), (sacg.core, 'rlrep_group_per_sample / rlrep_group_critic_step_weighted / rlrep_group_per_update')):
        assert fill(core) < 0 and word in err() and 'group_per_sample_fill' in err()
        assert lib.rlrep_group_critic_weights_arm(core.h, p(w), p(td)) < 0 and word in err() and 'group_critic_weights_arm' in err()
        assert update(core) < 0 and word in err() and 'group_per_update_td' in err()
    assert fill(cg.core, batch=Bt + 1) < 0 and 'rlrep_group_prepare first' in err() and 'group_per_sample_fill' in err()
    assert update(cg.core, batch=Bt + 1) < 0 and 'rlrep_group_prepare first' in err() and 'group_per_update_td' in err()
    assert fill(cg.core, capacity=gb.P + 1) < 0 and 'group_per_sample_fill' in err()
    assert fill(cg.core, capacity=0) < 0 and fill(cg.core, rings=False) < 0 and 'null' in err()
    assert update(cg.core, tdp=False) < 0 and 'null' in err()
    assert lib.rlrep_group_critic_weights_arm(cg.core.h, p(w), None) < 0 and 'group_critic_weights_arm' in err()
    assert lib.rlrep_group_critic_weights_arm(cg.core.h, p(w), p(td)) == 1 and lib.rlrep_group_critic_weights_arm(cg.core.h, None, None) == 0
    assert fill(cg.core) == 0 and update(cg.core) == 0           # ... and the group they are built for takes them
    infos = cg.train(gb, Bt)
    torch.cuda.synchronize()
    assert all(i is not None for i in infos) and all(_invariant(t) for t in _trees(gb))


# ---- 8. the launcher ----------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_with_group_critic_per(tmp_path):
    import glob
    import json
    from rlrep_amd import main
    agent, evals = main.run(['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--group-critic-per', '--max_timesteps', '200',
                             '--start_timesteps', '100', '--eval_freq', '100', '--batch_size', '64', '--eval_episodes', '1', '--log_root', str(tmp_path)])
    assert agent.R == 2 and agent.steps == 100 and len(evals) == 2 and all(len(e) >= 2 for e in evals)
    assert np.all(np.isfinite(np.asarray(evals, np.float64)))
    buf = agent.replay
    assert type(buf).__name__ == 'CriticPrioritizedReplayBufferGroup' and buf is agent._held_buffer and buf.beta == [1.0, 1.0]
    rows = [json.loads(line) for f in glob.glob(str(tmp_path / '**' / 'metrics.jsonl'), recursive=True) for line in open(f)]
    assert rows and all(np.isfinite(v) for row in rows for v in row.values())
    t = _trees(buf)
    for r in range(2):
        assert _invariant(t[r]) and np.all(t[r, buf.P:buf.P + buf.sizes[r]] > 0) and np.all(t[r, buf.P + buf.sizes[r]:] == 0)
        assert len(np.unique(t[r, buf.P:buf.P + buf.sizes[r]])) > 10          # priorities moved
