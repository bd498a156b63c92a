"""GPU: prioritized replay for sac seed groups (csrc/per_group.hip).  Member r of a SACSeedBatch training from a
PrioritizedReplayBufferGroup against its standalone twin -- SACAgent(seed=s_r) on a PrioritizedReplayBuffer(alpha_r, beta_r) fed the same rows
-- bit for bit; the group kernels against tests/per_reference.py (exact wherever no powf is involved); duplicates, retire / revive, the
launch count, the refusals and the launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

from per_reference import PER_STREAM, RefTree, f32
import seed_group_util as sg

pytestmark = pytest.mark.gpu

S, A, B = 3, 1, 64              # sac Pendulum dims
WL = 'sac_pendulum_b64'
SMALL = dict(hidden_dim=64)
N = 1000                        # ring rows: P = 1024, 24 padding leaves, and a wrap
P = 1024
RTOL = 1e-4                     # the repository's bar (tests/test_hip_parity.py)
PLAIN_SAC_LAUNCHES = 18         # kernels in a captured plain sac train() at the workload's own dims (tests/test_per.py): must not move
PER_GROUP_LAUNCHES = 21         # ... of a prioritized group: + sample, + gather, + update, as for the single agent
SEEDS = [3, 5, 11]
ALPHA, BETA = [0.6, 0.0, 0.9], [0.4, 1.0, 0.0]


def _rows(n, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, S)).astype(np.float32), r.uniform(-1, 1, size=(n, A)).astype(np.float32), r.normal(size=(n, S)).astype(np.float32),
            r.normal(size=n).astype(np.float32), (r.random(n) < 0.05).astype(np.float32))


def _gbuf(R, **kw):
    from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup
    return PrioritizedReplayBufferGroup(R, S, A, max_size=N, **kw)


def _prb(**kw):
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer
    return PrioritizedReplayBuffer(S, A, max_size=N, **kw)


def _trees(gb):
    torch.cuda.synchronize()
    return gb.trees.cpu().numpy()


def _invariant(tree):
    n = np.arange(1, len(tree) // 2)
    return bool(np.array_equal(tree[n], (tree[2 * n] + tree[2 * n + 1]).astype(f32)))


def _loaded(seeds, alpha, beta, n=300):
    """a buffer group and the twins' buffers, member r loaded with n rows of its own"""
    R = len(seeds)
    gb, alone = _gbuf(R, alpha=alpha, beta=beta), []
    for r in range(R):
        rows = _rows(n, 100 + r)
        gb.load(r, *rows)
        buf = _prb(alpha=float(np.asarray(alpha).reshape(-1)[r % np.asarray(alpha).size]), beta=float(np.asarray(beta).reshape(-1)[r % np.asarray(beta).size]))
        buf.load(*rows)
        alone.append(buf)
    return gb, alone


def _add_one(gb, alone, k):
    """one new transition per member (all members, retired ones included), the same row into the twin's ring"""
    R = gb.members
    rows = [_rows(1, 5000 + 37 * k + r) for r in range(R)]
    gb.add(*[np.stack([rows[r][q][0] for r in range(R)]) for q in range(5)])
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
    gi, gw = gb.draw_buffers(B)
    ti, tw = buf.draw_buffers(B)
    assert torch.equal(gi[r], ti) and torch.equal(gw[r], tw), (what, r, 'idx / w')


# ---- 1. member parity ----------------------------------------------------------------------------------------------------------------------
def test_members_equal_their_standalone_twins_bit_for_bit():
    g = sg.group(WL, SEEDS, **SMALL)
    twins = [sg.standalone(WL, s, **SMALL) for s in SEEDS]
    gb, alone = _loaded(SEEDS, ALPHA, BETA)
    for call in range(10):
        infos = g.train(gb, B)
        for r, (twin, buf) in enumerate(zip(twins, alone)):
            tinfo = twin.train(buf, B)
            sg.assert_info_equal(dict(infos[r]), dict(tinfo), (call, r))
            _same_member(g, gb, r, twin, buf, call)
        _add_one(gb, alone, call)                     # per_add and the fill level move during the run
    t = _trees(gb)
    assert all(_invariant(t[r]) for r in range(3)) and gb.sizes == [310] * 3
    assert np.all(t[1, P:P + 310] == 1.0)             # alpha = 0: every priority stays 1 (uniform replay, by the single agent's test)
    assert len(np.unique(t[0, P:P + 310])) > 50       # ... and the others' moved


# ---- 2. the kernels against the restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def grp():
    return sg.group(WL, SEEDS, **SMALL)


def _hand_set(alpha=ALPHA, beta=BETA, eps=(1e-6, 1e-3, 0.0)):
    """rings at size 700 with leaves set by hand, per member: a heavy leaf (at a different row per member), rows 512 .. 698 zeroed and a
    leaf at row size - 1, so the root's right subtree holds one leaf"""
    gb, refs = _gbuf(3, alpha=list(alpha), beta=list(beta), eps=list(eps)), []
    for m in range(3):
        gb.load(m, *_rows(700, m))
        leaves = (1.0 + np.random.default_rng(4 + m).random(700) * 9.0).astype(np.float32)
        leaves[137 + 50 * m] = f32(1e6)
        leaves[512:699] = 0
        gb.set_priorities(m, leaves, 1.0)
        ref = RefTree(N, alpha[m], beta[m], eps[m])
        ref.set_leaves(np.arange(700), leaves)
        refs.append(ref)
    t = _trees(gb)
    assert all(np.array_equal(t[m], refs[m].tree) for m in range(3))
    return gb, refs


@pytest.mark.parametrize('batch', [64, 300])          # 300: more than one pass of the 256 threads, and ragged
def test_group_sample_and_update_equal_the_reference(grp, batch):
    gb, refs = _hand_set()
    worst_w = worst_leaf = 0.0
    rng = np.random.default_rng(batch)
    for call in range(2):
        off = PER_STREAM + 1000 * batch + call
        idx, w = gb.draw(batch, off, core=grp.core)
        torch.cuda.synchronize()
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        td = (rng.random((3, batch)) * 4).astype(np.float32)
        gb.update(batch, td=torch.from_numpy(td).cuda(), core=grp.core)
        t = _trees(gb)
        for m in range(3):
            want = refs[m].sample(batch, SEEDS[m], off)
            assert np.array_equal(idx[m], want), (batch, call, m)
            assert idx[m].max() < 700 and not np.any((idx[m] >= 512) & (idx[m] < 699))
            wr, exact = refs[m].weights(want)
            assert np.all(w[m][exact] == 1.0)
            if BETA[m] == 0.0:
                assert np.all(w[m] == 1.0)
            err = np.abs(w[m] - wr) / wr
            worst_w = max(worst_w, float(err.max()))
            assert np.all(err <= RTOL), (batch, call, m, err.max())
            # the update: leaves within the bar of float64 pow (the maximum over the duplicates), everything above them exact
            new = refs[m].new_priorities(td[m])
            wantl = np.zeros(N)
            np.maximum.at(wantl, want, new)
            touched = np.unique(want)
            got = t[m, P + touched]
            lerr = np.abs(got - wantl[touched]) / wantl[touched]
            worst_leaf = max(worst_leaf, float(lerr.max()))
            assert np.all(lerr <= RTOL), (batch, call, m, lerr.max())
            untouched = np.setdiff1d(np.arange(N), touched)
            assert np.array_equal(t[m, P + untouched], refs[m].tree[P + untouched])
            refs[m].tree[P:] = t[m, P:]
            refs[m].rebuild()
            refs[m].max_p = f32(max(refs[m].max_p, got.max()))
            assert np.array_equal(t[m], refs[m].tree), (batch, call, m)
            assert gb.max_priority(m) == float(refs[m].max_p)
    print(f'per_sample_grp B={batch}: largest relative error of w against float64 pow {worst_w:.3e}')
    print(f'per_update_grp B={batch}: largest relative error of a leaf against float64 pow {worst_leaf:.3e}')
    # the given-indices mode: only the weights, from every member's own tree
    given = np.stack([(np.arange(batch, dtype=np.int32) * (7 + m)) % 512 for m in range(3)]).astype(np.int32)
    idx, w = gb.draw(batch, 0, core=grp.core, given=given)
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), given)
    w = w.cpu().numpy()
    for m in range(3):
        wr, exact = refs[m].weights(given[m])
        assert np.all(w[m][exact] == 1.0) and np.all(np.abs(w[m] - wr) / wr <= RTOL)


def test_group_sample_reads_every_members_own_counter(grp):
    """offset + the member's train() counter, as a graph replay draws"""
    gb, refs = _hand_set()
    idx, _ = gb.draw(50, PER_STREAM, core=grp.core, use_counter=True)
    torch.cuda.synchronize()
    for m in range(3):
        step = int(sg.steps_words(grp._members[m])[0])
        assert np.array_equal(idx[m].cpu().numpy(), refs[m].sample(50, SEEDS[m], PER_STREAM + step))


def test_group_add_follows_every_members_own_maximum(grp):
    """per_add_grp across the wrap, every member at the maximum ITS launch reads; add_device; load(r) of fewer rows"""
    gb, refs = _gbuf(3), [RefTree(N) for _ in range(3)]
    for m in range(3):
        gb.load(m, *_rows(850, m))
        gb.set_priorities(m, np.full(850, 1.5 + m, np.float32), 1.5 + m)
        refs[m].set_leaves(np.arange(850), 1.5 + m)
        refs[m].max_p = f32(1.5 + m)
    rows = [_rows(300, 50 + m) for m in range(3)]
    gb.add_batch(*[np.stack([rows[m][q] for m in range(3)]) for q in range(5)])      # 850 .. 1149 mod 1000
    gb.flush()
    t = _trees(gb)
    for m in range(3):
        refs[m].add(850, 300)
        assert np.array_equal(t[m], refs[m].tree) and t[m, P + 149] == f32(1.5 + m) and _invariant(t[m]), m
    assert gb.ptr == 150
    dev = [torch.from_numpy(np.stack([rows[m][q][:200] for m in range(3)])).cuda() for q in range(5)]
    gb.add_device(*dev)
    t = _trees(gb)
    for m in range(3):
        refs[m].add(150, 200)
        assert np.array_equal(t[m], refs[m].tree), m
    gb.load(1, *_rows(300, 9))
    refs[1].clear(); refs[1].add(0, 300)
    t = _trees(gb)
    assert np.array_equal(t[1], refs[1].tree) and np.all(t[1, P + 300:] == 0) and np.array_equal(t[0], refs[0].tree) and np.array_equal(t[2], refs[2].tree)


# ---- 3. duplicates -------------------------------------------------------------------------------------------------------------------------
def test_update_takes_the_maximum_of_duplicates_in_one_member_only(grp):
    gb, refs = _hand_set()
    one = np.zeros(700, np.float32)
    one[321] = 2.0
    gb.set_priorities(1, one, 2.0)                    # member 1: all its mass on one leaf
    before = _trees(gb).copy()
    grp.retire_members([0, 2])
    try:
        idx, w = gb.draw(B, PER_STREAM + 9, core=grp.core)
        td = (np.random.default_rng(1).random((3, B)) * 4).astype(np.float32)
        gb.update(B, td=torch.from_numpy(td).cuda(), core=grp.core)
        t = _trees(gb)
        assert np.all(idx[1].cpu().numpy() == 321) and np.all(w[1].cpu().numpy() == 1.0)
    finally:
        grp.revive_members([0, 2])
    want = f32(1.0)                                   # alpha_1 = 0: every new priority is 1
    assert t[1, P + 321] == want and t[1, 1] == want and _invariant(t[1]) and gb.max_priority(1) == 2.0
    assert t[0].tobytes() == before[0].tobytes() and t[2].tobytes() == before[2].tobytes()
    assert gb.max_priority(0) == 1.0 and gb.max_priority(2) == 1.0
    # ... and with an exponent: the maximum over the 64 duplicates, whatever order they arrive in
    gb.set_priorities(0, one, 2.0)
    gb.draw(B, PER_STREAM + 10, core=grp.core)
    gb.update(B, td=torch.from_numpy(td).cuda(), core=grp.core)
    t = _trees(gb)
    wantd = np.power(np.float64(f32(td[0].max() + f32(1e-6))), float(f32(ALPHA[0])))
    assert abs(t[0, P + 321] - wantd) / wantd <= RTOL and t[0, 1] == t[0, P + 321] and _invariant(t[0])
    assert gb.max_priority(0) == max(2.0, float(t[0, P + 321]))


# ---- 4. retire / revive --------------------------------------------------------------------------------------------------------------------
def test_a_retired_members_tree_only_follows_its_ring():
    seeds = [3, 5, 11, 7]
    g = sg.group(WL, seeds, **SMALL)
    twins = [sg.standalone(WL, s, **SMALL) if r != 2 else None for r, s in enumerate(seeds)]
    gb, alone = _loaded(seeds, 0.6, 0.4)
    alone[2] = None
    g.train(gb, B)                                    # one call with everybody, so member 2 has a |TD| buffer and moved priorities to keep
    for r in (0, 1, 3):
        twins[r].train(alone[r], B)
    g.retire_members([2])
    frozen = sg.state(g._members[2])
    td2 = g._members[2].per_td(B).clone()
    t0 = _trees(gb)[2].copy()
    mp2 = gb.max_priority(2)
    for call in range(5):
        _add_one(gb, alone, call)
        infos = g.train(gb, B)
        assert infos[2] is None
        for r in (0, 1, 3):
            tinfo = twins[r].train(alone[r], B)
            sg.assert_info_equal(dict(infos[r]), dict(tinfo), (call, r))
            _same_member(g, gb, r, twins[r], alone[r], ('retired', call))
    sg.assert_equal(sg.state(g._members[2]), frozen, 'member 2 frozen')
    torch.cuda.synchronize()
    assert torch.equal(g._members[2].per_td(B), td2) and gb.max_priority(2) == mp2
    t2 = _trees(gb)[2]
    added = np.arange(300, 305)
    assert np.all(t2[P + added] == f32(mp2))
    rest = np.setdiff1d(np.arange(P), added)
    assert np.array_equal(t2[P + rest], t0[P + rest]) and _invariant(t2)
    g.revive_members([2])
    for call in range(3):
        _add_one(gb, alone, 10 + call)
        infos = g.train(gb, B)
        assert infos[2] is not None
        for r in (0, 1, 3):
            twins[r].train(alone[r], B)
    t = _trees(gb)
    assert all(_invariant(t[r]) for r in range(4))
    for r in (0, 1, 3):
        _same_member(g, gb, r, twins[r], alone[r], 'after the revival')
    assert not np.array_equal(t[2, P:P + 308], t2[P:P + 308])         # member 2 trains again: its priorities move


# ---- 5. the launch count -------------------------------------------------------------------------------------------------------------------
def test_graph_launch_count_is_a_plain_group_train_plus_three():
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    g = sg.group(WL, SEEDS)
    plain, per = ReplayBufferGroup(3, S, A, max_size=N), _gbuf(3)
    for r in range(3):
        rows = _rows(700, r)
        plain.load(r, *rows)
        per.load(r, *rows)
    g.train(plain, B)
    torch.cuda.synchronize()
    n_plain = g._graph_launches
    assert g._graph_cache_key(plain, B) != g._graph_cache_key(per, B)
    g.train(per, B)
    torch.cuda.synchronize()
    n_per = g._graph_launches
    print(f'launches in a captured sac group train(): plain {n_plain}, prioritized {n_per}')
    assert n_plain == PLAIN_SAC_LAUNCHES
    assert n_per <= n_plain + 3 and n_per == PER_GROUP_LAUNCHES
    g.train(plain, B)
    torch.cuda.synchronize()
    assert g._graph_launches == PLAIN_SAC_LAUNCHES


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_everything_but_a_sac_seed_group_refuses_the_buffer_group(grp):
    from rlrep_amd._lib import lib
    gb, _ = _loaded(SEEDS, 0.6, 0.4)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBufferGroup'):
        grp.iterate(None, gb, B)
    a = sg.standalone(WL, 3, **SMALL)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBufferGroup'):
        a.train(gb, B)
    wl = 'ctrlsac_halfcheetah_f256_b256'
    _, cS, cA, cB, _ = sg.dims(wl)
    from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup
    cg = sg.group(wl, [0, 1])
    cb = PrioritizedReplayBufferGroup(2, cS, cA, max_size=256)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBufferGroup'):
        cg.train(cb, cB)
    # the new C entry points, by name: a single agent's handle and a ctrlsac group's
    idx, w = gb.draw_buffers(B)
    args = (C.c_void_p(gb.trees.data_ptr()), gb.P, C.c_void_p(gb._scal.data_ptr()), C.c_void_p(idx.data_ptr()))
    for core, word in ((a.core, 'not a seed group'), (cg.core, 'sac seed groups only')):
        rc = lib.rlrep_group_per_sample(core.h, *args, C.c_void_p(w.data_ptr()), B, 0, PER_STREAM, 0, None, 0, N, None)
        assert rc < 0 and word in lib.rlrep_last_error().decode() and 'group_per_sample' in lib.rlrep_last_error().decode()
        rc = lib.rlrep_group_critic_step_weighted(core.h, C.c_void_p(w.data_ptr()), C.c_void_p(w.data_ptr()), None)
        assert rc < 0 and word in lib.rlrep_last_error().decode() and 'group_critic_step_weighted' in lib.rlrep_last_error().decode()
        rc = lib.rlrep_group_per_update(core.h, *args, None, B, None)
        assert rc < 0 and word in lib.rlrep_last_error().decode() and 'group_per_update' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_per_td_dev(a.core.h) is None
    torch.cuda.synchronize()


# ---- 7. the launcher -----------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_with_group_per(tmp_path):
    from rlrep_amd import main
    agent, evaluations = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--group-per', '--batch_size', '64', '--eval_episodes', '1',
                                   '--start_timesteps', '300', '--eval_freq', '300', '--max_timesteps', '600', '--log_root', str(tmp_path)])
    assert np.all(np.isfinite(np.asarray(evaluations, np.float64))) and len(evaluations) == 2
    buf = agent.replay
    assert type(buf).__name__ == 'PrioritizedReplayBufferGroup' and agent._held_buffer is buf
    assert buf.beta == [1.0, 1.0] and np.all(buf._scal[:, 2].cpu().numpy() == 1.0)
    t = _trees(buf)
    assert all(_invariant(t[r]) for r in range(2)) and np.all(t[:, t.shape[1] // 2:][:, :600] > 0)
    assert len(np.unique(t[0, t.shape[1] // 2:][:600])) > 50          # priorities moved
