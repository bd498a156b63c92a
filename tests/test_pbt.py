"""Population-based training on seed groups on the MI355X: clone_members (include/rlrep.h rlrep_group_clone_members, one launch) makes member
dst what member src is, and set_member_hyper retunes a live member -- after either, the member computes, bit for bit, what the standalone
agent computes that was built with the member's seed and hyper-parameters and loaded the matching snapshot.  The kernels that train are the
existing group kernels, so every comparison is torch.equal: no tolerance."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import seed_group_util as sg  # noqa: E402

SEEDS = (3, 11, 42, 7, 19, 23, 5, 2)
# distinct lr, tau, discount, target_update_period per member
HYPERS = (dict(lr=1e-4, tau=0.005, discount=0.99, target_update_period=2),
          dict(lr=3e-4, tau=0.01, discount=0.95, target_update_period=1),
          dict(lr=2e-4, tau=0.02, discount=0.9, target_update_period=3),
          dict(lr=5e-5, tau=0.002, discount=0.98, target_update_period=2),
          dict(lr=1.5e-4, tau=0.03, discount=0.97, target_update_period=1))
SMALL_SAC, SMALL_CTRL = 'sac_pendulum_b64', 'ctrlsac_halfcheetah_f256_b256'
PAIRS = [(0, 2), (1, 3)]


def _members(n):
    return [(SEEDS[r], dict(HYPERS[r % len(HYPERS)])) for r in range(n)]


def _hyper_words(core):
    """words 1..5 (lr, beta1, beta2, eps, tau) of the four optimizer records"""
    torch.cuda.synchronize()
    return core.group_cfg()[:, 1:6].clone()


def _records(core):
    """the device records a checkpoint carries (HipCore.device_state), as 32-bit words, with the hyper words (1..5 of each optimizer record)
    blanked: what a clone copies of them"""
    torch.cuda.synchronize()
    cfg_off = core.group_cfg().data_ptr() - core.workspace.data_ptr()
    w = core.device_state().clone().view(torch.int32)
    for q in range(4):
        w[cfg_off // 4 + 22 * q + 1:cfg_off // 4 + 22 * q + 6] = 0
    return w


def _full(core):
    s = sg.state(core)
    s['hyper_words'] = _hyper_words(core)
    s['device_state'] = core.device_state().clone()
    return s


def _member_hyper_abi(grp, r):
    from rlrep_amd import _lib
    out = _lib.Hyper()
    assert _lib.lib.rlrep_group_get_member_hyper(grp.core.h, r, C.byref(out)) == 0
    return {f: getattr(out, f) for f, _ in _lib.Hyper._fields_}


def _twin(wl, grp, r, snapshot, **extra):
    """the standalone agent member r must equal from now on: built with r's seed and hyper-parameters, loaded with `snapshot` under r's seed"""
    snap = dict(snapshot)
    snap['seed'] = grp.seeds[r]
    a = sg.standalone(wl, grp.seeds[r], grp.member_hyper(r), **extra)
    a.load(snap)
    return a


# ---- 5. the twin test -----------------------------------------------------------------------------------------------------------------------
def _twin_test(wl, **extra):
    _, _, _, B, _ = sg.dims(wl, **extra)
    members = _members(4)
    grp = sg.group(wl, *zip(*members), **extra)
    rings, alone_rings = sg.rings(wl, range(4))
    for _ in range(5):
        grp.train(rings, B)
    snaps = {s: grp.member_snapshot(s) for s, _ in PAIRS}
    before = [_full(m) for m in grp._members]
    hyp_abi = [_member_hyper_abi(grp, r) for r in range(4)]
    records = [_records(m) for m in grp._members]
    grp.clone_members(PAIRS)
    after = [_full(m) for m in grp._members]
    for s, d in PAIRS:
        # immediately: dst's copied fields are src's, bit for bit ...
        sg.assert_equal(sg.state(grp._members[d]), {k: before[s][k] for k in sg.state(grp._members[d])}, ('clone', wl, s, d))
        assert torch.equal(_records(grp._members[d]), records[s]), ('device records', wl, s, d)
        # ... its optimizer words 1..5, its MemberHyper values and its seed are its own
        assert torch.equal(after[d]['hyper_words'], before[d]['hyper_words']), ('hyper words', wl, d)
        assert not torch.equal(after[d]['hyper_words'], before[s]['hyper_words'])
        assert _member_hyper_abi(grp, d) == hyp_abi[d] and grp.member_hyper(d) == dict(grp.sweep_defaults(), **members[d][1])
        assert grp.seeds[d] == members[d][0]               # (the device's copy of the seed shows in what the member draws: the twin's info dicts below)
        # the sources are untouched
        sg.assert_equal(after[s], before[s], ('source', wl, s))
    twins = {d: _twin(wl, grp, d, snaps[s], **extra) for s, d in PAIRS}
    for d, a in twins.items():
        sg.assert_equal(sg.state(grp._members[d]), sg.state(a.core), ('twin loaded', wl, d))
    for call in range(10):
        infos = grp.train(rings, B)
        for d, a in twins.items():
            ai = a.train(alone_rings[d], B)
            sg.assert_info_equal(infos[d], ai, ('twin', wl, call, d))
            if call in (0, 1, 9):
                sg.assert_equal(sg.state(grp._members[d]), sg.state(a.core), ('twin', wl, call, d))
    # the destinations really went on with their own hyper-parameters, rings and seeds: they left their sources
    for s, d in PAIRS:
        assert not torch.equal(grp._members[d].params, grp._members[s].params)


@pytest.mark.parametrize('wl', [SMALL_SAC, 'sac_halfcheetah_b256'])
def test_sac_cloned_member_equals_its_standalone_twin_bit_for_bit(wl):
    _twin_test(wl)


@pytest.mark.parametrize('use_feature_target', [True, False])
def test_ctrlsac_cloned_member_equals_its_standalone_twin_bit_for_bit(use_feature_target):
    _twin_test(SMALL_CTRL, use_feature_target=use_feature_target)


def test_ctrlsac_f2048_cloned_member_equals_its_standalone_twin_bit_for_bit():
    _twin_test('ctrlsac_halfcheetah_f2048_b256')


# ---- 6. a clone writes nothing outside its destinations ---------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_clone_writes_nothing_outside_its_destinations(wl):
    _, _, _, B, _ = sg.dims(wl)
    members = _members(5)
    runs = []
    for clone in (True, False):
        grp = sg.group(wl, *zip(*members))
        rings, _ = sg.rings(wl, range(5))
        for _ in range(5):
            grp.train(rings, B)
        if clone:
            block = grp.core._block.clone()
            grp.clone_members(PAIRS)
            torch.cuda.synchronize()
            # byte for byte: every member block but the destinations', and everything of the allocation behind the members
            stride, skew = grp.core.member_stride, grp.core._skew
            now = grp.core._block
            for r in (0, 1, 4):
                assert torch.equal(now[skew + r * stride:skew + (r + 1) * stride], block[skew + r * stride:skew + (r + 1) * stride]), (wl, r)
            assert torch.equal(now[:skew], block[:skew]) and torch.equal(now[skew + 5 * stride:], block[skew + 5 * stride:])
            # ... and of a destination's block, what is not copied: gradients, the workspace behind the device records (activations, metric
            # history, its MemberHyper record), the index / noise pools
            for _, d in PAIRS:
                m, lo = grp._members[d], skew + d * stride
                g0 = m.grads.data_ptr() - now.data_ptr()
                assert torch.equal(now[g0:g0 + 4 * m.grads.numel()], block[g0:g0 + 4 * m.grads.numel()]), (wl, d, 'grads')
                w0 = m.workspace.data_ptr() - now.data_ptr() + m.device_state().numel()
                w1 = m.workspace.data_ptr() - now.data_ptr() + m.workspace.numel()
                assert torch.equal(now[w0:w1], block[w0:w1]), (wl, d, 'workspace')
                e0 = lo + grp.core.member_extra_offset
                assert torch.equal(now[e0:lo + stride], block[e0:lo + stride]), (wl, d, 'pools')
            del block
        for _ in range(10):
            grp.train(rings, B)
        runs.append([sg.state(m) for m in grp._members])
    for r in (0, 1, 4):
        sg.assert_equal(runs[0][r], runs[1][r], (wl, 'member', r))
    for _, d in PAIRS:
        assert not torch.equal(runs[0][d]['params'], runs[1][d]['params'])


# ---- 7. no re-capture, one launch per call ------------------------------------------------------------------------------------------------
def test_clone_keeps_the_graph_and_is_one_launch():
    from rlrep_amd._lib import lib
    wl = 'sac_halfcheetah_b256'
    _, _, _, B, _ = sg.dims(wl)
    R = 8
    grp = sg.group(wl, *zip(*_members(R)))
    rings, _ = sg.rings(wl, range(R))
    for _ in range(3):
        grp.train(rings, B)
    graph, per_train, graph_launches = grp._graph, lib.rlrep_last_launch_count(grp.core.h), grp._graph_launches
    for pairs in ([(0, 1)], [(0, 2), (1, 3)], [(r, r + R // 2) for r in range(R // 2)]):
        n0 = lib.rlrep_launch_counter()
        grp.clone_members(pairs)
        assert lib.rlrep_launch_counter() - n0 == 1, pairs
        n0 = lib.rlrep_launch_counter()
        grp.train(rings, B)
        assert lib.rlrep_launch_counter() == n0                      # a replay issues no launch of the library's: nothing was captured again
        assert grp._graph is graph and grp._graph_launches == graph_launches
        assert lib.rlrep_last_launch_count(grp.core.h) == per_train
    assert [e['members'] for e in grp.lineage if e['kind'] == 'clone'][-4:] == [[0, 4], [1, 5], [2, 6], [3, 7]]


# ---- 8. set_member_hyper on a live member ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_retuned_member_equals_the_standalone_twin_with_the_new_values(wl):
    _, _, _, B, _ = sg.dims(wl)
    members = _members(3)
    new = dict(lr=7e-4, tau=0.05, target_update_period=3, auto_entropy_tuning=False)
    runs = []
    for retune in (True, False):
        grp = sg.group(wl, *zip(*members))
        rings, alone_rings = sg.rings(wl, range(3))
        for _ in range(5):
            grp.train(rings, B)
        if retune:
            graph = grp._graph
            with pytest.raises(ValueError, match='alpha is the initial temperature only'):
                grp.set_member_hyper(1, alpha=0.3)
            with pytest.raises(ValueError, match="unknown key 'hidden_dim'"):
                grp.set_member_hyper(1, hidden_dim=64)
            with pytest.raises(ValueError, match='lr=-1.0 is not valid'):
                grp.set_member_hyper(1, lr=-1.0)
            with pytest.raises(ValueError, match='member 3 outside'):
                grp.set_member_hyper(3, lr=1e-4)
            old = grp.member_hyper(1)
            grp.set_member_hyper(1, **new)
            assert grp.member_hyper(1) == dict(old, **new) == grp.member_snapshot(1)['hyper']
            assert grp.lineage[-1] == {'train_calls': 5, 'kind': 'retune', 'members': [1], 'old': {k: old[k] for k in new}, 'new': new}
            twin = _twin(wl, grp, 1, grp.member_snapshot(1))
            for call in range(10):
                infos = grp.train(rings, B)
                sg.assert_info_equal(infos[1], twin.train(alone_rings[1], B), ('retuned', wl, call))
            assert grp._graph is graph
            sg.assert_equal(sg.state(grp._members[1]), sg.state(twin.core), ('retuned', wl))
        else:
            for _ in range(10):
                grp.train(rings, B)
        runs.append([sg.state(m) for m in grp._members])
    for r in (0, 2):
        sg.assert_equal(runs[0][r], runs[1][r], (wl, 'untouched member', r))
    assert not torch.equal(runs[0][1]['params'], runs[1][1]['params'])


def test_set_member_hyper_makes_a_plain_seed_group_swept():
    wl = SMALL_SAC
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, (3, 11))
    rings, alone_rings = sg.rings(wl, range(2))
    for _ in range(3):
        grp.train(rings, B)
    grp.set_member_hyper(0, lr=1e-3, discount=0.9)
    assert grp._swept and grp.member_hyper(0)['lr'] == 1e-3 and grp.member_hyper(1)['lr'] == grp.sweep_defaults()['lr']
    twin = _twin(wl, grp, 0, grp.member_snapshot(0))
    for call in range(4):
        infos = grp.train(rings, B)
        sg.assert_info_equal(infos[0], twin.train(alone_rings[0], B), ('swept', call))
    sg.assert_equal(sg.state(grp._members[0]), sg.state(twin.core), 'swept')


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------
def test_clone_refusals_leave_every_member_as_it_was():
    from rlrep_amd._lib import lib
    from rlrep_amd.core import _stream
    wl = SMALL_SAC
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, *zip(*_members(4)))
    rings, _ = sg.rings(wl, range(4))
    for _ in range(3):
        grp.train(rings, B)
    before = [_full(m) for m in grp._members]
    launches = lib.rlrep_launch_counter()
    name = type(grp).__name__

    def raw(pairs, handle=None, n=None):
        k = max(len(pairs), 1)
        src, dst = (C.c_int32 * k)(*[s for s, _ in pairs]), (C.c_int32 * k)(*[d for _, d in pairs])
        rc = lib.rlrep_group_clone_members(handle if handle is not None else grp.core.h, src, dst, len(pairs) if n is None else n, _stream())
        return rc, (lib.rlrep_last_error() or b'').decode()

    for pairs, py_words, abi_words in (
            ([(0, 1), (1, 2)], 'member 1 is both a source and a destination', 'member 1 is both a source and a destination'),
            ([(2, 1), (0, 2)], 'member 2 is both a source and a destination', 'member 2 is both a source and a destination'),
            ([(0, 2), (1, 2)], 'member 2 is a destination twice', 'member 2 is a destination twice'),
            ([(0, 1), (0, 1)], 'member 1 is a destination twice', 'member 1 is a destination twice'),
            ([(3, 3)], 'copies member 3 onto itself', 'copies member 3 onto itself'),
            ([(0, 4)], 'outside [0, 4)', 'outside [0, 4)'),
            ([(-1, 2)], 'outside [0, 4)', 'outside [0, 4)'),
            ([], '0 pairs outside [1, 4]', 'n 0 outside [1, 4]'),
            ([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)], '5 pairs outside [1, 4]', 'n 5 outside [1, 4]')):
        with pytest.raises(ValueError) as e:
            grp.clone_members(pairs)
        assert py_words in str(e.value) and name in str(e.value), str(e.value)
        rc, msg = raw(pairs)
        assert rc == -1 and abi_words in msg and 'group_clone_members' in msg, (pairs, rc, msg)
    plain = sg.standalone(wl, 3, {})
    rc, msg = raw([(0, 1)], handle=plain.core.h)
    assert rc == -1 and 'not a seed group' in msg
    assert lib.rlrep_launch_counter() == launches                    # refused before anything is launched
    for r, m in enumerate(grp._members):
        sg.assert_equal(_full(m), before[r], ('refused', r))
    assert grp.lineage == []

    # inside a train(): between the group train prologue and the end of that train()
    ni, ne = grp._pool_sizes(B)
    ipool, epool = grp._buf('pool_idx', (ni,), torch.int32), grp._buf('pool_eps', (ne,))
    grp._draw_pools(rings, B, True, ipool, epool)
    inside = [_full(m) for m in grp._members]
    n0 = lib.rlrep_launch_counter()
    rc, msg = raw([(0, 1)])
    assert rc == -1 and 'inside a train()' in msg, (rc, msg)
    assert lib.rlrep_launch_counter() == n0
    for r, m in enumerate(grp._members):
        sg.assert_equal(_full(m), inside[r], ('refused inside a train()', r))
    assert lib.rlrep_end_train(grp.core.h) == 0
    rc, msg = raw([(0, 1)])
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(grp._members[1].params, grp._members[0].params)


# ---- 10. checkpoints ------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_after_clone_and_retune_resumes_with_adopt_hyper(tmp_path):
    wl = SMALL_SAC
    _, _, _, B, _ = sg.dims(wl)
    members = _members(4)
    grp = sg.group(wl, *zip(*members))
    rings, _ = sg.rings(wl, range(4))
    for _ in range(5):
        grp.train(rings, B)
    grp.clone_members([(0, 3)])
    grp.set_member_hyper(3, **{k: v for k, v in grp.member_hyper(0).items() if k != 'alpha'})
    grp.set_member_hyper(3, lr=grp.member_hyper(0)['lr'] * 1.2)
    for _ in range(3):
        grp.train(rings, B)
    path = os.path.join(tmp_path, 'pbt.pt')
    grp.save(path)
    assert [e['kind'] for e in grp.lineage] == ['clone', 'retune', 'retune'] and grp.lineage[0]['members'] == [0, 3]
    fresh = sg.group(wl, *zip(*members))                                      # the INITIAL values
    with pytest.raises(RuntimeError, match='member 3 hyper-parameters differ'):
        fresh.load(path)
    fresh.load(path, adopt_hyper=True)
    assert fresh.lineage == grp.lineage == torch.load(path)['lineage']
    assert [fresh.member_hyper(r) for r in range(4)] == [grp.member_hyper(r) for r in range(4)]
    assert [_member_hyper_abi(fresh, r) for r in range(4)] == [_member_hyper_abi(grp, r) for r in range(4)]
    for call in range(5):
        gi, fi = grp.train(rings, B), fresh.train(rings, B)
        for r in range(4):
            sg.assert_info_equal(gi[r], fi[r], ('resumed', call, r))
    for r in range(4):
        sg.assert_equal(_full(grp._members[r]), _full(fresh._members[r]), ('resumed', r))
    # the default is what it was: a checkpoint whose values are the group's loads without the flag
    same = sg.group(wl, [s for s, _ in members], [grp.member_hyper(r) for r in range(4)])
    same.load(path)
    assert same.lineage == grp.lineage


# ---- 11. the launcher -----------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_pbt_and_is_reproducible(tmp_path):
    """Two identical invocations write the same pbt.jsonl and the same metrics.jsonl rows.  (`steps_per_sec` is a wall-clock rate the launcher
    has always put into every metrics row: it is the one field left out of the comparison.)"""
    from rlrep_amd import main
    from rlrep_amd.agent import pbt
    outs = []
    for run in ('a', 'b'):
        root = os.path.join(tmp_path, run)
        agent, evals = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1,2,3', '--max_timesteps', '800', '--start_timesteps', '200',
                                 '--eval_freq', '200', '--pbt-interval', '200', '--pbt-keys', 'lr,tau', '--batch_size', '64',
                                 '--eval_episodes', '1', '--log_root', root])
        base = os.path.join(root, 'Pendulum-v1', 'sac', '0')
        events = [json.loads(l) for l in open(os.path.join(base, 'pbt.jsonl'))]
        metrics = []
        for s in range(4):
            rows = [json.loads(l) for l in open(os.path.join(base, str(s), 'metrics.jsonl'))]
            assert [row['step'] for row in rows] == [400, 600, 800]
            for row in rows:
                row.pop('steps_per_sec')
            metrics.append(rows)
        outs.append((open(os.path.join(base, 'pbt.jsonl')).read(), metrics, events, agent))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    text, _, events, agent = outs[0]
    # one event per destination per interval beyond start_timesteps: k = max(1, floor(0.25 * 4)) = 1 at steps 400, 600, 800
    assert [e['step'] for e in events] == [400, 600, 800]
    hyper = [dict(agent.sweep_defaults()) for _ in range(4)]
    rng = np.random.RandomState(0)
    for e in events:
        assert len(e['scores']) == 4
        assert pbt.plan_exploit(e['scores'], 0.25, rng) == [(e['src'], e['dst'])]
        want = pbt.perturb(hyper[e['src']], ['lr', 'tau'], [0.8, 1.2], rng)
        assert e['new'] == {k: want[k] for k in e['new']} and set(e['new']) == set(want) - {'alpha'}
        assert e['old'] == {k: hyper[e['dst']][k] for k in e['old']}
        assert e['new']['lr'] in (hyper[e['src']]['lr'] * 0.8, hyper[e['src']]['lr'] * 1.2)
        hyper[e['dst']] = dict(want, alpha=hyper[e['dst']]['alpha'])
    assert [agent.member_hyper(r) for r in range(4)] == hyper
    assert len([x for x in agent.lineage if x['kind'] == 'clone']) == 3
