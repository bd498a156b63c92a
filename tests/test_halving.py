"""Successive halving on seed groups on the MI355X: retire_members takes members out of every group launch (include/rlrep.h
rlrep_group_set_live: the live table every `*_grp` kernel form obeys), revive_members puts them back.  The live members go on computing, bit
for bit, what standalone agents with their seeds compute; nothing of a retired member is read or written; a revived member continues where it
stood.  The kernels that train are the existing group kernels behind one more test, so every comparison is torch.equal: no tolerance."""
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

SEEDS = (3, 11, 42, 7)
SMALL_SAC, SMALL_CTRL = 'sac_pendulum_b64', 'ctrlsac_halfcheetah_f256_b256'
WORKLOADS = (SMALL_SAC, 'sac_halfcheetah_b256', SMALL_CTRL, 'ctrlsac_halfcheetah_f2048_b256')


def _live_abi(grp):
    from rlrep_amd._lib import lib
    out = (C.c_int32 * grp.R)()
    assert lib.rlrep_group_get_live(grp.core.h, out) == 0
    return [bool(v) for v in out]


# ---- 1. live members are standalone agents ----------------------------------------------------------------------------------------------
def _live_members_test(wl, **extra):
    _, _, _, B, _ = sg.dims(wl, **extra)
    grp = sg.group(wl, SEEDS, **extra)
    rings, alone_rings = sg.rings(wl, range(4))
    alone = [sg.standalone(wl, s, **extra) for s in SEEDS]
    retire_after = {5: 1, 10: 3}
    assert grp.live == [True] * 4 == _live_abi(grp)
    for call in range(1, 26):
        live = grp.live
        infos = grp.train(rings, B)
        ainfos = [a.train(alone_rings[r], B) if live[r] else None for r, a in enumerate(alone)]
        assert len(infos) == 4 and [i is None for i in infos] == [not v for v in live], (wl, call)
        if call in (1, 6, 11, 25):
            for r in range(4):
                if live[r]:
                    sg.assert_info_equal(infos[r], ainfos[r], (wl, call, r))
                    sg.assert_equal(sg.state(grp._members[r]), sg.state(alone[r].core), (wl, call, r))
        if call in retire_after:
            grp.retire_members([retire_after[call]])
            assert grp.lineage[-1] == {'event': 'retire', 'kind': 'retire', 'members': [retire_after[call]], 'step': call}
    assert grp.live == [True, False, True, False] == _live_abi(grp)
    # the retired members stand where they were retired: the standalone agents stopped at the same call
    for r in (1, 3):
        sg.assert_equal(sg.state(grp._members[r]), sg.state(alone[r].core), (wl, 'retired', r))


@pytest.mark.parametrize('wl', WORKLOADS)
def test_live_members_equal_standalone_agents_bit_for_bit(wl):
    _live_members_test(wl)


def test_live_members_equal_standalone_agents_without_feature_target():
    _live_members_test(SMALL_CTRL, use_feature_target=False)


# ---- 2. a retired member is untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL, 'ctrlsac_halfcheetah_f2048_b256'])
def test_a_retired_members_block_is_not_written(wl):
    _, S, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, _ = sg.rings(wl, range(4))
    for _ in range(3):
        grp.train(rings, B)
    grp.select_action(np.zeros((4, S), np.float32), explore=True)
    for r in (2, 0):                                  # member 0 too: the programs' records are its, but its block is a member's like any other
        grp.retire_members([r])
        block = sg.member_bytes(grp, r)
        others = [sg.state(grp._members[q]) for q in range(4)]
        obs = np.random.RandomState(r).randn(4, S).astype(np.float32)
        for _ in range(5):
            grp.train(rings, B)
        for explore in (True, False, True):
            grp.select_action(obs, explore=explore)
        assert torch.equal(sg.member_bytes(grp, r), block), (wl, r)
        for q in range(4):
            assert torch.equal(sg.state(grp._members[q])['params'], others[q]['params']) == (not grp.live[q]), (wl, r, q)
        del block


# ---- 3. revive ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_a_revived_member_continues_where_it_stood(wl):
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, alone_rings = sg.rings(wl, range(4))
    twin = sg.standalone(wl, SEEDS[2])
    for call in range(1, 21):
        live = grp.live[2]
        infos = grp.train(rings, B)
        if live:
            sg.assert_info_equal(infos[2], twin.train(alone_rings[2], B), (wl, call))
        else:
            assert infos[2] is None
        if call == 5:
            grp.retire_members([2])
            frozen = sg.state(grp._members[2])
        if call == 12:
            sg.assert_equal(sg.state(grp._members[2]), frozen, (wl, 'frozen'))
            grp.revive_members([2])
            assert grp.lineage[-1] == {'event': 'revive', 'kind': 'revive', 'members': [2], 'step': 12} and grp.live == [True] * 4
    # 5 + 8 = 13 calls of its own: its index and noise draws followed its own step counter
    sg.assert_equal(sg.state(grp._members[2]), sg.state(twin.core), (wl, 'revived'))
    assert int(sg.steps_words(grp._members[2])[0]) == 13 and int(sg.steps_words(grp._members[0])[0]) == 20


# ---- 4. respawn: clone a winner into a retired slot, perturb, revive -----------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_respawn_a_retired_slot_from_a_clone(wl):
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, alone_rings = sg.rings(wl, range(4))
    for _ in range(5):
        grp.train(rings, B)
    grp.retire_members([2])
    for _ in range(3):
        grp.train(rings, B)
    graph = grp._graph
    snap = dict(grp.member_snapshot(0))
    grp.clone_members([(0, 2)])
    grp.set_member_hyper(2, lr=7e-4)
    assert grp.member_hyper(2)['lr'] == 7e-4 and grp.member_snapshot(2)['hyper']['lr'] == 7e-4      # (works on a retired member)
    grp.revive_members([2])
    snap['seed'] = grp.seeds[2]
    twin = sg.standalone(wl, grp.seeds[2], grp.member_hyper(2))
    twin.load(snap)
    sg.assert_equal(sg.state(grp._members[2]), sg.state(twin.core), (wl, 'respawned'))
    for call in range(8):
        infos = grp.train(rings, B)
        sg.assert_info_equal(infos[2], twin.train(alone_rings[2], B), (wl, call))
    assert grp._graph is graph
    sg.assert_equal(sg.state(grp._members[2]), sg.state(twin.core), (wl, 'respawned + 8'))
    assert not torch.equal(grp._members[2].params, grp._members[0].params)
    assert [e.get('event', e['kind']) for e in grp.lineage] == ['retire', 'clone', 'retune', 'revive']


# ---- 5. same graph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', ['sac_halfcheetah_b256', SMALL_CTRL])
def test_retiring_keeps_the_graph_and_is_at_most_one_launch(wl):
    from rlrep_amd._lib import lib
    _, _, _, B, _ = sg.dims(wl)
    R = 8
    grp = sg.group(wl, tuple(range(100, 100 + R)))
    rings, alone_rings = sg.rings(wl, range(R))
    a = sg.standalone(wl, 100)
    a.train(alone_rings[0], B)
    for _ in range(3):
        grp.train(rings, B)
    graph, per_train = grp._graph, lib.rlrep_last_launch_count(grp.core.h)
    assert grp._graph_launches == a._graph_launches
    for op, members in (('retire', [1]), ('retire', [0, 2, 5]), ('revive', [2]), ('retire', [3, 4, 6])):
        n0 = lib.rlrep_launch_counter()
        (grp.retire_members if op == 'retire' else grp.revive_members)(members)
        assert 0 <= lib.rlrep_launch_counter() - n0 <= 1, (op, members)
        n0 = lib.rlrep_launch_counter()
        infos = grp.train(rings, B)
        assert lib.rlrep_launch_counter() == n0                      # a replay issues no launch of the library's: nothing was captured again
        assert grp._graph is graph and grp._graph_launches == a._graph_launches
        assert lib.rlrep_last_launch_count(grp.core.h) == per_train
        assert [i is not None for i in infos] == grp.live == _live_abi(grp)
    assert grp.live == [False, False, True, False, False, False, False, True]
    for r in (2, 7):
        assert all(np.isfinite(float(v)) for v in infos[r].values())


# ---- 6. acting ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_select_action_with_members_retired(wl):
    from rlrep_amd._lib import lib
    _, S, A, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, alone_rings = sg.rings(wl, range(4))
    alone = [sg.standalone(wl, s) for s in SEEDS]
    for _ in range(3):
        grp.train(rings, B)
        for r, a in enumerate(alone):
            a.train(alone_rings[r], B)
    obs = np.random.RandomState(5).randn(4, S).astype(np.float32)
    full = grp.select_action(obs, explore=False)
    for r, a in enumerate(alone):
        assert np.array_equal(full[r], a.select_action(obs[r], explore=False))
    grp.retire_members([0, 3])
    for explore in (False, True, True, False):
        seen = obs.copy()
        seen[0], seen[3] = np.nan, 1e30               # a retired member's observation is not looked at
        n0 = lib.rlrep_launch_counter()
        acts = grp.select_action(seen, explore=explore)
        assert lib.rlrep_launch_counter() - n0 == 1
        assert acts.shape == (4, A)
        for r, a in enumerate(alone):
            ref = a.select_action(obs[r], explore=explore)
            assert a._ctr == grp._ctr
            if grp.live[r]:
                assert np.array_equal(acts[r], ref), (explore, r, acts[r], ref)
            else:
                assert np.array_equal(acts[r], np.zeros(A, np.float32)), (explore, r, acts[r])


# ---- 7. independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_live_members_do_not_depend_on_a_retired_member(wl):
    _, _, _, B, _ = sg.dims(wl)
    runs = []
    for bump in (0.0, 1e-3):                     # only retired member 1's parameters differ between the two groups
        g = sg.group(wl, SEEDS)
        rings, _ = sg.rings(wl, range(4))
        for _ in range(3):
            g.train(rings, B)
        g.retire_members([1])
        g._members[1].params.add_(bump)
        for _ in range(6):
            g.train(rings, B)
        runs.append([sg.state(m) for m in g._members])
    for r in (0, 2, 3):
        sg.assert_equal(runs[0][r], runs[1][r], (wl, 'member', r))
    assert not torch.equal(runs[0][1]['params'], runs[1][1]['params'])


# ---- 8. checkpoints -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl', [SMALL_SAC, SMALL_CTRL])
def test_checkpoint_carries_the_live_mask(wl, tmp_path):
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, _ = sg.rings(wl, range(4))
    for _ in range(4):
        grp.train(rings, B)
    grp.retire_members([3])
    for _ in range(3):
        grp.train(rings, B)
    grp.retire_members([0])
    grp.train(rings, B)
    path = os.path.join(tmp_path, 'halving.pt')
    grp.save(path)
    snap = torch.load(path)
    assert snap['live'] == [False, True, True, False] and snap['lineage'] == grp.lineage and len(grp.lineage) == 2
    fresh = sg.group(wl, SEEDS)
    fresh.load(path)
    assert fresh.live == grp.live == _live_abi(fresh) and fresh.lineage == grp.lineage
    for r in range(4):
        sg.assert_equal(sg.state(grp._members[r]), sg.state(fresh._members[r]), (wl, 'loaded', r))
    for call in range(4):
        gi, fi = grp.train(rings, B), fresh.train(rings, B)
        for r in range(4):
            if grp.live[r]:
                sg.assert_info_equal(gi[r], fi[r], (wl, 'resumed', call, r))
            else:
                assert gi[r] is None and fi[r] is None
    for r in range(4):
        sg.assert_equal(sg.state(grp._members[r]), sg.state(fresh._members[r]), (wl, 'resumed', r))
    # a checkpoint written before members could retire has no mask: everybody is live
    old = {k: v for k, v in snap.items() if k != 'live'}
    fresh.load(old)
    assert fresh.live == [True] * 4 == _live_abi(fresh)
    infos = fresh.train(rings, B)
    assert all(i is not None for i in infos)
    assert not torch.equal(sg.state(fresh._members[0])['params'], sg.state(grp._members[0])['params'])


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    from rlrep_amd._lib import lib
    from rlrep_amd.core import _stream
    wl = SMALL_SAC
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, _ = sg.rings(wl, range(4))
    for _ in range(3):
        grp.train(rings, B)
    grp.retire_members([1])
    before = [sg.member_bytes(grp, r) for r in range(4)]
    lineage = [dict(e) for e in grp.lineage]
    launches = lib.rlrep_launch_counter()
    name = type(grp).__name__

    def raw(mask, handle=None):
        m = (C.c_int32 * 4)(*mask)
        rc = lib.rlrep_group_set_live(handle if handle is not None else grp.core.h, m, _stream())
        return rc, (lib.rlrep_last_error() or b'').decode()

    for call, members, words in (
            (grp.retire_members, [0, 2, 3], 'the last live members'),
            (grp.retire_members, [4], 'member 4 outside [0, 4)'),
            (grp.retire_members, [-1], 'member -1 outside [0, 4)'),
            (grp.revive_members, [7], 'member 7 outside [0, 4)'),
            (grp.retire_members, [1], 'member 1 is retired already'),
            (grp.revive_members, [2], 'member 2 is live already'),
            (grp.retire_members, [2, 2], 'member 2 is named twice'),
            (grp.retire_members, [], 'no member named')):
        with pytest.raises(ValueError) as e:
            call(members)
        assert words in str(e.value) and name in str(e.value), str(e.value)
    for mask, words in (([0, 0, 0, 0], 'no live member'), ([1, 2, 1, 1], 'neither 0 nor 1'), ([1, -1, 1, 1], 'neither 0 nor 1')):
        rc, msg = raw(mask)
        assert rc == -1 and words in msg and 'group_set_live' in msg, (mask, rc, msg)
    plain = sg.standalone(wl, 3)
    rc, msg = raw([1, 1, 1, 1], handle=plain.core.h)
    assert rc == -1 and 'not a seed group' in msg
    out = (C.c_int32 * 4)()
    assert lib.rlrep_group_get_live(plain.core.h, out) == -1 and 'not a seed group' in lib.rlrep_last_error().decode()
    assert lib.rlrep_launch_counter() == launches                    # refused before anything is launched
    assert grp.live == [True, False, True, True] == _live_abi(grp) and grp.lineage == lineage

    # inside a train(): between the group train prologue and the end of that train()
    ni, ne = grp._pool_sizes(B)
    ipool, epool = grp._buf('pool_idx', (ni,), torch.int32), grp._buf('pool_eps', (ne,))
    grp._draw_pools(rings, B, True, ipool, epool)
    n0 = lib.rlrep_launch_counter()
    rc, msg = raw([1, 0, 0, 1])
    assert rc == -1 and 'inside a train()' in msg, (rc, msg)
    with pytest.raises(RuntimeError, match=r'inside a train\(\)'):
        grp.retire_members([2])
    with pytest.raises(RuntimeError, match=r'inside a train\(\)'):
        grp.revive_members([1])
    assert lib.rlrep_launch_counter() == n0
    assert grp.live == [True, False, True, True] == _live_abi(grp) and grp.lineage == lineage
    assert torch.equal(sg.member_bytes(grp, 1), before[1])             # (the prologue itself left the retired member alone)
    assert lib.rlrep_end_train(grp.core.h) == 0
    rc, msg = raw([1, 0, 0, 1])
    assert rc == 0, msg
    assert _live_abi(grp) == [True, False, False, True]


# ---- 10. the launcher ---------------------------------------------------------------------------------------------------------------------
def test_launcher_halves_twice(tmp_path):
    """eval_freq 200 and a halving every 400 steps: exactly two halving steps lie behind start_timesteps (400 and 800), and 200 more steps follow
    the second, so the survivor's metrics.jsonl outgrows both retired pairs'."""
    from rlrep_amd import main
    from rlrep_amd.agent import pbt
    agent, evals = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1,2,3', '--max_timesteps', '1000', '--start_timesteps', '200',
                             '--eval_freq', '200', '--halving-interval', '400', '--batch_size', '64', '--eval_episodes', '1',
                             '--log_root', str(tmp_path)])
    base = os.path.join(tmp_path, 'Pendulum-v1', 'sac', '0')
    events = [json.loads(l) for l in open(os.path.join(base, 'halving.jsonl'))]
    assert [e['step'] for e in events] == [400, 800] and [e['live'] for e in events] == [2, 1]
    assert [len(e['retired']) for e in events] == [2, 1]
    rows = [[json.loads(l) for l in open(os.path.join(base, str(s), 'metrics.jsonl'))] for s in range(4)]
    steps = [[row['step'] for row in member] for member in rows]
    live = [True] * 4
    for e in events:
        # the plan is the one pbt.plan_halving makes of the evaluations the launcher logged at that step
        scores = [([row['info/evaluation'] for row in rows[r] if row['step'] == e['step']] + [float('nan')])[0] for r in range(4)]
        assert e['retired'] == pbt.plan_halving(scores, live, 0.5) and e['seeds'] == e['retired']
        assert e['scores'] == [scores[r] for r in e['retired']]
        for r in e['retired']:
            live[r] = False
    assert agent.live == live and sum(live) == 1
    survivor = live.index(True)
    assert steps[survivor] == [400, 600, 800, 1000]
    for r in events[0]['retired']:
        assert steps[r] == [400]
    assert steps[events[1]['retired'][0]] == [400, 600, 800]
    assert [len(evals[r]) for r in range(4)] == [1 + len(steps[r]) + 1 for r in range(4)]          # (initial evaluation, step 200, then one per row)
    assert [e['event'] for e in agent.lineage] == ['retire', 'retire'] and [e['members'] for e in agent.lineage] == [ev['retired'] for ev in events]
    # the group went on training for the survivor alone: one train() per step beyond start_timesteps
    assert agent.steps == 800
