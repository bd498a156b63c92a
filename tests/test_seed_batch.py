"""Seed groups on the MI355X (rlrep_amd/agent/sac/seed_batch.py): every member of a SACSeedBatch computes, bit for bit, what a standalone
SACAgent with its seed computes on the same replay ring, in a train() graph of one agent's launch count."""
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

SEEDS = (3, 11, 42)
WORKLOADS = ('sac_pendulum_b64', 'sac_halfcheetah_b256')


@pytest.mark.parametrize('wl', WORKLOADS)
def test_members_equal_standalone_agents_bit_for_bit(wl):
    _, _, _, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, alone_rings = sg.rings(wl, range(len(SEEDS)))
    alone = [sg.standalone(wl, s) for s in SEEDS]
    for r in range(len(SEEDS)):
        sg.assert_equal(sg.state(grp._members[r]), sg.state(alone[r].core), ('init', r))
    for call in range(1, 26):
        infos = grp.train(rings, B)
        ainfos = [a.train(alone_rings[r], B) for r, a in enumerate(alone)]
        if call in (1, 2, 25):
            for r in range(len(SEEDS)):
                sg.assert_info_equal(infos[r], ainfos[r], (call, r))
                sg.assert_equal(sg.state(grp._members[r]), sg.state(alone[r].core), (call, r))


def test_group_graph_has_one_agents_launch_count():
    wl = 'sac_pendulum_b64'
    _, _, _, B, _ = sg.dims(wl)
    a = sg.standalone(wl, 3)
    buf, _ = bench.synth_buffer(*sg.dims(wl)[1:3], 0)
    a.train(buf, B)
    for R in (1, 3, 8):
        seeds = tuple(range(100, 100 + R))
        g = sg.group(wl, seeds)
        rings, _ = sg.rings(wl, range(R))
        g.train(rings, B)
        assert g._graph_launches == a._graph_launches, (R, g._graph_launches, a._graph_launches)


def test_members_are_independent():
    wl = 'sac_halfcheetah_b256'
    _, _, _, B, _ = sg.dims(wl)
    runs = []
    for data in ((0, 1, 2), (0, 7, 2)):           # only member 1's ring differs
        g = sg.group(wl, SEEDS)
        rings, _ = sg.rings(wl, data)
        for _ in range(5):
            g.train(rings, B)
        runs.append([sg.state(m) for m in g._members])
    sg.assert_equal(runs[0][0], runs[1][0], 'member 0')
    sg.assert_equal(runs[0][2], runs[1][2], 'member 2')
    assert not torch.equal(runs[0][1]['params'], runs[1][1]['params'])


def test_init_rule():
    for wl in WORKLOADS:
        grp = sg.group(wl, SEEDS)
        for r, s in enumerate(SEEDS):
            a = sg.standalone(wl, s)
            m = grp.member(r)
            for name, mod in (('critic', a.critic), ('critic_target', a.critic_target), ('actor', a.actor)):
                sd, gd = mod.state_dict(), getattr(m, name).state_dict()
                assert sd.keys() == gd.keys()
                for k in sd:
                    assert torch.equal(sd[k], gd[k]), (wl, r, name, k)
            assert torch.equal(m.log_alpha, a.log_alpha) and torch.equal(m.alpha, a.alpha)


def test_member_export_and_group_checkpoint(tmp_path):
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    wl = 'sac_pendulum_b64'
    _, S, A, B, kw = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, alone_rings = sg.rings(wl, range(len(SEEDS)))
    for _ in range(10):
        grp.train(rings, B)
    path = os.path.join(tmp_path, 'group.pt')
    grp.save(path)
    a = SACAgent(S, A, bench.Space(A), max_batch=B, seed=12345, **kw)
    a.load(grp.member_snapshot(2))
    grp2 = sg.group(wl, SEEDS)
    grp2.load(path)
    for _ in range(5):
        gi = grp.train(rings, B)
        ai = a.train(alone_rings[2], B)
        g2i = grp2.train(rings, B)
    sg.assert_info_equal(gi[2], ai, 'export')
    sg.assert_equal(sg.state(grp._members[2]), sg.state(a.core), 'export')
    for r in range(len(SEEDS)):
        sg.assert_info_equal(gi[r], g2i[r], ('checkpoint', r))
        sg.assert_equal(sg.state(grp._members[r]), sg.state(grp2._members[r]), ('checkpoint', r))


@pytest.mark.parametrize('wl', WORKLOADS)
def test_group_select_action_equals_standalone_in_one_launch(wl):
    from rlrep_amd._lib import lib
    _, S, A, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    rings, alone_rings = sg.rings(wl, range(len(SEEDS)))
    alone = [sg.standalone(wl, s) for s in SEEDS]
    for _ in range(3):                                  # trained actors, not just initial ones
        grp.train(rings, B)
        for r, a in enumerate(alone):
            a.train(alone_rings[r], B)
    obs = np.random.RandomState(5).randn(len(SEEDS), S).astype(np.float32)
    for explore in (False, True, True):
        n0 = lib.rlrep_launch_counter()
        acts = grp.select_action(obs, explore=explore)
        assert lib.rlrep_launch_counter() - n0 == 1
        assert acts.shape == (len(SEEDS), A)
        for r, a in enumerate(alone):
            ref = a.select_action(obs[r], explore=explore)
            assert a._ctr == grp._ctr
            assert np.array_equal(acts[r], ref), (wl, explore, r, acts[r], ref)


def test_entry_points_without_a_group_form_refuse_a_group():
    import ctypes as C
    from rlrep_amd._lib import lib
    wl = 'sac_pendulum_b64'
    _, S, A, B, _ = sg.dims(wl)
    grp = sg.group(wl, SEEDS)
    obs = torch.zeros(1, S).pin_memory()
    act = torch.zeros(1, A).pin_memory()
    rc = lib.rlrep_select_action(grp.core.h, C.c_void_p(obs.data_ptr()), 1, 0, 0, 0, -1.0, 1.0, C.c_void_p(act.data_ptr()), 1, None)
    assert rc == -1 and b'seed group' in lib.rlrep_last_error()
    rings, _ = sg.rings(wl, range(len(SEEDS)))
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    rc = lib.rlrep_replay_sample(grp.core.h, 0, C.c_void_p(rings.ring.data_ptr()), C.c_void_p(idx.data_ptr()), B, None)
    assert rc == -1 and b'seed group' in lib.rlrep_last_error()
    # the group prologue only writes pools that lie inside member 0's block (it writes them again at every member's stride)
    ipool = torch.zeros(B, dtype=torch.int32, device='cuda')
    epool = torch.zeros(2 * B * A, device='cuda')
    rc = lib.rlrep_group_train_prologue(grp.core.h, C.c_void_p(rings.ring.data_ptr()), 4 * rings.ring_stride, C.c_void_p(rings.size_dev().data_ptr()),
                                        C.c_void_p(ipool.data_ptr()), B, C.c_void_p(epool.data_ptr()), 2 * B * A, 1 << 40, 2 << 40, B, None)
    assert rc == -1 and b"inside member 0's block" in lib.rlrep_last_error()


def test_launcher_trains_several_seeds(tmp_path):
    import json
    from rlrep_amd import main
    agent, evals = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--max_timesteps', '600', '--start_timesteps', '300',
                             '--eval_freq', '300', '--batch_size', '64', '--eval_episodes', '1', '--log_root', str(tmp_path)])
    assert agent.R == 2 and agent.steps == 300 and len(evals) == 2
    for s in (0, 1):
        rows = [json.loads(l) for l in open(os.path.join(tmp_path, 'Pendulum-v1', 'sac', '0', str(s), 'metrics.jsonl'))]
        assert len(rows) >= 1 and all(np.isfinite(v) for r in rows for v in r.values())
        assert {'info/q_loss', 'info/actor_loss', 'info/alpha', 'info/evaluation'} <= set(rows[-1])
