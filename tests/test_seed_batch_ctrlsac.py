"""ctrlsac seed groups on the MI355X (rlrep_amd/agent/ctrlsac/seed_batch.py): every member of a CTRLSACSeedBatch computes, bit for bit, what
a standalone CTRLSACAgent(pipeline=False) with its seed computes on the same replay ring -- feature steps with their InfoNCE loss, the
frozen_phi copies, critic and actor steps -- in a train() graph of one such agent's launch count."""
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
WORKLOADS = ('ctrlsac_halfcheetah_f256_b256', 'ctrlsac_halfcheetah_f2048_b256')
SMALL = 'ctrlsac_halfcheetah_f256_b256'


def _frozen_equal_phi(agent_or_member):
    """quirk Q8: after a train(), frozen_phi holds phi's values"""
    phi, frozen = agent_or_member.phi.state_dict(), agent_or_member.frozen_phi.state_dict()
    return all(torch.equal(phi[k], frozen[k]) for k in phi)


def _bit_exact(wl, calls, **extra):
    _, _, _, B, _ = sg.dims(wl, **extra)
    grp = sg.group(wl, SEEDS, **extra)
    rings, alone_rings = sg.rings(wl, range(len(SEEDS)))
    alone = [sg.standalone(wl, s, **extra) for s in SEEDS]
    for r in range(len(SEEDS)):
        sg.assert_equal(sg.state(grp._members[r]), sg.state(alone[r].core), ('init', r))
    for call in range(1, calls + 1):
        infos = grp.train(rings, B)
        ainfos = [a.train(alone_rings[r], B) for r, a in enumerate(alone)]
        if call in (1, 2, calls):
            for r in range(len(SEEDS)):
                sg.assert_info_equal(infos[r], ainfos[r], (wl, call, r))
                sg.assert_equal(sg.state(grp._members[r]), sg.state(alone[r].core), (wl, call, r))
    for r in range(len(SEEDS)):
        assert _frozen_equal_phi(grp.member(r))
    return grp


@pytest.mark.parametrize('wl', WORKLOADS)
def test_members_equal_standalone_agents_bit_for_bit(wl):
    _bit_exact(wl, 25)


def test_members_equal_standalone_agents_without_feature_target():
    grp = _bit_exact(SMALL, 10, use_feature_target=False)
    assert not hasattr(grp.member(0), 'phi_target') and not hasattr(grp.member(0), 'frozen_phi_target')


def test_group_graph_has_one_agents_launch_count():
    _, _, _, B, _ = sg.dims(SMALL)
    a = sg.standalone(SMALL, 3)
    buf, _ = bench.synth_buffer(*sg.dims(SMALL)[1:3], 0)
    a.train(buf, B)
    for R in (1, 3, 8):
        g = sg.group(SMALL, tuple(range(100, 100 + R)))
        rings, _ = sg.rings(SMALL, range(R))
        g.train(rings, B)
        assert g._graph_launches == a._graph_launches, (R, g._graph_launches, a._graph_launches)


def test_members_are_independent():
    _, _, _, B, _ = sg.dims(SMALL)
    runs = []
    for bump in (0.0, 1e-3):                     # only member 1's parameters differ between the two groups
        g = sg.group(SMALL, SEEDS)
        rings, _ = sg.rings(SMALL, range(len(SEEDS)))
        g._members[1].params.add_(bump)
        for _ in range(5):
            g.train(rings, B)
        runs.append([sg.state(m) for m in g._members])
    sg.assert_equal(runs[0][0], runs[1][0], 'member 0')
    sg.assert_equal(runs[0][2], runs[1][2], 'member 2')
    assert not torch.equal(runs[0][1]['params'], runs[1][1]['params'])


def test_group_select_action_equals_standalone_in_one_launch():
    from rlrep_amd._lib import lib
    _, S, A, B, _ = sg.dims(SMALL)
    grp = sg.group(SMALL, SEEDS)
    rings, alone_rings = sg.rings(SMALL, range(len(SEEDS)))
    alone = [sg.standalone(SMALL, s) for s in SEEDS]
    for _ in range(3):
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
            assert np.array_equal(acts[r], ref), (explore, r, acts[r], ref)


def test_member_export_and_group_checkpoint(tmp_path):
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    _, S, A, B, kw = sg.dims(SMALL)
    grp = sg.group(SMALL, SEEDS)
    rings, alone_rings = sg.rings(SMALL, range(len(SEEDS)))
    for _ in range(6):
        grp.train(rings, B)
    path = os.path.join(tmp_path, 'group.pt')
    grp.save(path)
    a = CTRLSACAgent(S, A, bench.Space(A), max_batch=B, seed=12345, pipeline=False, **kw)
    a.load(grp.member_snapshot(2))
    grp2 = sg.group(SMALL, SEEDS)
    grp2.load(path)
    for _ in range(4):
        gi = grp.train(rings, B)
        ai = a.train(alone_rings[2], B)
        g2i = grp2.train(rings, B)
    sg.assert_info_equal(gi[2], ai, 'export')
    sg.assert_equal(sg.state(grp._members[2]), sg.state(a.core), 'export')
    for r in range(len(SEEDS)):
        sg.assert_info_equal(gi[r], g2i[r], ('checkpoint', r))
        sg.assert_equal(sg.state(grp._members[r]), sg.state(grp2._members[r]), ('checkpoint', r))


def test_launcher_trains_several_ctrlsac_seeds(tmp_path):
    import json
    from rlrep_amd import main
    agent, evals = main.run(['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--max_timesteps', '400', '--start_timesteps', '200',
                             '--eval_freq', '200', '--batch_size', '64', '--eval_episodes', '1', '--log_root', str(tmp_path)])
    assert agent.R == 2 and agent.steps == 200 and len(evals) == 2 and agent.feature_dim == 2048
    for s in (0, 1):
        rows = [json.loads(l) for l in open(os.path.join(tmp_path, 'Pendulum-v1', 'ctrlsac', '0', str(s), 'metrics.jsonl'))]
        assert len(rows) >= 1 and all(np.isfinite(v) for r in rows for v in r.values())
        assert 'info/evaluation' in rows[-1] and len([k for k in rows[-1] if k.startswith('info/')]) >= 3
