"""Hyper-parameter sweeps in seed groups on the MI355X (SeedBatchMixin member_hyper, include/rlrep.h rlrep_group_set_member_hyper): every
member of a sweep group computes, bit for bit, what the standalone agent built with its seed and its hyper-parameters computes on the same
replay ring, in a train() graph of one standalone agent's launch count."""
import ctypes as C
import json
import math
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

# (seed, member_hyper): lr x seeds with a repeated seed, and discount, tau, target_update_period 1 / 2 / 3, alpha, no temperature learning
SAC_MEMBERS = (
    (3, dict(lr=1e-4)),
    (3, dict(lr=3e-4, target_update_period=1)),
    (11, dict(lr=1e-4, discount=0.95, tau=0.01)),
    (11, dict(lr=3e-4, target_update_period=3, alpha=0.2)),
    (42, dict(lr=3e-4, auto_entropy_tuning=False, alpha=0.05)),
    (42, dict(lr=2e-4, tau=0.02, discount=0.9, target_update_period=2)),
)
CTRL_MEMBERS = (
    (3, dict(lr=1e-4)),
    (3, dict(lr=3e-4, tau=0.01)),
    (11, dict(feature_tau=0.01, discount=0.95)),
    (42, dict(lr=5e-5, feature_tau=0.02, tau=0.002, discount=0.98)),
)
CTRL_F2048_MEMBERS = ((3, dict(lr=1e-4)), (11, dict(lr=3e-4, feature_tau=0.02)))
SAC_WORKLOADS = ('sac_pendulum_b64', 'sac_halfcheetah_b256')
CTRL_SMALL = 'ctrlsac_halfcheetah_f256_b256'


def _swept_state(core):
    """sg.state and the optimizer records' hyper words: the member's lr / tau"""
    return sg.state(core, hyper=True)


def _bit_exact(wl, members, calls, **extra):
    _, _, _, B, _ = sg.dims(wl, **extra)
    grp = sg.group(wl, *zip(*members), **extra)
    rings, alone_rings = sg.rings(wl, range(len(members)))
    alone = [sg.standalone(wl, s, h, **extra) for s, h in members]
    for r in range(len(members)):
        sg.assert_equal(_swept_state(grp._members[r]), _swept_state(alone[r].core), ('init', r))
    for call in range(1, calls + 1):
        infos = grp.train(rings, B)
        ainfos = [a.train(alone_rings[r], B) for r, a in enumerate(alone)]
        if call in (1, 2, calls):
            for r in range(len(members)):
                sg.assert_info_equal(infos[r], ainfos[r], (wl, call, r))
                sg.assert_equal(_swept_state(grp._members[r]), _swept_state(alone[r].core), (wl, call, r))
    return grp


@pytest.mark.parametrize('wl', SAC_WORKLOADS)
def test_sac_sweep_members_equal_standalone_agents_bit_for_bit(wl):
    grp = _bit_exact(wl, SAC_MEMBERS, 25)
    # the members really differ: same seed, other hyper -> other parameters
    assert not torch.equal(grp._members[0].params, grp._members[1].params)
    # no temperature learning: log(alpha) stays where alpha put it
    assert grp._members[4].alpha_state[0].item() == float(np.log(0.05))


def test_ctrlsac_sweep_members_equal_standalone_agents_bit_for_bit():
    _bit_exact(CTRL_SMALL, CTRL_MEMBERS, 25)


def test_ctrlsac_sweep_without_feature_target():
    _bit_exact(CTRL_SMALL, CTRL_MEMBERS, 10, use_feature_target=False)


def test_ctrlsac_sweep_f2048_two_members():
    _bit_exact('ctrlsac_halfcheetah_f2048_b256', CTRL_F2048_MEMBERS, 10)


@pytest.mark.parametrize('wl, members', [('sac_halfcheetah_b256', SAC_MEMBERS), (CTRL_SMALL, CTRL_MEMBERS)])
def test_sweep_group_graph_has_one_agents_launch_count(wl, members):
    _, S, A, B, _ = sg.dims(wl)
    a = sg.standalone(wl, 3, {})
    buf, _ = bench.synth_buffer(S, A, 0)
    a.train(buf, B)
    for R in (1, 3, 8):
        mem = [(100 + (r % 2), dict(members[r % len(members)][1], discount=0.9 + 0.01 * r)) for r in range(R)]
        g = sg.group(wl, *zip(*mem))
        rings, _ = sg.rings(wl, range(R))
        g.train(rings, B)
        assert g._graph_launches == a._graph_launches, (wl, R, g._graph_launches, a._graph_launches)


def test_set_member_hyper_between_replays_changes_that_member_only():
    from rlrep_amd._lib import lib, check
    from rlrep_amd.core import _stream
    wl = 'sac_halfcheetah_b256'
    _, _, _, B, _ = sg.dims(wl)
    members = SAC_MEMBERS[:3]
    runs = []
    for change in (False, True):
        g = sg.group(wl, *zip(*members))
        rings, _ = sg.rings(wl, range(len(members)))
        for _ in range(3):
            g.train(rings, B)
        graph = g._graph
        if change:
            hp = dict(g.member_hyper(1), lr=1e-3, discount=0.8, tau=0.05, target_update_period=2, auto_entropy_tuning=False)
            check(lib.rlrep_group_set_member_hyper(g.core.h, 1, C.byref(g._hyper_struct(g.core, hp)), _stream()), 'set_member_hyper')
        for _ in range(4):
            g.train(rings, B)
        assert g._graph is graph                 # the same captured graph replays the new values: no re-capture
        runs.append([_swept_state(m) for m in g._members])
    sg.assert_equal(runs[0][0], runs[1][0], 'member 0')
    sg.assert_equal(runs[0][2], runs[1][2], 'member 2')
    for k in ('params', 'targets', 'alpha_state', 'optimizer_hyper'):
        assert not torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_member_hyper_abi_refusals_and_read_back():
    from rlrep_amd import _lib
    from rlrep_amd._lib import lib
    from rlrep_amd.core import _stream
    wl = 'sac_pendulum_b64'
    g = sg.group(wl, *zip(*SAC_MEMBERS[:2]))
    good = g._hyper_struct(g.core, g.member_hyper(1))
    out = _lib.Hyper()
    assert lib.rlrep_group_get_member_hyper(g.core.h, 1, C.byref(out)) == 0
    for f, _ in _lib.Hyper._fields_:
        assert getattr(out, f) == getattr(good, f), f
    assert lib.rlrep_group_set_member_hyper(g.core.h, 1, C.byref(good), _stream()) == 0

    def refused(h, words, member=1, handle=None):
        rc = lib.rlrep_group_set_member_hyper(handle if handle is not None else g.core.h, member, C.byref(h), _stream())
        msg = (lib.rlrep_last_error() or b'').decode()
        assert rc == -1 and words in msg, (words, rc, msg)

    def bad(**kw):
        h = _lib.Hyper.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(h, k, v)
        return h
    plain = sg.standalone(wl, 3, {})
    refused(good, 'not a seed group', handle=plain.core.h)
    refused(good, 'member 2 outside [0, 2)', member=2)
    refused(good, 'member -1 outside', member=-1)
    refused(bad(beta1=0.8), 'beta1 is structural')
    refused(bad(target_entropy=-3.0), 'target_entropy is structural')
    refused(bad(extra_feature_steps=2), 'extra_feature_steps is structural')
    refused(bad(world_size=2), 'world_size is structural')
    refused(bad(lr_critic=float('nan')), 'lr_critic nan is not a finite positive')
    refused(bad(lr_actor=0.0), 'lr_actor 0 is not a finite positive')
    refused(bad(lr_feature=-1e-4), 'lr_feature')
    refused(bad(lr_critic=float('inf')), 'lr_critic inf')
    refused(bad(tau=1.5), 'tau 1.5 outside [0, 1]')
    refused(bad(feature_tau=-0.1), 'feature_tau -0.1 outside [0, 1]')
    refused(bad(target_update_period=0), 'target_update_period 0 is below 1')
    # nothing refused reached the member: its values are still the good ones
    assert lib.rlrep_group_get_member_hyper(g.core.h, 1, C.byref(out)) == 0 and out.lr_critic == good.lr_critic and out.tau == good.tau


def test_member_export_and_sweep_group_checkpoint(tmp_path):
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    wl = 'sac_pendulum_b64'
    _, S, A, B, kw = sg.dims(wl)
    members = SAC_MEMBERS[:4]
    grp = sg.group(wl, *zip(*members))
    rings, alone_rings = sg.rings(wl, range(len(members)))
    for _ in range(6):
        grp.train(rings, B)
    path = os.path.join(tmp_path, 'group.pt')
    grp.save(path)
    assert [m['hyper'] for m in grp.state_snapshot()['members']] == [grp.member_hyper(r) for r in range(len(members))]
    r = 3
    a = SACAgent(S, A, bench.Space(A), max_batch=B, seed=12345, **kw, **grp.member_hyper(r))
    a.load(grp.member_snapshot(r))
    grp2 = sg.group(wl, *zip(*members))
    grp2.load(path)
    for _ in range(4):
        gi = grp.train(rings, B)
        ai = a.train(alone_rings[r], B)
        g2i = grp2.train(rings, B)
    sg.assert_info_equal(gi[r], ai, 'export')
    sg.assert_equal(_swept_state(grp._members[r]), _swept_state(a.core), 'export')
    for q in range(len(members)):
        sg.assert_info_equal(gi[q], g2i[q], ('checkpoint', q))
        sg.assert_equal(_swept_state(grp._members[q]), _swept_state(grp2._members[q]), ('checkpoint', q))
    other = [(s, dict(h)) for s, h in members]
    other[2][1]['tau'] = 0.03
    grp3 = sg.group(wl, *zip(*other))
    with pytest.raises(RuntimeError, match='member 2 hyper-parameters differ'):
        grp3.load(path)


def test_launcher_sweeps_lr_across_seeds(tmp_path):
    from rlrep_amd import main
    agent, evals = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--sweep', 'lr=1e-4,3e-4', '--max_timesteps', '400',
                             '--start_timesteps', '200', '--eval_freq', '200', '--batch_size', '64', '--eval_episodes', '1',
                             '--log_root', str(tmp_path)])
    assert agent.R == 4 and agent.seeds == [0, 1, 0, 1] and len(evals) == 4 and agent.steps == 200
    assert [agent.member_hyper(r)['lr'] for r in range(4)] == [1e-4, 1e-4, 3e-4, 3e-4]
    for tag in ('lr=0.0001', 'lr=0.0003'):
        for s in (0, 1):
            rows = [json.loads(l) for l in open(os.path.join(tmp_path, 'Pendulum-v1', 'sac', '0', tag, str(s), 'metrics.jsonl'))]
            assert len(rows) >= 1 and all(math.isfinite(v) for row in rows for v in row.values())
            assert 'info/evaluation' in rows[-1]
