"""What the seed-group tests share (test_seed_batch*.py, test_pbt*.py, test_halving*.py, test_device_env*.py): building a group, its
standalone twins and their replay rings from a bench.py workload, and `state` -- the one definition of "everything a train() writes and a
checkpoint restores".  A plain module, imported like fixture_io.py."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def dims(wl, **extra):
    """(alg, S, A, B, constructor kwargs) of bench.py workload `wl`, the kwargs updated with `extra`"""
    alg, S, A, B, kw = bench.WORKLOADS[wl]
    kw = dict(kw)
    kw.update(extra)
    return alg, S, A, B, kw


def standalone(wl, seed, hyper=None, **extra):
    """the standalone agent a group member with `seed` and the hyper-parameters `hyper` must equal (ctrlsac: the unpipelined agent)"""
    alg, S, A, B, kw = dims(wl, **extra)
    kw.update(hyper or {})
    torch.manual_seed(seed)
    if alg == 'sac':
        from rlrep_amd.agent.sac.sac_agent import SACAgent
        return SACAgent(S, A, bench.Space(A), max_batch=B, seed=seed, **kw)
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    return CTRLSACAgent(S, A, bench.Space(A), max_batch=B, seed=seed, pipeline=False, **kw)


def group(wl, seeds, member_hyper=None, **extra):
    """the seed group of `wl`'s algorithm; member_hyper: one dict per member (a sweep), or None / all None for a plain group"""
    alg, S, A, B, kw = dims(wl, **extra)
    if alg == 'sac':
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch as G
    else:
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch as G
    mh = None if member_hyper is None or all(h is None for h in member_hyper) else [dict(h) for h in member_hyper]
    return G(list(seeds), S, A, bench.Space(A), max_batch=B, member_hyper=mh, **kw)


def rings(wl, data_seeds):
    """The group's rings and the standalone rings: member r's ring holds bench.synth_buffer(S, A, data_seeds[r])."""
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    _, S, A, _, _ = dims(wl)
    g = ReplayBufferGroup(len(data_seeds), S, A, max_size=bench.REPLAY_N)
    alone = []
    for r, ds in enumerate(data_seeds):
        buf, data = bench.synth_buffer(S, A, ds)
        g.load(r, data['state'], data['action'], data['next_state'], data['reward'], data['done'])
        alone.append(buf)
    return g, alone


def steps_words(core):
    """the train() counter block of an agent / a group member (words 0 and 2: include/rlrep.h rlrep_steps_dev)"""
    from rlrep_amd._lib import lib
    ws0 = core._group.workspace if hasattr(core, '_group') else core.workspace
    off = lib.rlrep_steps_dev(core.h) - ws0.data_ptr()
    return core.workspace[off:off + 16].view(torch.int32).clone()


def state(core, hyper=False):
    """Everything a train() writes and a checkpoint restores: parameters and targets (ctrlsac: frozen_phi / frozen_phi_target included), Adam
    moments and step counts, the float64 temperature state, the train() counter.  hyper: also words 1..5 (lr, beta1, beta2, eps, tau) of the
    optimizer records, which are the member's own (a clone does not copy them)."""
    torch.cuda.synchronize()
    cfg = core.group_cfg()
    s = {'params': core.params.clone(), 'targets': core.targets.clone(), 'exp_avg': core.exp_avg.clone(),
         'exp_avg_sq': core.exp_avg_sq.clone(), 'alpha_state': core.alpha_state.clone(),
         'optimizer_steps': cfg[:, 0].view(torch.int32).clone(), 'train_steps': steps_words(core)}
    if hyper:
        s['optimizer_hyper'] = cfg[:, 1:6].clone()
    return s


def assert_equal(sa, sb, what):
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


def assert_info_equal(ia, ib, what):
    assert set(ia.keys()) == set(ib.keys())
    for k in ia.keys():
        a, b = ia[k], ib[k]
        a = a.item() if torch.is_tensor(a) else a
        b = b.item() if torch.is_tensor(b) else b
        assert a == b or (a != a and b != b), (what, k, a, b)


def member_bytes(grp, r):
    """member r's whole block of the group allocation: arenas, device records, workspace (slot buffers, history ring), pools"""
    torch.cuda.synchronize()
    stride, skew = grp.core.member_stride, grp.core._skew
    return grp.core._block[skew + r * stride:skew + (r + 1) * stride].clone()


def run_launcher(argv):
    """the launcher with `argv`, for the tests of its refusals (SystemExit before anything touches a GPU)"""
    from rlrep_amd import main
    main.run(argv)
