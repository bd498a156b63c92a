"""The one-graph simulator loop of a seed group (csrc/actor_tile.hip actor_tile_kernel_ctl_grp, csrc/elementwise.hip
replay_add_cols_kernel_ctl_grp, csrc/sim_step.hip sim_*_kernel_grp, envs/sim_loop.py SimLoopGroup, envs/fused_sim.py FusedSimGroup,
SeedBatchMixin.iterate_sim, main.py --seeds ... --torch-envs N --sim-graph --fused-sim) on the GPU.

Everything is exact (uint32 / uint64 views or torch.equal): plane r of every group launch is what the single form gives a standalone twin
with seed seeds[r], and a group run through iterate_sim ends bit-identical, member by member, to SACAgent / CTRLSACAgent twins run through
the single SimLoop + FusedSim + iterate_sim.  Hidden widths are 64, R = 3.  Reads nothing outside the repository.

The launch count of the separate route: the captured iteration holds four launches in front of train() -- the copy of the observations, act,
step, append -- of which `_sim_launches` (the library's launch counter) sees the library's three; the copy is torch's, as in the single
agent's tests (tests/test_fused_sim.py: + 3), and is shown to have run inside the graph by what it copied."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import fused_sim_reference as fref  # noqa: E402
import seed_group_util as sg  # noqa: E402
import sim_loop_group_reference as gref  # noqa: E402
import sim_loop_reference as ref  # noqa: E402
from test_device_env import dynamics_cases  # noqa: E402
from test_device_env_mountaincar import mountaincar_dynamics_cases  # noqa: E402
from test_device_env_single import _host_env  # noqa: E402

DEV = 'cuda'
SEEDS = (5, 9, 2)
R = len(SEEDS)
B = 64
KIND_ID = {'pendulum': fref.PENDULUM, 'mountaincar': fref.MOUNTAIN_CAR}
CASES = {'pendulum': dynamics_cases, 'mountaincar': mountaincar_dynamics_cases}
ARRAYS = ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')
NS = (1, 15, 16, 17, 33)
F32 = lambda x: float(np.float32(x))  # noqa: E731
CONFIGS = {                                 # name: (alg, S, A, kind or None, constructor extras)
    'sac_pendulum': ('sac', 3, 1, 'pendulum', dict(hidden_dim=64)),
    'sac_mountaincar': ('sac', 2, 1, 'mountaincar', dict(hidden_dim=64)),
    'sac_s17_a6': ('sac', 17, 6, None, dict(hidden_dim=64)),              # A = 6: u_j from two Philox blocks; K = 17
    'ctrlsac_f64': ('ctrlsac', 3, 1, 'pendulum', dict(hidden_dim=64, feature_dim=64, extra_feature_steps=3)),
}


def _space(cfg):
    _, _, A, kind, _ = CONFIGS[cfg]
    return _host_env(kind).action_space if kind else bench.Space(A)


def _group(cfg, seeds=SEEDS):
    alg, S, A, _, kw = CONFIGS[cfg]
    if alg == 'sac':
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch as G
    else:
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch as G
    return G(list(seeds), S, A, _space(cfg), max_batch=B, **kw)


def _twin(cfg, seed):
    """the standalone agent member `seed` must equal (ctrlsac: the unpipelined agent)"""
    alg, S, A, _, kw = CONFIGS[cfg]
    torch.manual_seed(seed)
    if alg == 'sac':
        from rlrep_amd.agent.sac.sac_agent import SACAgent
        return SACAgent(S, A, _space(cfg), max_batch=B, seed=seed, **kw)
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    return CTRLSACAgent(S, A, _space(cfg), max_batch=B, seed=seed, pipeline=False, **kw)


class _Still(object):
    """a simulator that only holds observations (the kernel tests launch the two forms themselves)"""

    def __init__(self, obs):
        self.obs = obs

    def step_(self, actions):
        raise AssertionError('not stepped')


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _words(loop):
    torch.cuda.synchronize()
    return loop.ctl.cpu().numpy().copy()


def _same(a, b):
    """bit for bit, NaNs included"""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


# ---- 1. the act form --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['sac_pendulum', 'sac_s17_a6'])
def test_act_form_planes_equal_the_twins_single_form_and_the_restated_mix(cfg):
    from rlrep_amd._lib import lib
    from rlrep_amd.envs import sim_loop as sl
    _, S, A, _, _ = CONFIGS[cfg]
    grp = _group(cfg)
    twins = [_twin(cfg, s) for s in SEEDS]
    lo, hi = grp.action_range
    gen = torch.Generator(device=DEV).manual_seed(7)
    CAP, PTRS, SIZES = 40, (30, 0, 39), (35, 0, 40)             # every member its own cursor and fill level
    mixed = 0
    for k, N in enumerate(NS):
        obs = torch.randn(R, N, S, device=DEV, generator=gen)
        calls, it = 100 + 7 * k, 3 + k
        want = []
        for r, twin in enumerate(twins):
            twin._ctr = calls
            want.append(twin.act_device(obs[r], explore=True).cpu().numpy())
        for eps, start, t in ((0.0, 0, 0), (0.5, 0, 5 * N), (0.0, 8 * N, 7 * N)):
            loop = sl.SimLoopGroup(grp, _Still(obs), eps_greedy=eps, start_timesteps=start)
            loop.set_counters(t, calls, it)
            w = _words(loop)
            w[:, sl.NEXT_PTR], w[:, sl.SIZE] = PTRS, SIZES
            loop._write(w)
            out = torch.full((R, N, A), 9.0, device=DEV)
            n0 = lib.rlrep_launch_counter()
            loop.act(obs, out, CAP)
            assert lib.rlrep_launch_counter() - n0 == 1
            warm = t < start
            got = out.cpu().numpy()
            for r, twin in enumerate(twins):
                single = sl.SimLoop(twin, _Still(obs[r]), eps_greedy=eps, start_timesteps=start)
                single.set_counters(t, calls, it)
                single.set_cursor(PTRS[r], [SIZES[r]])
                alone = torch.full((N, A), 9.0, device=DEV)
                single.act(obs[r], alone, CAP)
                assert np.array_equal(_bits(got[r]), _bits(alone.cpu().numpy())), (cfg, N, eps, start, r)
                exp, taken = ref.mix(want[r], SEEDS[r], it, warm, eps, lo, hi)
                assert np.array_equal(_bits(got[r]), _bits(exp)), (cfg, N, eps, start, r)
                assert taken.all() if warm else (eps > 0 or not taken.any())
                mixed += int(taken.sum()) if eps == 0.5 else 0
                ws = _words(single)                      # member r's cursor words are the single record's
                w2 = _words(loop)
                assert [w2[r, q] for q in (sl.START, sl.NEXT_PTR, sl.SIZE)] == [ws[q] for q in (sl.START, sl.NEXT_PTR, sl.SIZE)], (cfg, N, r)
            # the rule: what every workgroup read stands as it stood; one thread per member moved its cursor by N, one wrote WARM
            w2 = _words(loop)
            exp_w = w.copy()
            assert gref.act(exp_w, [True] * R, N, CAP, start) == (warm, calls, it)
            assert np.array_equal(w2, exp_w), (cfg, N, eps, w2, exp_w)
            assert (w2[0, sl.CALLS], w2[0, sl.T_GLOBAL], w2[0, sl.ITER], w2[0, sl.WARM]) == (calls, t, it, int(warm))
            for r in range(R):
                assert w2[r, sl.START] == PTRS[r] and w2[r, sl.NEXT_PTR] == (PTRS[r] + N) % CAP and w2[r, sl.SIZE] == min(SIZES[r] + N, CAP)
    assert 0 < mixed < R * sum(NS)              # eps = 0.5 took some rows and left some


# ---- 2. the append form -----------------------------------------------------------------------------------------------------------------------
def test_append_form_equals_add_device_on_a_twin_group_of_rings():
    """rings of 95 rows, N = 40 three times (the third wraps); the first iteration is a warm-up one"""
    from rlrep_amd._lib import lib
    from rlrep_amd.envs import sim_loop as sl
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    _, S, A, _, _ = CONFIGS['sac_pendulum']
    grp = _group('sac_pendulum')
    N, CAP = 40, 95
    bufs, bufs2 = ReplayBufferGroup(R, S, A, max_size=CAP), ReplayBufferGroup(R, S, A, max_size=CAP)
    gen = torch.Generator(device=DEV).manual_seed(3)
    obs = torch.randn(R, N, S, device=DEV, generator=gen)
    loop = sl.SimLoopGroup(grp, _Still(obs), 0.0, N)
    bufs.collect_on_device(loop)
    loop.set_counters(0, 11)
    scratch = torch.zeros(R, N, A, device=DEV)
    for k in range(3):
        s, a, s2 = (torch.randn(R, N, w, device=DEV, generator=gen) for w in (S, A, S))
        r, d = torch.randn(R, N, device=DEV, generator=gen), (torch.rand(R, N, device=DEV, generator=gen) < 0.3).to(torch.float32)
        with pytest.raises(RuntimeError, match='adopt_device_cursor'):
            bufs.add_device(s, a, s2, r, d)             # the loop owns the cursor
        loop.act(obs, scratch, CAP)
        n0 = lib.rlrep_launch_counter()
        loop.append(bufs, s, a, s2, r, d)
        assert lib.rlrep_launch_counter() - n0 == 1
        start2 = bufs2.ptr
        bufs2.add_device(s, a, s2, r, d)
        w = _words(loop)
        assert w[:, sl.START].tolist() == [start2] * R and w[:, sl.NEXT_PTR].tolist() == [bufs2.ptr] * R and w[:, sl.SIZE].tolist() == bufs2.sizes, (k, w)
        assert torch.equal(bufs.rings, bufs2.rings), k
        assert bufs._size_dev.cpu().tolist() == bufs2._size_dev.cpu().tolist() == bufs2.sizes          # published per member
        # the shared words advance ONCE: calls stands still in the warm-up iteration and moves by N otherwise
        assert (w[0, sl.CALLS], w[0, sl.T_GLOBAL], w[0, sl.ITER]) == (11 + N * k, N * (k + 1), k + 1), (k, w)
        assert not w[1:, [sl.CALLS, sl.T_GLOBAL, sl.ITER, sl.WARM]].any()
    assert bufs2.ptr == (3 * N) % CAP and bufs2.sizes == [CAP] * R
    rec = loop.state()
    assert rec['ring_ptr'].tolist() == [bufs2.ptr] * R and rec['ring_size'].tolist() == [CAP] * R and rec['iter'].tolist() == [3] * R
    bufs.adopt_device_cursor()
    assert (bufs.ptr, bufs.sizes) == (bufs2.ptr, bufs2.sizes)


# ---- 3. the simulator -------------------------------------------------------------------------------------------------------------------------
def _assert_planes(gsim, singles, what):
    torch.cuda.synchronize()
    for r, one in enumerate(singles):
        for name in ARRAYS:
            assert _same(getattr(gsim, name)[r], getattr(one, name)), (what, r, name)


@pytest.mark.parametrize('kind', sorted(KIND_ID))
def test_every_plane_of_the_group_simulator_is_the_single_simulator_of_its_seed(kind):
    """N = 300 (two workgroups, the second ragged), simulator seeds (11, 23, 11): reset, a step from the device environments' cases with a
    different action per member, the step that hits the time limit (restart from each member's own stream), MountainCar's goal row"""
    from rlrep_amd.envs.fused_sim import FusedSim, FusedSimGroup
    K, N, sim_seeds = KIND_ID[kind], 300, (11, 23, 11)
    limit = fref.LIMIT[K]
    grp = _group('sac_pendulum' if kind == 'pendulum' else 'sac_mountaincar')
    gsim = FusedSimGroup(K, R, N, DEV, seeds=sim_seeds, group=grp)
    singles = [FusedSim(K, N, DEV, seed=s) for s in sim_seeds]
    first = gsim.reset().clone()
    for one in singles:
        one.reset()
    _assert_planes(gsim, singles, 'reset')
    assert torch.equal(first[0], first[2]) and not torch.equal(first[0], first[1])
    base = CASES[kind]()
    cases = [base[e % len(base)] for e in range(N)]
    if kind == 'mountaincar':
        cases[7] = (F32(0.44), F32(0.05), 1.0, 10)      # one step from the goal: done = 1
    x0, x1, a, t = (np.array(col) for col in zip(*cases))
    for step, tt in enumerate((t.astype(np.int32), np.full(N, limit - 1, np.int32))):
        gsim.set_state(x0, x1, tt)
        acts = torch.from_numpy(np.stack([a * (1.0 - 0.25 * r) for r in range(R)]).astype(np.float32).reshape(R, N, 1)).to(DEV)
        for r, one in enumerate(singles):
            one.set_state(x0, x1, tt)
        nxt, rew, done = gsim.step_(acts)
        for r, one in enumerate(singles):
            n1, r1, d1 = one.step_(acts[r])
            assert _same(nxt[r], n1) and _same(rew[r], r1) and _same(done[r], d1), (kind, step, r)
        _assert_planes(gsim, singles, ('step', step))
        if step == 1:                                   # the limit's step: every environment restarted, members 0 and 2 alike
            assert gsim.episodes.min().item() >= 1 and gsim.t.abs().max().item() == 0 and not done.any()
            alike = gsim.starts[0] == gsim.starts[2]    # (the same index into the same stream: members 0 and 2 share a simulator seed)
            assert alike.sum().item() >= N // 2 and torch.equal(gsim.x0[0][alike], gsim.x0[2][alike]) and not torch.equal(gsim.x0[0], gsim.x0[1])
        elif kind == 'mountaincar':
            assert done[:, 7].tolist() == [1.0] * R and gsim.episodes[:, 7].tolist() == [1] * R
    # N = 1: one thread of one workgroup per member
    g1, o1 = FusedSimGroup(K, R, 1, DEV, seeds=sim_seeds, group=grp), [FusedSim(K, 1, DEV, seed=s) for s in sim_seeds]
    g1.reset()
    a1 = torch.full((R, 1, 1), 0.5, device=DEV)
    g1.step_(a1)
    for r, one in enumerate(o1):
        one.reset()
        one.step_(a1[r])
    _assert_planes(g1, o1, 'N = 1')


def test_without_auto_restart_an_ended_environment_of_a_member_is_frozen():
    from rlrep_amd.envs.fused_sim import FusedSim, FusedSimGroup
    cases = [(F32(0.44), F32(0.05), 1.0, 10), (F32(-0.5), 0.0, 0.5, 998), (F32(-0.5), 0.0, 0.5, 10), (F32(-0.7), F32(0.01), -0.5, 500)]
    N, K, sim_seeds = len(cases), fref.MOUNTAIN_CAR, (4, 5, 6)
    grp = _group('sac_mountaincar')
    gsim = FusedSimGroup(K, R, N, DEV, seeds=sim_seeds, auto_restart=False, group=grp)
    singles = [FusedSim(K, N, DEV, seed=s, auto_restart=False) for s in sim_seeds]
    x0, x1, a, t = (np.array(col) for col in zip(*cases))
    acts = torch.from_numpy(np.broadcast_to(a.astype(np.float32).reshape(1, N, 1), (R, N, 1)).copy()).to(DEV)
    for sim in [gsim] + singles:
        sim.set_state(x0, x1, t.astype(np.int32))
    for k in range(3):
        nxt, rew, done = gsim.step_(acts)
        for r, one in enumerate(singles):
            n1, r1, d1 = one.step_(acts[r])
            assert _same(nxt[r], n1) and _same(rew[r], r1) and _same(done[r], d1), (k, r)
        _assert_planes(gsim, singles, ('frozen', k))
        assert gsim.t[:, :2].tolist() == [[-1, -1]] * R and gsim.t[:, 2].tolist() == [11 + k] * R
        if k:
            assert not rew[:, :2].any() and not done[:, :2].any()
    assert gsim.starts.tolist() == [[0] * N] * R and gsim.episodes.tolist() == [[1, 1, 0, 0]] * R


# ---- 4 / 5. the loop --------------------------------------------------------------------------------------------------------------------------
N_LOOP, RING, EPS = 17, 95, 0.25


def _run(cfg, fused, warm, total, retire=None, preset=None, buffer_kw=None):
    """`total` iterations of the group's iterate_sim (the first `warm` warm-up ones) at N = 17, B = 64 on rings of 95 rows against one
    standalone twin per member run through the single SimLoop + FusedSim + iterate_sim.  retire = (member, first, count): the member leaves
    the launches before iteration `first` for `count` iterations; its twin stops there.  Returns a dict of everything."""
    from rlrep_amd.envs.fused_sim import FusedSim, FusedSimGroup
    from rlrep_amd.envs.sim_loop import SimLoop, SimLoopGroup
    from rlrep_amd.utils.buffer import ReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    _, S, A, kind, _ = CONFIGS[cfg]
    K, N, buffer_kw = KIND_ID[kind], N_LOOP, buffer_kw or {}
    grp = _group(cfg)
    gsim = FusedSimGroup(K, R, N, DEV, seeds=SEEDS, group=grp)
    gsim.reset()
    bufs = ReplayBufferGroup(R, S, A, max_size=RING, **buffer_kw)
    loop = SimLoopGroup(grp, gsim, eps_greedy=EPS, start_timesteps=warm * N, fused_append=fused)
    assert loop.fused_append == fused
    twins, sims, rings, loops = [], [], [], []
    for r, s in enumerate(SEEDS):
        twins.append(_twin(cfg, s))
        sims.append(FusedSim(K, N, DEV, seed=s))
        sims[-1].reset()
        rings.append(ReplayBuffer(S, A, max_size=RING, **buffer_kw))
        loops.append(SimLoop(twins[-1], sims[-1], eps_greedy=EPS, start_timesteps=warm * N, fused_append=fused))
    if preset is not None:
        preset(gsim, sims)
    _assert_planes(gsim, sims, 'start')
    out = dict(grp=grp, gsim=gsim, bufs=bufs, loop=loop, twins=twins, sims=sims, rings=rings, loops=loops, frozen=None, stood=[])

    def member_state(m):
        torch.cuda.synchronize()
        return dict(ring=bufs.rings[m].clone(), size=bufs._size_dev[m].clone(), ctl=loop.ctl[m].clone(), block=sg.member_bytes(grp, m),
                    **{name: getattr(gsim, name)[m].clone() for name in ARRAYS})
    for it in range(total):
        train = it >= warm
        if retire and it == retire[1]:
            grp.retire_members([retire[0]])
            out['frozen'] = member_state(retire[0])
        if retire and it == retire[1] + retire[2]:
            now = member_state(retire[0])
            for key, v in out['frozen'].items():        # the retired member stood still, bit for bit
                assert _same(now[key], v), ('retired', key)
            grp.revive_members([retire[0]])
            out['before_revival'] = _words(loop)
        obs_before = gsim.obs.clone()
        infos = grp.iterate_sim(loop, bufs, B, train=train)
        if not fused:                                   # the copy of the separate route ran inside the graph
            torch.cuda.synchronize()
            live = [r for r in range(R) if grp.live[r]]
            assert torch.equal(loop.obs0[live], obs_before[live])
        for r in range(R):
            if retire and r == retire[0] and it >= retire[1]:        # (its twin stopped where it was retired)
                assert it >= retire[1] + retire[2] or infos is None or infos[r] is None
                continue
            one = twins[r].iterate_sim(loops[r], rings[r], B, train=train)
            if train:
                sg.assert_info_equal({k: float(v) for k, v in infos[r].items()}, {k: float(v) for k, v in one.items()}, (cfg, fused, it, r))
            else:
                assert infos is None and one is None
        if it == warm - 1:
            assert grp._sim_launches == (2 if fused else 3) and grp._sim_captures == 1                 # the warm-up graph: the loop's launches alone
    assert grp._sim_captures == 2                                                                       # exactly one capture per form
    return out


def _assert_member_equals_twin(o, r, what):
    grp, bufs, loop, gsim = o['grp'], o['bufs'], o['loop'], o['gsim']
    torch.cuda.synchronize()
    assert torch.equal(bufs.rings[r], o['rings'][r].ring), (what, r, 'ring')
    assert bufs._size_dev[r].item() == o['rings'][r]._size_dev.item(), (what, r, 'size word')
    rec, one = loop.state()[r], o['loops'][r].state()[0]
    for key in ('ring_ptr', 'ring_size', 'start', 't_global', 'calls', 'iter'):
        assert rec[key] == one[key], (what, r, key, rec, one)
    for name in ARRAYS:
        assert _same(getattr(gsim, name)[r], getattr(o['sims'][r], name)), (what, r, name)
    sg.assert_equal(sg.state(grp._members[r]), sg.state(o['twins'][r].core), (what, r))
    assert grp.steps == o['twins'][r].steps and grp._ctr == o['twins'][r]._ctr


@pytest.mark.parametrize('cfg,fused', [('sac_pendulum', True), ('sac_pendulum', False), ('ctrlsac_f64', True)])
def test_loop_members_equal_their_standalone_twins_bit_for_bit(cfg, fused):
    """4 warm-up and 8 training iterations: the 17-row iterations wrap the rings of 95 rows on the sixth"""
    WARM, TRAIN = 4, 8
    o = _run(cfg, fused, WARM, WARM + TRAIN)
    grp, loop, bufs = o['grp'], o['loop'], o['bufs']
    for r in range(R):
        _assert_member_equals_twin(o, r, (cfg, fused))
    assert loop.counters() == ((WARM + TRAIN) * N_LOOP, grp._ctr, WARM + TRAIN) == (loop.t_global, loop.calls, loop.iter)
    assert loop.state()['ring_ptr'].tolist() == [((WARM + TRAIN) * N_LOOP) % RING] * R and bufs._size_dev.cpu().tolist() == [RING] * R
    assert not torch.equal(bufs.rings[0], bufs.rings[1])
    front = grp._sim_launches
    assert front == o['twins'][0]._sim_launches         # a member's iteration is a standalone agent's, launch for launch
    # the group train()'s own launch count: the cursor goes back to the host and one train() is captured alone
    bufs.adopt_device_cursor()
    grp.train(bufs, B)
    assert front == grp._graph_launches + (2 if fused else 3), (cfg, fused, front, grp._graph_launches)


def test_a_retired_member_stands_still_and_rejoins_at_its_own_cursor():
    """member 1 retired after 6 iterations for 3, revived for one more: no recapture, members 0 and 2 equal their twins throughout"""
    from rlrep_amd.envs import sim_loop as sl
    N = N_LOOP
    o = _run('sac_pendulum', True, 4, 10, retire=(1, 6, 3))
    grp, loop, bufs = o['grp'], o['loop'], o['bufs']
    for r in (0, 2):
        _assert_member_equals_twin(o, r, 'retired run')
    assert grp.live == [True] * R
    w0, w = o['before_revival'], _words(loop)
    assert np.array_equal(w0[1], o['frozen']['ctl'].cpu().numpy())
    # the revived member's iteration wrote N rows at ITS cursor, which lags the others by 3 N mod 95
    assert w[1, sl.START] == w0[1, sl.NEXT_PTR] == (6 * N) % RING and w[1, sl.NEXT_PTR] == (7 * N) % RING
    assert w[0, sl.START] == w[2, sl.START] == (9 * N) % RING and (int(w[0, sl.START]) - int(w[1, sl.START])) % RING == (3 * N) % RING
    assert w[1, sl.SIZE] == min(int(w0[1, sl.SIZE]) + N, RING) == bufs._size_dev[1].item()
    exp = gref.new_record(R, capacity=RING)
    live = [True] * R
    for it in range(10):
        live[1] = not 6 <= it < 9
        gref.iteration(exp, live, N, RING, 4 * N)
    exp[0, gref.CALLS] = w[0, sl.CALLS]                 # (the call counter also counts the captures: compared with the twins above)
    assert np.array_equal(w, exp), (w, exp)
    ring1, old = bufs.rings[1].cpu().numpy(), o['frozen']['ring'].cpu().numpy()
    rows = [(6 * N + e) % RING for e in range(N)]
    others = [q for q in range(RING) if q not in rows]
    assert np.array_equal(ring1[others], old[others]) and not np.array_equal(ring1[rows], old[rows])
    # its rows continue its own rollout: s of the new rows is s' of the rows it wrote last, three iterations ago
    S, A = 3, 1
    last = [(5 * N + e) % RING for e in range(N)]
    assert np.array_equal(ring1[rows][:, :S], old[last][:, S + A:2 * S + A])


def test_mountaincar_members_write_terminal_rows_inside_the_graph():
    """member 2's environments 1 and 9 stand one step from the goal: its ring holds done = 1 rows, written by the replayed graph, and the
    rows that follow start new episodes; the other members' rings hold none"""
    S, A, N = 2, 1, N_LOOP

    def preset(gsim, sims):
        st = sims[2].state()
        x0, x1 = st['x0'].copy(), st['x1'].copy()
        for e in (1, 9):
            x0[e], x1[e] = F32(0.44), F32(0.05)
        sims[2].set_state(x0, x1, 0)
        g = gsim.state()
        gx0, gx1 = g['x0'].copy(), g['x1'].copy()
        gx0[2], gx1[2] = x0, x1
        gsim.set_state(gx0, gx1, 0)
    o = _run('sac_mountaincar', True, 2, 5, preset=preset)
    for r in range(R):
        _assert_member_equals_twin(o, r, 'mountaincar')
    rings = o['bufs'].rings.cpu().numpy()
    done = rings[:, :5 * N, 2 * S + A + 1].reshape(R, 5, N)
    assert done[2, 0].nonzero()[0].tolist() == [1, 9] and not done[0].any() and not done[1].any()
    assert np.all(rings[2, [1, 9], 2 * S + A] > 99.0)
    for e in (1, 9):
        assert not np.array_equal(rings[2, N + e, :S], rings[2, e, S + A:2 * S + A])
    assert np.array_equal(rings[2, N, :S], rings[2, 0, S + A:2 * S + A])
    assert o['gsim'].episodes[2].tolist() == [1 if e in (1, 9) else 0 for e in range(N)] and not o['gsim'].episodes[:2].any()


# ---- 6. refusals and n-step -------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_before_anything_is_launched():
    from rlrep_amd._lib import lib
    from rlrep_amd.envs.fused_sim import FusedSim, FusedSimGroup, SimKind, example_kind
    from rlrep_amd.envs.sim_loop import SimLoop, SimLoopGroup
    from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup, PrioritizedReplayBufferGroup, ReplayBufferGroup
    N = N_LOOP
    grp, other, single = _group('sac_pendulum'), _group('sac_pendulum'), _twin('sac_pendulum', 5)
    gsim = FusedSimGroup('Pendulum-v1', R, N, DEV, seeds=SEEDS)
    with pytest.raises(RuntimeError, match='FusedSimGroup.reset: no seed group yet'):
        gsim.reset()
    loop = SimLoopGroup(grp, gsim, eps_greedy=0.1)
    assert gsim.group is grp
    with pytest.raises(ValueError, match='another group'):
        gsim.bind_group(other)
    gsim.reset()
    kind = SimKind(example_kind('pendulum'))
    cgrp = _group('ctrlsac_f64')
    cloop = SimLoopGroup(cgrp, FusedSimGroup('Pendulum-v1', R, N, DEV, seeds=SEEDS), eps_greedy=0.1)
    lone = FusedSim('Pendulum-v1', N, DEV)
    torch.cuda.synchronize()
    n0 = lib.rlrep_launch_counter()
    with pytest.raises(RuntimeError, match='iterate_sim: PrioritizedReplayBufferGroup'):
        grp.iterate_sim(loop, PrioritizedReplayBufferGroup(R, 3, 1, max_size=RING), B)
    with pytest.raises(RuntimeError, match='iterate_sim: CriticPrioritizedReplayBufferGroup'):
        grp.iterate_sim(loop, CriticPrioritizedReplayBufferGroup(R, 3, 1, max_size=RING), B)
    with pytest.raises(ValueError, match='another group'):
        other.iterate_sim(loop, ReplayBufferGroup(R, 3, 1, max_size=RING), B)
    with pytest.raises(ValueError, match=f'{N} environments for rings of 16 rows'):
        grp.iterate_sim(loop, ReplayBufferGroup(R, 3, 1, max_size=16), B)
    with pytest.raises(ValueError, match=f'ReplayBufferGroup of {R} members'):
        grp.iterate_sim(loop, ReplayBufferGroup(2, 3, 1, max_size=RING), B)
    for dims in ((4, 1), (3, 2)):                       # (the separate route would read the loop's planes with the buffers' strides)
        with pytest.raises(ValueError, match=f'ReplayBufferGroup of {R} members, 3 observations and 1 actions'):
            grp.iterate_sim(loop, ReplayBufferGroup(R, dims[0], dims[1], max_size=RING), B)
    with pytest.raises(ValueError, match='n_stride'):
        grp.iterate_sim(loop, ReplayBufferGroup(R, 3, 1, max_size=RING, n_step=3, n_stride=1), B)
    with pytest.raises(ValueError, match='needs a single agent.*SimLoopGroup'):
        SimLoop(grp, gsim)
    with pytest.raises(ValueError, match='needs a seed group'):
        SimLoopGroup(single, lone)
    with pytest.raises(ValueError, match='FusedSimGroup: a kind compiled at run time'):
        FusedSimGroup(kind, R, N, DEV, seeds=SEEDS, group=grp)
    with pytest.raises(RuntimeError, match=r'CTRLSACSeedBatch.iterate_sim: ReplayBufferGroup\(n_step=3\)'):
        cgrp.iterate_sim(cloop, ReplayBufferGroup(R, 3, 1, max_size=RING, n_step=3, n_stride=N), B)
    # the C entry points, by name: a single agent's handle is not a seed group
    obs, act, ctl = torch.zeros(R, N, 3, device=DEV), torch.zeros(R, N, 1, device=DEV), torch.zeros(R, 8, dtype=torch.int64, device=DEV)
    ring, P = torch.zeros(R, RING, 9, device=DEV), lambda t: t.data_ptr()  # noqa: E731
    import ctypes as C
    h, st, sd = single.core.h, C.byref(gsim._st), P(gsim.seeds_dev)
    for who, call in (
            ('group_act_device_ctl', lambda: lib.rlrep_group_act_device_ctl(h, P(obs), N, -2.0, 2.0, P(act), P(ctl), RING, 0.0, 0, None)),
            ('group_replay_add_cols_ctl', lambda: lib.rlrep_group_replay_add_cols_ctl(h, P(ring), RING, 9, 3, 1, P(obs), 3, P(act), 1, P(obs), 3, P(act), P(act), N,
                                                                                     RING * 9, None, P(ctl), None)),
            ('group_sim_start', lambda: lib.rlrep_group_sim_start(h, st, sd, None)),
            ('group_sim_step', lambda: lib.rlrep_group_sim_step(h, st, sd, P(act), 1, P(gsim.next_obs), P(gsim.reward), P(gsim.done), None)),
            ('group_sim_step_append_ctl', lambda: lib.rlrep_group_sim_step_append_ctl(h, st, sd, P(act), 1, P(ring), RING, 9, RING * 9, None, P(ctl), None))):
        rc = call()
        msg = lib.rlrep_last_error().decode()
        assert rc == -1 and msg.startswith(who + ':') and 'not a seed group' in msg, (who, rc, msg)
    assert lib.rlrep_launch_counter() == n0


def test_nstep_group_buffer_matches_the_standalone_twins():
    """ReplayBufferGroup(n_step=3, n_stride=N): 2 warm-up and 5 training iterations, the wrap inside the sixth"""
    o = _run('sac_pendulum', True, 2, 7, buffer_kw=dict(n_step=3, n_stride=N_LOOP))
    for r in range(R):
        _assert_member_equals_twin(o, r, 'n-step')
    assert o['grp'].steps == 5


# ---- 7. launcher ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env_name', ['Pendulum-v1', 'MountainCarContinuous-v0'])
def test_launcher_runs_the_group_loop_as_one_graph(env_name, tmp_path, monkeypatch):
    import json
    from rlrep_amd import main
    from rlrep_amd.envs import fused_sim
    from test_host_envs import _keep_instances
    sims = _keep_instances(monkeypatch, fused_sim, 'FusedSimGroup')
    argv = ['--alg', 'sac', '--env', env_name, '--seeds', '0,1', '--torch-envs', '8', '--sim-graph', '--fused-sim', '--max_timesteps', '320',
            '--start_timesteps', '160', '--eval_freq', '160', '--batch_size', '64', '--eval_episodes', '2', '--hidden_dim', '64', '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert agent.R == 2 and agent.steps == 20 and agent._sim_captures == 2  # 40 iterations of 8 steps per member, 20 of them warm-up; one capture per form
    assert len(evaluations) == 2 and all(len(e) == 2 and np.all(np.isfinite(e)) for e in evaluations)      # two evaluations, one return per member
    train, ev = sims
    assert (train.members, train.num_envs, train.auto_restart, train.seeds) == (2, 8, True, [0, 1])
    assert (ev.members, ev.num_envs, ev.auto_restart, ev.seeds) == (2, 2, False, [100, 101])
    assert train.t.tolist() == [[40] * 8] * 2 and ev.t.tolist() == [[-1, -1]] * 2 and ev.episodes.tolist() == [[2, 2]] * 2       # (one episode per evaluation)
    assert [e[-1] for e in evaluations] == [float(v) for v in ev.last_return.mean(dim=1).cpu()]
    replay = agent.replay
    assert replay._device_env is not None              # the loop owns the cursor
    replay.adopt_device_cursor()
    assert replay.sizes == [320, 320] and replay.ptr == 0 and replay.size_dev().cpu().tolist() == [320, 320]
    for seed in (0, 1):
        rows = [json.loads(l) for l in open(tmp_path / env_name / 'sac' / '0' / str(seed) / 'metrics.jsonl')]
        assert [row['step'] for row in rows] == [320] and all(np.isfinite(v) for row in rows for v in row.values())
        assert 'info/q_loss' in rows[0] and rows[0]['steps_per_sec'] > 0
