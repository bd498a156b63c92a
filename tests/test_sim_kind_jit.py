"""Simulator kinds compiled at run time (csrc/sim_jit.h, csrc/sim_jit.hip, envs/fused_sim.py SimKind / CustomFusedSim,
main.py --fused-sim-source) on the GPU.

The example Pendulum, compiled at run time, against the built-in FusedSim('Pendulum-v1') from identical states: counters and done exactly;
s' and r within 2 fp32 ulp, the state within 1e-12 relative, restart states within 1e-14 -- the bounds tests/test_fused_sim.py holds the
built-in to against the host environment (the built-in may contract a + b u, the run-time compile does not).  The point mass against its
NumPy twin (same bounds; every operation is IEEE-exact, so 0 ulp is what to expect): the ends of an episode, the freeze, the restarts.  Ring
rows for A = 2 against step + add_device.  The loop: 5 warm-up and 20 training iterations of iterate_sim, bit-identical to a twin on the
eager route.  Kinds as objects; the launcher.  Hidden widths are 64.  Reads nothing outside the repository."""
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
import sim_kind_reference as kref  # noqa: E402
import sim_loop_reference as ref  # noqa: E402
from test_device_env import dynamics_cases, _ulps  # noqa: E402
from test_device_env_single import _agent  # noqa: E402

DEV = 'cuda'
SEED = 5
B = 64
ARRAYS = ('x', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')
_KINDS = {}


def _kind(which):
    """ONE run-time compile per example and test session"""
    from rlrep_amd.envs.fused_sim import SimKind
    if which not in _KINDS:
        _KINDS[which] = SimKind(kref.source(which))
    return _KINDS[which]


def _sim(which, N, seed=11, **kw):
    from rlrep_amd.envs.fused_sim import CustomFusedSim
    return CustomFusedSim(_kind(which), N, DEV, seed=seed, **kw)


def _bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.where(got == want, 0.0, np.abs(got - want) / np.maximum(np.abs(want), 1e-300)), initial=0.0))


# ---- 1. the example Pendulum against the built-in kind ----------------------------------------------------------------------------------------
def _pendulum_pair(N, cases, seed=11):
    from rlrep_amd.envs.fused_sim import FusedSim
    jit, built = _sim('pendulum', N, seed=seed), FusedSim('Pendulum-v1', N, DEV, seed=seed)
    x0, x1, a, t = (np.array(col) for col in zip(*cases))
    jit.set_state(np.stack([x0, x1]), t.astype(np.int32))
    built.set_state(x0, x1, t.astype(np.int32))
    for sim in (jit, built):
        sim.ep_return.fill_(-7.5)
    assert torch.equal(jit.obs, built.obs)
    act = torch.from_numpy(a.astype(np.float32).reshape(-1, 1)).to(DEV)
    out = [tuple(v.cpu().numpy() for v in sim.step_(act)) for sim in (jit, built)]
    return jit.state(), built.state(), out[0], out[1]


def test_jit_pendulum_steps_as_the_built_in_kind_does():
    """N = 300: two workgroups, the second ragged; the dynamics cases of tests/test_fused_sim.py tiled over the environments; then N = 1.
    Measured on an MI355X (docs/history/sim_kind_jit.md): 0 ulp on s' and r, the state bit-identical, restart states within 4.4e-16."""
    base = dynamics_cases()
    N = 300
    assert len(base) <= N
    cases = [base[e % len(base)] for e in range(N)]
    sj, sb, (nj, rj, dj), (nb, rb, db) = _pendulum_pair(N, cases)
    for name in ('t', 'episodes', 'starts'):
        assert np.array_equal(sj[name], sb[name]), name
    assert np.array_equal(dj, db) and not dj.any()
    ulp = int(max(_ulps(nj, nb).max(), _ulps(rj, rb).max()))
    ended = sb['episodes'] == 1
    assert ended.sum() >= 6 and (sj['t'][ended] == 0).all() and (sj['starts'][ended] == 1).all()
    rel = max(_rel(sj['x'][0][~ended], sb['x0'][~ended]), _rel(sj['x'][1][~ended], sb['x1'][~ended]))
    restart = float(max(np.abs(sj['x'][0][ended] - sb['x0'][ended]).max(), np.abs(sj['x'][1][ended] - sb['x1'][ended]).max()))
    obs_ulp = int(_ulps(sj['obs'], sb['obs']).max())
    same = np.array_equal(_bits32(nj), _bits32(nb)) and np.array_equal(_bits32(rj), _bits32(rb)) and np.array_equal(sj['x'][0][~ended], sb['x0'][~ended])
    print(f'jit pendulum vs built-in over {N} environments: worst {ulp} fp32 ulp on (s\', r), {rel:.3e} relative on the state, {restart:.3e} on restart states, '
          f'{obs_ulp} ulp on obs; step bit-identical: {same}')
    assert ulp <= 2 and rel <= 1e-12 and restart <= 1e-14 and obs_ulp <= 2
    assert np.array_equal(sj['ep_return'][ended], np.zeros(int(ended.sum()))) and np.array_equal(sj['last_return'][ended], -7.5 + rj[ended].astype(np.float64))
    assert np.array_equal(sj['ep_return'][~ended], -7.5 + rj[~ended].astype(np.float64)) and np.isnan(sj['last_return'][~ended]).all()
    # N = 1: environment 0 alone gives what it gave among the 300
    s1, b1, (n1, r1, d1), _ = _pendulum_pair(1, cases[:1])
    assert np.array_equal(_bits32(n1[0]), _bits32(nj[0])) and _bits32(r1)[0] == _bits32(rj)[0] and d1[0] == dj[0]
    assert np.array_equal(s1['x'][:, 0], sj['x'][:, 0]) and s1['t'][0] == sj['t'][0]


def test_jit_pendulum_reset_draws_the_built_in_kinds_start_states():
    import fused_sim_reference as fref
    from rlrep_amd.envs.fused_sim import FusedSim
    N, seed = 7, 23
    jit, built = _sim('pendulum', N, seed=seed), FusedSim('Pendulum-v1', N, DEV, seed=seed)
    jit.reset(), built.reset()
    sj, sb = jit.state(), built.state()
    for e in range(N):
        x = fref.start_state(fref.PENDULUM, seed, e, 0)
        assert abs(sj['x'][0][e] - x[0]) <= 1e-14 and abs(sj['x'][1][e] - x[1]) <= 1e-14
        assert _ulps(sj['obs'][e], fref.observe(fref.PENDULUM, *x)).max() <= 2
    assert np.abs(sj['x'][0] - sb['x0']).max() <= 1e-14 and np.abs(sj['x'][1] - sb['x1']).max() <= 1e-14
    assert sj['starts'].tolist() == [1] * N and sj['t'].tolist() == [0] * N and np.isnan(sj['last_return']).all() and sj['episodes'].tolist() == [0] * N


# ---- 2. the point mass against its NumPy twin -------------------------------------------------------------------------------------------------
def _check_against_the_twin(N, x, a, t, seed=11, auto_restart=True):
    from rlrep_amd.envs import point_mass as pm
    sim = _sim('point_mass', N, seed=seed, auto_restart=auto_restart)
    sim.set_state(x, t)
    sim.ep_return.fill_(-2.5)
    assert np.array_equal(sim.obs.cpu().numpy(), pm.observe(np.broadcast_to(np.asarray(x, np.float64).reshape(4, -1), (4, N))))
    nxt, rew, done = (v.cpu().numpy() for v in sim.step_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)))
    st = sim.state()
    want = pm.step_sim(np.broadcast_to(np.asarray(x, np.float64).reshape(4, -1), (4, N)), np.broadcast_to(t, (N,)), a, auto_restart=auto_restart)
    ulp = int(max(_ulps(nxt, want['next_obs']).max(), _ulps(rew, want['reward']).max()))
    assert ulp <= 2, ulp
    assert np.array_equal(done, want['done']) and np.array_equal(st['t'], want['t'])
    ended = want['ended']
    assert np.array_equal(st['episodes'], ended.astype(np.int64))
    go_on = ~ended if auto_restart else np.ones(N, bool)
    rel = _rel(st['x'][:, go_on], want['x'][:, go_on])
    assert rel <= 1e-12, rel
    assert np.array_equal(st['ep_return'][go_on], -2.5 + rew[go_on].astype(np.float64))
    assert np.array_equal(st['last_return'][ended], -2.5 + rew[ended].astype(np.float64)) and np.isnan(st['last_return'][~ended]).all()
    worst_start = 0.0
    if auto_restart:
        assert np.array_equal(st['starts'], ended.astype(np.int64)) and (st['ep_return'][ended] == 0.0).all()
        for e in np.nonzero(ended)[0]:
            xs = pm.start_state(seed, int(e), 0)
            worst_start = max(worst_start, float(np.abs(st['x'][:, e] - xs).max()))
            assert np.array_equal(st['obs'][e], pm.observe(st['x'][:, e:e + 1])[0]) and not np.array_equal(st['obs'][e], nxt[e])
        assert worst_start <= 1e-14, worst_start
        assert np.array_equal(_bits32(st['obs'][go_on]), _bits32(nxt[go_on]))
    else:
        assert (st['starts'] == 0).all() and np.array_equal(_bits32(st['obs']), _bits32(nxt))
    return ulp, rel, worst_start, (nxt, rew, done, st)


def test_point_mass_steps_as_its_numpy_twin_does():
    """N = 300 random cases (walls, speed clamps, the force clip, around the goal radius, the limit's step), then N = 1.
    Measured on an MI355X (docs/history/sim_kind_jit.md): 0 ulp, 0 relative, restart states equal."""
    N = 300
    x, a, t = kref.point_mass_cases(N)
    ulp, rel, ws, (nxt, rew, done, st) = _check_against_the_twin(N, x, a, t)
    assert done.sum() >= 5 and (st['episodes'] == 1).sum() >= 40
    print(f'point mass vs the NumPy twin over {N} environments: worst {ulp} fp32 ulp on (s\', r), {rel:.3e} relative on the state, {ws:.3e} on restart states')
    u1, r1, w1, (n1, rw1, d1, s1) = _check_against_the_twin(1, x[:, :1], a[:1], t[:1])
    assert np.array_equal(_bits32(n1[0]), _bits32(nxt[0])) and _bits32(rw1)[0] == _bits32(rew)[0] and d1[0] == done[0] and s1['t'][0] == st['t'][0]


@pytest.mark.parametrize('N', [300, 1])
def test_point_mass_episode_ends(N):
    """the goal before the limit (done = 1); the goal on the limit's step (done = 0); the limit without the goal; neither; each forced with
    set_state, tiled over the environments; the restart is the restated start state"""
    cases = [kref.FORCED[e % len(kref.FORCED)] for e in range(N)]
    x = np.array([c[0] for c in cases]).T
    a = np.array([c[1] for c in cases], np.float32)
    t = np.array([c[2] for c in cases], np.int32)
    _, _, _, (nxt, rew, done, st) = _check_against_the_twin(N, x, a, t, seed=23)
    assert done.tolist() == [c[3] for c in cases] and st['episodes'].tolist() == [int(c[4]) for c in cases]
    assert st['t'].tolist() == [0 if c[4] else c[2] + 1 for c in cases]
    assert rew[0] == np.float32(-0.05 + 10.0)
    if N > 1:
        px, py = 1.0 + (0.0 + 0.5 * 0.1) * 0.1, 1.0 + (0.0 + -0.5 * 0.1) * 0.1
        assert rew[1] == rew[0] and rew[2] == rew[3] == np.float32((-np.sqrt(px * px + py * py) - 0.01 * (0.25 + 0.25)) + 0.0)


def test_point_mass_without_auto_restart_an_ended_environment_is_frozen():
    cases = kref.FORCED[:4]
    N = len(cases)
    x = np.array([c[0] for c in cases]).T
    a = np.array([c[1] for c in cases], np.float32)
    t = np.array([c[2] for c in cases], np.int32)
    _, _, _, (nxt, rew, done, st) = _check_against_the_twin(N, x, a, t, auto_restart=False)
    assert st['t'].tolist() == [-1, -1, -1, 11] and done.tolist() == [1.0, 0.0, 0.0, 0.0]
    sim = _sim('point_mass', N, auto_restart=False)
    sim.set_state(x, t)
    act = torch.from_numpy(a).to(DEV)
    sim.step_(act)
    st = sim.state()
    for k in range(3):
        n2, r2, d2 = (v.cpu().numpy() for v in sim.step_(act))
        now = sim.state()
        for e in (0, 1, 2):
            assert np.array_equal(n2[e], st['obs'][e]) and r2[e] == 0.0 and d2[e] == 0.0
            for name in ARRAYS:
                got, was = (now[name][:, e], st[name][:, e]) if name == 'x' else (now[name][e], st[name][e])
                assert np.array_equal(got, was, equal_nan=True), (k, e, name)
        assert now['t'][3] == 12 + k and now['ep_return'][3] < st['ep_return'][3]
    sim.reset()                                         # a reset thaws it
    assert sim.t.tolist() == [0] * N and sim.starts.tolist() == [1] * N and sim.episodes.tolist() == [1, 1, 1, 0]


def test_equal_seeds_restart_alike_over_three_restarts_and_another_seed_differs():
    from rlrep_amd.envs import point_mass as pm
    N = 6
    a, b, c = _sim('point_mass', N, seed=3), _sim('point_mass', N, seed=3), _sim('point_mass', N, seed=4)
    act = torch.zeros(N, 2, device=DEV)
    for sim in (a, b, c):
        sim.reset()
    seen = []
    for k in range(3):
        for sim in (a, b, c):
            sim.t.fill_(99)
            sim.step_(act)
        for name in ARRAYS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        assert not torch.equal(a.x, c.x) and not torch.equal(a.obs, c.obs)
        seen.append(a.x.clone())
        x = a.x.cpu().numpy()
        for e in range(N):
            assert np.abs(x[:, e] - pm.start_state(3, e, k + 1)).max() <= 1e-14
    assert a.starts.tolist() == [4] * N and a.episodes.tolist() == [3] * N
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- 3. ring rows for A = 2 -------------------------------------------------------------------------------------------------------------------
def test_step_append_packs_the_rows_step_and_add_device_leave():
    """N = 40 into a ring of 95 rows, three times: the third wraps inside the step.  The loop record is written as the act launch leaves it
    (START, NEXT, SIZE, WARM); the second iteration is a warm-up one (CALLS stays)."""
    from rlrep_amd.utils.buffer import ReplayBuffer
    N, RING, S, A = 40, 95, 4, 2
    sim, twin = _sim('point_mass', N), _sim('point_mass', N)
    buf, buf2 = ReplayBuffer(S, A, max_size=RING), ReplayBuffer(S, A, max_size=RING)
    x, a, t = kref.point_mass_cases(N, seed=3)
    for s in (sim, twin):
        s.set_state(x, t)
    ctl = torch.zeros(8, dtype=torch.int64, device=DEV)
    g = np.random.RandomState(4)
    calls = t_global = 0
    for it in range(3):
        act = torch.from_numpy(g.uniform(-1.5, 1.5, (N, A)).astype(np.float32)).to(DEV)
        warm = it == 1
        words = [calls, t_global, it, ((it + 1) * N) % RING, (it * N) % RING, min((it + 1) * N, RING), int(warm), 0]
        ctl.copy_(torch.tensor(words, dtype=torch.int64))
        obs0 = twin.obs.clone()
        sim.step_append_(act, buf, ctl)
        nxt, rew, done = twin.step_(act)
        buf2.add_device(obs0, act, nxt, rew, done)
        calls, t_global = calls + (0 if warm else N), t_global + N
        torch.cuda.synchronize()
        assert torch.equal(buf.ring, buf2.ring), it
        assert buf._size_dev.cpu().tolist() == buf2._size_dev.cpu().tolist() == [min((it + 1) * N, RING)]
        assert ctl.cpu().tolist() == [calls, t_global, it + 1] + words[3:], it
        for name in ARRAYS:
            p, q = getattr(sim, name), getattr(twin, name)
            assert torch.equal(p, q) or (name == 'last_return' and np.array_equal(p.cpu().numpy(), q.cpu().numpy(), equal_nan=True)), (it, name)
    rows = buf.ring.cpu().numpy()
    assert np.array_equal(rows[(2 * N + N - 1) % RING, S:S + A], act[N - 1].cpu().numpy()) and (2 * N + N - 1) % RING < N      # the wrap
    with pytest.raises(ValueError, match='4 observations and 2 actions'):
        sim.step_append_(act, ReplayBuffer(3, 1, max_size=RING), ctl)


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------------------
def _loop_against_the_eager_route(which, make, preset):
    """tests/test_fused_sim.py's loop comparison on a CustomFusedSim with its step_append_ hook: 5 warm-up and 20 training iterations of
    iterate_sim, N = 16, B = 64, a ring of 95 rows, eps_greedy 0.25, against a twin: act_device -> the restated mix -> step_ of a second
    simulator -> add_device -> train()"""
    from rlrep_amd.envs.sim_loop import SimLoop
    from rlrep_amd.utils.buffer import ReplayBuffer
    N, WARM, TRAIN, EPS, RING = 16, 5, 20, 0.25, 95
    agent, twin = make(), make(pipeline=False)
    S, A = agent.state_dim, agent.action_dim
    lo, hi = agent.action_range
    sims = []
    for _ in range(2):
        sim = _sim(which, N)
        sim.reset()
        preset(sim)
        sims.append(sim)
    sim, sim2 = sims
    assert torch.equal(sim.obs, sim2.obs) and (sim.state_dim, sim.action_dim) == (S, A)
    buf, buf2 = ReplayBuffer(S, A, max_size=RING), ReplayBuffer(S, A, max_size=RING)
    loop = SimLoop(agent, sim, eps_greedy=EPS, start_timesteps=WARM * N)
    assert loop.fused_append
    infos, early = [], None
    for it in range(WARM + TRAIN):
        out = agent.iterate_sim(loop, buf, B, train=it >= WARM)
        if it == 2:
            early = buf.ring.clone()
        if it < WARM:
            assert out is None
        else:
            infos.append({k: float(v) for k, v in out.items()})
        if it == WARM - 1:
            assert agent._sim_launches == 2 and agent._sim_captures == 1      # the warm-up graph: the act launch and the step-and-append launch
    assert agent._sim_captures == 2                                           # one capture per form
    mixed = 0
    for it in range(WARM + TRAIN):
        warm = it < WARM
        if it == WARM:
            twin.prepare(buf2, B)
        obs0 = sim2.obs.clone()
        pol = np.zeros((N, A), np.float32) if warm else twin.act_device(obs0, explore=True).cpu().numpy()
        acts, taken = ref.mix(pol, SEED, it, warm, EPS, lo, hi)
        mixed += 0 if warm else int(taken.sum())
        a = torch.from_numpy(acts).to(DEV)
        nxt, rew, done = sim2.step_(a)
        buf2.add_device(obs0, a, nxt, rew, done)
        if it == 2:
            assert torch.equal(early, buf2.ring)
        if not warm:
            sg.assert_info_equal(infos[it - WARM], {k: float(v) for k, v in twin.train(buf2, B).items()}, (which, it))
    assert 0 < mixed < TRAIN * N
    torch.cuda.synchronize()
    assert torch.equal(buf.ring, buf2.ring)
    assert buf._size_dev.cpu().tolist() == buf2._size_dev.cpu().tolist() == [RING]
    sg.assert_equal(sg.state(agent.core), sg.state(twin.core), which)
    assert agent.steps == twin.steps == TRAIN and agent._ctr == twin._ctr
    assert loop.counters() == ((WARM + TRAIN) * N, agent._ctr, WARM + TRAIN) == (loop.t_global, loop.calls, loop.iter)
    assert int(loop.state()['ring_ptr'][0]) == ((WARM + TRAIN) * N) % RING == buf2.ptr
    for name in ARRAYS:
        p, q = getattr(sim, name), getattr(sim2, name)
        assert torch.equal(p, q) or (name == 'last_return' and np.array_equal(p.cpu().numpy(), q.cpu().numpy(), equal_nan=True)), name
    assert agent._sim_launches == twin._graph_launches + 2, (which, agent._sim_launches, twin._graph_launches)
    return agent, loop, early, sim


def test_point_mass_loop_equals_the_eager_route_bit_for_bit():
    """sac, S = 4, A = 2.  Environments 1 and 9 stand inside the goal radius' reach (the first step ends them with done = 1), environment 6
    on the step before the time limit, and t = 88 elsewhere puts every other restart in the 12th iteration, inside the replayed training graph"""
    N, S, A = 16, 4, 2

    def preset(sim):
        st = sim.state()
        x, t = st['x'].copy(), np.full(N, 88, np.int32)
        for e in (1, 9):
            x[:, e] = (0.02, -0.03, 0.0, 0.0)
        t[6] = 98
        sim.set_state(x, t)
    agent, loop, early, sim = _loop_against_the_eager_route(
        'point_mass', lambda **kw: _agent('sac', S=S, A=A, space=bench.Space(A), seed=SEED, hidden_dim=64, **kw), preset)
    ring = early.cpu().numpy()                          # rows of iterations 0, 1, 2: row i * N + e
    done = ring[:3 * N, 2 * S + A + 1].reshape(3, N)
    assert done[0].nonzero()[0].tolist() == [1, 9] and done[1][6] == 0.0   # the goal twice; the time limit (done = 0)
    assert np.all(ring[[1, 9], 2 * S + A] > 9.0)                           # the bonus
    for i, e in ((0, 1), (0, 9), (1, 6)):               # the row that follows an end starts a new episode: speed 0, another position
        row, nxt = ring[i * N + e], ring[(i + 1) * N + e]
        assert not np.array_equal(nxt[:S], row[S + A:2 * S + A]) and nxt[2] == nxt[3] == 0.0, (i, e, row, nxt)
    assert np.array_equal(ring[N + 0][:S], ring[0][S + A:2 * S + A])       # elsewhere the rollout continues
    assert (sim.episodes >= 1).all() and int(sim.starts.min()) >= 2
    assert not bool(torch.isnan(sim.last_return).any())


def test_vlsac_loop_on_the_jit_pendulum_equals_the_eager_route_bit_for_bit():
    """vlsac, F = 64, on the example Pendulum compiled at run time; t is preset to 187: every environment restarts in the 13th iteration"""
    from test_sim_loop import _make
    agent, loop, buf, sim = _loop_against_the_eager_route('pendulum', lambda **kw: _make('vlsac_f64', **kw)[0], lambda s: s.t.fill_(187))
    assert sim.episodes.tolist() == [1] * 16 and sim.t.tolist() == [12] * 16 and sim.starts.tolist() == [2] * 16


# ---- 5. kinds as objects ----------------------------------------------------------------------------------------------------------------------
def test_two_kinds_live_at_once_and_are_destroyed_in_either_order():
    from rlrep_amd.envs.fused_sim import CustomFusedSim, SimKind
    for order in ((0, 1), (1, 0)):
        kinds = [SimKind(kref.source('pendulum')), SimKind(kref.source('point_mass'))]
        sims = [CustomFusedSim(kinds[0], 5, DEV, seed=1), CustomFusedSim(kinds[1], 5, DEV, seed=1)]
        for sim in sims:
            sim.reset()
            sim.step_(torch.zeros(5, sim.action_dim, device=DEV))
        torch.cuda.synchronize()
        assert sims[0].t.tolist() == sims[1].t.tolist() == [1] * 5 and (sims[0].state_dim, sims[1].state_dim) == (3, 4)
        kinds[order[0]].destroy()
        live = sims[order[1]]
        live.step_(torch.zeros(5, live.action_dim, device=DEV))
        torch.cuda.synchronize()
        assert live.t.tolist() == [2] * 5
        kinds[order[1]].destroy()
        kinds[order[1]].destroy()                                           # twice is once


def test_a_syntax_error_raises_with_the_users_identifier_and_other_constants_are_refused():
    from rlrep_amd.envs.fused_sim import CustomFusedSim, SimKind
    text = kref.source('point_mass')
    with pytest.raises(RuntimeError, match='my_own_missing_term') as e:
        CustomFusedSim(text.replace('const double d = sqrt', 'const double d = my_own_missing_term + sqrt'), 4, DEV)
    assert 'sim_kind_compile' in str(e.value)
    with pytest.raises(RuntimeError, match="the struct's S differs from the description"):
        SimKind(text, S=5)
    with pytest.raises(RuntimeError, match="the struct's LIMIT differs from the description"):
        CustomFusedSim(text, 4, DEV, limit=50)
    with pytest.raises(ValueError, match='num_envs'):
        CustomFusedSim(text, 0, DEV)


def test_kernel_info_reports_no_scratch_for_the_examples():
    for which in ('pendulum', 'point_mass'):
        info = _sim(which, 4).kernel_info()
        print(which, info)
        assert sorted(info) == ['start', 'step', 'step_append_ctl']
        for k, v in info.items():
            assert v['scratch_bytes'] == 0 and v['lds_bytes'] == 0 and 0 < v['regs'] <= 128, (which, k, v)


# ---- 6. launcher ------------------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_a_kind_of_its_own(tmp_path, monkeypatch):
    import json
    from rlrep_amd import main
    from rlrep_amd.envs import fused_sim
    from rlrep_amd.utils import buffer
    from test_host_envs import _keep_instances
    made = _keep_instances(monkeypatch, buffer, 'ReplayBuffer')
    sims = _keep_instances(monkeypatch, fused_sim, 'CustomFusedSim')
    argv = ['--alg', 'sac', '--env', 'PointMass', '--fused-sim-source', os.path.join(fused_sim.KINDS_DIR, 'point_mass.h'), '--torch-envs', '8', '--sim-graph',
            '--fused-sim', '--max_timesteps', '320', '--start_timesteps', '160', '--eval_freq', '320', '--batch_size', '64', '--eval_episodes', '2',
            '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert (agent.state_dim, agent.action_dim) == (4, 2)
    assert agent.steps == 20 and agent._sim_captures == 2                   # 40 iterations of 8 steps, 20 of them warm-up; one capture per form
    assert len(made) == 1 and (made[0].state_dim, made[0].action_dim) == (4, 2)
    made[0].adopt_device_cursor()
    assert made[0].size == 320 and made[0].ptr == 0
    train, ev = sims
    assert train.kind is ev.kind                                            # ONE compile
    assert (train.num_envs, train.auto_restart, train.seed) == (8, True, 0) and (ev.num_envs, ev.auto_restart, ev.seed) == (2, False, 100)
    assert int(train.starts.min()) >= 1 and ev.t.tolist() == [-1, -1] and ev.starts.tolist() == [1, 1] and ev.episodes.tolist() == [1, 1]
    assert len(evaluations) == 1 and np.isfinite(evaluations[0]) and evaluations[0] == float(ev.last_return.mean())
    rows = [json.loads(l) for l in open(tmp_path / 'PointMass' / 'sac' / '0' / '0' / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [320] and all(np.isfinite(v) for row in rows for v in row.values())
