"""The fused simulators (DESIGN.md 6i "Fused simulators"; csrc/sim_step.hip, envs/fused_sim.py FusedSim, SimLoop's step_append_ route,
main.py --fused-sim) on the GPU.

One step against the host environments (the bound tests/test_device_env.py derives: both sides compute in fp64 and round to fp32 once, plus
one last-bit difference of the two libms -- 2 fp32 ulp on s' and r, 1e-12 relative on the state words) and against the device environments'
kernels (the same Env::dynamics on the same device: bit for bit); episode ends, restarts from the restated start states, the freeze of
auto_restart=False; 5 warm-up and 20 training iterations of iterate_sim, in the separate and in the fused-append form, bit-identical to a twin
that runs the eager route; the launcher.  Hidden widths are 64 in the loop tests.  Reads nothing outside the repository."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fused_sim_reference as fref  # noqa: E402
import seed_group_util as sg  # noqa: E402
import sim_loop_reference as ref  # noqa: E402
from test_device_env import dynamics_cases, _ulps  # noqa: E402
from test_device_env_mountaincar import mountaincar_dynamics_cases  # noqa: E402
from test_device_env_single import _agent, _env  # noqa: E402
from test_sim_loop import _make  # noqa: E402

DEV = 'cuda'
SEED = 5
B = 64
KINDS = {'pendulum': fref.PENDULUM, 'mountaincar': fref.MOUNTAIN_CAR}
CASES = {'pendulum': dynamics_cases, 'mountaincar': mountaincar_dynamics_cases}
ARRAYS = ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')
F32 = lambda x: float(np.float32(x))  # noqa: E731


def _sim(kind, N, seed=11, **kw):
    from rlrep_amd.envs.fused_sim import FusedSim
    return FusedSim(KINDS[kind], N, DEV, seed=seed, **kw)


def _put(sim, cases, ep_return=-7.5):
    """environment e stands at case e's state and step; returns the [N, 1] actions of the cases"""
    x0, x1, a, t = (np.array(col) for col in zip(*cases))
    sim.set_state(x0, x1, t.astype(np.int32))
    sim.ep_return.fill_(ep_return)
    return torch.from_numpy(a.astype(np.float32).reshape(-1, 1)).to(DEV)


def _bits32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _is_start(kind, x0, x1):
    if kind == 'pendulum':
        return abs(x0) <= np.pi and abs(x1) <= 1.0
    return F32(-0.6) <= x0 <= F32(-0.4) and x1 == 0.0 and x0 == F32(x0)


# ---- 1. dynamics ------------------------------------------------------------------------------------------------------------------------------
def _device_kernel_step(kind, cases):
    """the device environments' own kernel (DevicePendulum / DeviceMountainCar, 64 environments per launch) from the same states with
    forced actions -> (s' [n, S], r [n], done [n], x0' [n], x1' [n])"""
    from rlrep_amd.utils.buffer import ReplayBuffer
    S = fref.S[KINDS[kind]]
    E = 64
    agent = _agent('sac', kind, hidden_dim=64)
    env, buf = _env(agent, kind, num_envs=E), ReplayBuffer(S, 1, max_size=E)
    out = []
    for k0 in range(0, len(cases), E):
        chunk = cases[k0:k0 + E]
        chunk = chunk + [chunk[-1]] * (E - len(chunk))
        rec = env.state()
        for e, (x0, x1, a, t) in enumerate(chunk):
            rec['theta'][0, e], rec['theta_dot'][0, e], rec['t'][0, e] = x0, x1, t
            rec['obs'][0, e][:S] = fref.observe(KINDS[kind], x0, x1)
            rec['force'][0, e], rec['force_action'][0, e] = 1, a
            rec['ring_ptr'][0, e], rec['episode_return'][0, e] = e, -7.5
        env.set_state(rec)
        env.step(buf, 0.0, 0)
        rows, new = buf.ring[:E].cpu().numpy(), env.state()
        out.append((rows[:, S + 1:2 * S + 1], rows[:, 2 * S + 1], rows[:, 2 * S + 2], new['theta'][0].copy(), new['theta_dot'][0].copy()))
    return [np.concatenate(col)[:len(cases)] for col in zip(*out)]


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_one_step_matches_the_host_environment_and_the_device_kernels(kind):
    """N = 300: two workgroups, the second ragged; the cases of the device environments' tests tiled over the environments.  Against the host
    environment at most 2 fp32 ulp on s' and r (done exactly) and 1e-12 relative on the state words; against group_env.hip's kernels every
    bit.  Then N = 1."""
    N, K = 300, KINDS[kind]
    base = CASES[kind]()
    assert len(base) <= N
    cases = [base[e % len(base)] for e in range(N)]
    sim = _sim(kind, N)
    act = _put(sim, cases)
    obs0 = sim.obs.clone()
    nxt, rew, done = (v.cpu().numpy() for v in sim.step_(act))
    st = sim.state()
    worst_ulp, worst_rel, ended = 0, 0.0, 0
    for e, (x0, x1, a, t) in enumerate(cases):
        want = fref.host_step(K, x0, x1, a, t)
        d = int(max(_ulps(nxt[e], want['obs']).max(), _ulps(rew[e:e + 1], np.array([want['reward']])).max()))
        worst_ulp = max(worst_ulp, d)
        assert d <= 2, (e, cases[e], nxt[e], rew[e], want)
        assert done[e] == want['done_bool'], (e, cases[e], done[e], want)
        if want['ended']:
            ended += 1
            assert st['t'][e] == 0 and st['episodes'][e] == 1 and st['ep_return'][e] == 0.0 and st['starts'][e] == 1
            assert st['last_return'][e] == -7.5 + float(rew[e])
            assert _is_start(kind, st['x0'][e], st['x1'][e]) and not np.array_equal(st['obs'][e], nxt[e])
        else:
            got, exp = (st['x0'][e], st['x1'][e]), want['state']
            rel = 0.0 if got == exp else max(abs(g - w) / max(abs(w), 1e-300) for g, w in zip(got, exp))
            worst_rel = max(worst_rel, rel)
            assert rel <= 1e-12, (e, cases[e], got, exp)
            assert st['t'][e] == t + 1 and st['episodes'][e] == 0 and st['starts'][e] == 0 and np.isnan(st['last_return'][e])
            assert st['ep_return'][e] == -7.5 + float(rew[e]) and np.array_equal(_bits32(st['obs'][e]), _bits32(nxt[e]))
    assert ended >= 6
    print(f'{kind}: fused step vs the host environment over {N} environments: worst {worst_ulp} fp32 ulp on (s\', r), worst {worst_rel:.3e} relative on the state')
    # the device environments' kernels: the same Env::dynamics on the same device
    k_nxt, k_rew, k_done, k_x0, k_x1 = _device_kernel_step(kind, cases)
    ulp = int(max(_ulps(nxt, k_nxt).max(), _ulps(rew, k_rew).max()))
    print(f'{kind}: fused step vs the device environments\' kernels: worst {ulp} fp32 ulp on (s\', r)')
    assert np.array_equal(_bits32(nxt), _bits32(k_nxt)) and np.array_equal(_bits32(rew), _bits32(k_rew)) and np.array_equal(done, k_done)
    go_on = np.array([not fref.host_step(K, *c)['ended'] for c in cases])          # (an ended record restarts from its own stream)
    assert np.array_equal(_bits64(st['x0'][go_on]), _bits64(k_x0[go_on])) and np.array_equal(_bits64(st['x1'][go_on]), _bits64(k_x1[go_on]))
    # N = 1: environment 0 alone gives what it gave among the 300
    one = _sim(kind, 1)
    a1 = _put(one, cases[:1])
    n1, r1, d1 = (v.cpu().numpy() for v in one.step_(a1))
    assert np.array_equal(_bits32(n1[0]), _bits32(nxt[0])) and _bits32(r1)[0] == _bits32(rew)[0] and d1[0] == done[0]
    s1 = one.state()
    assert s1['x0'][0] == st['x0'][0] and s1['x1'][0] == st['x1'][0] and s1['t'][0] == st['t'][0]
    assert torch.equal(obs0, torch.from_numpy(np.stack([fref.observe(K, c[0], c[1]) for c in cases])).to(DEV))


# ---- 2. episode ends --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_the_limits_step_files_the_return_and_restarts_from_the_restated_start_state(kind):
    K, N, seed = KINDS[kind], 7, 23
    limit = fref.LIMIT[K]
    sim = _sim(kind, N, seed=seed)
    first = sim.reset().clone()
    st = sim.state()
    for e in range(N):                                  # reset: start state 0 of every environment
        x = fref.start_state(K, seed, e, 0)
        assert abs(st['x0'][e] - x[0]) <= (1e-14 if kind == 'pendulum' else 0.0) and abs(st['x1'][e] - x[1]) <= (1e-14 if kind == 'pendulum' else 0.0)
        assert _ulps(st['obs'][e], fref.observe(K, *x)).max() <= 2
    assert st['starts'].tolist() == [1] * N and st['t'].tolist() == [0] * N and np.isnan(st['last_return']).all() and st['episodes'].tolist() == [0] * N
    ks = np.array([1, 2, 3, 5, 8, 13, 40], np.int64)
    sim.starts.copy_(torch.from_numpy(ks))
    base = CASES[kind]()[:N]
    act = _put(sim, [(x0, x1, a, limit - 1) for x0, x1, a, _ in base], ep_return=-3.25)
    nxt, rew, done = (v.cpu().numpy() for v in sim.step_(act))
    st = sim.state()
    assert not done.any()                               # an end by the time limit is not a terminal state
    for e in range(N):
        assert st['last_return'][e] == -3.25 + float(rew[e]) and st['episodes'][e] == 1 and st['t'][e] == 0 and st['ep_return'][e] == 0.0
        assert st['starts'][e] == ks[e] + 1
        x = fref.start_state(K, seed, e, int(ks[e]))
        if kind == 'pendulum':                          # (the device may contract a + b u into one fma: one fp64 rounding of a value below 2 pi)
            assert abs(st['x0'][e] - x[0]) <= 1e-14 and abs(st['x1'][e] - x[1]) <= 1e-14, (e, st['x0'][e], st['x1'][e], x)
        else:
            assert (st['x0'][e], st['x1'][e]) == x, (e, st['x0'][e], st['x1'][e], x)
        assert _ulps(st['obs'][e], fref.observe(K, *x)).max() <= 2 and not np.array_equal(st['obs'][e], nxt[e])
    assert not torch.equal(first, sim.obs)


def test_mountaincar_goal_is_terminal_before_the_limit_only():
    K, limit = fref.MOUNTAIN_CAR, 999
    near = (F32(0.44), F32(0.05), 1.0)
    cases = [near + (10,), near + (limit - 1,), (F32(-0.5), 0.0, 0.5, limit - 1), (F32(-0.5), 0.0, 0.5, 10), near[:2] + (3.0, 10)]
    sim = _sim('mountaincar', len(cases))
    act = _put(sim, cases, ep_return=0.0)
    nxt, rew, done = (v.cpu().numpy() for v in sim.step_(act))
    st = sim.state()
    assert done.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]                       # the goal; the goal on the limit's step; the time limit; neither; the goal
    assert rew[0] == np.float32(100.0 - 0.1 * 1.0) and rew[1] == rew[0] and rew[4] == np.float32(100.0 - 0.1 * 9.0)     # (the RAW action's square)
    assert rew[2] == rew[3] == np.float32(-0.1 * 0.25)
    assert st['episodes'].tolist() == [1, 1, 1, 0, 1] and st['t'].tolist() == [0, 0, 0, 11, 0] and st['starts'].tolist() == [1, 1, 1, 0, 1]
    for e in (0, 1, 2, 4):
        assert st['last_return'][e] == float(rew[e]) and _is_start('mountaincar', st['x0'][e], st['x1'][e])
        assert (st['x0'][e], st['x1'][e]) == fref.start_state(K, 11, e, 0)
    assert np.isnan(st['last_return'][3]) and st['ep_return'][3] == float(rew[3])


def test_equal_seeds_restart_alike_and_another_seed_differs():
    N = 6
    a, b, c = _sim('pendulum', N, seed=3), _sim('pendulum', N, seed=3), _sim('pendulum', N, seed=4)
    act = torch.zeros(N, 1, device=DEV)
    for sim in (a, b, c):
        sim.reset()
    seen = []
    for k in range(3):
        for sim in (a, b, c):
            sim.t.fill_(199)
            sim.step_(act)
        for name in ARRAYS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        assert not torch.equal(a.x0, c.x0) and not torch.equal(a.obs, c.obs)
        seen.append(a.x0.clone())
    assert a.starts.tolist() == [4] * N and a.episodes.tolist() == [3] * N
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- 3. auto_restart=False --------------------------------------------------------------------------------------------------------------------
def test_without_auto_restart_an_ended_environment_is_frozen():
    limit = 999
    cases = [(F32(0.44), F32(0.05), 1.0, 10), (F32(-0.5), 0.0, 0.5, limit - 1), (F32(-0.5), 0.0, 0.5, 10), (F32(-0.7), F32(0.01), -0.5, 500)]
    N = len(cases)
    sim = _sim('mountaincar', N, auto_restart=False)
    act = _put(sim, cases, ep_return=-1.0)
    nxt, rew, done = (v.clone() for v in sim.step_(act))
    st = sim.state()
    assert st['t'].tolist() == [-1, -1, 11, 501] and st['episodes'].tolist() == [1, 1, 0, 0] and st['starts'].tolist() == [0] * N
    assert done.tolist() == [1.0, 0.0, 0.0, 0.0]
    for e in (0, 1):                                    # ended where it stood: the last step's state, observation and return
        assert st['last_return'][e] == st['ep_return'][e] == -1.0 + float(rew[e])
        assert np.array_equal(st['obs'][e], nxt[e].cpu().numpy()) and (F32(st['x0'][e]), F32(st['x1'][e])) == tuple(float(v) for v in st['obs'][e])
    for k in range(3):
        n2, r2, d2 = sim.step_(act)
        now = sim.state()
        for e in (0, 1):
            assert np.array_equal(n2[e].cpu().numpy(), st['obs'][e]) and float(r2[e]) == 0.0 and float(d2[e]) == 0.0
            for name in ARRAYS:
                assert np.array_equal(now[name][e], st[name][e], equal_nan=True) if now[name].dtype.kind == 'f' else now[name][e] == st[name][e], (k, e, name)
        assert now['t'].tolist() == [-1, -1, 12 + k, 502 + k] and float(r2[2]) == float(r2[3]) == float(np.float32(-0.1 * 0.25))
        assert now['ep_return'][2] < st['ep_return'][2] and not np.array_equal(now['obs'][2], st['obs'][2])
    sim.reset()                                         # a reset thaws it
    assert sim.t.tolist() == [0] * N and sim.starts.tolist() == [1] * N and sim.episodes.tolist() == [1, 1, 0, 0]


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------------------
def _loop_against_the_eager_route(kind, make, fused, preset):
    """5 warm-up and 20 training iterations of iterate_sim on a FusedSim, N = 16, B = 64, a ring of 95 rows (the wrap falls inside an
    iteration), eps_greedy 0.25, against a twin: act_device -> the restated mix -> FusedSim.step_ of a second simulator -> add_device ->
    train().  Returns (agent, loop, ring snapshots after iteration 2: the loop's and the twin's, sim)."""
    from rlrep_amd.envs.sim_loop import SimLoop
    from rlrep_amd.utils.buffer import ReplayBuffer
    N, WARM, TRAIN, EPS, RING = 16, 5, 20, 0.25, 95
    agent, twin = make(), make(pipeline=False)
    S, A = agent.state_dim, agent.action_dim
    lo, hi = agent.action_range
    sims = []
    for _ in range(2):
        sim = _sim(kind, N)
        sim.reset()
        preset(sim)
        sims.append(sim)
    sim, sim2 = sims
    assert torch.equal(sim.obs, sim2.obs)
    buf, buf2 = ReplayBuffer(S, A, max_size=RING), ReplayBuffer(S, A, max_size=RING)
    loop = SimLoop(agent, sim, eps_greedy=EPS, start_timesteps=WARM * N, fused_append=fused)
    assert loop.fused_append == fused
    infos, early = [], None
    for it in range(WARM + TRAIN):
        out = agent.iterate_sim(loop, buf, B, train=it >= WARM)
        if it < WARM:
            assert out is None
        else:
            infos.append({k: float(v) for k, v in out.items()})
        if it == 2:
            early = buf.ring.clone()
        if it == WARM - 1:
            assert agent._sim_launches == (2 if fused else 3) and agent._sim_captures == 1     # the warm-up graph: the loop's launches alone
    assert agent._sim_captures == 2                                                             # one capture per form
    mixed, early2 = 0, None
    for it in range(WARM + TRAIN):
        warm = it < WARM
        if it == WARM:
            twin.prepare(buf2, B)               # (iterate_sim captures its training graph, which counts one call, before it acts)
        obs0 = sim2.obs.clone()
        pol = np.zeros((N, A), np.float32) if warm else twin.act_device(obs0, explore=True).cpu().numpy()
        acts, taken = ref.mix(pol, SEED, it, warm, EPS, lo, hi)
        mixed += 0 if warm else int(taken.sum())
        a = torch.from_numpy(acts).to(DEV)
        nxt, rew, done = sim2.step_(a)
        buf2.add_device(obs0, a, nxt, rew, done)
        if it == 2:
            early2 = buf2.ring.clone()
        if not warm:
            sg.assert_info_equal(infos[it - WARM], {k: float(v) for k, v in twin.train(buf2, B).items()}, (kind, fused, it))
    assert 0 < mixed < TRAIN * N
    torch.cuda.synchronize()
    assert torch.equal(buf.ring, buf2.ring) and torch.equal(early, early2)
    assert buf._size_dev.cpu().tolist() == buf2._size_dev.cpu().tolist() == [RING]
    sg.assert_equal(sg.state(agent.core), sg.state(twin.core), (kind, fused))
    assert agent.steps == twin.steps == TRAIN and agent._ctr == twin._ctr
    assert loop.counters() == ((WARM + TRAIN) * N, agent._ctr, WARM + TRAIN) == (loop.t_global, loop.calls, loop.iter)
    assert int(loop.state()['ring_ptr'][0]) == ((WARM + TRAIN) * N) % RING == buf2.ptr
    for name in ARRAYS:
        x, y = getattr(sim, name), getattr(sim2, name)
        assert torch.equal(x, y) or (name == 'last_return' and np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)), name
    assert agent._sim_launches == twin._graph_launches + (2 if fused else 3), (kind, fused, agent._sim_launches, twin._graph_launches)
    return agent, loop, early, sim


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('cfg', ['sac_pendulum', 'vlsac_f64'])
def test_loop_equals_the_eager_route_bit_for_bit(cfg, fused):
    """Pendulum's t is preset to 187: every environment restarts in the 13th of the 25 iterations, inside the replayed training graph"""
    agent, loop, early, sim = _loop_against_the_eager_route('pendulum', lambda **kw: _make(cfg, **kw)[0], fused, lambda s: s.t.fill_(187))
    assert sim.episodes.tolist() == [1] * 16 and sim.t.tolist() == [12] * 16 and sim.starts.tolist() == [2] * 16
    assert not bool(torch.isnan(sim.last_return).any())


@pytest.mark.parametrize('fused', [True, False])
def test_mountaincar_loop_writes_terminal_rows_and_restarts_inside_the_graph(fused):
    """sac at MountainCar's dims; environments 1 and 9 stand one step from the goal, 4 two steps, 6 on the step before the time limit: the
    ring holds rows with done = 1, and the row that follows one starts a new episode instead of continuing the rollout"""
    N, S, A = 16, 2, 1

    def preset(sim):
        st = sim.state()
        x0, x1, t = st['x0'].copy(), st['x1'].copy(), np.zeros(N, np.int32)
        for e, (p, v) in {1: (0.44, 0.05), 9: (0.44, 0.05), 4: (0.40, 0.04)}.items():
            x0[e], x1[e] = F32(p), F32(v)
        t[6] = 997
        sim.set_state(x0, x1, t)
    agent, loop, early, sim = _loop_against_the_eager_route('mountaincar', lambda **kw: _agent('sac', 'mountaincar', hidden_dim=64, **kw), fused, preset)
    ring = early.cpu().numpy()                          # rows of iterations 0, 1, 2: row i * N + e
    done = ring[:3 * N, 2 * S + A + 1].reshape(3, N)
    assert done[0].nonzero()[0].tolist() == [1, 9] and done[1].nonzero()[0].tolist() == [4] and not done[2].any()
    assert np.all(ring[[1, 9, N + 4], 2 * S + A] > 99.0)                    # +100 - 0.1 a^2
    for i, e in ((0, 1), (0, 9), (1, 4), (1, 6)):       # the goal three times; the time limit (done = 0) once
        row, nxt = ring[i * N + e], ring[(i + 1) * N + e]
        assert not np.array_equal(nxt[:S], row[S + A:2 * S + A]) and _is_start('mountaincar', float(nxt[0]), float(nxt[1])), (i, e, row, nxt)
    assert done[1][6] == 0.0
    for i, e in ((0, 0), (1, 1), (0, 4)):               # everywhere else the rollout continues
        assert np.array_equal(ring[(i + 1) * N + e][:S], ring[i * N + e][S + A:2 * S + A])
    assert sim.episodes.tolist() == [1 if e in (1, 4, 6, 9) else 0 for e in range(N)]
    assert sim.starts.tolist() == [2 if e in (1, 4, 6, 9) else 1 for e in range(N)]


# ---- 5. launcher ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('env_name', ['Pendulum-v1', 'MountainCarContinuous-v0'])
def test_launcher_runs_the_fused_simulator_loop(env_name, tmp_path, monkeypatch):
    import json
    from rlrep_amd import main
    from rlrep_amd.envs import fused_sim
    from rlrep_amd.utils import buffer
    from test_host_envs import _keep_instances
    made = _keep_instances(monkeypatch, buffer, 'ReplayBuffer')
    sims = _keep_instances(monkeypatch, fused_sim, 'FusedSim')
    argv = ['--alg', 'sac', '--env', env_name, '--torch-envs', '8', '--sim-graph', '--fused-sim', '--max_timesteps', '320', '--start_timesteps', '160',
            '--eval_freq', '320', '--batch_size', '64', '--eval_episodes', '2', '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert agent.steps == 20 and agent._sim_captures == 2                   # 40 iterations of 8 steps, 20 of them warm-up; one capture per form
    assert agent._ctr >= 20 * 8                                             # 8 exploring rows per training iteration
    assert len(made) == 1 and made[0]._device_env is not None              # the loop owns the cursor
    made[0].adopt_device_cursor()
    assert made[0].size == 320 and made[0].ptr == 0 and made[0].size_dev().cpu().tolist() == [320]
    assert len(evaluations) == 1 and np.isfinite(evaluations[0]) and (evaluations[0] < 0 or env_name != 'Pendulum-v1')
    train, ev = sims
    assert (train.num_envs, train.auto_restart, train.seed) == (8, True, 0) and (ev.num_envs, ev.auto_restart, ev.seed) == (2, False, 100)
    assert train.t.tolist() == [40] * 8 and ev.t.tolist() == [-1, -1] and ev.starts.tolist() == [1, 1] and ev.episodes.tolist() == [1, 1]
    assert evaluations[0] == float(ev.last_return.mean())
    rows = [json.loads(l) for l in open(tmp_path / env_name / 'sac' / '0' / '0' / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [320] and all(np.isfinite(v) for row in rows for v in row.values())
    assert 'info/q_loss' in rows[0] and 'info/actor_loss' in rows[0] and rows[0]['steps_per_sec'] > 0
