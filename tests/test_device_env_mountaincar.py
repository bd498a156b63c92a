"""MountainCarContinuous-v0 on the device (rlrep_amd/envs/device.py DeviceMountainCarGroup, csrc/group_env.hip) on the GPU: the device step
against the host MountainCarContinuousEnv, terminal rows (done_bool = 1) through the device loop against the host loop bit for bit, episode
ends by goal and by time limit, the early exit of the evaluation kernel, retired members, checkpoints and the launcher.  Reads nothing outside
the repository."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seed_group_util as sg  # noqa: E402
from test_device_env import _ulps  # noqa: E402

SEEDS = (3, 11, 42, 7)
R = len(SEEDS)
B = 64
LIMIT = 999
F32 = lambda x: float(np.float32(x))  # noqa: E731


# ---- helpers that need no GPU (tests/test_device_env_mountaincar_cpu.py checks them on the host) ---------------------------------------------
def mountaincar_dynamics_cases():
    """(p, v, a, t) cases of the one-step comparison; p, v and a are fp32 values (the state an observation shows, the action a policy hands
    over).  Random states, both speed clips, the left wall with v < 0, the right clip, |a| > 1, the goal before the limit, the goal on step
    999, the time limit without the goal."""
    g = np.random.RandomState(0)
    cases = [(g.uniform(-1.2, 0.6), g.uniform(-0.07, 0.07), g.uniform(-1, 1), int(g.randint(0, LIMIT - 2))) for _ in range(200)]
    for k in range(6):
        cases.append((-0.5 - 0.02 * k, 0.0695 + 0.0001 * k, 1.0, 3 + k))                  # speed clip, high
        cases.append((-0.5 + 0.02 * k, -0.0695 - 0.0001 * k, -1.0, 3 + k))                # speed clip, low
        cases.append((-1.19 - 0.002 * k, -0.02 - 0.008 * k, -1.0 + 0.3 * k, 40 + k))      # the left wall, moving left
        cases.append((0.55 + 0.01 * k, 0.06 + 0.002 * k, 0.2 * k, 100 + k))               # the right clip (a goal)
        cases.append((g.uniform(-1.0, 0.3), g.uniform(-0.05, 0.05), (1.0000001, -1.5, 3.0, -10.0, 1e3, -1e6)[k], 7))       # |a| > 1
        cases.append((0.40 + 0.008 * k, 0.055, 1.0 - 0.3 * k, 10 * k))                    # the goal before the limit
        cases.append((0.41 + 0.007 * k, 0.05 + 0.002 * k, 0.5, LIMIT - 1))                # the goal on step 999
        cases.append((-0.9 + 0.2 * k, 0.01 * (k - 3), -0.5 + 0.2 * k, LIMIT - 1))         # the time limit without the goal
    cases.append((-0.5, 0.0, 0.0, 0))
    cases.append((-1.2, -0.01, -1.0, 0))
    cases.append((0.44, 0.05, 1.0, LIMIT - 2))
    return [(F32(p), F32(v), F32(a), int(t)) for p, v, a, t in cases]


def host_step(p, v, a, t):
    """MountainCarContinuousEnv.step from state (p, v) at episode step t with action a -> (obs fp32 [2], reward fp32, done, goal, done_bool
    by main.py's rule, the unrounded (p', v') the goal was decided on)"""
    from rlrep_amd.envs.mountain_car import MountainCarContinuousEnv
    env = MountainCarContinuousEnv()
    env._p, env._v, env._t = p, v, t
    obs, rew, done, _ = env.step(np.asarray([a], np.float32))
    goal = bool(env._unrounded[0] >= 0.45 and env._unrounded[1] >= 0.0)
    done_bool = float(done) if t + 1 < LIMIT else 0.0          # main.py: `float(done) if ep_steps < max_length else 0`
    return obs, np.float32(rew), bool(done), goal, done_bool, env._unrounded


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------------------
def _space():
    from rlrep_amd.envs.mountain_car import MountainCarContinuousEnv
    return MountainCarContinuousEnv().action_space


def _group(alg, seeds=SEEDS, **extra):
    if alg == 'sac':
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
        return SACSeedBatch(list(seeds), 2, 1, _space(), max_batch=B, hidden_dim=256, **extra)
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    return CTRLSACSeedBatch(list(seeds), 2, 1, _space(), max_batch=B, hidden_dim=256, feature_dim=256, extra_feature_steps=3, **extra)


def _env(grp, **kw):
    from rlrep_amd.envs.device import DeviceMountainCarGroup
    return DeviceMountainCarGroup(grp, **kw)


def _rings(members, n):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    return ReplayBufferGroup(members, 2, 1, max_size=n)


def _put(env, members, episode_return=0.0):
    """set_state: member r of `members` = {r: (p, v, a, t)} stands at (p, v), step t of its episode, and takes action a next"""
    rec = env.state()
    for r, (p, v, a, t) in members.items():
        rec['theta'][r], rec['theta_dot'][r], rec['t'][r] = p, v, t
        rec['obs'][r][:2] = np.array([p, v], np.float32)
        rec['force'][r], rec['force_action'][r] = 1, a
        rec['episode_return'][r] = episode_return
    env.set_state(rec)
    return rec


def _is_start(p, v):
    return F32(-0.6) <= p <= F32(-0.4) and v == 0.0 and p == F32(p)


# ---- 1. dynamics ------------------------------------------------------------------------------------------------------------------------------
def test_device_step_matches_the_host_environment():
    """Both sides compute in fp64 and round to fp32 once: one fp32 rounding step, plus one for a last-bit difference of the two libms' cos.
    Bound: 2 fp32 ulp per element of s' (the bound of tests/test_device_env.py); r and done_bool exactly.
    Measured on an MI355X (profiles/seed_batch_device_env_mountaincar.txt): worst 0 ulp on s'."""
    grp = _group('sac')
    env, buf = _env(grp), _rings(R, 4)
    cases = mountaincar_dynamics_cases()
    buf.collect_on_device(env)
    worst = 0
    for k0 in range(0, len(cases), R):
        chunk = cases[k0:k0 + R]
        chunk = chunk + [chunk[-1]] * (R - len(chunk))
        rec = _put(env, dict(enumerate(chunk)), episode_return=-7.5)
        rec['ring_ptr'], rec['episodes_done'] = 2, 0
        env.set_state(rec)
        before = rec.copy()
        grp.iterate(env, buf, B, train=False)
        rows = buf.rings[:, 2].cpu().numpy()
        new = env.state()
        for r, (p, v, a, t) in enumerate(chunk):
            obs, rew, done, goal, done_bool, _ = host_step(p, v, a, t)
            row = rows[r]
            assert np.array_equal(row[:2], before['obs'][r][:2]) and row[2] == np.float32(a), (k0 + r, row)
            d = int(_ulps(row[3:5], obs).max())
            worst = max(worst, d)
            assert d <= 2, (k0 + r, chunk[r], row, obs)
            assert row[5] == rew and row[6] == done_bool, (k0 + r, chunk[r], row, rew, done_bool)
            assert new['ring_ptr'][r] == 3 and new['ring_size'][r] >= 1 and new['force'][r] == 0 and new['act'][r] == np.float32(a)
            p2, v2 = float(new['theta'][r]), float(new['theta_dot'][r])
            assert p2 == F32(p2) and v2 == F32(v2)                                  # the state is held as fp32 values
            assert np.array_equal(new['obs'][r][:2], np.array([p2, v2], np.float32)) and new['obs'][r][2] == 0.0
            if done:
                assert new['t'][r] == 0 and new['episodes_done'][r] == 1 and new['episode_return'][r] == 0.0
                assert new['returns'][r][0] == -7.5 + float(row[5])
                assert _is_start(p2, v2), (k0 + r, p2, v2)
            else:
                assert (p2, v2) == (float(row[3]), float(row[4]))
                assert new['t'][r] == t + 1 and new['episodes_done'][r] == 0 and new['episode_return'][r] == -7.5 + float(row[5])
    print(f'device step vs MountainCarContinuousEnv.step over {len(cases)} cases: worst {worst} fp32 ulp on s\', r and done_bool equal')


# ---- 2. acting --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ['sac', 'ctrlsac'])
def test_device_action_equals_select_action_bit_for_bit(alg):
    grp, twin = _group(alg), _group(alg)
    env, buf = _env(grp, eps_greedy=0.0, start_timesteps=0), _rings(R, 32)
    for k in range(4):
        grp.iterate(env, buf, B, train=False)
        rows = buf.rings[:, k].cpu().numpy()
        twin._ctr = grp._ctr - 1                                    # the same call counter
        act = twin.select_action(rows[:, :2], explore=True)
        assert twin._ctr == grp._ctr
        assert np.array_equal(act.reshape(-1).view(np.uint32), rows[:, 2].copy().view(np.uint32)), (alg, k, act.reshape(-1), rows[:, 2])
        assert np.all(np.abs(act) <= 1.0) and len(set(act.reshape(-1).tolist())) == R


# ---- 3. the device loop is the host loop, terminal rows included ------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ['sac', 'ctrlsac'])
def test_device_loop_equals_host_loop_on_the_same_transitions(alg):
    """Every member reaches the goal on its first and on its 31st step (set_state / force), so each ring of 128 holds two rows with
    done_bool = 1 among the 95 that 25 batches of 64 are drawn from: the critic's (1 - done) factor sees them."""
    warm, calls = 70, 25
    grp = _group(alg)
    env, buf = _env(grp, eps_greedy=0.05, start_timesteps=warm), _rings(R, 128)
    for k in range(warm):
        if k in (0, 30):
            if k == 0:
                buf.collect_on_device(env)
            _put(env, {r: (F32(0.44), F32(0.05), 1.0, 5 + r) for r in range(R)})
        assert grp.iterate(env, buf, B, train=False) is None
    infos = []
    for _ in range(calls):
        out = grp.iterate(env, buf, B)
        infos.append([{k: float(v) for k, v in i.items()} for i in out])
    torch.cuda.synchronize()
    rows = buf.rings.cpu().numpy()
    n = warm + calls
    assert np.array_equal(rows[:, :n, 6] == 1.0, np.broadcast_to(np.isin(np.arange(n), [0, 30]), (R, n)))       # done_bool = 1: those rows only
    assert np.all(rows[:, [0, 30], 5] > 99.0)
    rec = env.state()
    assert list(rec['ring_ptr']) == [n] * R and list(rec['episodes_done']) == [2] * R
    twin, buf2 = _group(alg), _rings(R, 128)
    for t in range(n):
        r = rows[:, t]
        buf2.add(r[:, :2], r[:, 2:3], r[:, 3:5], r[:, 5], r[:, 6])
        if t >= warm:
            out2 = twin.train(buf2, B)
            for m in range(R):
                sg.assert_info_equal(infos[t - warm][m], out2[m], (alg, t, m))
    assert twin.steps == grp.steps == calls
    for m in range(R):
        sg.assert_equal(sg.state(grp._members[m]), sg.state(twin._members[m]), (alg, m))
    assert torch.equal(buf2.rings[:, :n].cpu(), buf.rings[:, :n].cpu())
    # the transitions are a rollout except behind an episode's end (and where set_state moved the car)
    keep = [t for t in range(1, n) if t not in (1, 30, 31)]
    assert np.array_equal(rows[:, keep, :2], rows[:, [t - 1 for t in keep], 3:5])
    assert all(_is_start(float(rows[m, t, 0]), float(rows[m, t, 1])) for m in range(R) for t in (1, 31))


# ---- 4. episodes ------------------------------------------------------------------------------------------------------------------------------
def test_episode_ends_by_goal_and_by_time_limit():
    grp = _group('sac')
    env, buf = _env(grp, eps_greedy=0.0, start_timesteps=10 ** 6), _rings(R, 1024)            # uniform actions throughout: they reach no goal
    buf.collect_on_device(env)
    put = {0: (F32(0.44), F32(0.05), 1.0, 10), 1: (F32(0.44), F32(0.05), 1.0, LIMIT - 1), 2: (F32(-0.5), 0.0, 0.5, LIMIT - 1),
           3: (F32(-0.5), 0.0, 0.5, 500)}
    _put(env, put, episode_return=-7.5)
    assert env.returns() == [[]] * R
    grp.iterate(env, buf, B, train=False)
    rec = env.state()
    row = buf.rings[:, 0].cpu().numpy()
    assert row[:, 6].tolist() == [1.0, 0.0, 0.0, 0.0]               # goal; goal on step 999; time limit; neither
    assert row[0, 5] == np.float32(99.9) and row[1, 5] == np.float32(99.9) and row[2, 5] == np.float32(-0.025)
    assert list(rec['episodes_done']) == [1, 1, 1, 0] and list(rec['t']) == [0, 0, 0, 501]
    for m in range(3):
        assert rec['returns'][m][0] == -7.5 + float(row[m, 5]) and rec['episode_return'][m] == 0.0
        assert _is_start(float(rec['theta'][m]), float(rec['theta_dot'][m])) and np.array_equal(rec['obs'][m][:2], [np.float32(rec['theta'][m]), 0])
    assert len({float(rec['theta'][m]) for m in range(3)}) == 3
    assert rec['episode_return'][3] == -7.5 + float(row[3, 5])
    # a whole time limit further: the new episodes of members 0..2 end on their 999th step, member 3's on its 499th step from here
    for _ in range(LIMIT):
        grp.iterate(env, buf, B, train=False)
    rec = env.state()
    assert list(rec['episodes_done']) == [2, 2, 2, 1] and list(rec['t']) == [0, 0, 0, 501] and list(rec['nsteps']) == [LIMIT + 1] * R
    rows = buf.rings.cpu().numpy()
    assert np.all(rows[:, 1:LIMIT + 1, 6] == 0.0) and np.all(rows[:, 1:LIMIT + 1, 5] <= 0.0)      # time limits only: never done_bool
    got = env.returns()
    for m in range(R):
        first = 1 if m < 3 else 0
        total = 0.0 if m < 3 else -7.5
        for v in rows[m, first:(LIMIT + 1 if m < 3 else 499), 5]:
            total += float(v)                          # fp64 sum of the fp32 rewards, in step order
        want = [-7.5 + float(row[m, 5]), total] if m < 3 else [total]
        assert got[m] == want, (m, got[m], want)
    assert env.returns() == [[]] * R                                                # drained


# ---- 5. scoring -------------------------------------------------------------------------------------------------------------------------------
def _write_actor(grp, r, chase):
    """Member r's actor by hand.  chase: the mean action follows the sign of the velocity -- first-layer unit 0 reads obs[1] with gain 1e4,
    unit 0 of the second layer passes it on, the head is 20 h - 10 (v <= 0: h in (-1, 0], tanh(<= -10) = -1; v > 1e-4: tanh(>= 10) = +1).
    Otherwise a constant +1 (head bias 10, every weight 0)."""
    with torch.no_grad():
        mats = [q for _, q in grp.member(r).actor.named_parameters()]
        for q in mats:
            q.zero_()
        W = [q for q in mats if q.dim() == 2]
        b = [q for q in mats if q.dim() == 1]
        assert [tuple(q.shape) for q in W] == [(256, 2), (256, 256), (2, 256)] and [tuple(q.shape) for q in b] == [(256,), (256,), (2,)]
        if chase:
            W[0][0, 1], W[1][0, 0], W[2][0, 0], b[2][0] = 1e4, 1.0, 20.0, -10.0
        else:
            b[2][0] = 10.0
    torch.cuda.synchronize()


def _host_scores(grp, starts, perturb=None):
    """Returns of host rollouts from the device's start states, [R, E]: MountainCarContinuousEnv stepped with select_action(explore=False)
    until done.  perturb: a RandomState that moves every observation the policy sees by one fp32 ulp in a random direction.  Also the
    episode lengths."""
    from rlrep_amd.envs.mountain_car import MountainCarContinuousEnv
    members, E = starts.shape[:2]
    total, steps = np.zeros((members, E)), np.zeros((members, E), np.int64)
    for e in range(E):
        envs_ = [MountainCarContinuousEnv() for _ in range(members)]
        obs = np.zeros((members, 2), np.float32)
        for r, me in enumerate(envs_):
            me._p, me._v, me._t = float(starts[r, e, 0]), float(starts[r, e, 1]), 0
            obs[r] = me._obs()
        over = [False] * members
        while not all(over):
            seen = obs
            if perturb is not None:
                seen = np.nextafter(obs, np.where(perturb.randint(0, 2, size=obs.shape) > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
            act = grp.select_action(seen)
            for r, me in enumerate(envs_):
                if not over[r]:
                    obs[r], rew, over[r], _ = me.step(act[r])
                    total[r, e] += float(np.float32(rew))
                    steps[r, e] += 1
    return total, steps


def test_device_scores_equal_host_rollouts_and_the_goal_ends_an_episode():
    """Members 0, 1 chase the velocity's sign and reach the goal (the evaluation loop leaves early: a loop that ran on would collect further
    rewards and differ from the host rollout, which stops at done); members 2, 3 push right all the time and run into the time limit.
    Tolerance as in tests/test_device_env.py: 10 x the spread of the host rollout under 1-ulp perturbed observations; equality where that is 0.
    Measured on an MI355X (profiles/seed_batch_device_env_mountaincar.txt): |device - host| 0, host spread 1.5e-8."""
    E = 3
    grp = _group('sac')
    env = _env(grp)
    for r in range(R):
        _write_actor(grp, r, chase=r < 2)
    out = torch.full((R, E), float('nan'), dtype=torch.float64, device='cuda')
    env.evaluate(E, 5, out)
    scores = out.cpu().numpy()
    mean = grp.evaluate(env, E, eval_index=5)
    assert np.allclose(mean, scores.mean(axis=1), rtol=1e-13, atol=0.0)
    starts = env.eval_starts(E)
    assert starts.shape == (R, E, 2) and np.all(starts[..., 1] == 0.0) and np.all(starts[..., 0] >= F32(-0.6)) and np.all(starts[..., 0] <= F32(-0.4))
    assert np.array_equal(starts[..., 0], starts[..., 0].astype(np.float32).astype(np.float64)) and len(np.unique(starts[..., 0])) == R * E
    host, steps = _host_scores(grp, starts)
    moved, _ = _host_scores(grp, starts, np.random.RandomState(1))
    spread = float(np.abs(host - moved).max())
    diff = float(np.abs(scores - host).max())
    print(f'evaluate vs host rollouts: device {scores.tolist()}, host {host.tolist()}, host episode lengths {steps.tolist()}, '
          f'|device - host| max {diff:.3e}, host spread under 1-ulp observations {spread:.3e}')
    assert diff <= 10 * spread, (scores, host, diff, spread)
    assert np.all(steps[:2] < 200) and np.all(scores[:2] > 80.0) and np.all(scores[:2] < 100.0)           # the goal, early
    assert np.all(steps[2:] == LIMIT) and np.all(np.abs(scores[2:] + 99.9) < 1e-4)                          # 999 steps of -0.1
    other = grp.evaluate(env, E, eval_index=6)
    assert not np.array_equal(env.eval_starts(E), starts) and np.all(np.isfinite(other))


# ---- 6. retired members -----------------------------------------------------------------------------------------------------------------------
def test_a_retired_member_is_not_touched():
    grp = _group('sac')
    env, buf = _env(grp, eps_greedy=0.05, start_timesteps=5), _rings(R, 128)
    for t in range(12):
        grp.iterate(env, buf, B, train=t >= 5)
    grp.retire_members([2])
    block, ring, rec = sg.member_bytes(grp, 2), buf.rings[2].clone(), env.state()
    for _ in range(6):
        out = grp.iterate(env, buf, B)
        assert out[2] is None and all(out[q] is not None for q in (0, 1, 3))
    scores = grp.evaluate(env, 2)
    assert np.isnan(scores[2]) and np.all(np.isfinite(scores[[0, 1, 3]]))
    now = env.state()
    assert torch.equal(sg.member_bytes(grp, 2), block) and torch.equal(buf.rings[2], ring) and now[2].tobytes() == rec[2].tobytes()
    assert buf.size_dev().cpu().tolist() == [18, 18, 12, 18]
    assert [int(now['nsteps'][q]) for q in (0, 1, 3)] == [18] * 3 and env.counters()[0] == 18


# ---- 7. checkpoints ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_continues_bit_identically_and_carries_the_kind(tmp_path):
    from rlrep_amd.envs.device import DevicePendulumGroup
    from rlrep_amd.envs.pendulum import PendulumEnv
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    grp = _group('sac')
    env, buf = _env(grp, eps_greedy=0.05, start_timesteps=20), _rings(R, 128)
    buf.collect_on_device(env)
    _put(env, {0: (F32(0.44), F32(0.05), 1.0, 3)})                   # a filed return and a terminal row travel with the checkpoint
    for _ in range(30):
        grp.iterate(env, buf, B, train=False)
    # trained state for the checkpoint, through train(): capturing a training graph counts one call in the noise counter (SeedBatchMixin.
    # _sample_into 'warm'), so the group that goes on and the one that is loaded both capture their iterate(train=True) graph below
    buf.adopt_device_cursor()
    for _ in range(5):
        grp.train(buf, B)
    assert env.state()['episodes_done'][0] == 1 and buf.rings[0, 0, 6].item() == 1.0
    path = str(tmp_path / 'group.pt')
    grp.save(path, env=env)
    grp2 = _group('sac')
    env2, buf2 = _env(grp2, eps_greedy=0.05, start_timesteps=20), _rings(R, 128)
    grp2.load(path, env=env2)
    buf2.rings.copy_(buf.rings)
    buf2.ptr, buf2.sizes = buf.ptr, list(buf.sizes)
    assert np.array_equal(env2.state(), env.state()) and env2.counters() == env.counters() and env2.kind == 2
    for _ in range(5):
        a, b = grp.iterate(env, buf, B), grp2.iterate(env2, buf2, B)
        for m in range(R):
            sg.assert_info_equal(a[m], b[m], m)
    for m in range(R):
        sg.assert_equal(sg.state(grp._members[m]), sg.state(grp2._members[m]), m)
    assert np.array_equal(env2.state(), env.state()) and torch.equal(buf.rings, buf2.rings)
    pend = SACSeedBatch(list(SEEDS), 3, 1, PendulumEnv().action_space, max_batch=B, hidden_dim=256)
    penv = DevicePendulumGroup(pend)
    with pytest.raises(RuntimeError, match='does not match this device environment'):
        penv.load_snapshot(torch.load(path)['device_env'])
    with pytest.raises(RuntimeError, match='does not match this device environment'):
        env.load_snapshot(penv.snapshot())


# ---- 8. launcher ------------------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_the_device_loop(tmp_path):
    import json
    from rlrep_amd import main
    argv = ['--alg', 'sac', '--env', 'MountainCarContinuous-v0', '--seeds', '0,1', '--device-env', '--max_timesteps', '450', '--start_timesteps', '150',
            '--eval_freq', '150', '--batch_size', '64', '--eval_episodes', '2', '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert agent.steps == 300 and agent.state_dim == 2
    root = tmp_path / 'MountainCarContinuous-v0' / 'sac' / '0'
    for r, s in enumerate((0, 1)):
        rows = [json.loads(l) for l in open(root / str(s) / 'metrics.jsonl')]
        assert [row['step'] for row in rows] == [300, 450]
        assert all({'step', 'info/evaluation', 'steps_per_sec', 'info/q_loss', 'info/actor_loss', 'info/alpha'} <= set(row) for row in rows)
        assert all(np.isfinite(v) for row in rows for v in row.values() if isinstance(v, (int, float)))
        assert len(evaluations[r]) == 4 and all(np.isfinite(v) for v in evaluations[r])
