"""The device environment of a SINGLE agent (rlrep_amd/envs/device.py DeviceEnv, SACAgent.iterate / evaluate, csrc/group_env.hip env_*_kernel)
on the GPU, for all five algorithms: the contracts of the seed group's device environments at R = 1 -- acting against select_action, the
device step against the host environments, the device loop against the host loop on the same transitions (bit for bit), scoring against host
rollouts, the ring wrap, interleaving with train(), checkpoints, refusals and the launcher.  Reads nothing outside the repository."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seed_group_util as sg  # noqa: E402
from test_device_env import dynamics_cases, host_step as pendulum_host_step, _ulps  # noqa: E402
from test_device_env_mountaincar import mountaincar_dynamics_cases, host_step as mountaincar_host_step, LIMIT  # noqa: E402

ALGS = ('sac', 'vlsac', 'ctrlsac', 'spedersac', 'diffsrsac')
B = 64
RING = 95                   # rows: 70 warm-up steps + 25 training steps fill it exactly, anything more wraps
SEED = 5
F32 = lambda x: float(np.float32(x))  # noqa: E731
KINDS = {'pendulum': (3, 1), 'mountaincar': (2, 1)}


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _host_env(kind):
    if kind == 'pendulum':
        from rlrep_amd.envs.pendulum import PendulumEnv
        return PendulumEnv()
    from rlrep_amd.envs.mountain_car import MountainCarContinuousEnv
    return MountainCarContinuousEnv()


def _agent(alg, kind='pendulum', seed=SEED, S=None, A=None, space=None, **extra):
    """agent of `alg` with the kind's dimensions and widths of 256, initialised as `torch.manual_seed(seed); Agent(..., seed=seed)`"""
    S0, A0 = KINDS[kind]
    S, A = S or S0, A or A0
    space = space or _host_env(kind).action_space
    kw = dict(max_batch=B, seed=seed, hidden_dim=256)
    if alg == 'sac':
        from rlrep_amd.agent.sac.sac_agent import SACAgent as cls
    elif alg == 'vlsac':
        from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent as cls
        kw.update(feature_dim=256, extra_feature_steps=3)
    elif alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent as cls
        kw.update(feature_dim=256, extra_feature_steps=3)
    elif alg == 'spedersac':
        from rlrep_amd.agent.spedersac.spedersac_agent import SPEDERSACAgent as cls
        kw.update(phi_and_mu_lr=1e-5, phi_hidden_dim=256, phi_hidden_depth=1, mu_hidden_dim=256, mu_hidden_depth=0, critic_and_actor_lr=3e-4,
                  critic_and_actor_hidden_dim=256, feature_dim=256, extra_feature_steps=3)
    else:
        from rlrep_amd.agent.diffsrsac.diffsrsac_agent import DIFFSRSACAgent as cls
        kw.update(feature_dim=256, extra_feature_steps=3)
    kw.update(extra)
    torch.manual_seed(seed)
    return cls(S, A, space, **kw)


def _env(agent, kind='pendulum', **kw):
    from rlrep_amd.envs.device import DevicePendulum, DeviceMountainCar
    return (DevicePendulum if kind == 'pendulum' else DeviceMountainCar)(agent, **kw)


def _ring(kind='pendulum', n=RING, **kw):
    from rlrep_amd.utils.buffer import ReplayBuffer
    S, A = KINDS[kind]
    return ReplayBuffer(S, A, max_size=n, **kw)


def _rows(buf):
    torch.cuda.synchronize()
    return buf.ring.cpu().numpy()


def _add(buf, row, S):
    buf.add(row[:S], row[S:S + 1], row[S + 1:2 * S + 1], row[2 * S + 1], row[2 * S + 2])


def _put(env, x0, x1, obs, a, t, **fields):
    """the record stands at state (x0, x1) with observation `obs`, step t of its episode, and takes action a next"""
    rec = env.state()
    rec['theta'][0], rec['theta_dot'][0], rec['t'][0] = x0, x1, t
    rec['obs'][0][:len(obs)] = np.asarray(obs, np.float32)
    rec['force'][0], rec['force_action'][0] = 1, a
    for k, v in fields.items():
        rec[k][0] = v
    env.set_state(rec)
    return rec


# ---- 1. acting --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ALGS)
def test_device_action_equals_select_action_bit_for_bit(alg):
    agent, twin = _agent(alg), _agent(alg)
    env, buf = _env(agent, eps_greedy=0.0, start_timesteps=0), _ring(n=32)
    acts = []
    for k in range(4):
        assert agent.iterate(env, buf, B, train=False) is None
        row = _rows(buf)[k]
        twin._ctr = agent._ctr - 1                                  # the same call counter
        act = twin.select_action(row[:3], explore=True)
        assert twin._ctr == agent._ctr
        assert np.array_equal(act.view(np.uint32), row[3:4].copy().view(np.uint32)), (alg, k, act, row[3])
        assert abs(float(act[0])) <= 2.0
        acts.append(float(act[0]))
    assert len(set(acts)) == 4
    # ... and select_action between two device steps moves the counter the device step continues from
    agent.select_action(np.zeros(3, np.float32), explore=True)
    agent.iterate(env, buf, B, train=False)
    row = _rows(buf)[4]
    twin._ctr = agent._ctr - 1
    assert np.array_equal(twin.select_action(row[:3], explore=True).view(np.uint32), row[3:4].copy().view(np.uint32))
    assert env.counters() == (5, agent._ctr) and int(env.state()['nsteps'][0]) == 5


# ---- 2. dynamics ------------------------------------------------------------------------------------------------------------------------------
def test_pendulum_step_matches_the_host_environment():
    """0 fp32 ulp on s' and r against envs/pendulum.py over test_device_env.dynamics_cases() (the group form measured 0:
    profiles/seed_batch_device_env.txt; the single form runs the same body)."""
    agent = _agent('sac')
    env, buf = _env(agent), _ring(n=4)
    worst = 0
    for k, (th, thd, u, t) in enumerate(dynamics_cases()):
        buf.collect_on_device(env)
        before = _put(env, th, thd, [np.cos(th), np.sin(th), thd], u, t, ring_ptr=2, episode_return=-7.5, episodes_done=0).copy()
        agent.iterate(env, buf, B, train=False)
        row, new = _rows(buf)[2], env.state()
        obs, rew, done, (th2, thd2) = pendulum_host_step(th, thd, u, t)
        assert np.array_equal(row[:3], before['obs'][0][:3]) and row[3] == np.float32(u) and row[8] == 0.0, (k, row)
        d = int(max(_ulps(row[4:7], obs).max(), _ulps(row[7:8], np.array([rew])).max()))
        worst = max(worst, d)
        assert d == 0, (k, (th, thd, u, t), row, obs, rew)
        assert new['ring_ptr'][0] == 3 and new['force'][0] == 0 and new['act'][0] == np.float32(u)
        if done:
            assert new['t'][0] == 0 and new['episodes_done'][0] == 1 and new['returns'][0][0] == -7.5 + float(row[7])
            assert -np.pi <= new['theta'][0] <= np.pi and -1.0 <= new['theta_dot'][0] <= 1.0
        else:
            assert new['t'][0] == t + 1 and new['episode_return'][0] == -7.5 + float(row[7]) and np.array_equal(new['obs'][0][:3], row[4:7])
            assert abs(new['theta'][0] - th2) <= 1e-12 * max(abs(th2), 1e-300) and abs(new['theta_dot'][0] - thd2) <= 1e-12 * max(abs(thd2), 1e-300)
    print(f'single-agent device step vs PendulumEnv.step: worst {worst} fp32 ulp on (s\', r)')


def test_mountaincar_step_matches_the_host_environment():
    """0 fp32 ulp on s' and r and an equal done_bool against envs/mountain_car.py over the existing MountainCar case list."""
    agent = _agent('sac', 'mountaincar')
    env, buf = _env(agent, 'mountaincar'), _ring('mountaincar', n=4)
    for k, (p, v, a, t) in enumerate(mountaincar_dynamics_cases()):
        buf.collect_on_device(env)
        before = _put(env, p, v, [p, v], a, t, ring_ptr=2, episode_return=-7.5, episodes_done=0).copy()
        agent.iterate(env, buf, B, train=False)
        row, new = _rows(buf)[2], env.state()
        obs, rew, done, goal, done_bool, _ = mountaincar_host_step(p, v, a, t)
        assert np.array_equal(row[:2], before['obs'][0][:2]) and row[2] == np.float32(a), (k, row)
        assert int(_ulps(row[3:5], obs).max()) == 0 and int(_ulps(row[5:6], np.array([rew])).max()) == 0, (k, (p, v, a, t), row, obs, rew)
        assert row[6] == done_bool, (k, (p, v, a, t), row, done_bool)
        if done:
            assert new['t'][0] == 0 and new['episodes_done'][0] == 1 and new['returns'][0][0] == -7.5 + float(row[5])
            assert F32(-0.6) <= new['theta'][0] <= F32(-0.4) and new['theta_dot'][0] == 0.0
        else:
            assert new['t'][0] == t + 1 and (float(new['theta'][0]), float(new['theta_dot'][0])) == (float(row[3]), float(row[4]))


# ---- 3. the device loop is the host loop, and one graph replay --------------------------------------------------------------------------------
def _device_loop_against_the_twin(alg, kind, force_goal_at=(), **extra):
    """70 warm-up steps and 25 training iterations on the device; a twin of the same class and seed, built with pipeline=False, is fed the
    rows the device wrote through ReplayBuffer.add and trained by train(): bit-identical state and info dicts.  The captured iterate() holds
    the twin's whole-train() graph launches plus one."""
    S = KINDS[kind][0]
    warm, calls = 70, 25
    agent = _agent(alg, kind, **extra)
    env, buf = _env(agent, kind, eps_greedy=0.05, start_timesteps=warm), _ring(kind)
    for k in range(warm):
        if k in force_goal_at:
            buf.collect_on_device(env)
            _put(env, F32(0.44), F32(0.05), [0.44, 0.05], 1.0, 5)
        assert agent.iterate(env, buf, B, train=False) is None
    assert agent._iter_launches == 1                                # the warm-up graph is the step launch alone
    infos = []
    for _ in range(calls):
        infos.append({k: float(v) for k, v in agent.iterate(env, buf, B).items()})
    rows = _rows(buf)
    n = warm + calls
    rec = env.state()
    assert int(rec['ring_ptr'][0]) == n % RING and int(rec['ring_size'][0]) == n and buf.size_dev().cpu().tolist() == [n]
    assert env.counters() == (n, agent._ctr)
    twin, buf2 = _agent(alg, kind, pipeline=False, **extra), _ring(kind)
    for t in range(n):
        _add(buf2, rows[t], S)
        if t >= warm:
            sg.assert_info_equal(infos[t - warm], twin.train(buf2, B), (alg, t))
    assert twin.steps == agent.steps == calls
    sg.assert_equal(sg.state(agent.core), sg.state(twin.core), alg)
    assert torch.equal(buf2.ring.cpu(), buf.ring.cpu())
    assert agent._iter_launches == twin._graph_launches + 1, (alg, agent._iter_launches, twin._graph_launches)
    return rows


@pytest.mark.parametrize('alg', ALGS + ('vlsac_f64',))
def test_device_loop_equals_host_loop_on_the_same_transitions(alg):
    """vlsac_f64: feature_dim 64, below one 128-wide tile of the 16-row engine"""
    extra = dict(feature_dim=64) if alg == 'vlsac_f64' else {}
    rows = _device_loop_against_the_twin(alg.split('_')[0], 'pendulum', **extra)
    # the transitions are a rollout (no episode ended), warm-up actions are uniform draws in [-2, 2]
    assert np.array_equal(rows[1:, :3], rows[:-1, 4:7]) and np.all(rows[:, 8] == 0.0)
    assert np.all(np.abs(rows[:70, 3]) <= 2.0) and np.abs(rows[:70, 3]).max() > 1.5


@pytest.mark.parametrize('alg', ['sac', 'vlsac'])
def test_device_loop_equals_host_loop_with_terminal_rows(alg):
    """The car reaches the goal on its first and on its 31st step (set_state / force): the ring holds two rows with done_bool = 1 among the
    95 the 25 batches are drawn from, so the critic's (1 - done) factor sees them."""
    rows = _device_loop_against_the_twin(alg, 'mountaincar', force_goal_at=(0, 30))
    assert np.array_equal(rows[:, 6] == 1.0, np.isin(np.arange(RING), [0, 30])) and np.all(rows[[0, 30], 5] > 99.0)
    keep = [t for t in range(1, RING) if t not in (1, 30, 31)]
    assert np.array_equal(rows[keep, :2], rows[[t - 1 for t in keep], 3:5])


# ---- 4. scoring -------------------------------------------------------------------------------------------------------------------------------
def _host_scores(agent, kind, starts, perturb=None):
    """Returns and lengths of host rollouts from the device's start states, [E] each: the host environment stepped with
    select_action(explore=False) until done.  perturb: a RandomState that moves every observation the policy sees by one fp32 ulp in a random
    direction (the last-bit difference the dynamics tests allow between the device's observations and the host's)."""
    total, steps = np.zeros(len(starts)), np.zeros(len(starts), np.int64)
    for e, (x0, x1) in enumerate(starts):
        he = _host_env(kind)
        if kind == 'pendulum':
            he._th, he._thd, he._t = float(x0), float(x1), 0
        else:
            he._p, he._v, he._t = float(x0), float(x1), 0
        obs, over = np.asarray(he._obs(), np.float32), False
        while not over:
            seen = obs
            if perturb is not None:
                seen = np.nextafter(obs, np.where(perturb.randint(0, 2, size=obs.shape) > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
            obs, rew, over, _ = he.step(agent.select_action(seen))
            obs = np.asarray(obs, np.float32)
            total[e] += float(np.float32(rew))
            steps[e] += 1
    return total, steps


def _scores_against_host(agent, env, kind, E, index, what):
    """one device evaluation at `index` against host rollouts from its start states; the rule of tests/test_device_env.py: |device - host| <=
    10 x the spread a one-ulp perturbation of the host's observations produces"""
    from rlrep_amd._lib import lib
    out = torch.full((1, E), float('nan'), dtype=torch.float64, device='cuda')
    n0 = lib.rlrep_launch_counter()
    env.evaluate(E, index, out)
    assert lib.rlrep_launch_counter() == n0 + 1                     # one launch
    scores = out.cpu().numpy()[0]
    mean = agent.evaluate(env, E, eval_index=index)
    assert isinstance(mean, float) and np.isclose(mean, scores.mean(), rtol=1e-13, atol=0.0)
    starts = env.eval_starts(E)
    assert starts.shape == (1, E, 2) and len(np.unique(starts[0, :, 0])) == E
    assert agent.evaluate(env, E, eval_index=index) == mean and np.array_equal(env.eval_starts(E), starts)       # the same index: the same scores
    host, steps = _host_scores(agent, kind, starts[0])
    moved, _ = _host_scores(agent, kind, starts[0], np.random.RandomState(1))
    spread, diff = float(np.abs(host - moved).max()), float(np.abs(scores - host).max())
    print(f'{what}: device {scores.tolist()}, host {host.tolist()}, lengths {steps.tolist()}, |device - host| max {diff:.3e}, '
          f'host spread under 1-ulp observations {spread:.3e}')
    assert diff <= 10 * spread, (what, scores, host, diff, spread)
    return scores, steps, starts


def _refused_episode_counts(agent, env):
    for episodes in (0, 65):
        with pytest.raises(RuntimeError, match=f'env_evaluate: episodes {episodes} outside'):
            agent.evaluate(env, episodes, eval_index=0)


@pytest.mark.parametrize('alg', ['sac', 'vlsac'])
def test_pendulum_scores_equal_host_rollouts(alg):
    agent = _agent(alg)
    env, buf = _env(agent, eps_greedy=0.05, start_timesteps=40), _ring(n=512)
    for phase in ('initialisation', 'after 100 training iterations'):
        _, steps, starts = _scores_against_host(agent, env, 'pendulum', 4, 5, f'{alg} pendulum, {phase}')
        assert np.all(steps == 200) and np.all(np.abs(starts[0, :, 0]) <= np.pi) and np.all(np.abs(starts[0, :, 1]) <= 1.0)
        agent.evaluate(env, 4, eval_index=6)
        assert not np.array_equal(env.eval_starts(4), starts)
        if phase == 'initialisation':
            for t in range(140):
                agent.iterate(env, buf, B, train=t >= 40)
    # evaluate() counts evaluations by itself: fresh starts every time
    i0 = env.eval_index
    agent.evaluate(env, 3)
    s1 = env.eval_starts(3)
    agent.evaluate(env, 3)
    assert env.eval_index == i0 + 2 and not np.array_equal(s1, env.eval_starts(3))
    _refused_episode_counts(agent, env)


def _write_actor(agent, chase):
    """The actor by hand (tests/test_device_env_mountaincar.py _write_actor).  chase: the mean action follows the sign of the velocity and
    reaches the goal; otherwise a constant +1, which runs into the time limit."""
    with torch.no_grad():
        mats = [q for _, q in agent.actor.named_parameters()]
        for q in mats:
            q.zero_()
        W, b = [q for q in mats if q.dim() == 2], [q for q in mats if q.dim() == 1]
        assert [tuple(q.shape) for q in W] == [(256, 2), (256, 256), (2, 256)] and [tuple(q.shape) for q in b] == [(256,), (256,), (2,)]
        if chase:
            W[0][0, 1], W[1][0, 0], W[2][0, 0], b[2][0] = 1e4, 1.0, 20.0, -10.0
        else:
            b[2][0] = 10.0
    torch.cuda.synchronize()


def test_mountaincar_scores_equal_host_rollouts_and_the_goal_ends_an_episode():
    agent = _agent('sac', 'mountaincar')
    env, buf = _env(agent, 'mountaincar', eps_greedy=0.05, start_timesteps=40), _ring('mountaincar', n=512)
    _scores_against_host(agent, env, 'mountaincar', 2, 5, 'sac mountaincar, initialisation')
    for t in range(140):
        agent.iterate(env, buf, B, train=t >= 40)
    _scores_against_host(agent, env, 'mountaincar', 2, 5, 'sac mountaincar, after 100 training iterations')
    # an actor that reaches the goal: the evaluation loop leaves early (a loop that ran on would collect further rewards) ...
    _write_actor(agent, chase=True)
    scores, steps, starts = _scores_against_host(agent, env, 'mountaincar', 3, 7, 'sac mountaincar, chasing actor')
    assert np.all(steps < 200) and np.all(scores > 80.0) and np.all(scores < 100.0)
    assert np.all(starts[0, :, 1] == 0.0) and np.all(starts[0, :, 0] >= F32(-0.6)) and np.all(starts[0, :, 0] <= F32(-0.4))
    # ... and one that pushes right all the time: 999 steps of -0.1
    _write_actor(agent, chase=False)
    scores, steps, _ = _scores_against_host(agent, env, 'mountaincar', 2, 8, 'sac mountaincar, constant actor')
    assert np.all(steps == LIMIT) and np.all(np.abs(scores + 99.9) < 1e-4)
    _refused_episode_counts(agent, env)


# ---- 5. the ring wraps ------------------------------------------------------------------------------------------------------------------------
def test_ring_wrap_and_the_host_cursor():
    agent = _agent('sac')
    env, buf = _env(agent, eps_greedy=0.0, start_timesteps=1000), _ring(n=16)
    seen = []
    for t in range(40):
        agent.iterate(env, buf, B, train=False)
        if t in (15, 23):
            seen.append(buf.ring.clone())
    rec = env.state()
    assert int(rec['ring_ptr'][0]) == 8 and int(rec['ring_size'][0]) == 16 and buf.size_dev().cpu().tolist() == [16]
    assert not torch.equal(seen[0][:8], seen[1][:8]) and torch.equal(seen[0][8:], seen[1][8:])                # rows 0..7 were overwritten
    assert np.array_equal(buf.ring[0, :3].cpu().numpy(), buf.ring[15, 4:7].cpu().numpy())                   # the rollout wraps with the ring
    one = (np.ones(3, np.float32), np.full(1, 0.5, np.float32), np.ones(3, np.float32), -1.0, 0.0)
    with pytest.raises(RuntimeError, match='adopt_device_cursor'):
        buf.add(*one)
    buf.adopt_device_cursor()
    assert buf.ptr == 8 and buf.size == 16
    keep = buf.ring.clone()
    buf.add(*one)
    buf.flush()
    torch.cuda.synchronize()
    assert buf.ptr == 9 and buf.ring[8].cpu().tolist() == [1, 1, 1, 0.5, 1, 1, 1, -1, 0]
    assert torch.equal(buf.ring[:8], keep[:8]) and torch.equal(buf.ring[9:], keep[9:])
    agent.iterate(env, buf, B, train=False)                                         # the device takes the cursor again, behind the host's row
    assert int(env.state()['ring_ptr'][0]) == 10 and not torch.equal(buf.ring[9], keep[9])
    assert buf.ring[8].cpu().tolist() == [1, 1, 1, 0.5, 1, 1, 1, -1, 0]


# ---- 6. train() between iterate() calls -------------------------------------------------------------------------------------------------------
def test_two_chain_train_interleaves_with_iterate():
    """vlsac's default train() runs two chains on two streams and may still be in flight when it returns: iterate() finishes it first.  The
    twin (pipeline=False) sees the same rows and the same calls in the same order."""
    agent = _agent('vlsac')
    env, buf = _env(agent, eps_greedy=0.05, start_timesteps=70), _ring()
    twin, buf2 = _agent('vlsac', pipeline=False), _ring()
    fed = [0]

    def feed():                                                     # the twin's ring follows the device's
        rows = _rows(buf)
        upto = int(env.state()['nsteps'][0])
        for t in range(fed[0], upto):
            _add(buf2, rows[t], 3)
        fed[0] = upto

    for _ in range(70):
        agent.iterate(env, buf, B, train=False)
    feed()
    for _ in range(3):
        agent.train(buf, B)
        twin.train(buf2, B)
    assert agent._pending == 2                                      # the two-chain form, its last critic / actor pair still to be waited for
    for _ in range(3):
        a = agent.iterate(env, buf, B)
        feed()
        sg.assert_info_equal({k: float(v) for k, v in a.items()}, twin.train(buf2, B), 'iterate after train')
    assert not agent._pending
    agent.train(buf, B)
    twin.train(buf2, B)
    a = agent.iterate(env, buf, B)
    feed()
    sg.assert_info_equal({k: float(v) for k, v in a.items()}, twin.train(buf2, B), 'iterate after the second train')
    assert agent.steps == twin.steps == 8
    sg.assert_equal(sg.state(agent.core), sg.state(twin.core), 'interleaved')
    assert torch.equal(buf.ring.cpu(), buf2.ring.cpu())


# ---- 7. checkpoints ---------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_continues_bit_identically_and_carries_the_kind(tmp_path):
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.envs.device import DevicePendulumGroup
    agent = _agent('sac')
    env, buf = _env(agent, eps_greedy=0.05, start_timesteps=20), _ring(n=128)
    for _ in range(30):
        agent.iterate(env, buf, B, train=False)
    # trained state for the checkpoint, through train(): capturing a training graph counts one call in the noise counter (_warm), so the agent
    # that goes on and the one that is loaded both capture their iterate(train=True) graph below
    buf.adopt_device_cursor()
    assert buf.ptr == 30 and buf.size == 30
    for _ in range(5):
        agent.train(buf, B)
    path = str(tmp_path / 'agent.pt')
    agent.save(path, env=env)
    agent2 = _agent('sac')
    env2, buf2 = _env(agent2, eps_greedy=0.05, start_timesteps=20), _ring(n=128)
    agent2.load(path, env=env2)
    buf2.ring.copy_(buf.ring)
    buf2.ptr, buf2.size = buf.ptr, buf.size
    assert np.array_equal(env2.state(), env.state()) and env2.counters() == env.counters() == (30, 10) and agent2._ctr == agent._ctr
    for _ in range(5):
        sg.assert_info_equal(agent.iterate(env, buf, B), agent2.iterate(env2, buf2, B), 'after load')
    sg.assert_equal(sg.state(agent.core), sg.state(agent2.core), 'after load')
    assert np.array_equal(env2.state(), env.state()) and torch.equal(buf.ring, buf2.ring) and int(env.state()['nsteps'][0]) == 35
    # a checkpoint without an environment resets it; one of another kind, or of a group, is refused
    agent.save(path)
    agent2.load(path, env=env2)
    assert env2.counters()[0] == 0 and int(env2.state()['nsteps'][0]) == 0
    car = _agent('sac', 'mountaincar')
    with pytest.raises(RuntimeError, match='does not match this device environment'):
        _env(car, 'mountaincar').load_snapshot(env.snapshot())
    grp = SACSeedBatch([SEED], 3, 1, _host_env('pendulum').action_space, max_batch=B, hidden_dim=256)
    genv = DevicePendulumGroup(grp)
    with pytest.raises(RuntimeError, match='environment of a group'):
        env.load_snapshot(genv.snapshot())
    with pytest.raises(RuntimeError, match='environment of a single'):
        genv.load_snapshot(env.snapshot())


# ---- 8. refusals that need a real agent -------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    import bench
    from rlrep_amd._lib import lib
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    out = C.c_void_p()
    space = _host_env('pendulum').action_space
    grp = SACSeedBatch([0, 1], 3, 1, space, max_batch=B, hidden_dim=256)
    assert lib.rlrep_env_create(grp.core.h, 0, 0, C.byref(out)) == -1 and 'takes rlrep_group_env_create' in lib.rlrep_last_error().decode()
    wide = _agent('sac', S=17, A=6, space=bench.Space(6))
    assert lib.rlrep_env_create(wide.core.h, 0, 0, C.byref(out)) == -1 and '3 observations and 1 action' in lib.rlrep_last_error().decode()
    assert lib.rlrep_env_create(wide.core.h, 2, 0, C.byref(out)) == -1 and '2 observations and 1 action' in lib.rlrep_last_error().decode()
    assert not out.value
    agent, other = _agent('sac'), _agent('sac', seed=6)
    assert lib.rlrep_group_env_create(agent.core.h, 0, C.byref(out)) == -1 and 'not a seed group' in lib.rlrep_last_error().decode()
    env, buf = _env(agent), _ring(n=16)
    before = env.state()
    with pytest.raises(ValueError, match='another agent'):
        other.iterate(env, _ring(n=16), B)
    with pytest.raises(ValueError, match='another agent'):
        other.evaluate(env, 2)
    with pytest.raises(ValueError, match='sharded'):
        agent.iterate(env, _ring(n=16, shard=(0, 2)), B)
    with pytest.raises(ValueError, match='ReplayBuffer of 3 observations and 1 actions'):
        agent.iterate(env, _ring('mountaincar', n=16), B)
    with pytest.raises(RuntimeError, match='graph=False'):
        eager = _agent('sac', graph=False)
        eager.iterate(_env(eager), _ring(n=16), B)
    h, size = agent.core.h, C.c_void_p(buf.size_dev().data_ptr())
    assert lib.rlrep_env_step(h, env.h, None, 16, size, -2.0, 2.0, 0.0, 0, None) == -1 and 'env_step: null ring' in lib.rlrep_last_error().decode()
    assert lib.rlrep_env_step(h, env.h, C.c_void_p(buf.ring.data_ptr()), 0, size, -2.0, 2.0, 0.0, 0, None) == -1
    assert 'env_step: capacity 0' in lib.rlrep_last_error().decode()
    assert lib.rlrep_env_step(other.core.h, env.h, C.c_void_p(buf.ring.data_ptr()), 16, size, -2.0, 2.0, 0.0, 0, None) == -1
    assert 'env_step: the environment was created for another agent' in lib.rlrep_last_error().decode()
    assert lib.rlrep_env_evaluate(other.core.h, env.h, 4, 0, C.c_void_p(buf.ring.data_ptr()), None) == -1 and 'another agent' in lib.rlrep_last_error().decode()
    rec = env.state()
    assert lib.rlrep_env_state(env.h, 0, C.c_void_p(rec.ctypes.data), rec.nbytes - 1, 0, None) == -1 and 'holds 256 bytes' in lib.rlrep_last_error().decode()
    assert lib.rlrep_env_state(env.h, 2, C.c_void_p(rec.ctypes.data), 0, 1, None) == -1                  # the start states are read-only
    assert np.array_equal(env.state(), before) and env.counters() == (0, 0)         # nothing was launched


# ---- 9. launcher ------------------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_the_device_loop(tmp_path):
    import json
    from rlrep_amd import main
    from rlrep_amd.envs.device import RECORD_DTYPE
    argv = ['--alg', 'vlsac', '--env', 'Pendulum-v1', '--device-loop', '--max_timesteps', '450', '--start_timesteps', '150', '--eval_freq', '150',
            '--eval_episodes', '2', '--batch_size', '64', '--save_model', '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert agent.steps == 300 and agent.ALG == 'vlsac'
    root = tmp_path / 'Pendulum-v1' / 'vlsac' / '0' / '0'
    rows = [json.loads(l) for l in open(root / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [300, 450]
    keys = {'step', 'info/evaluation', 'steps_per_sec'} | {f'info/{k}' for k in agent.FEATURE_KEYS + agent.CRITIC_KEYS + agent.ACTOR_KEYS}
    assert 'info/q1_loss' in keys and 'info/actor_loss' in keys and 'info/alpha' in keys and 'info/vae_loss' in keys
    assert all(set(row) == keys for row in rows), (keys, [set(row) for row in rows])          # what the host loop writes for this agent
    assert all(np.isfinite(v) for row in rows for v in row.values())
    assert len(evaluations) == 4 and all(np.isfinite(v) and v < 0 for v in evaluations)
    snap = torch.load(root / 'agent.pt')
    rec = snap['device_env']['records'].numpy().view(RECORD_DTYPE)
    assert snap['device_env']['t_global'] == 450 and snap['device_env']['form'] == 'single' and snap['device_env']['kind'] == 0
    assert int(rec['nsteps'][0]) == 450 and int(rec['episodes_done'][0]) == 2 and snap['steps'] == 300
