"""The simulator loop as one graph replay (csrc/actor_tile.hip actor_tile_kernel_ctl, csrc/elementwise.hip
replay_add_cols_kernel_ctl, envs/sim_loop.py SimLoop, SACAgent.iterate_sim, TorchPendulum(capturable=True)) on the GPU.

Everything is exact.  The act form gives the bytes of act_device(explore=True) of a same-seed twin at the same counter, and with the
exploration mix the bytes of tests/sim_loop_reference.py applied to the twin's actions; the append form leaves what add_device leaves on a
twin ring; 5 warm-up and 20 training iterations of iterate_sim end bit-identical to a twin that runs the eager route (act_device, the restated
mix, a twin simulator stepped eagerly, add_device, train()).  Hidden widths are 64.  Reads nothing outside the repository."""
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
import sim_loop_reference as ref  # noqa: E402
from test_device_env_single import _agent  # noqa: E402

DEV = 'cuda'
SEED = 5
B = 64
CONFIGS = {                                 # name: (alg, S, A, constructor extras)
    'sac_pendulum': ('sac', 3, 1, dict(hidden_dim=64)),
    'sac_s17_a6': ('sac', 17, 6, dict(hidden_dim=64)),            # A = 6: u_j from two Philox blocks; K = 17
    'vlsac_f64': ('vlsac', 3, 1, dict(hidden_dim=64, feature_dim=64)),
}
NS = (1, 15, 16, 17, 33)                    # below, at and above one 16-row tile; several workgroups; a last tile of one row


def _make(cfg, **extra):
    alg, S, A, kw = CONFIGS[cfg]
    return _agent(alg, S=S, A=A, space=bench.Space(A) if A != 1 else None, seed=SEED, **dict(kw, **extra)), S, A


class _Still(object):
    """a simulator that only holds observations (the kernel tests launch the two forms themselves)"""

    def __init__(self, obs):
        self.obs = obs

    def step_(self, actions):
        raise AssertionError('not stepped')


def _loop(agent, obs, eps=0.0, start=0):
    from rlrep_amd.envs.sim_loop import SimLoop
    return SimLoop(agent, _Still(obs), eps_greedy=eps, start_timesteps=start)


def _ctl(loop):
    torch.cuda.synchronize()
    return loop.ctl.cpu().numpy().tolist()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the act form --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_act_form_equals_act_device_and_the_restated_mix(cfg):
    from rlrep_amd._lib import lib
    from rlrep_amd.envs import sim_loop as sl
    agent, S, A = _make(cfg)
    twin = _make(cfg)[0]
    lo, hi = agent.action_range
    gen = torch.Generator(device=DEV).manual_seed(7)
    CAP, PTR, SIZE = 40, 30, 35
    mixed = 0
    for k, N in enumerate(NS):
        obs = torch.randn(N, S, device=DEV, generator=gen)
        calls, it = 100 + 7 * k, 3 + k
        twin._ctr = calls
        want = twin.act_device(obs, explore=True).cpu().numpy()
        # (eps_greedy, start_timesteps, t_global): the policy alone; half the rows mixed; warm-up
        for eps, start, t in ((0.0, 0, 0), (0.5, 0, 5 * N), (0.0, 8 * N, 7 * N)):
            loop = _loop(agent, obs, eps, start)
            loop.set_counters(t, calls, it)
            loop.set_cursor(PTR, [SIZE])
            out = torch.full((N, A), 9.0, device=DEV)
            n0 = lib.rlrep_launch_counter()
            loop.act(obs, out, CAP)
            assert lib.rlrep_launch_counter() - n0 == 1
            warm = t < start
            exp, taken = ref.mix(want, SEED, it, warm, eps, lo, hi)
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(exp)), (cfg, N, eps, start)
            if eps == 0.0 and not warm:
                assert not taken.any() and np.array_equal(_bits(exp), _bits(want))
            if warm:
                assert taken.all()
            mixed += int(taken.sum()) if eps == 0.5 else 0
            # the rule: what every workgroup read stands as it stood; one thread moved the cursor by N
            w = _ctl(loop)
            assert (w[sl.CALLS], w[sl.T_GLOBAL], w[sl.ITER]) == (calls, t, it), (cfg, N, w)
            assert w[sl.START] == PTR and w[sl.NEXT_PTR] == (PTR + N) % CAP and w[sl.SIZE] == min(SIZE + N, CAP) and w[sl.WARM] == int(warm), (cfg, N, w)
    assert 0 < mixed < sum(NS)              # eps = 0.5 took some rows and left some
    assert twin._ctr == 100 + 7 * (len(NS) - 1) + NS[-1]


def test_act_form_refusals():
    agent, S, A = _make('sac_pendulum')
    obs = torch.zeros(17, S, device=DEV)
    loop = _loop(agent, obs)
    out = torch.zeros(17, A, device=DEV)
    with pytest.raises(RuntimeError, match='act_device_ctl.*max_size'):
        loop.act(obs, out, 16)                          # a ring smaller than the launch's rows
    from rlrep_amd.envs.sim_loop import SimLoop
    with pytest.raises(ValueError, match='multiple'):
        SimLoop(agent, _Still(obs), start_timesteps=18)
    with pytest.raises(ValueError, match='sim.obs'):
        SimLoop(agent, _Still(torch.zeros(17, S)))
    with pytest.raises(ValueError, match='sim.obs'):
        SimLoop(agent, _Still(torch.zeros(17, S + 1, device=DEV)))


# ---- 2. the append form -----------------------------------------------------------------------------------------------------------------------
def test_append_form_equals_add_device_on_a_twin_ring():
    """a ring of 95 rows, N = 40 three times (the third wraps); the first iteration is a warm-up one"""
    from rlrep_amd._lib import lib
    from rlrep_amd.envs import sim_loop as sl
    from rlrep_amd.utils.buffer import ReplayBuffer
    agent, S, A = _make('sac_pendulum')
    N, CAP = 40, 95
    buf, buf2 = ReplayBuffer(S, A, max_size=CAP), ReplayBuffer(S, A, max_size=CAP)
    gen = torch.Generator(device=DEV).manual_seed(3)
    obs = torch.randn(N, S, device=DEV, generator=gen)
    loop = _loop(agent, obs, 0.0, N)
    buf.collect_on_device(loop)
    loop.set_counters(0, 11)
    scratch = torch.zeros(N, A, device=DEV)
    for k in range(3):
        s, a, s2 = (torch.randn(N, w, device=DEV, generator=gen) for w in (S, A, S))
        r, d = torch.randn(N, device=DEV, generator=gen), (torch.rand(N, device=DEV, generator=gen) < 0.3).to(torch.float32)
        with pytest.raises(RuntimeError, match='adopt_device_cursor'):
            buf.add_device(s, a, s2, r, d)              # the loop owns the cursor
        loop.act(obs, scratch, CAP)
        n0 = lib.rlrep_launch_counter()
        loop.append(buf, s, a, s2, r, d)
        assert lib.rlrep_launch_counter() - n0 == 1
        start2 = buf2.ptr
        buf2.add_device(s, a, s2, r, d)
        w = _ctl(loop)
        assert w[sl.START] == start2 and w[sl.NEXT_PTR] == buf2.ptr and w[sl.SIZE] == buf2.size, (k, w)
        assert torch.equal(buf.ring, buf2.ring), k
        assert buf._size_dev.cpu().tolist() == buf2._size_dev.cpu().tolist() == [buf2.size]
        # calls stands still in the warm-up iteration and moves by N otherwise; steps and iterations always count
        assert (w[sl.CALLS], w[sl.T_GLOBAL], w[sl.ITER]) == (11 + N * k, N * (k + 1), k + 1), (k, w)
    assert buf2.ptr == (3 * N) % CAP and buf2.size == CAP
    # the cursor goes back to the host: add_device continues at the next row
    rec = loop.state()
    assert int(rec['ring_ptr'][0]) == buf2.ptr and int(rec['ring_size'][0]) == CAP
    buf.adopt_device_cursor()
    assert (buf.ptr, buf.size) == (buf2.ptr, buf2.size)
    s, a, s2 = (torch.randn(7, w, device=DEV, generator=gen) for w in (S, A, S))
    r, d = torch.randn(7, device=DEV, generator=gen), torch.zeros(7, device=DEV)
    buf.add_device(s, a, s2, r, d)
    buf2.add_device(s, a, s2, r, d)
    assert torch.equal(buf.ring, buf2.ring) and (buf.ptr, buf.size) == (buf2.ptr, buf2.size)
    assert buf._size_dev.cpu().tolist() == buf2._size_dev.cpu().tolist()


# ---- 3. the loop ------------------------------------------------------------------------------------------------------------------------------
def _sims(N, at_step):
    """two capturable simulators from the same generator seed, `at_step` steps into their episodes"""
    from rlrep_amd.envs.torch_pendulum import TorchPendulum
    out = []
    for _ in range(2):
        sim = TorchPendulum(N, DEV, seed=11, capturable=True)
        sim.reset()
        sim.steps.fill_(at_step)
        out.append(sim)
    assert torch.equal(out[0].obs, out[1].obs)
    return out


@pytest.mark.parametrize('cfg', ['sac_pendulum', 'vlsac_f64'])
def test_loop_equals_the_eager_route_bit_for_bit(cfg):
    """5 warm-up and 20 training iterations, N = 16, B = 64, a ring of 512 rows, eps_greedy 0.25; the episodes end (and restart from the
    simulator's generator) in the 13th iteration, inside the graph"""
    from rlrep_amd.envs.sim_loop import SimLoop
    from rlrep_amd.utils.buffer import ReplayBuffer
    N, WARM, TRAIN, EPS = 16, 5, 20, 0.25
    agent, S, A = _make(cfg)
    twin = _make(cfg, pipeline=False)[0]
    lo, hi = agent.action_range
    sim, sim2 = _sims(N, 187)
    buf, buf2 = ReplayBuffer(S, A, max_size=512), ReplayBuffer(S, A, max_size=512)
    loop = SimLoop(agent, sim, eps_greedy=EPS, start_timesteps=WARM * N)
    infos = []
    for it in range(WARM + TRAIN):
        out = agent.iterate_sim(loop, buf, B, train=it >= WARM)
        if it < WARM:
            assert out is None
        else:
            infos.append({k: float(v) for k, v in out.items()})
        if it == WARM - 1:
            assert agent._sim_launches == 2 and agent._sim_captures == 1       # the warm-up graph: the two forms alone
    assert agent._sim_captures == 2                                             # one capture per form
    mixed = 0
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
        if not warm:
            sg.assert_info_equal(infos[it - WARM], {k: float(v) for k, v in twin.train(buf2, B).items()}, (cfg, it))
    assert 0 < mixed < TRAIN * N
    torch.cuda.synchronize()
    assert torch.equal(buf.ring, buf2.ring)
    assert buf._size_dev.cpu().tolist() == buf2._size_dev.cpu().tolist() == [(WARM + TRAIN) * N]
    sg.assert_equal(sg.state(agent.core), sg.state(twin.core), cfg)
    assert agent.steps == twin.steps == TRAIN and agent._ctr == twin._ctr
    assert loop.counters() == ((WARM + TRAIN) * N, agent._ctr, WARM + TRAIN) == (loop.t_global, loop.calls, loop.iter)
    for k in ('th', 'thd', 'obs', 'ep_return', 'last_return', 'steps', 'episodes_dev'):
        assert torch.equal(getattr(sim, k), getattr(sim2, k)), k
    assert sim.episodes_dev.tolist() == [1] * N and sim.steps.tolist() == [12] * N
    assert agent._sim_launches == twin._graph_launches + 2, (cfg, agent._sim_launches, twin._graph_launches)
    assert not torch.equal(buf.ring[13 * N + 1, :S], buf.ring[12 * N + 1, S + A:2 * S + A])      # the restart broke the rollout there
    assert torch.equal(buf.ring[15 * N + 1, :S], buf.ring[14 * N + 1, S + A:2 * S + A])


# ---- 4. buffers -------------------------------------------------------------------------------------------------------------------------------
def test_nstep_buffer_and_refusals():
    from nstep_reference import nstep_slot
    from rlrep_amd.envs.sim_loop import SimLoop
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from test_nstep import _assert_slot, _slot
    N, RING = 16, 95
    agent, S, A = _make('sac_pendulum')
    sim = _sims(N, 0)[0]
    loop = SimLoop(agent, sim, eps_greedy=0.1)
    with pytest.raises(RuntimeError, match='PrioritizedReplayBuffer'):
        agent.iterate_sim(loop, PrioritizedReplayBuffer(S, A, max_size=RING), B)
    with pytest.raises(ValueError, match='n_stride'):
        agent.iterate_sim(loop, ReplayBuffer(S, A, max_size=RING, n_step=3, n_stride=1), B)
    with pytest.raises(ValueError, match='another agent'):
        _make('sac_pendulum')[0].iterate_sim(loop, ReplayBuffer(S, A, max_size=RING), B)
    with pytest.raises(RuntimeError, match='graph=False'):
        other = _make('sac_pendulum', graph=False)[0]
        other.iterate_sim(SimLoop(other, sim), ReplayBuffer(S, A, max_size=RING), B)
    buf = ReplayBuffer(S, A, max_size=RING, n_step=3, n_stride=N)
    for k in range(8):                      # 128 rows into a ring of 95: the wrap falls inside an iteration
        agent.iterate_sim(loop, buf, B)
        torch.cuda.synchronize()
        ring = buf.ring.cpu().numpy()
        size = min(N * (k + 1), RING)
        idx = agent._bufs['pool_idx'].cpu().numpy().astype(np.int64)[:B]
        want = nstep_slot(ring, idx, size, 3, N, np.float32(agent.discount), S, A)
        _assert_slot(_slot(agent.core, B), want, S, ('iterate_sim slot', k), xf2_tail=False)
    assert want['m'].max() == 3
    assert agent._sim_captures == 1 and agent.steps == 8


# ---- 5. launcher ------------------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_the_simulator_loop_as_one_graph(tmp_path, monkeypatch):
    import json
    from rlrep_amd import main
    from rlrep_amd.utils import buffer
    from test_host_envs import _keep_instances
    made = _keep_instances(monkeypatch, buffer, 'ReplayBuffer')
    argv = ['--alg', 'sac', '--env', 'Pendulum-v1', '--torch-envs', '8', '--sim-graph', '--max_timesteps', '320', '--start_timesteps', '160',
            '--eval_freq', '320', '--batch_size', '64', '--eval_episodes', '2', '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert agent.steps == 20 and agent._sim_captures == 2                   # 40 iterations of 8 steps, 20 of them warm-up; one capture per form
    assert agent._ctr >= 20 * 8                                             # 8 exploring rows per training iteration
    assert len(made) == 1 and made[0]._device_env is not None              # the loop owns the cursor
    made[0].adopt_device_cursor()
    assert made[0].size == 320 and made[0].ptr == 0 and made[0].size_dev().cpu().tolist() == [320]
    assert len(evaluations) == 1 and np.isfinite(evaluations[0]) and evaluations[0] < 0
    rows = [json.loads(l) for l in open(tmp_path / 'Pendulum-v1' / 'sac' / '0' / '0' / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [320] and all(np.isfinite(v) for row in rows for v in row.values())
    assert 'info/q_loss' in rows[0] and 'info/actor_loss' in rows[0] and rows[0]['steps_per_sec'] > 0
