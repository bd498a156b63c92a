"""Vector host environments on the GPU (csrc/elementwise.hip select_action_kernel_n / _grp_n, SACAgent.select_actions,
SeedBatchMixin.select_actions, add_batch, util.eval_policy_vec, main.py --host-envs): every row of one launch is bit for bit the single call
for that observation at that call counter, for single agents and for seed groups (retired members untouched); a loop of select_actions +
add_batch + train() ends bit-identical to a twin's E select_action + E add + train(); a lockstep evaluation equals the sequential one per
episode; the launcher runs.  The kernels include the body the single call runs, so every comparison is exact: no tolerance.  Reads nothing
outside the repository."""
import ctypes as C
import json
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
from test_device_env_single import _agent, _env, B, RING  # noqa: E402

CONFIGS = {                                 # name: (alg, S, A, constructor extras)
    'sac_pendulum': ('sac', 3, 1, {}),
    'sac_halfcheetah': ('sac', 17, 6, {}),              # A = 6: both Box-Muller halves of a Philox block, and a second block
    'vlsac_f64': ('vlsac', 3, 1, dict(feature_dim=64)),
}


def _make(cfg, seed=5):
    alg, S, A, extra = CONFIGS[cfg]
    return _agent(alg, S=S, A=A, space=bench.Space(A) if A != 1 else None, seed=seed, **extra), S, A


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. rows equal single calls ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_rows_equal_single_calls_bit_for_bit(cfg):
    from rlrep_amd._lib import lib
    agent, S, A = _make(cfg)
    twin, _, _ = _make(cfg)
    rng = np.random.RandomState(7)
    for E in (1, 3, 5):
        for explore in (False, True, True):
            obs = rng.randn(E, S).astype(np.float32)
            ctr = agent._ctr
            n0 = lib.rlrep_launch_counter()
            acts = agent.select_actions(obs, explore=explore)
            assert lib.rlrep_launch_counter() - n0 == 1                     # ONE launch
            assert acts.shape == (E, A) and acts.dtype == np.float32
            want = np.stack([twin.select_action(obs[e], explore=explore) for e in range(E)])
            assert np.array_equal(_bits(acts), _bits(want)), (cfg, E, explore, acts, want)
            assert agent._ctr == twin._ctr == ctr + (E if explore else 0)
            if explore and E > 1:
                assert len({a.tobytes() for a in agent.select_actions(np.repeat(obs[:1], E, 0), explore=True)}) == E      # a draw per row
                twin._ctr += E
    assert sorted(agent._sel_n) == [1, 3, 5]                                # pinned buffers kept per E


def test_256_rows_in_one_launch():
    from rlrep_amd._lib import lib
    agent, S, A = _make('sac_halfcheetah')
    twin, _, _ = _make('sac_halfcheetah')
    obs = np.random.RandomState(8).randn(256, S).astype(np.float32)
    ctr = agent._ctr
    n0 = lib.rlrep_launch_counter()
    acts = agent.select_actions(obs, explore=True)
    assert lib.rlrep_launch_counter() - n0 == 1
    assert acts.shape == (256, A) and np.all(np.isfinite(acts)) and np.all(np.abs(acts) <= 1.0) and agent._ctr == ctr + 256
    for e in (0, 255):
        twin._ctr = ctr + e
        assert np.array_equal(_bits(twin.select_action(obs[e], explore=True)), _bits(acts[e])), e
    for bad in (np.zeros((257, S), np.float32), np.zeros((0, S), np.float32), np.zeros((4, S + 1), np.float32), np.zeros(S, np.float32)):
        with pytest.raises(ValueError, match='select_actions'):
            agent.select_actions(bad)
    assert agent._ctr == ctr + 256


def test_one_row_gives_the_bytes_of_the_existing_entry_point_and_handles_are_checked():
    """rows == 1 through the C ABI against rlrep_select_action; a group handle given to the single form, a single agent's to the group form
    and unpinned group buffers are refused by name before anything is launched."""
    from rlrep_amd._lib import lib
    agent, S, A = _make('sac_halfcheetah')
    grp = sg.group('sac_halfcheetah_b256', (3, 11))
    obs = torch.from_numpy(np.random.RandomState(9).randn(2, 2, S).astype(np.float32)).pin_memory()
    a_old, a_new = torch.zeros(1, A).pin_memory(), torch.zeros(1, A).pin_memory()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for explore in (0, 1):
        assert lib.rlrep_select_action(agent.core.h, ptr(obs), 1, explore, 5, 9 << 20, -1.0, 1.0, ptr(a_old), 1, None) == 0
        assert lib.rlrep_select_action_n(agent.core.h, ptr(obs), 1, 1, explore, 5, 9 << 20, -1.0, 1.0, ptr(a_new), 1, None) == 0
        torch.cuda.synchronize()
        assert a_old.numpy().tobytes() == a_new.numpy().tobytes() and np.any(a_old.numpy() != 0.0)
    g_old, g_new = torch.zeros(2, 1, A).pin_memory(), torch.zeros(2, 1, A).pin_memory()
    one = obs[:, :1].contiguous().pin_memory()
    assert lib.rlrep_group_select_action(grp.core.h, ptr(one), 1, 9 << 20, -1.0, 1.0, ptr(g_old), None) == 0
    assert lib.rlrep_group_select_action_n(grp.core.h, ptr(one), 1, 1, 9 << 20, -1.0, 1.0, ptr(g_new), None) == 0
    torch.cuda.synchronize()
    assert g_old.numpy().tobytes() == g_new.numpy().tobytes() and np.any(g_old.numpy() != 0.0)
    n0 = lib.rlrep_launch_counter()
    acts = torch.zeros(2, 2, A).pin_memory()
    assert lib.rlrep_select_action_n(grp.core.h, ptr(obs), 1, 2, 0, 5, 0, -1.0, 1.0, ptr(acts), 1, None) == -1
    msg = lib.rlrep_last_error().decode()
    assert msg.startswith('select_action_n:') and 'seed group' in msg, msg
    assert lib.rlrep_group_select_action_n(agent.core.h, ptr(obs), 2, 0, 0, -1.0, 1.0, ptr(acts), None) == -1
    msg = lib.rlrep_last_error().decode()
    assert msg.startswith('group_select_action_n:') and 'not a seed group' in msg, msg
    pageable_obs, pageable_act = torch.zeros(2, 2, S), torch.zeros(2, 2, A)
    for o, a, what in ((pageable_obs, acts, 'observations'), (obs, pageable_act, 'action buffer')):
        assert lib.rlrep_group_select_action_n(grp.core.h, ptr(o), 2, 0, 0, -1.0, 1.0, ptr(a), None) == -1
        msg = lib.rlrep_last_error().decode()
        assert msg.startswith('group_select_action_n:') and what in msg and 'pinned' in msg, msg
    assert lib.rlrep_launch_counter() == n0 and not np.any(acts.numpy())


# ---- 2. groups --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wl, seeds', [('sac_pendulum_b64', (3, 11, 42)), ('ctrlsac_halfcheetah_f256_b256', (3, 11))])
def test_group_rows_equal_the_standalone_agents_single_calls(wl, seeds):
    from rlrep_amd._lib import lib
    _, S, A, Bw, _ = sg.dims(wl)
    R, E = len(seeds), 3
    grp = sg.group(wl, seeds)
    rings, alone_rings = sg.rings(wl, range(R))
    alone = [sg.standalone(wl, s) for s in seeds]
    for _ in range(3):
        grp.train(rings, Bw)
        for r, a in enumerate(alone):
            a.train(alone_rings[r], Bw)
    rng = np.random.RandomState(5)
    for explore in (False, True, True):
        obs = rng.randn(R, E, S).astype(np.float32)
        n0 = lib.rlrep_launch_counter()
        acts = grp.select_actions(obs, explore=explore)
        assert lib.rlrep_launch_counter() - n0 == 1
        assert acts.shape == (R, E, A)
        for r, a in enumerate(alone):
            for e in range(E):
                want = a.select_action(obs[r, e], explore=explore)
                assert np.array_equal(_bits(acts[r, e]), _bits(want)), (wl, explore, r, e)
            assert a._ctr == grp._ctr
    # a retired member: its rows are zeros, its observations are not read and its block is not written
    grp.retire_members([1])
    block = sg.member_bytes(grp, 1)
    obs = rng.randn(R, E, S).astype(np.float32)
    obs[1] = np.nan
    for explore in (True, False):
        acts = grp.select_actions(obs, explore=explore)
        assert not np.any(acts[1]) and np.all(np.isfinite(acts))
        for r in [q for q in range(R) if q != 1]:
            for e in range(E):
                assert np.array_equal(_bits(acts[r, e]), _bits(alone[r].select_action(obs[r, e], explore=explore))), (wl, 'retired', r, e)
            assert alone[r]._ctr == grp._ctr
    assert torch.equal(sg.member_bytes(grp, 1), block)


# ---- 3. loop equivalence ----------------------------------------------------------------------------------------------------------------------
E_LOOP, PREFILL, ITERS = 3, 40, 25          # 40 + 75 rows through a ring of 95: batch 19 wraps it (rows 94, 0, 1)


def _synthetic(rng, lead, S):
    """what the environments answer: next states, rewards, done flags (one in five)"""
    return (np.asarray(rng.randn(*lead, S), np.float32), np.asarray(rng.randn(*lead), np.float32),
            np.asarray(rng.uniform(size=lead) < 0.2, np.float32))


@pytest.mark.parametrize('cfg', ['sac_pendulum', 'vlsac_f64'])
def test_vector_loop_equals_the_loop_of_single_calls(cfg):
    from rlrep_amd.utils.buffer import ReplayBuffer
    agents = [_make(cfg)[0] for _ in range(2)]
    _, S, A, _ = CONFIGS[cfg]
    bufs = [ReplayBuffer(S, A, max_size=RING) for _ in range(2)]
    rng = np.random.RandomState(11)
    for _ in range(PREFILL):
        s, a, (s2, r, d) = rng.randn(S), rng.uniform(-1, 1, A), _synthetic(rng, (), S)
        for buf in bufs:
            buf.add(s, a, s2, r, d)
    states = rng.randn(E_LOOP, S).astype(np.float32)
    for it in range(ITERS):
        s2, r, d = _synthetic(rng, (E_LOOP,), S)
        acts = agents[0].select_actions(states, explore=True)
        bufs[0].add_batch(states, acts, s2, r, d)
        info = agents[0].train(bufs[0], B)
        for e in range(E_LOOP):
            a = agents[1].select_action(states[e], explore=True)
            assert np.array_equal(_bits(a), _bits(acts[e])), (cfg, it, e)
            bufs[1].add(states[e], a, s2[e], r[e], d[e])
        sg.assert_info_equal(info, agents[1].train(bufs[1], B), (cfg, it))
        states = s2
    sg.assert_equal(sg.state(agents[0].core), sg.state(agents[1].core), cfg)
    assert agents[0]._ctr == agents[1]._ctr and (bufs[0].ptr, bufs[0].size) == (bufs[1].ptr, bufs[1].size) == ((PREFILL + 75) % RING, RING)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0].ring, bufs[1].ring)
    if cfg != 'sac_pendulum':
        return
    # the call counters are reconciled: a device environment continues from them
    agent, twin, buf = agents[0], agents[1], bufs[0]
    env = _env(agent, eps_greedy=0.0, start_timesteps=0)
    ptr = buf.ptr
    assert agent.iterate(env, buf, B, train=False) is None
    torch.cuda.synchronize()
    row = buf.ring[ptr].cpu().numpy()
    assert np.array_equal(_bits(twin.select_action(row[:3], explore=True)), _bits(row[3:4])) and env.counters() == (1, agent._ctr) and twin._ctr == agent._ctr


def test_vector_loop_of_a_group_equals_the_loop_of_single_calls():
    from rlrep_amd.envs.device import DevicePendulumGroup
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    wl, seeds, R, S, A = 'sac_pendulum_b64', (3, 11), 2, 3, 1
    grps = [sg.group(wl, seeds) for _ in range(2)]
    bufs = [ReplayBufferGroup(R, S, A, max_size=RING) for _ in range(2)]
    rng = np.random.RandomState(12)
    for _ in range(PREFILL):
        s, a, (s2, r, d) = rng.randn(R, S), rng.uniform(-1, 1, (R, A)), _synthetic(rng, (R,), S)
        for buf in bufs:
            buf.add(s, a, s2, r, d)
    states = rng.randn(R, E_LOOP, S).astype(np.float32)
    for it in range(ITERS):
        s2, r, d = _synthetic(rng, (R, E_LOOP), S)
        acts = grps[0].select_actions(states, explore=True)
        bufs[0].add_batch(states, acts, s2, r, d)
        infos = grps[0].train(bufs[0], B)
        for e in range(E_LOOP):
            a = grps[1].select_action(states[:, e], explore=True)
            assert np.array_equal(_bits(a), _bits(acts[:, e])), (it, e)
            bufs[1].add(states[:, e], a, s2[:, e], r[:, e], d[:, e])
        twin_infos = grps[1].train(bufs[1], B)
        for m in range(R):
            sg.assert_info_equal(infos[m], twin_infos[m], (it, m))
        states = s2
    for m in range(R):
        sg.assert_equal(sg.state(grps[0]._members[m]), sg.state(grps[1]._members[m]), m)
    assert grps[0]._ctr == grps[1]._ctr and (bufs[0].ptr, bufs[0].sizes) == (bufs[1].ptr, bufs[1].sizes) == ((PREFILL + 75) % RING, [RING] * R)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0].rings, bufs[1].rings)
    # the call counters are reconciled: a device environment continues from them
    grp, twin, buf = grps[0], grps[1], bufs[0]
    env = DevicePendulumGroup(grp, eps_greedy=0.0, start_timesteps=0)
    ptr = buf.ptr
    assert grp.iterate(env, buf, B, train=False) is None
    torch.cuda.synchronize()
    rows = buf.rings[:, ptr].cpu().numpy()
    assert np.array_equal(_bits(twin.select_action(rows[:, :3], explore=True)), _bits(rows[:, 3:4])) and env.counters() == (1, grp._ctr)


# ---- 4. evaluation ----------------------------------------------------------------------------------------------------------------------------
def test_lockstep_evaluation_equals_the_sequential_one_per_episode():
    from rlrep_amd import envs
    from rlrep_amd.utils import util
    from test_host_envs_cpu import _sequential
    agent, _, _ = _make('sac_pendulum')
    E, episodes = 3, 4
    want, lengths = _sequential(agent, [envs.make('Pendulum-v1', seed=30 + i) for i in range(E)], episodes)
    ctr = agent._ctr
    got = util.eval_policy_vec(agent, [envs.make('Pendulum-v1', seed=30 + i) for i in range(E)], episodes)
    assert got.returns == want and float(got) == float(np.mean(want)) and lengths == [200] * episodes and agent._ctr == ctr
    assert len(set(want)) == episodes and all(np.isfinite(w) and w < 0 for w in want)


# ---- 5. launcher ------------------------------------------------------------------------------------------------------------------------------
ARGV = ['--alg', 'sac', '--env', 'Pendulum-v1', '--host-envs', '4', '--max_timesteps', '400', '--start_timesteps', '200', '--eval_freq', '200',
        '--batch_size', '64', '--eval_episodes', '2']


def _keep_instances(monkeypatch, module, name):
    """every `name` the launcher builds"""
    made = []
    cls = getattr(module, name)

    class Kept(cls):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(module, name, Kept)
    return made


def test_launcher_runs_several_host_environments(tmp_path, monkeypatch):
    from rlrep_amd import main
    from rlrep_amd.utils import buffer
    made = _keep_instances(monkeypatch, buffer, 'ReplayBuffer')
    agent, evaluations = main.run(ARGV + ['--log_root', str(tmp_path)])
    assert agent.steps == 50                                                # 100 iterations of 4 steps, 50 of them warm-up
    assert len(made) == 1 and made[0].size == 400 and made[0].ptr == 0
    assert agent._ctr >= 50 * 4                                             # a select_actions of 4 rows per training iteration
    assert len(evaluations) == 3 and all(np.isfinite(v) and v < 0 for v in evaluations)         # the initial one and two more
    assert all(len(v.returns) == 2 for v in evaluations)
    rows = [json.loads(l) for l in open(tmp_path / 'Pendulum-v1' / 'sac' / '0' / '0' / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [400] and all(np.isfinite(v) for row in rows for v in row.values())
    assert 'info/q_loss' in rows[0] and 'info/actor_loss' in rows[0] and rows[0]['steps_per_sec'] > 0


def test_launcher_runs_several_host_environments_per_seed(tmp_path, monkeypatch):
    from rlrep_amd import main
    from rlrep_amd.utils import buffer_group
    made = _keep_instances(monkeypatch, buffer_group, 'ReplayBufferGroup')
    grp, evaluations = main.run(ARGV + ['--seeds', '0,1', '--log_root', str(tmp_path)])
    assert grp.R == 2 and grp.steps == 50 and [len(e) for e in evaluations] == [3, 3]
    assert len(made) == 1 and made[0].sizes == [400, 400] and made[0].ptr == 0
    assert all(np.isfinite(v) and v < 0 for e in evaluations for v in e) and evaluations[0] != evaluations[1]
    for seed in (0, 1):
        rows = [json.loads(l) for l in open(tmp_path / 'Pendulum-v1' / 'sac' / '0' / str(seed) / 'metrics.jsonl')]
        assert [row['step'] for row in rows] == [400] and all(np.isfinite(v) for row in rows for v in row.values())
