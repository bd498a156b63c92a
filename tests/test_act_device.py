"""Acting on device-resident observation batches and appending device transitions (csrc/actor_tile.hip actor_tile_kernel / _grp,
csrc/elementwise.hip replay_add_cols_kernel / _grp, SACAgent.act_device, SeedBatchMixin.act_device, ReplayBuffer.add_device,
ReplayBufferGroup.add_device, envs/torch_pendulum.py, main.py --torch-envs).

Against the existing path (select_actions, one workgroup per row) the bar is the project's parity bar, 1e-4 absolute: both sides are fp32 with
different summation orders.  Everything else is exact: a row's action does not depend on the batch it travels in, a group member's plane is
the standalone agent's, add_device leaves the bytes add_batch + flush leave, and a loop fed through add_device ends bit-identical to one fed
the same rows through the host.  Reads nothing outside the repository."""
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
    'sac_pendulum': ('sac', 3, 1, {}),                  # K = 3 and 2A = 2: neither a multiple of 4, one partial column tile
    'sac_halfcheetah': ('sac', 17, 6, {}),              # K = 17, 2A = 12; A = 6: both Box-Muller halves of a Philox block, and a second block
    'vlsac_f64': ('vlsac', 3, 1, dict(feature_dim=64)),
    'sac_h70': ('sac', 5, 3, dict(hidden_dim=70)),      # Ha = 70: no multiple of 4 (4-byte weight loads over two 64-wide inner steps), 5 column tiles
    'sac_h1024': ('sac', 3, 1, dict(hidden_dim=1024)),  # 132 KB of LDS: above the default dynamic limit of a launch
}
NS = (1, 15, 16, 17, 33, 257)               # below, at and above one 16-row tile; several workgroups; a last tile of one row
BAR = 1e-4                                  # README: "~1e-6 (bar: 1e-4)"
DEV = 'cuda'


def _make(cfg, seed=5, **extra):
    alg, S, A, kw = CONFIGS[cfg]
    return _agent(alg, S=S, A=A, space=bench.Space(A) if A != 1 else None, seed=seed, **dict(kw, **extra)), S, A


@pytest.fixture(scope='module')
def twins():
    """per configuration: (agent, its same-seed twin, S, A), built once"""
    made = {}

    def get(cfg):
        if cfg not in made:
            a, S, A = _make(cfg)
            made[cfg] = (a, _make(cfg)[0], S, A)
        return made[cfg]
    return get


def _chunks(twin, obs, explore):
    """select_actions over at most 256 rows at a time: the twin's counter runs through the chunks as the one call's offsets do"""
    obs = obs.cpu().numpy()
    return np.concatenate([twin.select_actions(obs[k:k + 256], explore=explore) for k in range(0, len(obs), 256)])


# ---- 1. against the existing path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_rows_agree_with_select_actions_in_one_launch_each(cfg, twins):
    from rlrep_amd._lib import lib
    agent, twin, S, A = twins(cfg)
    gen = torch.Generator(device=DEV).manual_seed(7)
    worst = 0.0
    for N in NS:
        for explore in (False, True):
            obs = torch.randn(N, S, device=DEV, generator=gen)
            ctr = agent._ctr
            n0 = lib.rlrep_launch_counter()
            got = agent.act_device(obs, explore=explore)
            assert lib.rlrep_launch_counter() - n0 == 1                     # ONE launch, whatever N was before
            assert got.is_cuda and got.shape == (N, A) and got.dtype == torch.float32
            want = _chunks(twin, obs, explore)
            delta = float(np.abs(got.cpu().numpy() - want).max())
            worst = max(worst, delta)
            print(f'act_device vs select_actions {cfg} N={N} explore={explore}: max |delta| = {delta:.3e}')
            assert delta <= BAR, (cfg, N, explore, delta)
            assert agent._ctr == twin._ctr == ctr + (N if explore else 0)
            if explore and N > 1:
                same = agent.act_device(obs[:1].expand(N, S).contiguous(), explore=True)
                assert len({bytes(r) for r in same.cpu().numpy()}) == N    # a draw per row
                twin._ctr += N
    print(f'act_device vs select_actions {cfg}: worst max |delta| = {worst:.3e}')


def test_65536_rows_in_one_launch(twins):
    from rlrep_amd._lib import lib
    agent, twin, S, A = twins('sac_pendulum')
    obs = torch.randn(65536, S, device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    ctr = agent._ctr
    n0 = lib.rlrep_launch_counter()
    got = agent.act_device(obs, explore=True)
    assert lib.rlrep_launch_counter() - n0 == 1 and agent._ctr == ctr + 65536
    want = _chunks(twin, obs, True)
    delta = float(np.abs(got.cpu().numpy() - want).max())
    print(f'act_device vs select_actions sac_pendulum N=65536 explore=True: max |delta| = {delta:.3e}')
    assert delta <= BAR and twin._ctr == agent._ctr
    for bad in (torch.zeros(65537, S, device=DEV), torch.zeros(0, S, device=DEV), torch.zeros(4, S + 1, device=DEV), torch.zeros(S, device=DEV),
                torch.zeros(4, S), torch.zeros(4, S, device=DEV, dtype=torch.float64), torch.zeros(S, 4, device=DEV).t()):
        with pytest.raises(ValueError, match='act_device'):
            agent.act_device(bad)
    with pytest.raises(ValueError, match='act_device.*out'):
        agent.act_device(obs[:4], out=torch.zeros(5, A, device=DEV))
    assert agent._ctr == ctr + 65536


# ---- 2. row independence, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_a_row_does_not_depend_on_the_batch_it_travels_in(cfg, twins):
    agent, _, S, A = twins(cfg)
    gen = torch.Generator(device=DEV).manual_seed(9)
    N = 33
    obs = torch.randn(N, S, device=DEV, generator=gen)
    base = agent.act_device(obs)
    perm = torch.randperm(N, device=DEV, generator=gen)
    assert torch.equal(agent.act_device(obs[perm]), base[perm])
    assert torch.equal(agent.act_device(obs[:17]), base[:17]) and torch.equal(agent.act_device(obs[16:]), base[16:])
    # row e of an exploring call at counter c is row 0 of a one-row call at counter c + e
    c = agent._ctr
    many = agent.act_device(obs, explore=True)
    assert agent._ctr == c + N and not torch.equal(many, base)
    for e in (0, 1, 15, 16, 32):
        agent._ctr = c + e
        assert torch.equal(agent.act_device(obs[e:e + 1], explore=True), many[e:e + 1]), (cfg, e)
    agent._ctr = c + N
    # a column view of a wider tensor (ld_obs = S + 3) and an out view (ld_act = A + 1): the same bytes, the padding untouched
    wide = torch.full((N, S + 3), float('nan'), device=DEV)
    wide[:, :S] = obs
    out_wide = torch.full((N, A + 1), 7.0, device=DEV)
    res = agent.act_device(wide[:, :S], out=out_wide[:, :A])
    assert res.data_ptr() == out_wide.data_ptr() and torch.equal(out_wide[:, :A], base) and bool((out_wide[:, A] == 7.0).all())
    # rows beyond N of an over-allocated out
    big = torch.full((32, A), 7.0, device=DEV)
    agent.act_device(obs[:17], out=big[:17])
    assert torch.equal(big[:17], base[:17]) and bool((big[17:] == 7.0).all())


# ---- 3. groups --------------------------------------------------------------------------------------------------------------------------------
def test_group_planes_equal_the_standalone_agents_and_handles_are_checked():
    from rlrep_amd._lib import lib
    wl, seeds = 'sac_pendulum_b64', (3, 11, 42)
    _, S, A, Bw, _ = sg.dims(wl)
    R, N = len(seeds), 33
    grp = sg.group(wl, seeds)
    rings, alone_rings = sg.rings(wl, range(R))
    alone = [sg.standalone(wl, s) for s in seeds]
    for _ in range(3):
        grp.train(rings, Bw)
        for r, a in enumerate(alone):
            a.train(alone_rings[r], Bw)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for explore in (False, True, True):
        obs = torch.randn(R, N, S, device=DEV, generator=gen)
        n0 = lib.rlrep_launch_counter()
        acts = grp.act_device(obs, explore=explore)
        assert lib.rlrep_launch_counter() - n0 == 1 and acts.shape == (R, N, A)
        for r, a in enumerate(alone):
            assert torch.equal(acts[r], a.act_device(obs[r], explore=explore)), (explore, r)
            assert a._ctr == grp._ctr
    # a retired member: its plane of `out` and its whole block stay as they were, its observations are not read; a fresh result has zeros
    grp.retire_members([1])
    block = sg.member_bytes(grp, 1)
    obs = torch.randn(R, N, S, device=DEV, generator=gen)
    obs[1] = float('nan')
    out = torch.full((R, N, A), 7.0, device=DEV)
    for explore in (True, False):
        assert grp.act_device(obs, explore=explore, out=out) is out
        fresh = grp.act_device(obs, explore=False)
        assert bool((out[1] == 7.0).all()) and not bool(fresh[1].any()) and bool(torch.isfinite(fresh).all())
        for r in (0, 2):
            assert torch.equal(out[r], alone[r].act_device(obs[r], explore=explore)), ('retired', explore, r)
            assert alone[r]._ctr == grp._ctr
    assert torch.equal(sg.member_bytes(grp, 1), block)
    # handles and strides, refused by name before anything is launched
    agent = alone[0]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    one, act = obs[0].contiguous(), torch.zeros(N, A, device=DEV)
    n0 = lib.rlrep_launch_counter()
    assert lib.rlrep_act_device(grp.core.h, ptr(one), S, N, 0, 5, 0, -1.0, 1.0, ptr(act), A, None) == -1
    msg = lib.rlrep_last_error().decode()
    assert msg.startswith('act_device:') and 'seed group' in msg, msg
    assert lib.rlrep_group_act_device(agent.core.h, ptr(one), N, 0, 0, -1.0, 1.0, ptr(act), None) == -1
    msg = lib.rlrep_last_error().decode()
    assert msg.startswith('group_act_device:') and 'not a seed group' in msg, msg
    for ld_obs, ld_act in ((S - 1, A), (S, A - 1)):
        assert lib.rlrep_act_device(agent.core.h, ptr(one), ld_obs, N, 0, 5, 0, -1.0, 1.0, ptr(act), ld_act, None) == -1
        msg = lib.rlrep_last_error().decode()
        assert msg.startswith('act_device:') and 'stride' in msg, msg
    assert lib.rlrep_launch_counter() == n0 and not bool(act.any())


def test_shapes_beyond_the_lds_of_a_workgroup_are_refused_by_name():
    """two 16-row tiles of Ha = 1400 floats need 2 x 16 x 1416 x 4 bytes = 181 KB: more than the 160 KiB a gfx950 workgroup may have"""
    from rlrep_amd._lib import lib
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    torch.manual_seed(0)
    agent = SACAgent(3, 1, bench.Space(1), hidden_dim=1400, max_batch=16, seed=0)
    obs = torch.zeros(4, 3, device=DEV)
    n0 = lib.rlrep_launch_counter()
    with pytest.raises(RuntimeError, match='act_device: .*LDS'):
        agent.act_device(obs)
    assert lib.rlrep_launch_counter() == n0


# ---- 4. add_device ----------------------------------------------------------------------------------------------------------------------------
def _rows(gen, S, A, lead):
    r = lambda *shape: torch.randn(*lead, *shape, device=DEV, generator=gen)  # noqa: E731
    return r(S), r(A), r(S), r(), torch.rand(*lead, device=DEV, generator=gen) < 0.3


def _host(rows):
    return [x.cpu().numpy().astype(np.float32) for x in rows]


def test_add_device_leaves_the_bytes_add_batch_and_flush_leave():
    """a ring of 95 and N = 40 three times: the third call wraps the ring inside the launch; host add() calls wait in the staging buffer in
    front of the second call, which flushes them first"""
    from rlrep_amd._lib import lib
    from rlrep_amd.utils.buffer import ReplayBuffer
    S, A = 17, 6
    dev, host = ReplayBuffer(S, A, max_size=RING), ReplayBuffer(S, A, max_size=RING)
    gen = torch.Generator(device=DEV).manual_seed(3)
    rng = np.random.RandomState(3)
    for it in range(3):
        if it == 1:
            for _ in range(5):
                one = [rng.randn(S), rng.randn(A), rng.randn(S), rng.randn(), 1.0]
                dev.add(*one)
                host.add(*one)
        rows = _rows(gen, S, A, (40,))
        n0 = lib.rlrep_launch_counter()
        dev.add_device(*rows)
        assert lib.rlrep_launch_counter() - n0 == (2 if it == 1 else 1)     # the staged host rows' launch, then ONE
        host.add_batch(*_host(rows))
        host.flush()
        torch.cuda.synchronize()
        assert torch.equal(dev.ring, host.ring), it
        assert (dev.ptr, dev.size, dev.device_epoch, dev._staged) == (host.ptr, host.size, host.device_epoch, 0)
        assert dev._size_pushed == dev.size and int(dev._size_dev.item()) == int(host._size_dev.item()) == dev.size
    assert dev.ptr == 125 % RING and dev.size == RING
    # strided arguments (column views of one wide tensor) and a bool done column
    wide = torch.randn(40, 2 * S + A + 1, device=DEV, generator=gen)
    views = (wide[:, :S], wide[:, S:S + A], wide[:, S + A:2 * S + A], wide[:, 2 * S + A], wide[:, 0] > 0)
    dev.add_device(*views)
    host.add_batch(*_host(views))
    host.flush()
    torch.cuda.synchronize()
    assert torch.equal(dev.ring, host.ring) and dev.ptr == host.ptr
    with pytest.raises(ValueError, match='add_device.*max_size'):
        dev.add_device(*_rows(gen, S, A, (RING + 1,)))
    with pytest.raises(ValueError, match='add_device'):
        dev.add_device(*[x.cpu() for x in rows])


def test_add_device_on_a_group_of_rings():
    from rlrep_amd._lib import lib
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    R, S, A = 2, 3, 1
    dev, host = ReplayBufferGroup(R, S, A, max_size=RING), ReplayBufferGroup(R, S, A, max_size=RING)
    gen = torch.Generator(device=DEV).manual_seed(4)
    rng = np.random.RandomState(4)
    for it in range(3):
        if it == 2:
            one = [rng.randn(R, S), rng.randn(R, A), rng.randn(R, S), rng.randn(R), np.ones(R)]
            dev.add(*one)
            host.add(*one)
        rows = _rows(gen, S, A, (R, 40))
        n0 = lib.rlrep_launch_counter()
        dev.add_device(*rows)
        assert lib.rlrep_launch_counter() - n0 == (2 if it == 2 else 1)
        host.add_batch(*_host(rows))
        host.flush()
        torch.cuda.synchronize()
        assert torch.equal(dev.rings, host.rings) and (dev.ptr, dev.sizes) == (host.ptr, host.sizes)
        assert torch.equal(dev._size_dev, host._size_dev) and dev._size_dev.tolist() == dev.sizes
    assert dev.ptr == 121 % RING and dev.sizes == [RING] * R and not torch.equal(dev.rings[0], dev.rings[1])


def test_add_device_is_refused_while_a_device_environment_owns_the_cursor(twins):
    from rlrep_amd.utils.buffer import ReplayBuffer
    agent = twins('sac_pendulum')[0]
    buf = ReplayBuffer(3, 1, max_size=RING)
    rows = _rows(torch.Generator(device=DEV).manual_seed(6), 3, 1, (4,))
    buf.add_device(*rows)
    env = _env(agent, eps_greedy=0.0, start_timesteps=0)
    buf.collect_on_device(env)
    with pytest.raises(RuntimeError, match='ReplayBuffer.add_device.*adopt_device_cursor'):
        buf.add_device(*rows)
    buf.adopt_device_cursor()
    buf.add_device(*rows)
    assert (buf.ptr, buf.size) == (8, 8)


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------------------------
N_LOOP, PREFILL, ITERS = 4, 40, 25          # 40 + 100 rows through a ring of 95: iteration 13 wraps it (rows 92 .. 94, 0)


@pytest.mark.parametrize('cfg', ['sac_pendulum', 'vlsac_f64'])
def test_device_loop_equals_the_loop_fed_through_the_host(cfg):
    """act_device -> TorchPendulum.step -> add_device -> train() against a twin given the same device rows, copied to the host, through
    add_batch, with the same train() calls: the only difference is how the rows reached the ring"""
    from rlrep_amd.envs.torch_pendulum import TorchPendulum
    from rlrep_amd.utils.buffer import ReplayBuffer
    extra = dict(pipeline=False) if cfg == 'vlsac_f64' else {}
    agents = [_make(cfg, **extra)[0] for _ in range(2)]
    _, S, A, _ = CONFIGS[cfg]
    bufs = [ReplayBuffer(S, A, max_size=RING) for _ in range(2)]
    rng = np.random.RandomState(11)
    for _ in range(PREFILL):
        one = [rng.randn(S), rng.uniform(-1, 1, A), rng.randn(S), rng.randn(), float(rng.uniform() < 0.2)]
        for buf in bufs:
            buf.add(*one)
    env = TorchPendulum(N_LOOP, DEV, seed=2)
    obs = env.reset()
    ctr = agents[0]._ctr
    for it in range(ITERS):
        acts = agents[0].act_device(obs, explore=True)
        assert torch.equal(acts, agents[1].act_device(obs, explore=True)), (cfg, it)
        nxt, rew, done = env.step(acts)
        bufs[0].add_device(obs, acts, nxt, rew, done)
        bufs[1].add_batch(*_host((obs, acts, nxt, rew, done)))
        info = agents[0].train(bufs[0], B)
        sg.assert_info_equal(info, agents[1].train(bufs[1], B), (cfg, it))
        obs = env.obs
    sg.assert_equal(sg.state(agents[0].core), sg.state(agents[1].core), cfg)
    assert agents[0]._ctr == agents[1]._ctr >= ctr + ITERS * N_LOOP          # (a capture draws from the counter too)
    assert (bufs[0].ptr, bufs[0].size) == (bufs[1].ptr, bufs[1].size) == ((PREFILL + ITERS * N_LOOP) % RING, RING)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0].ring, bufs[1].ring) and bool(torch.isfinite(bufs[0].ring).all())


# ---- 6. launcher ------------------------------------------------------------------------------------------------------------------------------
ARGV = ['--alg', 'sac', '--env', 'Pendulum-v1', '--torch-envs', '8', '--max_timesteps', '800', '--start_timesteps', '400', '--eval_freq', '400',
        '--batch_size', '64', '--eval_episodes', '2']


def test_launcher_runs_a_torch_simulator(tmp_path, monkeypatch):
    from rlrep_amd import main
    from rlrep_amd.utils import buffer
    from test_host_envs import _keep_instances
    made = _keep_instances(monkeypatch, buffer, 'ReplayBuffer')
    agent, evaluations = main.run(ARGV + ['--log_root', str(tmp_path)])
    assert agent.steps == 50                                                # 100 iterations of 8 steps, 50 of them warm-up
    assert len(made) == 1 and made[0].size == 800 and made[0].ptr == 0 and made[0]._staged == 0
    assert agent._ctr >= 50 * 8                                             # an act_device of 8 rows per training iteration
    assert len(evaluations) == 2 and all(np.isfinite(v) and v < 0 for v in evaluations)
    rows = [json.loads(l) for l in open(tmp_path / 'Pendulum-v1' / 'sac' / '0' / '0' / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [800] and all(np.isfinite(v) for row in rows for v in row.values())
    assert 'info/q_loss' in rows[0] and 'info/actor_loss' in rows[0] and rows[0]['steps_per_sec'] > 0
