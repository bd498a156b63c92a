"""Several device environments per member / agent (num_envs = E; rlrep_amd/envs/device.py, csrc/group_env.hip *_kernel_n) on the GPU: E = 1
through create_n is the old path byte for byte, environment 0 is the single environment, the other environments draw from streams of their
own (against the NumPy stream table of tests/test_device_env_vec_cpu.py), the E actions of a step are select_action's at E successive call
counters, training is bit-identical to a twin fed the same rows in environment order (ring wrap inside a step included), retired members are
not touched, the iterate graph is train()'s launches plus one for every E, the cursor goes back to the host, checkpoints carry E, and the
launcher runs --num-envs.  Reads nothing outside the repository."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seed_group_util as sg  # noqa: E402
from test_device_env import _group as _pendulum_group  # noqa: E402
from test_device_env_mountaincar import _group as _mountaincar_group  # noqa: E402
from test_device_env_single import _agent, _env, _ring, _add, KINDS, B, RING, F32  # noqa: E402
from test_device_env_vec_cpu import start_state, start_obs  # noqa: E402

SEEDS = (3, 11, 42)
KIND_ID = {'pendulum': 0, 'mountaincar': 2}
LIMITS = {'pendulum': 200, 'mountaincar': 999}


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------------
def _group(alg, kind='pendulum', seeds=SEEDS[:2]):
    return (_pendulum_group if kind == 'pendulum' else _mountaincar_group)(alg, seeds=seeds)


def _genv(grp, kind='pendulum', **kw):
    from rlrep_amd.envs.device import DeviceEnvGroup
    return DeviceEnvGroup(grp, KIND_ID[kind], **kw)


def _rings(R, kind='pendulum', n=RING):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    S, A = KINDS[kind]
    return ReplayBufferGroup(R, S, A, max_size=n)


def _through_create_n(cls):
    """`cls` whose handle always comes from the create_n entry point, also for one environment"""
    class ThroughCreateN(cls):
        def _create(self, *args):
            h = C.c_void_p()
            self._call('create_n', *args, self.num_envs, C.byref(h))
            self.h = h
    return ThroughCreateN


def _ring_of(buf):
    """[R, capacity, row] host copy of a ReplayBuffer's or a ReplayBufferGroup's rows"""
    torch.cuda.synchronize()
    t = buf.rings if hasattr(buf, 'rings') else buf.ring[None]
    return t.cpu().numpy()


def _records(env):
    """[R, E] records, whatever E"""
    return env.state().reshape(env.R, env.num_envs)


def _iterate(agent, env, buf, train=True):
    """one iterate -> the info dicts as a list over members (a single agent: one member) with float values"""
    out = agent.iterate(env, buf, B, train=train)
    if out is None:
        return None
    out = out if isinstance(out, list) else [out]
    return [None if i is None else {k: float(v) for k, v in i.items()} for i in out]


# ---- 1. E = 1 is the old path -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['pendulum', 'mountaincar'])
@pytest.mark.parametrize('form', ['group', 'single'])
def test_one_environment_through_create_n_is_the_old_path(form, kind):
    """30 step launches (12 of warm-up, eps_greedy 0.05), an episode end by the time limit inside them: records, rings, size words and counters
    of a create_n(..., 1) environment and of a create environment are byte-identical."""
    from rlrep_amd._lib import lib
    from rlrep_amd.envs.device import DeviceEnvGroup, DeviceEnv
    runs = []
    for via_n in (False, True):
        if form == 'group':
            agent = _group('sac', kind)
            cls = _through_create_n(DeviceEnvGroup) if via_n else DeviceEnvGroup
            buf = _rings(2, kind)
            count = lib.rlrep_group_env_num_envs
        else:
            agent = _agent('sac', kind)
            cls = _through_create_n(DeviceEnv) if via_n else DeviceEnv
            buf = _ring(kind)
            count = lib.rlrep_env_num_envs
        env = cls(agent, KIND_ID[kind], eps_greedy=0.05, start_timesteps=12, num_envs=1)
        assert count(env.h) == 1 and env.state().shape == (env.R,)
        buf.collect_on_device(env)
        rec = env.state()
        rec['t'] = LIMITS[kind] - 2                                          # the second step ends the episode
        env.set_state(rec)
        for _ in range(30):
            env.step(buf, env.eps_greedy, env.start_timesteps)
        runs.append((env.state(), _ring_of(buf), buf.size_dev().cpu().numpy() if form == 'group' else buf._size_dev.cpu().numpy(), env.counters()))
    (rec_a, ring_a, size_a, ctr_a), (rec_b, ring_b, size_b, ctr_b) = runs
    assert rec_a.tobytes() == rec_b.tobytes() and ring_a.tobytes() == ring_b.tobytes() and size_a.tobytes() == size_b.tobytes()
    assert ctr_a == ctr_b == (30, 18)
    assert list(rec_a['episodes_done']) == [1] * len(rec_a) and list(rec_a['nsteps']) == [30] * len(rec_a) and list(rec_a['ring_ptr']) == [30] * len(rec_a)
    assert size_a.tolist() == [30] * len(rec_a) and np.any(ring_a[:, :30] != 0.0)


# ---- 2. / 3. environment 0 is the single environment; the others have streams of their own -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _warm_up_runs(form, kind):
    """20 warm-up steps (uniform actions from RL_STREAM_ENV) of an E = 4 and of an E = 1 environment with equal seeds -> for each: the
    records after reset [R, E], after every step [20, R, E], and the final ring [R, capacity, row]"""
    out = {}
    for E in (4, 1):
        if form == 'group':
            agent = _group('sac', kind)
            env, buf = _genv(agent, kind, start_timesteps=1000, num_envs=E), _rings(2, kind)
        else:
            agent = _agent('sac', kind)
            env, buf = _env(agent, kind, start_timesteps=1000, num_envs=E), _ring(kind)
        first, steps = _records(env).copy(), []
        for _ in range(20):
            assert agent.iterate(env, buf, B, train=False) is None
            steps.append(_records(env).copy())
        seeds = list(agent.seeds) if form == 'group' else [agent._seed]
        out[E] = (first, np.stack(steps), _ring_of(buf), [int(s) for s in seeds], env.counters(), buf.size_dev().cpu().tolist())
    return out


@pytest.mark.parametrize('kind', ['pendulum', 'mountaincar'])
@pytest.mark.parametrize('form', ['group', 'single'])
def test_environment_0_is_the_single_environment(form, kind):
    runs = _warm_up_runs(form, kind)
    first4, steps4, ring4, _, ctr4, size4 = runs[4]
    first1, steps1, ring1, _, ctr1, size1 = runs[1]
    R = first1.shape[0]
    fields = [n for n in first1.dtype.names if n not in ('ring_ptr', 'ring_size')]
    for n in fields:
        assert np.array_equal(first4[:, 0][n], first1[:, 0][n]), ('reset', n)
        assert np.array_equal(steps4[:, :, 0][n], steps1[:, :, 0][n]), n
    # its rows are the single environment's rows, at stride 4; every environment's cursor runs 4 rows at a time from its own start
    assert np.array_equal(ring4[:, 0:80:4], ring1[:, :20])
    for e in range(4):
        assert np.array_equal(steps4[:, :, e]['ring_ptr'], np.tile(4 * np.arange(1, 21)[:, None] + e, (1, R)))
        assert np.array_equal(steps4[:, :, e]['ring_size'], np.tile(4 * np.arange(1, 21)[:, None], (1, R)))
        assert np.array_equal(steps4[:, :, e]['nsteps'], np.tile(np.arange(1, 21)[:, None], (1, R)))
    assert np.array_equal(first4['ring_ptr'], np.tile(np.arange(4), (R, 1)))
    assert ctr4 == (80, 0) and ctr1 == (20, 0) and size4 == [80] * R and size1 == [20] * R
    assert np.all(ring4[:, 80:] == 0.0) and np.all(ring1[:, 20:] == 0.0)


@pytest.mark.parametrize('kind', ['pendulum', 'mountaincar'])
@pytest.mark.parametrize('form', ['group', 'single'])
def test_the_environments_of_a_member_draw_from_streams_of_their_own(form, kind):
    """Start states after reset against the NumPy stream table: equal fp32 observations, the fp64 state to 1e-12 relative (the bound of
    tests/test_device_env.py: the device may contract a + b * u into one fma, and its libm is not NumPy's)."""
    first4, steps4, ring4, seeds, _, _ = _warm_up_runs(form, kind)[4]
    S = KINDS[kind][0]
    for m, seed in enumerate(seeds):
        got = [(float(first4[m, e]['theta']), float(first4[m, e]['theta_dot'])) for e in range(4)]
        assert len({g[0] for g in got}) == 4, got                             # pairwise different
        for e in range(4):
            x0, x1 = start_state(KIND_ID[kind], seed, 0, e)
            print(f'{form} {kind} member {m} environment {e}: device start {got[e]}, table {(x0, x1)}')
            for g, w in zip(got[e], (x0, x1)):
                assert g == w or abs(g - w) <= 1e-12 * max(abs(w), 1e-300), (m, e, g, w)
            assert np.array_equal(first4[m, e]['obs'][:S], start_obs(KIND_ID[kind], x0, x1)), (m, e, first4[m, e]['obs'], start_obs(KIND_ID[kind], x0, x1))
            assert np.all(first4[m, e]['obs'][S:] == 0.0)
        # 20 warm-up steps: no two environments of the member take the same action sequence (nor, at any step, the same action)
        acts = [ring4[m, e:80:4, S] for e in range(4)]
        lo, hi = (-2.0, 2.0) if kind == 'pendulum' else (-1.0, 1.0)
        assert all(np.all(a >= lo) and np.all(a <= hi) for a in acts)
        for e in range(4):
            for f in range(e + 1, 4):
                assert not np.array_equal(acts[e], acts[f]) and not np.any(acts[e] == acts[f]), (m, e, f)
    if form == 'group':
        assert not np.array_equal(first4[0]['theta'], first4[1]['theta'])      # another seed: other starts


# ---- 4. actions ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['group', 'single'])
def test_the_actions_of_a_step_are_select_action_at_successive_call_counters(form):
    E = 3
    if form == 'group':
        agent, twin = _group('sac'), _group('sac')
        env, buf = _genv(agent, eps_greedy=0.0, start_timesteps=0, num_envs=E), _rings(2, n=32)
    else:
        agent, twin = _agent('sac'), _agent('sac')
        env, buf = _env(agent, eps_greedy=0.0, start_timesteps=0, num_envs=E), _ring(n=32)
    seen = []
    for k in range(3):
        calls0 = agent._ctr
        assert agent.iterate(env, buf, B, train=False) is None
        ring = _ring_of(buf)
        for e in range(E):
            rows = ring[:, E * k + e]                                       # row e of the step, of every member
            twin._ctr = calls0 + e                                          # one call per environment, in environment order
            act = twin.select_action(rows[:, :3] if form == 'group' else rows[0, :3], explore=True)
            assert twin._ctr == calls0 + e + 1
            assert np.array_equal(np.asarray(act, np.float32).reshape(-1).view(np.uint32), rows[:, 3].copy().view(np.uint32)), (form, k, e, act, rows[:, 3])
            seen += rows[:, 3].tolist()
        assert agent._ctr == calls0 + E and env.counters() == (E * (k + 1), agent._ctr) and (env.t_global, env.calls) == env.counters()
    assert len(set(seen)) == len(seen)
    # select_action between two device steps moves the counter the device step continues from
    agent.select_action(np.zeros((2, 3) if form == 'group' else 3, np.float32), explore=True)
    calls0 = agent._ctr
    agent.iterate(env, buf, B, train=False)
    rows = _ring_of(buf)[:, 3 * E + 1]
    twin._ctr = calls0 + 1
    act = twin.select_action(rows[:, :3] if form == 'group' else rows[0, :3], explore=True)
    assert np.array_equal(np.asarray(act, np.float32).reshape(-1).view(np.uint32), rows[:, 3].copy().view(np.uint32))


# ---- 5. training is bit-identical to a twin fed the same rows -------------------------------------------------------------------------------------
def _loop_against_the_twin(make, make_twin, kind, R, E=4, calls=25, before=None):
    """`calls` iterate calls with E environments on a ring of 95 (25 x 4 = 100 rows: the wrap falls inside the last step but one); the
    twin receives each step's E rows through add, in environment order, and calls train().  Everything a train() writes, the info dicts, the
    rings and the counters are equal.  before(env): called once the ring has handed its cursor over.  Returns (agent, env, buf, rows per step)."""
    S = KINDS[kind][0]
    group = R is not None
    members = R or 1
    agent = make()
    if group:
        env, buf = _genv(agent, kind, eps_greedy=0.05, start_timesteps=0, num_envs=E), _rings(members, kind)
    else:
        env, buf = _env(agent, kind, eps_greedy=0.05, start_timesteps=0, num_envs=E), _ring(kind)
    if before is not None:
        buf.collect_on_device(env)
        before(env)
    infos, steps = [], []
    for k in range(calls):
        infos.append(_iterate(agent, env, buf))
        pos = [(E * k + e) % RING for e in range(E)]
        steps.append(_ring_of(buf)[:, pos].copy())                           # [members, E, row]: the step's rows in environment order
    live = list(range(members))
    rec = _records(env)
    n = E * calls
    assert all(int(rec[m, e]['ring_ptr']) == (n + e) % RING and int(rec[m, e]['ring_size']) == min(n, RING) for m in live for e in range(E))
    assert env.counters() == (n, agent._ctr) == (env.t_global, env.calls)
    twin = make_twin()
    buf2 = _rings(members, kind) if group else _ring(kind)
    for k in range(calls):
        for e in range(E):
            r = steps[k][:, e]
            if group:
                buf2.add(r[:, :S], r[:, S:S + 1], r[:, S + 1:2 * S + 1], r[:, 2 * S + 1], r[:, 2 * S + 2])
            else:
                _add(buf2, r[0], S)
        out2 = twin.train(buf2, B)
        out2 = out2 if isinstance(out2, list) else [out2]
        for m in live:
            sg.assert_info_equal(infos[k][m], out2[m], (kind, k, m))
    assert twin.steps == agent.steps == calls
    for m in live:
        a, b = (agent._members[m], twin._members[m]) if group else (agent.core, twin.core)
        sg.assert_equal(sg.state(a), sg.state(b), (kind, m))
    ring, ring2 = _ring_of(buf), _ring_of(buf2)
    assert all(np.array_equal(ring[m], ring2[m]) for m in live)
    assert agent._iter_launches == twin._graph_launches + 1, (agent._iter_launches, twin._graph_launches)
    return agent, env, buf, steps


@pytest.mark.parametrize('alg, R', [('sac', 3), ('ctrlsac', 2)])
def test_group_training_equals_a_twin_fed_the_same_rows(alg, R):
    agent, env, buf, steps = _loop_against_the_twin(lambda: _group(alg, seeds=SEEDS[:R]), lambda: _group(alg, seeds=SEEDS[:R]), 'pendulum', R)
    assert buf.size_dev().cpu().tolist() == [RING] * R
    # every environment's rows are a rollout of its own: s of its next row is s' of this one (no episode ended in 25 steps)
    for e in range(4):
        assert all(np.array_equal(steps[k + 1][:, e, :3], steps[k][:, e, 4:7]) for k in range(24))
    assert env.returns() == [[]] * R


@pytest.mark.parametrize('alg', ['sac', 'vlsac_f64'])
def test_single_agent_training_equals_a_twin_fed_the_same_rows(alg):
    extra = dict(feature_dim=64) if alg == 'vlsac_f64' else {}
    name = alg.split('_')[0]
    agent, env, buf, steps = _loop_against_the_twin(lambda: _agent(name, **extra), lambda: _agent(name, pipeline=False, **extra), 'pendulum', None)
    assert buf.size_dev().cpu().tolist() == [RING] and env.state().shape == (1, 4)
    for e in range(4):
        assert all(np.array_equal(steps[k + 1][:, e, :3], steps[k][:, e, 4:7]) for k in range(24))


def test_a_terminal_row_of_one_environment_sits_in_its_place():
    """MountainCar, environment 2 one step before the goal: the step's row 2 carries done_bool = 1 and the +100, the episode is filed under
    that environment, and the twin's critic sees the row where the device wrote it."""
    def before(env):
        rec = env.state()
        assert rec.shape == (1, 4) and list(rec['ring_ptr'][0]) == [0, 1, 2, 3]
        r = rec[0, 2]
        r['theta'], r['theta_dot'], r['t'], r['force'], r['force_action'], r['episode_return'] = F32(0.44), F32(0.05), 5, 1, 1.0, -7.5
        r['obs'][:2] = np.array([0.44, 0.05], np.float32)
        rec[0, 2] = r
        env.set_state(rec)

    agent, env, buf, steps = _loop_against_the_twin(lambda: _agent('sac', 'mountaincar'), lambda: _agent('sac', 'mountaincar', pipeline=False),
                                                    'mountaincar', None, before=before)
    done = np.stack([s[0, :, 6] for s in steps])                            # [step, environment]
    assert done[0].tolist() == [0.0, 0.0, 1.0, 0.0] and np.all(done[1:] == 0.0)
    row = steps[0][0, 2]
    assert row[5] > 99.0 and row[2] == 1.0 and np.array_equal(row[:2], np.array([0.44, 0.05], np.float32))
    rec = env.state()
    assert list(rec['episodes_done'][0]) == [0, 0, 1, 0] and list(rec['t'][0]) == [25, 25, 24, 25]
    assert env.returns() == [[-7.5 + float(row[5])]] and env.returns() == [[]]


# ---- 6. retired members ---------------------------------------------------------------------------------------------------------------------------
def test_a_retired_members_environments_are_not_touched():
    """R = 3, E = 4: member 1 is retired after 3 calls; in the 10 calls that follow its 4 records, its ring and its size word do not change,
    members 0 and 2 equal their twins (a group that retires member 1 at the same call), and t_global advances by 4 per call."""
    grp = _group('sac', seeds=SEEDS)
    env, buf = _genv(grp, eps_greedy=0.05, start_timesteps=0, num_envs=4), _rings(3)
    infos, steps = [], []
    for k in range(13):
        if k == 3:
            grp.retire_members([1])
            marks = dict(block=sg.member_bytes(grp, 1), ring=buf.rings[1].clone(), rec=_records(env)[1].copy(), size=buf.size_dev().cpu().tolist(),
                         t=env.counters()[0])
        out = _iterate(grp, env, buf)
        assert (out[1] is None) == (k >= 3) and out[0] is not None and out[2] is not None
        infos.append(out)
        steps.append(_ring_of(buf)[:, [4 * k + e for e in range(4)]].copy())
    rec = _records(env)
    assert marks['size'] == [12, 12, 12] and marks['t'] == 12
    assert torch.equal(sg.member_bytes(grp, 1), marks['block']) and torch.equal(buf.rings[1], marks['ring']) and rec[1].tobytes() == marks['rec'].tobytes()
    assert buf.size_dev().cpu().tolist() == [52, 12, 52]
    assert env.counters()[0] == 12 + 4 * 10 == env.t_global
    for m in (0, 2):
        assert [int(rec[m, e]['ring_ptr']) for e in range(4)] == [52, 53, 54, 55] and list(rec[m]['nsteps']) == [13] * 4
    assert list(rec[1]['nsteps']) == [3] * 4 and [int(p) for p in rec[1]['ring_ptr']] == [12, 13, 14, 15]
    twin, buf2 = _group('sac', seeds=SEEDS), _rings(3)
    for k in range(13):
        if k == 3:
            twin.retire_members([1])
        for e in range(4):
            r = steps[k][:, e]
            buf2.add(r[:, :3], r[:, 3:4], r[:, 4:7], r[:, 7], r[:, 8])
        out2 = twin.train(buf2, B)
        for m in (0, 2):
            sg.assert_info_equal(infos[k][m], out2[m], (k, m))
    for m in (0, 2):
        sg.assert_equal(sg.state(grp._members[m]), sg.state(twin._members[m]), m)
        assert torch.equal(buf.rings[m], buf2.rings[m])


# ---- 7. graph -------------------------------------------------------------------------------------------------------------------------------------
def test_the_iterate_graph_is_trains_launches_plus_one_for_every_num_envs():
    twin, buf2 = _agent('sac', pipeline=False), _ring()
    for k in range(8):
        buf2.add(np.full(3, 0.1 * k), np.full(1, 0.1), np.full(3, 0.1 * k + 0.1), -1.0, 0.0)
    twin.train(buf2, B)
    gtwin, gbuf2 = _group('sac'), _rings(2)
    for k in range(8):
        gbuf2.add(np.full((2, 3), 0.1 * k), np.full((2, 1), 0.1), np.full((2, 3), 0.1 * k + 0.1), np.full(2, -1.0), np.zeros(2))
    gtwin.train(gbuf2, B)
    assert twin._graph_launches > 1 and gtwin._graph_launches > 1
    for E in (1, 4, 16):
        for form in ('single', 'group'):
            if form == 'single':
                agent = _agent('sac')
                env, buf, want = _env(agent, num_envs=E), _ring(), twin._graph_launches
            else:
                agent = _group('sac')
                env, buf, want = _genv(agent, num_envs=E), _rings(2), gtwin._graph_launches
            agent.iterate(env, buf, B, train=False)
            assert agent._iter_launches == 1, (form, E)
            agent.iterate(env, buf, B)
            assert agent._iter_launches == want + 1, (form, E, agent._iter_launches, want)
            assert env.counters()[0] == 2 * E and buf.size_dev().cpu().tolist() == [2 * E] * env.R


# ---- 8. cursor and checkpoints ----------------------------------------------------------------------------------------------------------------
def test_cursor_goes_back_to_the_host_and_checkpoints_carry_num_envs(tmp_path):
    agent = _agent('sac')
    env, buf = _env(agent, eps_greedy=0.05, start_timesteps=8, num_envs=4), _ring()
    for _ in range(7):
        agent.iterate(env, buf, B, train=False)
    one = (np.ones(3, np.float32), np.full(1, 0.5, np.float32), np.ones(3, np.float32), -1.0, 0.0)
    with pytest.raises(RuntimeError, match='adopt_device_cursor'):
        buf.add(*one)
    buf.adopt_device_cursor()
    assert buf.ptr == 28 % RING and buf.size == 28
    keep = buf.ring.clone()
    buf.add(*one)
    buf.flush()
    torch.cuda.synchronize()
    assert buf.ptr == 29 and buf.ring[28].cpu().tolist() == [1, 1, 1, 0.5, 1, 1, 1, -1, 0] and torch.equal(buf.ring[:28], keep[:28])
    for _ in range(5):
        agent.train(buf, B)
    path = str(tmp_path / 'agent.pt')
    agent.save(path, env=env)
    agent2 = _agent('sac')
    env2, buf2 = _env(agent2, eps_greedy=0.05, start_timesteps=8, num_envs=4), _ring()
    agent2.load(path, env=env2)
    buf2.ring.copy_(buf.ring)
    buf2.ptr, buf2.size = buf.ptr, buf.size
    assert env2.state().tobytes() == env.state().tobytes() and env2.counters() == env.counters() and agent2._ctr == agent._ctr
    for _ in range(5):
        sg.assert_info_equal(agent.iterate(env, buf, B), agent2.iterate(env2, buf2, B), 'after load')
    sg.assert_equal(sg.state(agent.core), sg.state(agent2.core), 'after load')
    rec = env.state()
    assert env2.state().tobytes() == rec.tobytes() and torch.equal(buf.ring, buf2.ring)
    assert list(rec['nsteps'][0]) == [12] * 4 and list(rec['ring_ptr'][0]) == [49, 50, 51, 52] and env.counters()[0] == 48
    # another E is refused; a snapshot from before num_envs is one environment's
    snap = env.snapshot()
    assert snap['num_envs'] == 4
    three, single = _env(_agent('sac'), num_envs=3), _env(_agent('sac'))
    with pytest.raises(RuntimeError, match='does not match this device environment'):
        three.load_snapshot(snap)
    with pytest.raises(RuntimeError, match='does not match this device environment'):
        single.load_snapshot(snap)
    donor = _env(_agent('sac'), eps_greedy=0.05, start_timesteps=0)
    donor_buf = _ring()
    for _ in range(3):
        donor.agent.iterate(donor, donor_buf, B, train=False)
    old = donor.snapshot()
    assert old.pop('num_envs') == 1
    single.load_snapshot(old)
    assert single.state().tobytes() == donor.state().tobytes() and single.counters() == donor.counters() == (3, 3)
    with pytest.raises(RuntimeError, match='does not match this device environment'):
        env.load_snapshot(old)


# ---- 9. launcher ----------------------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_several_environments(tmp_path):
    from rlrep_amd import main
    argv = ['--alg', 'sac', '--env', 'Pendulum-v1', '--device-loop', '--num-envs', '4', '--max_timesteps', '480', '--start_timesteps', '160',
            '--eval_freq', '160', '--batch_size', '64', '--log_root', str(tmp_path / 'single')]
    agent, evaluations = main.run(argv)
    assert agent.steps == 80                                                # 480 / 4 iterate calls, 40 of them warm-up
    assert len(evaluations) == 4 and all(np.isfinite(v) and v < 0 for v in evaluations)         # the initial one and three more
    rows = [json.loads(l) for l in open(tmp_path / 'single' / 'Pendulum-v1' / 'sac' / '0' / '0' / 'metrics.jsonl')]
    assert [row['step'] for row in rows] == [320, 480]
    keys = {'step', 'info/evaluation', 'steps_per_sec'} | {f'info/{k}' for k in agent.FEATURE_KEYS + agent.CRITIC_KEYS + agent.ACTOR_KEYS}
    assert 'info/q_loss' in keys and 'info/actor_loss' in keys and 'info/alpha' in keys
    assert all(set(row) == keys for row in rows), (keys, [set(row) for row in rows])
    assert all(np.isfinite(v) for row in rows for v in row.values())
    argv = ['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--device-env', '--num-envs', '4', '--max_timesteps', '480',
            '--start_timesteps', '160', '--eval_freq', '160', '--batch_size', '64', '--log_root', str(tmp_path / 'group')]
    grp, evaluations = main.run(argv)
    assert grp.R == 2 and grp.steps == 80 and [len(e) for e in evaluations] == [4, 4]
    for seed in (0, 1):
        rows = [json.loads(l) for l in open(tmp_path / 'group' / 'Pendulum-v1' / 'sac' / '0' / str(seed) / 'metrics.jsonl')]
        assert [row['step'] for row in rows] == [320, 480] and all(np.isfinite(v) for row in rows for v in row.values())
