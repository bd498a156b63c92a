"""Device environments of a seed group (rlrep_amd/envs/device.py, csrc/group_env.hip) on the GPU: the device step against the host
PendulumEnv, acting against select_action, the device loop against the host loop on the same transitions (bit for bit), episodes, retired
members, scoring and the ring wrap.  Reads nothing outside the repository."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import seed_group_util as sg  # noqa: E402

SEEDS = (3, 11, 42)
B = 64


# ---- helpers that need no GPU (tests/test_device_env_cpu.py checks them on the host) --------------------------------------------------------
def dynamics_cases():
    """(theta, theta_dot, u, t) cases of the one-step comparison: random states, both speed clips, the torque clip, theta at and around +-pi
    and several turns away, the last step of an episode.  u is an fp32 value (the action a policy hands over)."""
    g = np.random.RandomState(0)
    pi = np.pi
    cases = [(g.uniform(-pi, pi), g.uniform(-8, 8), g.uniform(-2, 2), int(g.randint(0, 199))) for _ in range(200)]
    for s in (1.0, -1.0):
        for k in range(8):                              # the speed clip: already near the limit, pushed further by gravity and torque
            cases.append((s * (pi / 2 + 0.1 * k), s * (7.6 + 0.05 * k), s * 2.0, k))
        for u in (2.0000002, 2.5, 3.0, 10.0, 1e6):      # the torque clip
            cases.append((g.uniform(-pi, pi), g.uniform(-1, 1), s * u, 5))
        for th in (pi, np.nextafter(pi, 4.0), np.nextafter(pi, 0.0), pi - 1e-9, pi + 1e-9, pi - 1e-3):
            cases.append((s * th, g.uniform(-8, 8), g.uniform(-2, 2), 17))
        for turns in (2, 3, 5, 17, 100, 12345):         # several wraps away
            cases.append((s * (g.uniform(-pi, pi) + 2 * pi * turns), g.uniform(-8, 8), g.uniform(-2, 2), 100))
            cases.append((s * (pi + 2 * pi * turns), g.uniform(-1, 1), g.uniform(-2, 2), 100))
        for k in range(6):                              # the time limit
            cases.append((g.uniform(-pi, pi) + s * 2 * pi * k, g.uniform(-8, 8), s * (0.5 + k), 199))
    cases.append((0.0, 0.0, 0.0, 0))
    cases.append((0.0, 8.0, 2.0, 198))
    return [(float(th), float(thd), float(np.float32(u)), int(t)) for th, thd, u, t in cases]


def host_step(th, thd, u, t):
    """PendulumEnv.step from state (th, thd) at episode step t with action u -> (obs fp32 [3], reward fp32, done, (theta', theta_dot'))"""
    from rlrep_amd.envs.pendulum import PendulumEnv
    env = PendulumEnv()
    env._th, env._thd, env._t = th, thd, t
    obs, rew, done, _ = env.step(np.asarray([u], np.float32))
    return obs, np.float32(rew), bool(done), (float(env._th), float(env._thd))


def _ulps(a, b):
    """distance of two fp32 arrays in units in the last place (0 for equal values, +0 / -0 included)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------------------
def _space():
    from rlrep_amd.envs.pendulum import PendulumEnv
    return PendulumEnv().action_space


def _group(alg, seeds=SEEDS, **extra):
    if alg == 'sac':
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
        return SACSeedBatch(list(seeds), 3, 1, _space(), max_batch=B, hidden_dim=256, **extra)
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    return CTRLSACSeedBatch(list(seeds), 3, 1, _space(), max_batch=B, hidden_dim=256, feature_dim=256, extra_feature_steps=3, **extra)


def _env(grp, **kw):
    from rlrep_amd.envs.device import DevicePendulumGroup
    return DevicePendulumGroup(grp, **kw)


def _rings(R, n):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    return ReplayBufferGroup(R, 3, 1, max_size=n)


# ---- 1. dynamics ------------------------------------------------------------------------------------------------------------------------------
def test_device_step_matches_the_host_environment():
    """Both sides compute in fp64 and round to fp32 once: one fp32 rounding step, plus one for a last-bit difference of the two libms' sin /
    cos.  Bound: 2 fp32 ulp per element of s', r; theta and theta_dot of the record to 1e-12 relative.
    Measured on an MI355X (profiles/seed_batch_device_env.txt): worst 0 ulp on s' and r, 3.3e-16 relative on the record."""
    R = 8
    grp = _group('sac', seeds=range(R))
    env, buf = _env(grp), _rings(R, 4)
    cases = dynamics_cases()
    worst_ulp, worst_rel = 0, 0.0
    for k0 in range(0, len(cases), R):
        chunk = cases[k0:k0 + R]
        chunk = chunk + [chunk[-1]] * (R - len(chunk))
        rec = env.state()
        for r, (th, thd, u, t) in enumerate(chunk):
            rec['theta'][r], rec['theta_dot'][r], rec['t'][r] = th, thd, t
            rec['obs'][r][:3] = np.array([np.cos(th), np.sin(th), thd], np.float32)
            rec['force'][r], rec['force_action'][r] = 1, u
            rec['ring_ptr'][r], rec['episode_return'][r], rec['episodes_done'][r] = 2, -7.5, 0
        env.set_state(rec)
        before = rec.copy()
        env.step(buf, 0.0, 0)
        rows = buf.rings[:, 2].cpu().numpy()
        new = env.state()
        for r, (th, thd, u, t) in enumerate(chunk):
            obs, rew, done, (th2, thd2) = host_step(th, thd, u, t)
            row = rows[r]
            assert np.array_equal(row[:3], before['obs'][r][:3]) and row[3] == np.float32(u) and row[8] == 0.0, (k0 + r, row)
            d = int(max(_ulps(row[4:7], obs).max(), _ulps(row[7:8], np.array([rew])).max()))
            worst_ulp = max(worst_ulp, d)
            assert d <= 2, (k0 + r, chunk[r], row, obs, rew)
            assert new['ring_ptr'][r] == 3 and new['ring_size'][r] >= 1 and new['force'][r] == 0 and new['act'][r] == np.float32(u)
            if done:
                assert new['t'][r] == 0 and new['episodes_done'][r] == 1 and new['episode_return'][r] == 0.0
                assert new['returns'][r][0] == -7.5 + float(row[7])
                assert -np.pi <= new['theta'][r] <= np.pi and -1.0 <= new['theta_dot'][r] <= 1.0
            else:
                rel = max(abs(new['theta'][r] - th2) / max(abs(th2), 1e-300), abs(new['theta_dot'][r] - thd2) / max(abs(thd2), 1e-300))
                rel = 0.0 if (new['theta'][r] == th2 and new['theta_dot'][r] == thd2) else rel
                worst_rel = max(worst_rel, rel)
                assert rel <= 1e-12, (k0 + r, chunk[r], new['theta'][r], th2, new['theta_dot'][r], thd2)
                assert new['t'][r] == t + 1 and new['episodes_done'][r] == 0 and new['episode_return'][r] == -7.5 + float(row[7])
                assert np.array_equal(new['obs'][r][:3], row[4:7])
    print(f'device step vs PendulumEnv.step over {len(cases)} cases: worst {worst_ulp} fp32 ulp on (s\', r), worst {worst_rel:.3e} relative on (theta, theta_dot)')


# ---- 2. acting --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ['sac', 'ctrlsac'])
def test_device_action_equals_select_action_bit_for_bit(alg):
    grp, twin = _group(alg), _group(alg)
    env, buf = _env(grp, eps_greedy=0.0, start_timesteps=0), _rings(3, 32)
    for k in range(4):
        grp.iterate(env, buf, B, train=False)
        rows = buf.rings[:, k].cpu().numpy()
        twin._ctr = grp._ctr - 1                                    # the same call counter
        act = twin.select_action(rows[:, :3], explore=True)
        assert twin._ctr == grp._ctr
        assert np.array_equal(act.reshape(-1).view(np.uint32), rows[:, 3].copy().view(np.uint32)), (alg, k, act.reshape(-1), rows[:, 3])
        assert np.all(np.abs(act) <= 2.0) and len(set(act.reshape(-1).tolist())) == 3
    # ... and select_action between two device steps moves the counter the device step continues from
    grp.select_action(np.zeros((3, 3), np.float32), explore=True)
    grp.iterate(env, buf, B, train=False)
    rows = buf.rings[:, 4].cpu().numpy()
    twin._ctr = grp._ctr - 1
    assert np.array_equal(twin.select_action(rows[:, :3], explore=True).reshape(-1).view(np.uint32), rows[:, 3].copy().view(np.uint32))


# ---- 3. the device loop is the host loop ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ['sac', 'ctrlsac'])
def test_device_loop_equals_host_loop_on_the_same_transitions(alg):
    warm, calls = 70, 25
    grp = _group(alg)
    env, buf = _env(grp, eps_greedy=0.05, start_timesteps=warm), _rings(3, 256)
    for _ in range(warm):
        assert grp.iterate(env, buf, B, train=False) is None
    infos = []
    for _ in range(calls):
        out = grp.iterate(env, buf, B)
        infos.append([{k: float(v) for k, v in i.items()} for i in out])
    torch.cuda.synchronize()
    rows = buf.rings.cpu().numpy()
    rec = env.state()
    assert list(rec['ring_ptr']) == [warm + calls] * 3 and list(rec['ring_size']) == [warm + calls] * 3
    assert buf.size_dev().cpu().tolist() == [warm + calls] * 3
    twin, buf2 = _group(alg), _rings(3, 256)
    for t in range(warm + calls):
        r = rows[:, t]
        buf2.add(r[:, :3], r[:, 3:4], r[:, 4:7], r[:, 7], r[:, 8])
        if t >= warm:
            out2 = twin.train(buf2, B)
            for m in range(3):
                sg.assert_info_equal(infos[t - warm][m], out2[m], (alg, t, m))
    assert twin.steps == grp.steps == calls
    for m in range(3):
        sg.assert_equal(sg.state(grp._members[m]), sg.state(twin._members[m]), (alg, m))
    assert torch.equal(buf2.rings[:, :warm + calls].cpu(), buf.rings[:, :warm + calls].cpu())
    # the transitions are a rollout: s of row t + 1 is s' of row t (no episode ended), warm-up actions are uniform draws in [-2, 2]
    assert np.array_equal(rows[:, 1:warm + calls, :3], rows[:, :warm + calls - 1, 4:7])
    assert np.all(np.abs(rows[:, :warm, 3]) <= 2.0) and np.abs(rows[:, :warm, 3]).max() > 1.5


# ---- 4. episodes ------------------------------------------------------------------------------------------------------------------------------
def test_episodes_end_are_filed_and_reset():
    grp, same, other = _group('sac'), _group('sac'), _group('sac', seeds=(4, 12, 43))
    runs = []
    for g in (grp, same, other):
        env, buf = _env(g, eps_greedy=0.05, start_timesteps=50), _rings(3, 256)
        for _ in range(199):
            g.iterate(env, buf, B, train=False)
        assert env.returns() == [[], [], []] and list(env.state()['episodes_done']) == [0, 0, 0]
        g.iterate(env, buf, B, train=False)
        runs.append((env, buf))
    env, buf = runs[0]
    rec = env.state()
    assert list(rec['episodes_done']) == [1, 1, 1] and list(rec['t']) == [0, 0, 0] and list(rec['nsteps']) == [200] * 3
    rows = buf.rings.cpu().numpy()
    got = env.returns()
    for m in range(3):
        total = 0.0
        for v in rows[m, :200, 7]:
            total += float(v)                          # fp64 sum of the fp32 rewards, in step order
        assert got[m] == [total], (m, got[m], total)
        assert -np.pi <= rec['theta'][m] <= np.pi and -1.0 <= rec['theta_dot'][m] <= 1.0
        assert rec['obs'][m][2] == np.float32(rec['theta_dot'][m])
        assert _ulps(rec['obs'][m][:2], np.array([np.cos(rec['theta'][m]), np.sin(rec['theta'][m])], np.float32)).max() <= 2
        assert not np.array_equal(rec['obs'][m][:3], rows[m, 199, 4:7])             # a reset draw, not the last s'
    assert env.returns() == [[], [], []]                                            # drained
    assert len({float(rec['theta'][m]) for m in range(3)}) == 3
    assert torch.equal(runs[0][1].rings, runs[1][1].rings)                          # equal seeds: identical rings
    assert np.array_equal(runs[0][0].state(), runs[1][0].state())
    assert not torch.equal(runs[0][1].rings[:, :, :3], runs[2][1].rings[:, :, :3])  # other seeds: other transitions
    # the next episode goes on from the reset state
    grp.iterate(env, buf, B, train=False)
    row = buf.rings[:, 200].cpu().numpy()
    assert np.array_equal(row[:, :3], rec['obs'][:, :3]) and list(env.state()['t']) == [1, 1, 1]


# ---- 5. retired members -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ['sac', 'ctrlsac'])
def test_a_retired_member_is_not_touched_and_continues_when_revived(alg):
    seeds = (3, 11, 42, 7)
    grp = _group(alg, seeds=seeds)
    env, buf = _env(grp, eps_greedy=0.05, start_timesteps=5), _rings(4, 128)
    for t in range(12):
        grp.iterate(env, buf, B, train=t >= 5)
    grp.retire_members([2])
    block, ring, rec = sg.member_bytes(grp, 2), buf.rings[2].clone(), env.state()
    others = [sg.state(grp._members[q])['params'] for q in range(4)]
    for _ in range(6):
        out = grp.iterate(env, buf, B)
        assert out[2] is None and all(out[q] is not None for q in (0, 1, 3))
    scores = grp.evaluate(env, 2)
    assert np.isnan(scores[2]) and np.all(np.isfinite(scores[[0, 1, 3]])) and np.all(scores[[0, 1, 3]] < 0)
    now = env.state()
    assert torch.equal(sg.member_bytes(grp, 2), block) and torch.equal(buf.rings[2], ring) and now[2].tobytes() == rec[2].tobytes()
    assert buf.size_dev().cpu().tolist() == [18, 18, 12, 18]
    for q in (0, 1, 3):
        assert now['nsteps'][q] == 18 and now['ring_ptr'][q] == 18
        assert not torch.equal(sg.state(grp._members[q])['params'], others[q])
        assert not torch.equal(buf.rings[q, 12:18], torch.zeros_like(buf.rings[q, 12:18]))
    assert env.counters()[0] == 18                                                  # the group's step counter does not wait for a retired member
    grp.revive_members([2])
    out = grp.iterate(env, buf, B)
    assert out[2] is not None
    after = env.state()
    assert after['nsteps'][2] == 13 and after['ring_ptr'][2] == 13 and after['t'][2] == 13
    row = buf.rings[2, 12].cpu().numpy()
    assert np.array_equal(row[:3], rec['obs'][2][:3])                               # it went on from its own record
    assert np.all(np.isfinite(grp.evaluate(env, 2)))


# ---- 6. scoring -------------------------------------------------------------------------------------------------------------------------------
def _host_scores(grp, starts, perturb=None):
    """Mean return of host rollouts from the device's start states, [R]: PendulumEnv stepped with select_action(explore=False).  perturb: a
    RandomState that moves every observation the policy sees by one fp32 ulp in a random direction (the last-bit difference test 1 allows
    between the device's observations and the host's)."""
    from rlrep_amd.envs.pendulum import PendulumEnv
    R, E = starts.shape[:2]
    total = np.zeros((R, E))
    for e in range(E):
        envs_ = [PendulumEnv() for _ in range(R)]
        obs = np.zeros((R, 3), np.float32)
        for r, pe in enumerate(envs_):
            pe._th, pe._thd, pe._t = float(starts[r, e, 0]), float(starts[r, e, 1]), 0
            obs[r] = pe._obs()
        for _ in range(200):
            seen = obs
            if perturb is not None:
                seen = np.nextafter(obs, np.where(perturb.randint(0, 2, size=obs.shape) > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
            act = grp.select_action(seen)
            for r, pe in enumerate(envs_):
                obs[r], rew, _, _ = pe.step(act[r])
                total[r, e] += float(np.float32(rew))
    return total.mean(axis=1)


def test_device_scores_equal_host_rollouts():
    """Tolerance: the device's observations may differ from the host's in the last bit (test 1), and a rollout amplifies that.  How much is
    measured on the host path alone: the same host rollout with every observation moved by one ulp.  10 x that spread is allowed.
    Measured on an MI355X (profiles/seed_batch_device_env.txt): |device - host| 0 at initialisation and after training; host spread 3.9e-6
    and 6.2e-6."""
    grp = _group('sac')
    env, buf = _env(grp, eps_greedy=0.05, start_timesteps=40), _rings(3, 512)
    for phase in ('initialisation', 'after training'):
        a = grp.evaluate(env, 4, eval_index=5)
        starts = env.eval_starts(4)
        b = grp.evaluate(env, 4, eval_index=5)
        assert np.array_equal(a, b)                                                 # the same index: bit-identical scores
        assert np.array_equal(starts, env.eval_starts(4))
        c = grp.evaluate(env, 4, eval_index=6)
        other = env.eval_starts(4)
        assert not np.array_equal(other, starts) and not np.array_equal(a, c)
        assert np.all(np.abs(starts[..., 0]) <= np.pi) and np.all(np.abs(starts[..., 1]) <= 1.0)
        assert len(np.unique(starts[..., 0])) == 12
        host = _host_scores(grp, starts)
        moved = _host_scores(grp, starts, np.random.RandomState(1))
        spread = float(np.abs(host - moved).max())
        diff = float(np.abs(a - host).max())
        print(f'evaluate vs host rollouts ({phase}): device {a}, host {host}, |device - host| max {diff:.3e}, host spread under 1-ulp observations {spread:.3e}')
        assert diff <= 10 * spread, (phase, a, host, diff, spread)
        if phase == 'initialisation':
            for t in range(140):
                grp.iterate(env, buf, B, train=t >= 40)
    # evaluate() counts evaluations by itself: fresh starts every time
    i0 = env.eval_index
    grp.evaluate(env, 3)
    s1 = env.eval_starts(3)
    grp.evaluate(env, 3)
    assert env.eval_index == i0 + 2 and not np.array_equal(s1, env.eval_starts(3))
    with pytest.raises(RuntimeError, match='episodes 0 outside'):
        grp.evaluate(env, 0, eval_index=0)


# ---- 7. the ring wraps ------------------------------------------------------------------------------------------------------------------------
def test_ring_wrap_and_the_host_cursor():
    grp = _group('sac')
    env, buf = _env(grp, eps_greedy=0.0, start_timesteps=1000), _rings(3, 16)
    rows = []
    for t in range(40):
        grp.iterate(env, buf, B, train=False)
        if t in (15, 23):
            rows.append(buf.rings.clone())
    rec = env.state()
    assert list(rec['ring_ptr']) == [8, 8, 8] and list(rec['ring_size']) == [16, 16, 16] and buf.size_dev().cpu().tolist() == [16] * 3
    assert not torch.equal(rows[0][:, :8], rows[1][:, :8]) and torch.equal(rows[0][:, 8:], rows[1][:, 8:])      # rows 0..7 were overwritten
    assert np.array_equal(buf.rings[:, 0, :3].cpu().numpy(), buf.rings[:, 15, 4:7].cpu().numpy())             # the rollout wraps with the ring
    one = (np.ones((3, 3), np.float32), np.full((3, 1), 0.5, np.float32), np.ones((3, 3), np.float32), np.full(3, -1.0), np.zeros(3))
    with pytest.raises(RuntimeError, match='adopt_device_cursor'):
        buf.add(*one)
    buf.adopt_device_cursor()
    assert buf.ptr == 8 and buf.sizes == [16, 16, 16]
    keep = buf.rings.clone()
    buf.add(*one)
    buf.flush()
    torch.cuda.synchronize()
    assert buf.ptr == 9 and buf.rings[:, 8].cpu().tolist() == [[1, 1, 1, 0.5, 1, 1, 1, -1, 0]] * 3
    assert torch.equal(buf.rings[:, :8], keep[:, :8]) and torch.equal(buf.rings[:, 9:], keep[:, 9:])
    grp.iterate(env, buf, B, train=False)                                           # the device takes the cursor again, behind the host's row
    assert list(env.state()['ring_ptr']) == [10, 10, 10] and not torch.equal(buf.rings[:, 9], keep[:, 9])
    assert buf.rings[:, 8].cpu().tolist() == [[1, 1, 1, 0.5, 1, 1, 1, -1, 0]] * 3


# ---- ABI refusals that need a real agent ------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason():
    import ctypes as C
    from rlrep_amd._lib import lib
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    import bench
    out = C.c_void_p()
    single = SACAgent(3, 1, _space(), max_batch=B, seed=0, hidden_dim=256)
    assert lib.rlrep_group_env_create(single.core.h, 0, C.byref(out)) == -1 and 'not a seed group' in lib.rlrep_last_error().decode()
    wide = SACSeedBatch([0, 1], 17, 6, bench.Space(6), max_batch=B, hidden_dim=256)
    assert lib.rlrep_group_env_create(wide.core.h, 0, C.byref(out)) == -1 and '3 observations and 1 action' in lib.rlrep_last_error().decode()
    assert not out.value
    grp, other = _group('sac'), _group('sac', seeds=(0, 1))
    env, buf = _env(grp), _rings(3, 16)
    with pytest.raises(ValueError, match='another group'):
        other.iterate(env, _rings(2, 16), B)
    with pytest.raises(ValueError, match='ReplayBufferGroup of 3 members'):
        grp.iterate(env, _rings(2, 16), B)
    h = grp.core.h
    assert lib.rlrep_group_env_step(h, env.h, None, buf.ring_stride, 16, C.c_void_p(buf.size_dev().data_ptr()), -2.0, 2.0, 0.0, 0, None) == -1
    assert 'null ring' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_env_step(h, env.h, C.c_void_p(buf.rings.data_ptr()), 16 * 9 - 1, 16, C.c_void_p(buf.size_dev().data_ptr()), -2.0, 2.0, 0.0, 0, None) == -1
    assert 'ring stride' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_env_evaluate(h, env.h, 65, 0, C.c_void_p(buf.rings.data_ptr()), None) == -1 and 'episodes 65' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_env_evaluate(other.core.h, env.h, 4, 0, C.c_void_p(buf.rings.data_ptr()), None) == -1
    assert 'another group' in lib.rlrep_last_error().decode()
    rec = env.state()
    assert lib.rlrep_group_env_state(env.h, 0, C.c_void_p(rec.ctypes.data), rec.nbytes - 1, 0, None) == -1 and 'holds 768 bytes' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_env_state(env.h, 2, C.c_void_p(rec.ctypes.data), 0, 1, None) == -1            # the start states are read-only
    assert np.array_equal(env.state(), rec)                                         # nothing was launched


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_the_device_loop_with_halving_and_checkpoints(tmp_path):
    import json
    from rlrep_amd import main
    from rlrep_amd.envs.device import RECORD_DTYPE
    argv = ['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1,2,3', '--device-env', '--max_timesteps', '450', '--start_timesteps', '150',
            '--eval_freq', '150', '--eval_episodes', '2', '--batch_size', '64', '--halving-interval', '300', '--save_model', '--log_root', str(tmp_path)]
    agent, evaluations = main.run(argv)
    assert agent.live.count(True) == 2 and agent.steps == 300
    root = tmp_path / 'Pendulum-v1' / 'sac' / '0'
    for r, s in enumerate((0, 1, 2, 3)):
        rows = [json.loads(l) for l in open(root / str(s) / 'metrics.jsonl')]
        assert [row['step'] for row in rows] == ([300, 450] if agent.live[r] else [300])
        assert all({'step', 'info/evaluation', 'steps_per_sec', 'info/q_loss', 'info/actor_loss', 'info/alpha'} <= set(row) for row in rows)
        assert len(evaluations[r]) == (4 if agent.live[r] else 3) and all(np.isfinite(v) and v < 0 for v in evaluations[r])
    assert len([json.loads(l) for l in open(root / 'halving.jsonl')]) == 1
    snap = torch.load(root / 'seed_batch.pt')
    rec = snap['device_env']['records'].numpy().view(RECORD_DTYPE)
    assert snap['device_env']['t_global'] == 450 and [int(n) for n in rec['nsteps']] == [450 if v else 300 for v in agent.live]
    assert [int(n) for n in rec['episodes_done']] == [2 if v else 1 for v in agent.live]
