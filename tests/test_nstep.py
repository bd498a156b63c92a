"""GPU: n-step replay for sac (csrc/nstep.hip).  The gather kernel against tests/nstep_reference.py bit for bit, a ring without
chains as plain replay, an n-step ring against the CPU oracle fed the restated batch, the graph forms against train_injected, prioritized
n-step replay, seed groups with per-member discounts, the device loop, the refusals and the launcher."""
import ctypes as C

import numpy as np
import pytest
import torch

import seed_group_util as sg
from nstep_reference import nstep_batch, nstep_slot, ring_of, trajectories
from seed_group_util import assert_equal, assert_info_equal, standalone, state

pytestmark = pytest.mark.gpu

S, A, B = 3, 1, 64              # sac Pendulum dims
WL = 'sac_pendulum_b64'
SMALL = dict(hidden_dim=64)
RTOL = 1e-4                     # the repository's bar (tests/test_hip_parity.py)
PLAIN, NSTEP, PER_NSTEP = 18, 19, 21       # kernels in a captured sac train(): plain (must not move), n-step, prioritized (with or without n-step)
GAMMA = 0.97
SLOT = ('XE', 'XF', 'XF2', 'XFpi', 'R', 'D')


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _buf(cls=None, max_size=256, s=S, a=A, **kw):
    from rlrep_amd.utils.buffer import ReplayBuffer
    return (cls or ReplayBuffer)(s, a, max_size=max_size, **kw)


def _feed(buf, rows, stride, start=0, stop=None):
    """rows [start, stop) through add_batch, `stride` at a time: what a loop over `stride` environments does"""
    stop = len(rows[3]) if stop is None else stop
    for t in range(start, stop, stride):
        buf.add_batch(*[x[t:min(t + stride, stop)] for x in rows])
    buf.flush()


def _slot(core, batch, s=S, a=A):
    """the six arrays of minibatch slot 0 of an agent / a group member, read back"""
    from rlrep_amd._lib import lib
    torch.cuda.synchronize()
    ws0 = core._group.workspace if hasattr(core, '_group') else core.workspace
    shapes = dict(XE=(batch, 2 * s + a), XF=(batch, s + a), XF2=(batch, s + a), XFpi=(batch, s + a), R=(batch,), D=(batch,))
    out = {}
    for which, k in enumerate(SLOT):
        off = lib.rlrep_slot_dev(core.h, 0, which) - ws0.data_ptr()
        n = int(np.prod(shapes[k]))
        out[k] = core.workspace[off:off + 4 * n].view(torch.float32).cpu().numpy().reshape(shapes[k])
    return out


def _assert_slot(got, want, s, what, xf2_tail=True):
    """every array the gather writes, bit for bit (of XF2 and XFpi the gather writes columns [0, S))"""
    for k in SLOT:
        g, w = np.asarray(got[k]).reshape(want[k].shape), want[k]
        if k in ('XF2', 'XFpi') and not xf2_tail:
            g, w = g[:, :s], w[:, :s]
        assert np.array_equal(_bits(g), _bits(w)), (what, k)


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', [1, 4])
@pytest.mark.parametrize('s,a', [(3, 1), (17, 6), (67, 2)])
def test_kernel_equals_the_restatement(s, a, stride):
    """a ring of 256 rows of interleaved trajectories with terminal rows and time-limit breaks, partly filled (chains run into the fill level)
    and full with the newest row in front of the oldest; every row is a base row at least once"""
    rows = trajectories(s, a, 256 + 37, stride, 100 + s + stride)
    longest = 0
    for n_rows in (150, 256 + 37):
        ring, ptr, size = ring_of([x[:n_rows] for x in rows], 256)
        for n in (1, 3, 5):
            buf = _buf(s=s, a=a, n_step=n, n_stride=stride)
            _feed(buf, rows, stride, 0, n_rows)
            torch.cuda.synchronize()
            assert (buf.ptr, buf.size) == (ptr, size) and np.array_equal(buf.ring.cpu().numpy(), ring)
            for batch in (64, 300):
                base = np.resize(np.random.default_rng(batch).permutation(size), -(-size // batch) * batch).reshape(-1, batch)
                for idx in base:
                    got = buf.gather_nstep(idx, GAMMA)
                    torch.cuda.synchronize()
                    want = nstep_slot(ring, idx, size, n, stride, GAMMA, s, a)
                    _assert_slot({k: v.cpu().numpy() for k, v in buf._nstep_last.items()}, want, s, (n_rows, n, batch))
                    assert np.array_equal(_bits(got.next_state.cpu().numpy()), _bits(want['XE'][:, s + a:]))
                    longest = max(longest, int(want['m'].max()))
                    if n == 1:
                        assert np.array_equal(want['R'], ring[idx, -2]) and np.array_equal(want['D'], ring[idx, -1])
    assert longest == 5          # chains of every length up to n occur


# ---- 2. a ring without chains is plain replay ---------------------------------------------------------------------------------------------
def _independent_rows(n, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, S)).astype(np.float32), r.uniform(-1, 1, size=(n, A)).astype(np.float32), r.normal(size=(n, S)).astype(np.float32),
            r.normal(size=n).astype(np.float32), (r.random(n) < 0.05).astype(np.float32))


def _draws(agent):
    """the indices and the noise the last graph call of `agent` drew"""
    torch.cuda.synchronize()
    idx = agent._bufs['pool_idx'].cpu().numpy().astype(np.int64)[:B]
    eps = agent._bufs['pool_eps'].cpu().numpy().reshape(2, B, A)
    return idx, [eps[0].copy(), eps[1].copy()]


def _same_agents(a, b, what):
    sa, sb = state(a.core), state(b.core)
    for st in (sa, sb):
        st.pop('train_steps')           # (the counter block's mirror word is the graph prologue's own; the counter itself: a.steps == b.steps)
    assert_equal(sa, sb, what)


def test_a_ring_without_chains_is_plain_replay_bit_for_bit():
    rows = _independent_rows(700, 3)
    nbuf, plain = _buf(max_size=1000, n_step=3), _buf(max_size=1000)
    nbuf.load(*rows)
    plain.load(*rows)
    a, twin, p = standalone(WL, 11), standalone(WL, 11), standalone(WL, 11)
    for call in range(10):
        info = a.train(nbuf, B)
        idx, eps = _draws(a)
        tinfo = twin.train_injected(plain, B, [idx], eps)
        assert_info_equal(dict(info), dict(tinfo), call)
        _same_agents(a, twin, call)
    p.train(plain, B)
    torch.cuda.synchronize()
    print(f'launches in a captured sac train(): plain {p._graph_launches}, n-step {a._graph_launches}')
    assert (p._graph_launches, a._graph_launches) == (PLAIN, NSTEP)
    assert a._graph_cache_key(plain, B) != a._graph_cache_key(nbuf, B)
    a.train(plain, B)                   # one agent, both buffers: the graph cache key tells them apart
    torch.cuda.synchronize()
    assert a._graph_launches == PLAIN


# ---- 3. the oracle on the restated batch; the graph form ----------------------------------------------------------------------------------
def test_nstep_training_matches_the_oracle_on_the_restated_batch():
    from fixture_io import Case, rel_l2
    from oracle.agents import OracleSAC, gather_batch
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    c = Case('sac_tiny')

    class Space:
        low, high = -c.meta['bound'] * np.ones(c.A, np.float32), c.meta['bound'] * np.ones(c.A, np.float32)
    agent = SACAgent(state_dim=c.S, action_dim=c.A, action_space=Space(), max_batch=B, graph=False, **c.kw)
    agent.core.load_state(c.init)
    rows = trajectories(c.S, c.A, 400, 1, 31)
    buf = _buf(max_size=512, s=c.S, a=c.A, n_step=3)
    _feed(buf, rows, 1)
    ring, _, size = ring_of(rows, 512)
    o = OracleSAC(c.S, c.A, c.init, **c.kw)
    torch.set_num_threads(4)
    rs = np.random.RandomState(5)
    gamma = np.float32(agent.discount)
    for t in range(5):
        idx = rs.randint(0, size, size=B)
        eps = [rs.standard_normal((B, c.A)).astype(np.float32) for _ in range(2)]
        info = agent.train_injected(buf, B, [idx], eps)
        want = nstep_slot(ring, idx, size, 3, 1, gamma, c.S, c.A)
        _assert_slot(_slot(agent.core, B, c.S, c.A), want, c.S, ('slot', t), xf2_tail=False)
        assert want['m'].max() == 3 and want['m'].min() == 1
        oinfo = o.train([gather_batch(nstep_batch(ring, idx, size, 3, 1, gamma, c.S, c.A), np.arange(B))], [torch.as_tensor(e) for e in eps])
        for k, v in oinfo.items():
            assert abs(info[k] - v) <= RTOL * max(abs(v), 1e-2), (t, k, info[k], v)
    st, Pm = agent.core.state(), o.state()
    worst = max(rel_l2(st[k].numpy(), Pm[k].numpy()) for k in st if k in Pm)
    print(f'n-step parity: largest relative L2 error of a parameter against the oracle {worst:.3e}')
    assert worst < RTOL


def test_graph_form_equals_train_injected_with_the_read_back_draws():
    rows = trajectories(S, A, 700, 1, 8)
    bufs = [_buf(max_size=1000, n_step=3) for _ in range(2)]
    for b in bufs:
        _feed(b, rows, 1, 0, 600)
    a, twin = standalone(WL, 2), standalone(WL, 2)
    for call in range(10):
        info = a.train(bufs[0], B)
        idx, eps = _draws(a)
        tinfo = twin.train_injected(bufs[1], B, [idx], eps)
        assert_info_equal(dict(info), dict(tinfo), call)
        _same_agents(a, twin, call)
        for b in bufs:                  # the ring grows between the calls
            _feed(b, rows, 1, 600 + 10 * call, 610 + 10 * call)
    assert a._graph_launches == NSTEP
    ring, _, size = ring_of([x[:690] for x in rows], 1000)
    _assert_slot(_slot(a.core, B), nstep_slot(ring, idx, size, 3, 1, np.float32(a.discount), S, A), S, 'last slot', xf2_tail=False)


# ---- 4. prioritized n-step replay ---------------------------------------------------------------------------------------------------------
def _tree_ok(buf):
    torch.cuda.synchronize()
    t = buf.tree.cpu().numpy()
    n = np.arange(1, len(t) // 2)
    return bool(np.array_equal(t[n], (t[2 * n] + t[2 * n + 1]).astype(np.float32)))


def test_prioritized_nstep_replay():
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer
    rows = trajectories(S, A, 700, 1, 9)
    bufs = [_buf(PrioritizedReplayBuffer, max_size=1000, n_step=3, alpha=0.6, beta=0.4) for _ in range(2)]
    for b in bufs:
        _feed(b, rows, 1)
    a, twin = standalone(WL, 4), standalone(WL, 4)
    for call in range(50):
        info = a.train(bufs[0], B)
        if call % 10 == 9 or call < 10:
            torch.cuda.synchronize()
            idx = bufs[0].draw_buffers(B)[0].cpu().numpy().astype(np.int64)
            assert idx.min() >= 0 and idx.max() < 700 and _tree_ok(bufs[0])
        if call < 10:                   # the graph form against train_injected on a twin with the read-back indices
            eps = a._bufs['pool_eps'].cpu().numpy().reshape(2, B, A)
            tinfo = twin.train_injected(bufs[1], B, [idx], [eps[0].copy(), eps[1].copy()])
            assert_info_equal(dict(info), dict(tinfo), call)
            _same_agents(a, twin, call)
            torch.cuda.synchronize()
            assert torch.equal(bufs[0].tree, bufs[1].tree)
    assert a._graph_launches == PER_NSTEP
    assert all(bool(torch.isfinite(v.float()).all()) for v in state(a.core).values())


# ---- 5. seed groups -----------------------------------------------------------------------------------------------------------------------
SEEDS = [3, 5, 11]
DISCOUNTS = [0.9, 0.97, 0.99]


def _group_rings(cls, single_cls, R, **kw):
    """a buffer group and the twins' buffers, member r holding 300 rows of a trajectory of its own; returns (group buffers, twins', rows)"""
    gb = cls(R, S, A, max_size=1000, n_step=3, **kw)
    rows = [trajectories(S, A, 400, 1, 200 + r) for r in range(R)]
    alone = []
    for r in range(R):
        gb.load(r, *[x[:300] for x in rows[r]])
        buf = single_cls(S, A, max_size=1000, n_step=3, **kw)
        buf.load(*[x[:300] for x in rows[r]])
        alone.append(buf)
    return gb, alone, rows


def _add_step(gb, alone, rows, t):
    """row t of every member's trajectory into its ring and into its twin's"""
    gb.add(*[np.stack([rows[r][q][t] for r in range(gb.members)]) for q in range(5)])
    gb.flush()
    for r, buf in enumerate(alone):
        if buf is not None:
            buf.add(*[rows[r][q][t] for q in range(5)])
            buf.flush()


def _member_pool_idx(g, r):
    """the first B entries of member r's index pool: what its last train prologue drew"""
    c = g.core
    off = g._buf('pool_idx', (B,), torch.int32).data_ptr() - c._block.data_ptr() + r * c.member_stride
    return c._block[off:off + 4 * B].view(torch.int32).cpu().numpy().astype(np.int64)


def test_group_members_equal_their_twins_and_read_their_own_discount():
    from rlrep_amd.utils.buffer import ReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    mh = [dict(discount=d) for d in DISCOUNTS]
    g = sg.group(WL, SEEDS, member_hyper=mh, **SMALL)
    twins = [standalone(WL, s, hyper=h, **SMALL) for s, h in zip(SEEDS, mh)]
    gb, alone, rows = _group_rings(ReplayBufferGroup, ReplayBuffer, 3)
    for call in range(10):
        infos = g.train(gb, B)
        for r, (twin, buf) in enumerate(zip(twins, alone)):
            tinfo = twin.train(buf, B)
            assert_info_equal(dict(infos[r]), dict(tinfo), (call, r))
            assert_equal(state(g._members[r]), state(twin.core), (call, r))
        _add_step(gb, alone, rows, 300 + call)
    assert g._graph_launches == NSTEP and twins[0]._graph_launches == NSTEP
    # a retuned member takes its new discount at the next replay, nobody else's moves: every member's slot against the restatement at its
    # own discount, on the indices its own prologue drew
    g.set_member_hyper(1, discount=0.5)
    twins[1] = None
    g.train(gb, B)
    for r in (0, 2):
        twins[r].train(alone[r], B)
        assert_equal(state(g._members[r]), state(twins[r].core), ('after the retune', r))
    torch.cuda.synchronize()
    for r, gamma in enumerate((0.9, 0.5, 0.99)):
        want = nstep_slot(gb.rings[r].cpu().numpy(), _member_pool_idx(g, r), 310, 3, 1, np.float32(gamma), S, A)
        _assert_slot(_slot(g._members[r], B), want, S, ('member slot', r), xf2_tail=False)
        assert want['m'].max() == 3
    # a retired member's block is byte-identical afterwards
    g.retire_members([2])
    before = sg.member_bytes(g, 2)
    for call in range(3):
        _add_step(gb, [alone[0], None, None], rows, 310 + call)
        infos = g.train(gb, B)
        assert infos[2] is None
        twins[0].train(alone[0], B)
    assert torch.equal(sg.member_bytes(g, 2), before)
    assert_equal(state(g._members[0]), state(twins[0].core), 'beside a retired member')


def test_group_launch_counts_and_prioritized_members():
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup, PrioritizedReplayBufferGroup
    g = sg.group(WL, SEEDS, **SMALL)
    plain = ReplayBufferGroup(3, S, A, max_size=1000)
    for r in range(3):
        plain.load(r, *[x[:300] for x in trajectories(S, A, 300, 1, 200 + r)])
    g.train(plain, B)
    torch.cuda.synchronize()
    assert g._graph_launches == PLAIN
    g = sg.group(WL, SEEDS, **SMALL)
    twins = [standalone(WL, s, **SMALL) for s in SEEDS]
    gb, alone, rows = _group_rings(PrioritizedReplayBufferGroup, PrioritizedReplayBuffer, 3, alpha=0.6, beta=0.4)
    for call in range(10):
        infos = g.train(gb, B)
        for r, (twin, buf) in enumerate(zip(twins, alone)):
            tinfo = twin.train(buf, B)
            assert_info_equal(dict(infos[r]), dict(tinfo), (call, r))
            assert_equal(state(g._members[r]), state(twin.core), (call, r))
            torch.cuda.synchronize()
            assert torch.equal(gb.trees[r], buf.tree), (call, r)
        _add_step(gb, alone, rows, 300 + call)
    assert g._graph_launches == PER_NSTEP and twins[0]._graph_launches == PER_NSTEP
    assert g._graph_cache_key(plain, B) != g._graph_cache_key(gb, B)


# ---- 6. the device loop -------------------------------------------------------------------------------------------------------------------
def test_iterate_trains_on_nstep_rows_of_interleaved_environments():
    from test_device_env_single import _agent, _env, RING
    E = 4
    agent, twin = _agent('sac'), _agent('sac', pipeline=False)
    env = _env(agent, 'pendulum', eps_greedy=0.05, start_timesteps=0, num_envs=E)
    with pytest.raises(ValueError, match='n_stride'):
        agent.iterate(env, _buf(max_size=RING, n_step=3, n_stride=1), B)
    buf, buf2 = _buf(max_size=RING, n_step=3, n_stride=E), _buf(max_size=RING, n_step=3, n_stride=E)
    for k in range(30):                 # 120 rows into a ring of 95: the wrap falls inside a step, and 95 % 4 != 0
        info = agent.iterate(env, buf, B)
        torch.cuda.synchronize()
        ring = buf.ring.cpu().numpy()
        pos = [(E * k + e) % RING for e in range(E)]
        step = ring[pos]
        buf2.add_batch(step[:, :S], step[:, S:S + A], step[:, S + A:2 * S + A], step[:, 2 * S + A], step[:, 2 * S + A + 1])
        tinfo = twin.train(buf2, B)
        assert_info_equal({k_: float(v) for k_, v in info.items()}, {k_: float(v) for k_, v in tinfo.items()}, k)
        # the device batch of this call: the ring as it stands through the restatement, at the indices the call drew
        size = min(E * (k + 1), RING)
        idx = agent._bufs['pool_idx'].cpu().numpy().astype(np.int64)[:B]
        want = nstep_slot(ring, idx, size, 3, E, np.float32(agent.discount), S, A)
        _assert_slot(_slot(agent.core, B), want, S, ('iterate slot', k), xf2_tail=False)
    assert want['m'].max() == 3
    assert_equal(state(agent.core), state(twin.core), 'iterate against the twin')
    assert agent._iter_launches == twin._graph_launches + 1 == NSTEP + 1


def test_group_iterate_trains_on_nstep_rows():
    from rlrep_amd.envs.device import DevicePendulumGroup
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    from test_device_env import _group
    from test_device_env_single import RING
    E, R = 4, 2
    g, twin = _group('sac', seeds=[3, 11]), _group('sac', seeds=[3, 11])
    env = DevicePendulumGroup(g, eps_greedy=0.05, start_timesteps=0, num_envs=E)
    with pytest.raises(ValueError, match='n_stride'):
        g.iterate(env, ReplayBufferGroup(R, S, A, max_size=RING, n_step=3, n_stride=1), B)
    gb, gb2 = (ReplayBufferGroup(R, S, A, max_size=RING, n_step=3, n_stride=E) for _ in range(2))
    for k in range(30):
        infos = g.iterate(env, gb, B)
        torch.cuda.synchronize()
        rings = gb.rings.cpu().numpy()
        pos = [(E * k + e) % RING for e in range(E)]
        step = rings[:, pos]
        gb2.add_batch(step[:, :, :S], step[:, :, S:S + A], step[:, :, S + A:2 * S + A], step[:, :, 2 * S + A], step[:, :, 2 * S + A + 1])
        tinfos = twin.train(gb2, B)
        for r in range(R):
            assert_info_equal({k_: float(v) for k_, v in infos[r].items()}, {k_: float(v) for k_, v in tinfos[r].items()}, (k, r))
    for r in range(R):
        assert_equal(state(g._members[r]), state(twin._members[r]), ('group iterate', r))
    assert g._iter_launches == twin._graph_launches + 1 == NSTEP + 1


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_everything_but_sac_refuses_an_nstep_buffer():
    from fixture_io import Case
    from rlrep_amd._lib import lib
    from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    c = Case('vlsac_tiny')

    class Space:
        low, high = -np.ones(c.A, np.float32), np.ones(c.A, np.float32)
    v = VLSACAgent(state_dim=c.S, action_dim=c.A, action_space=Space(), max_batch=c.B, vae_hidden_dim=c.meta['patch_vae_hidden'], **c.kw)
    with pytest.raises(RuntimeError, match=r'ReplayBuffer\(n_step=3\)'):
        v.train(_buf(s=c.S, a=c.A, n_step=3), c.B)
    cg = sg.group('ctrlsac_pendulum_b64', [0, 1]) if 'ctrlsac_pendulum_b64' in sg.bench.WORKLOADS else None
    if cg is None:
        from test_device_env import _group
        cg = _group('ctrlsac', seeds=[0, 1])
    with pytest.raises(RuntimeError, match=r'ReplayBufferGroup\(n_step=3\)'):
        cg.train(ReplayBufferGroup(2, S, A, max_size=256, n_step=3), B)
    # the C entry points with the wrong kind of handle, by name
    g, a = sg.group(WL, [0, 1], **SMALL), standalone(WL, 3, **SMALL)
    buf = _buf(n_step=3)
    buf.load(*[x for x in trajectories(S, A, 100, 1, 0)])
    idx = torch.zeros(B, dtype=torch.int32, device='cuda')
    args = (C.c_void_p(buf.ring.data_ptr()), C.c_void_p(idx.data_ptr()), B, buf.max_size, C.c_void_p(buf.size_dev().data_ptr()), 3, 1, None)
    for core, word in ((g.core, 'seed group'), (v.core, 'sac only')):
        rc = lib.rlrep_replay_sample_nstep(core.h, 0, *args)
        assert rc < 0 and word in lib.rlrep_last_error().decode() and 'replay_sample_nstep' in lib.rlrep_last_error().decode()
    rc = lib.rlrep_group_replay_gather_nstep(a.core.h, C.c_void_p(buf.ring.data_ptr()), 0, C.c_void_p(idx.data_ptr()), 1, B, buf.max_size,
                                             C.c_void_p(buf.size_dev().data_ptr()), 3, 1, None)
    assert rc < 0 and 'not a seed group' in lib.rlrep_last_error().decode() and 'group_replay_gather_nstep' in lib.rlrep_last_error().decode()
    rc = lib.rlrep_group_replay_gather_nstep(cg.core.h, C.c_void_p(buf.ring.data_ptr()), 0, C.c_void_p(idx.data_ptr()), 1, B, buf.max_size,
                                             C.c_void_p(buf.size_dev().data_ptr()), 3, 1, None)
    assert rc < 0 and 'sac seed groups only' in lib.rlrep_last_error().decode()
    for n, stride in ((0, 1), (17, 1), (3, 0)):
        rc = lib.rlrep_replay_sample_nstep(a.core.h, 0, *args[:5], n, stride, None)
        assert rc < 0 and 'replay_sample_nstep' in lib.rlrep_last_error().decode()
    torch.cuda.synchronize()


# ---- 8. the launcher ----------------------------------------------------------------------------------------------------------------------
def test_launcher_runs_with_nstep_and_per(tmp_path):
    from rlrep_amd import main
    agent, evaluations = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--n-step', '3', '--per', '--batch_size', '64', '--eval_episodes', '1',
                                   '--log_root', str(tmp_path), '--start_timesteps', '300', '--eval_freq', '300', '--max_timesteps', '600'])
    assert np.all(np.isfinite(evaluations)) and len(evaluations) >= 2
    buf = agent._held_buffer
    assert type(buf).__name__ == 'PrioritizedReplayBuffer' and (buf.n_step, buf.n_stride) == (3, 1) and _tree_ok(buf)
    assert agent._graph_launches == PER_NSTEP


@pytest.mark.parametrize('extra, cls, stride', [
    (['--seeds', '0,1', '--sweep', 'discount=0.97,0.99', '--start_timesteps', '300', '--eval_freq', '300', '--max_timesteps', '600'], 'ReplayBufferGroup', 1),
    (['--seeds', '0,1', '--group-per', '--start_timesteps', '300', '--eval_freq', '300', '--max_timesteps', '600'], 'PrioritizedReplayBufferGroup', 1),
    (['--seeds', '0,1', '--device-env', '--num-envs', '4', '--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '480'], 'ReplayBufferGroup', 4),
    (['--device-loop', '--num-envs', '4', '--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '480'], 'ReplayBuffer', 4),
    (['--host-envs', '4', '--start_timesteps', '160', '--eval_freq', '160', '--max_timesteps', '480'], 'ReplayBuffer', 4),
    (['--torch-envs', '8', '--start_timesteps', '304', '--eval_freq', '304', '--max_timesteps', '608'], 'ReplayBuffer', 8),
])
def test_launcher_loops_build_nstep_buffers_with_their_own_stride(tmp_path, extra, cls, stride):
    from rlrep_amd import main
    agent, evaluations = main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--n-step', '3', '--batch_size', '64', '--eval_episodes', '1',
                                   '--log_root', str(tmp_path)] + extra)
    assert np.all(np.isfinite(np.asarray(evaluations, np.float64)))
    device = '--device-env' in extra or '--device-loop' in extra
    # what the captured graph baked in: the cache key ends in the buffer's ('nstep', n_step, n_stride)
    key = next(iter(agent._iter_graphs))[0] if device else agent._graph_key
    assert key[-3:] == ('nstep', 3, stride)
    buf = getattr(agent, 'replay', None) or agent.__dict__.get('_held_env_buffer')        # (the plain single-agent loops keep no handle on the ring)
    if buf is not None:
        assert type(buf).__name__ == cls and (buf.n_step, buf.n_stride) == (3, stride)
    launches = agent._iter_launches - 1 if device else agent._graph_launches
    assert launches == (PER_NSTEP if '--group-per' in extra else NSTEP)
