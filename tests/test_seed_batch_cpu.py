"""Seed groups (include/rlrep.h rlrep_group_create, rlrep_amd/agent/sac/seed_batch.py) on the host: argument checks of the C ABI and the
staging / wrap logic of ReplayBufferGroup.  No GPU."""
import ctypes as C

import numpy as np
import pytest


def _create(alg=0, members=2, stride=None, world=1, span_pad=0):
    """rlrep_group_create with fake (never dereferenced) arena pointers laid out back to back; returns (rc, error message)."""
    from rlrep_amd import _lib
    d = _lib.Dims()
    d.alg, d.state_dim, d.action_dim, d.hidden_dim, d.actor_hidden_dim, d.max_batch, d.world_size = alg, 3, 1, 256, 256, 64, world
    if alg != 0:
        d.feature_dim, d.vae_hidden_dim, d.num_noise = 256, 256, 20
    h = _lib.Hyper()
    h.world_size = world
    info = _lib.LayoutInfo()
    sizes = [1 << 20] * 7
    if alg == 0:
        assert _lib.lib.rlrep_layout(C.byref(d), C.byref(info), None, 0) == 0
        sizes = [4 * info.param_floats, 4 * info.target_floats, 4 * info.grad_floats, 4 * info.param_floats, 4 * info.param_floats,
                 int(info.workspace_bytes), 32]
    base, ptrs = 1 << 32, []
    for n in sizes:
        ptrs.append(base)
        base += (n + 255) & ~255
    span = base - (1 << 32)
    a = _lib.Arenas(*ptrs)
    out = C.c_void_p()
    rc = _lib.lib.rlrep_group_create(C.byref(d), C.byref(h), C.byref(a), members, span if stride is None else stride, None, C.byref(out))
    return rc, (_lib.lib.rlrep_last_error() or b'').decode(), span


@pytest.mark.parametrize('case, kw, words', [
    ('not sac', dict(alg=1), 'sac only'),
    ('no members', dict(members=0), 'members 0 outside'),
    ('too many members', dict(members=100000), 'outside'),
    ('data parallel', dict(world=2), 'data parallel'),
    ('stride not a multiple of 256', dict(stride=(1 << 24) + 4), 'multiple of 256'),
    ('stride below the span', dict(stride=256), 'smaller than the member span'),
])
def test_group_create_rejects_bad_arguments_with_a_message(case, kw, words):
    rc, msg, _ = _create(**kw)
    assert rc == -1, (case, rc)             # RLREP_ERR_ARG
    assert words in msg, (case, msg)


def test_group_limits():
    from rlrep_amd import _lib
    assert _lib.lib.rlrep_group_max_members() >= 16
    assert _lib.lib.rlrep_group_members(None) < 0


def test_group_entry_points_refuse_a_plain_or_missing_agent():
    from rlrep_amd import _lib
    seeds = (C.c_uint64 * 2)(1, 2)
    assert _lib.lib.rlrep_group_set_seeds(None, C.cast(seeds, C.c_void_p), 2, None) < 0
    assert 'one seed per member' in _lib.lib.rlrep_last_error().decode()
    assert _lib.lib.rlrep_group_train_prologue(None, None, 0, None, None, 0, None, 0, 0, 0, 64, None) < 0
    assert 'not a seed group' in _lib.lib.rlrep_last_error().decode()
    assert _lib.lib.rlrep_group_replay_add_sized(None, 0, 2, 16, 9, 0, None, 0, 1, None, 1, None) < 0
    assert 'bad argument' in _lib.lib.rlrep_last_error().decode()


def test_replay_buffer_group_staging_and_wrap_on_the_host():
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    R, S, A, cap = 3, 2, 1, 5
    g = ReplayBufferGroup(R, S, A, max_size=cap, device='cpu', stage_rows=3)
    row = 2 * S + A + 2
    assert g.rings.shape == (R, cap, row) and g.ring_stride == cap * row and g.ring.data_ptr() == g.rings.data_ptr()

    def tr(t):          # member r's transition t: every field encodes (member, step)
        m = np.arange(R, dtype=np.float32)[:, None]
        return (100 * m + t + np.zeros((R, S)), 100 * m + t + 0.5 + np.zeros((R, A)), -(100 * m + t) + np.zeros((R, S)),
                (100 * m[:, 0] + t), (t % 2) + np.zeros(R))
    for t in range(7):                   # 7 rows into a 5-row ring through a 3-row stage: two automatic flushes and a wrap
        g.add(*tr(t))
    g.flush()
    assert g.sizes == [cap] * R and g.ptr == 7 % cap
    for r in range(R):
        for t in range(7):
            if t < 2:
                continue                  # overwritten by t = 5, 6
            rowv = g.rings[r, t % cap].numpy()
            assert rowv[0] == 100 * r + t and rowv[S] == 100 * r + t + 0.5 and rowv[S + A] == -(100 * r + t)
            assert rowv[2 * S + A] == 100 * r + t and rowv[2 * S + A + 1] == t % 2
    assert list(g.size_dev().numpy()) == [cap] * R


def test_replay_buffer_group_load_is_per_member():
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    g = ReplayBufferGroup(2, 1, 1, max_size=8, device='cpu')
    n = 3
    g.load(1, np.ones((n, 1)), 2 * np.ones((n, 1)), 3 * np.ones((n, 1)), 4 * np.ones(n), np.zeros(n))
    assert g.sizes == [0, 3] and float(g.rings[0].abs().sum()) == 0.0
    assert g.rings[1, :n].tolist() == [[1, 2, 3, 4, 0]] * n


def test_launcher_seeds_refuses_other_algorithms_before_the_gpu():
    from rlrep_amd import main
    with pytest.raises(SystemExit, match='sac only'):
        main.run(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '0,1'])
    with pytest.raises(SystemExit, match='distinct'):
        main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '1,1'])
