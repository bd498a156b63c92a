"""ctrlsac seed groups (include/rlrep.h rlrep_group_create, rlrep_amd/agent/ctrlsac/seed_batch.py) on the host: the C ABI takes ctrlsac
through its group argument checks, still refuses the other representation agents first, and the launcher checks its seeds before anything
else.  No GPU."""
import ctypes as C

import pytest


def _ctrlsac_create(alg=2, members=2, stride=None, world=1, flags=0):
    """rlrep_group_create for a small ctrlsac agent with fake (never dereferenced) arena pointers laid out back to back at their real sizes;
    returns (rc, error message, member span)."""
    from rlrep_amd import _lib
    d = _lib.Dims()
    d.alg, d.state_dim, d.action_dim, d.hidden_dim, d.actor_hidden_dim, d.max_batch, d.world_size = alg, 3, 1, 256, 256, 64, world
    d.feature_dim, d.phi_hidden_dim, d.phi_hidden_depth, d.mu_hidden_dim, d.mu_hidden_depth, d.num_noise = 256, 256, 2, 256, 2, 20
    d.flags = flags
    h = _lib.Hyper()
    h.world_size = world
    sizes = [1 << 20] * 7
    if alg == 2 and world == 1:
        info = _lib.LayoutInfo()
        assert _lib.lib.rlrep_layout(C.byref(d), C.byref(info), None, 0) == 0, _lib.lib.rlrep_last_error()
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


@pytest.mark.parametrize('use_feature_target', [True, False])
@pytest.mark.parametrize('case, kw, words', [
    ('stride below the span', dict(stride=256), 'smaller than the member span'),
    ('data parallel', dict(world=2), 'data parallel'),
    ('stride not a multiple of 256', dict(stride=(1 << 24) + 4), 'multiple of 256'),
    ('no members', dict(members=0), 'members 0 outside'),
])
def test_ctrlsac_group_create_reaches_the_group_argument_checks(case, kw, words, use_feature_target):
    from rlrep_amd import _lib
    rc, msg, _ = _ctrlsac_create(flags=0 if use_feature_target else _lib.FLAG_NO_FEATURE_TARGET, **kw)
    assert rc == -1, (case, rc, msg)            # RLREP_ERR_ARG
    assert words in msg and 'sac only' not in msg, (case, msg)


@pytest.mark.parametrize('alg', [1, 3, 4])
def test_other_representation_agents_are_still_refused_first(alg):
    # (vlsac, spedersac, diffsrsac) -- rejected before any other check: a bad stride and a data-parallel world do not change the message
    for kw in (dict(), dict(stride=256), dict(world=2), dict(members=0)):
        rc, msg, _ = _ctrlsac_create(alg=alg, **kw)
        assert rc == -1, (alg, kw, rc)
        assert 'sac only' in msg and f'alg {alg}' in msg, (alg, kw, msg)


def test_launcher_checks_ctrlsac_seeds_before_the_gpu():
    from rlrep_amd import main
    with pytest.raises(SystemExit, match='distinct'):
        main.run(['--alg', 'ctrlsac', '--env', 'Pendulum-v1', '--seeds', '1,1'])
    # the distinct-seeds check does not depend on the algorithm
    with pytest.raises(SystemExit, match='distinct'):
        main.run(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '2,2'])
    for alg in ('vlsac', 'spedersac', 'diffsrsac'):
        with pytest.raises(SystemExit, match='sac only'):
            main.run(['--alg', alg, '--env', 'Pendulum-v1', '--seeds', '0,1'])


def test_ctrlsac_seed_batch_refuses_the_pipelined_form_before_the_gpu():
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    with pytest.raises(RuntimeError, match='pipeline'):
        CTRLSACSeedBatch([0, 1], 3, 1, None, pipeline=True)
