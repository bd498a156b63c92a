"""CPU-only: the library accepts every vlsac feature_dim that is a positive multiple of 4 (the LDS-table rule of the fp32 noise-critic forward
is gone: csrc/nc_fwd_body.h stages the table in 256-column chunks where it does not fit), and the planner's choice of engine at the new widths.
Host-only code paths: rlrep_layout sizes the workspace in a dry pass, rlrep_nc_fwd_plan only plans."""
import ctypes as C

import pytest


def _vlsac_dims(F, num_noise=20):
    from rlrep_amd import _lib
    d = _lib.Dims()
    d.alg = _lib.ALG['vlsac']
    d.state_dim, d.action_dim, d.hidden_dim, d.actor_hidden_dim = 17, 6, 256, 256
    d.feature_dim, d.vae_hidden_dim, d.num_noise, d.max_batch = F, 256, num_noise, 256
    return d


def _layout(d):
    from rlrep_amd import _lib
    info = _lib.LayoutInfo()
    rc = _lib.lib.rlrep_layout(C.byref(d), C.byref(info), None, 0)
    return rc, info, (_lib.lib.rlrep_last_error() or b'').decode()


def test_layout_accepts_widths_past_the_old_lds_table_limit():
    """432 was the widest accepted width (36 rows x 448 floats = 64 512 B of LDS table); 436 and everything above was refused."""
    sizes = []
    for F in (432, 436, 448, 512, 1024, 4096):
        rc, info, err = _layout(_vlsac_dims(F))
        assert rc == 0, (F, err)
        assert info.param_floats > 0 and info.workspace_bytes > 0 and info.n_tensors > 0, F
        sizes.append((info.param_floats, info.target_floats, info.grad_floats, info.workspace_bytes))
    for a, b in zip(sizes, sizes[1:]):
        assert all(y > x for x, y in zip(a, b)), (a, b)          # parameters, targets, gradients and workspace all grow with F


def test_the_rules_that_stay():
    rc, _, err = _layout(_vlsac_dims(510))
    assert rc < 0 and 'multiple of 4' in err, err
    rc, _, err = _layout(_vlsac_dims(512, num_noise=16))
    assert rc < 0 and 'num_noise' in err, err
    rc, _, err = _layout(_vlsac_dims(0))
    assert rc < 0 and 'multiple of 4' in err, err


@pytest.mark.parametrize('F,engine', [(448, 1), (512, 1), (1024, 1), (436, 0), (500, 0)])
def test_planner_engine_at_the_new_widths(F, engine, monkeypatch):
    """bf16x3 (engine 1) streams K in 32-deep steps: F % 32 == 0; every other width keeps the fp32 forward (engine 0)."""
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    out = [C.c_int32() for _ in range(3)]
    assert _lib.lib.rlrep_nc_fwd_plan(2, 37, F, 96, *[C.byref(o) for o in out]) == 0
    assert out[0].value == engine, (F, out[0].value)
    monkeypatch.setenv('RLREP_DISABLE', 'x3')
    assert _lib.lib.rlrep_nc_fwd_plan(2, 37, F, 96, *[C.byref(o) for o in out]) == 0 and out[0].value == 0


def test_abi_version_is_unchanged():
    from rlrep_amd import _lib
    assert _lib.lib.rlrep_abi_version() == 4


def _oracle_self_error(S, A, B, F, H, replay_n, trains=2):
    """Worst per-tensor relative L2 between the fp32 oracle and its fp64 form after the train() calls of test_large_dims._run, on _run's draws
    (same seeds, same order)."""
    import numpy as np
    import torch
    from fixture_io import rel_l2
    import synth
    from oracle import make_oracle
    from oracle.agents import gather_batch
    from oracle.shapes import param_shapes
    from test_large_dims import _retie
    kw = dict(hidden_dim=H, feature_dim=F, extra_feature_steps=1)
    init = synth.init_like(param_shapes('vlsac', S, A, **kw), seed=99)
    _retie('vlsac', init)
    init['log_alpha'] = np.log(np.float64(0.1))
    init['critic.noise'] = np.random.RandomState(5).standard_normal(init['critic.noise'].shape).astype(np.float32)
    init['critic_target.noise'] = init['critic.noise'].copy()
    data = synth.replay(S, A, replay_n, seed=3)
    o32, o64 = make_oracle('vlsac', S, A, init, **kw), make_oracle('vlsac', S, A, init, dtype=torch.float64, **kw)
    rs = np.random.RandomState(11)
    for _ in range(trains):
        idx = [rs.randint(0, replay_n, size=B) for _ in range(o32.n_batches())]
        eps = [rs.standard_normal((B, F)).astype(np.float32) for _ in range(2)] + [rs.standard_normal((B, A)).astype(np.float32) for _ in range(2)]
        o32.train([gather_batch(data, i) for i in idx], [torch.as_tensor(e) for e in eps])
        o64.train([gather_batch(data, i, dtype=torch.float64) for i in idx], [torch.as_tensor(e).double() for e in eps])
    a, b = o32.state(), o64.state()
    return max(rel_l2(a[k].numpy().astype(np.float64), b[k].numpy().astype(np.float64)) for k in a if not k.endswith('noise') and k != 'log_alpha')


def test_the_oracle_is_a_reference_on_every_gpu_case():
    """The GPU cases of tests/test_vlsac_widths.py hold the library to the fp32 oracle at 1e-4.  That is a check of the library only where the
    oracle's own rounding stays far inside the bar: a ReLU whose pre-activation is a few 1e-7 from zero can take either side in fp32, and the
    two sides differ by a whole gradient element (seen at (17, 6, 260, 512, 256) on a 4096-row ring: 3.8e-4; the table there says what was
    done).  Here: fp32 oracle against fp64 oracle on every case's draws, ten times inside the bar."""
    import test_vlsac_widths as g
    for S, A, B, F, H, _, replay_n in g.CASES:
        e = _oracle_self_error(S, A, B, F, H, replay_n)
        assert e < 1e-5, ((S, A, B, F, H, replay_n), e)
    for S, A, B, F, H in g.IDENTITY_CASES:
        e = _oracle_self_error(S, A, B, F, H, 4096)
        assert e < 1e-5, ((S, A, B, F, H), e)
