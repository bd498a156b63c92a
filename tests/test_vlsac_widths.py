"""vlsac at feature widths past 432, the widest the library used to accept (the fp32 noise-critic forward kept its whole mean / sigma / noise
table in LDS; csrc/nc_fwd_body.h now stages it in 256-column chunks where it does not fit).  No kernel of the family had run above F = 256:
every case here is two train() calls against the CPU oracle (test_large_dims._run: synthetic parameters, graph=False, injected draws, 1e-4 on
metrics and on per-tensor relative L2), at the smallest shapes that still reach each new path."""
import json
import os
import types

import numpy as np
import pytest

from fixture_io import rel_l2      # noqa: F401  (puts tests/golden on sys.path)
import synth
from test_large_dims import _retie, _run

pytestmark = pytest.mark.gpu

VLSAC = ('rlrep_amd.agent.vlsac.vlsac_agent', 'VLSACAgent')
CHUNKED = '[K-chunked]'


def _stage_names(agent):
    return [n for p in range(7) for n in agent.core.stages(p)]


def _plan_engine(B, F, H):
    import ctypes as C
    from rlrep_amd import _lib
    out = [C.c_int32() for _ in range(3)]
    assert _lib.lib.rlrep_nc_fwd_plan(2, B, F, H, *[C.byref(o) for o in out]) == 0
    return out[0].value


# S, A, B, F, H, engines, replay_n.  engines: 'fp32' = F % 32 != 0 keeps the fp32 forward; 'both' = the bf16x3 run and a second one under RLREP_DISABLE=x3.
# replay_n is _run's ring size (its default 4096 but for the last case): it decides which rows the fixed-seed index draws pick.  The bar is
# the fp32 oracle's, so a case is a check only where that oracle agrees with ITSELF in exact arithmetic: tests/test_vlsac_widths_cpu.py holds
# the fp32 oracle against its fp64 form on every case's draws (< 1e-5).  At (17, 6, 260, 512, 256) the draws of a 4096-row ring fail that:
# one decoder.l1 pre-activation (batch row 46, unit 159 of the first feature step) is +1.5e-7 in the fp32 oracle and -1.0e-7 in the fp64 one,
# the ReLU mask flips, and the fp32 oracle's own encoder tensors are off by 1.2e-4 ... 3.8e-4 (encoder.log_std_linear.bias) from exact
# arithmetic -- the library lands on the fp64 side, to the same three digits under every kernel form.  Rings of 1024, 2048 and 8192 rows have
# no such tie (2.2e-7 ... 2.8e-7), so that case draws from 8192: same shape, same kernels and paths, a reference that can be met.
# THIS IS A DEPARTURE from the case as first specified (the helper's default ring), made because the case missed the bar on that ring;
# docs/history/vlsac_feature_dim.md has the account.
CASES = [
    (9, 2, 37, 436, 40, 'fp32', 4096),       # the first width refused before: chunked table, ragged last chunk (Fp = 448); B % 4 != 0; H % 16 != 0
    (9, 2, 37, 500, 96, 'fp32', 4096),       # ragged chunk, K loop end != chunk end; fp32 dX / dW past 432
    (11, 3, 50, 448, 96, 'x3', 4096),        # 14 K steps; bf16x3 dX (H % 32 == 0); 7 column tiles
    (9, 2, 37, 512, 96, 'both', 4096),       # both engines at one width; the row ends on a chunk boundary
    (5, 2, 5, 1024, 32, 'both', 4096),       # a batch smaller than one tile; 32 K steps; 16 column tiles; rl_nc_dw_splits clamped by the batch
    (17, 6, 260, 512, 256, 'x3', 8192),      # one split of 260 rows; the 128-column forward (nc_fwd_x3q_kernel); the slab fold in the optimizer launch
]
IDENTITY_CASES = [(9, 2, 37, 96, 72), (17, 6, 64, 432, 64)]


@pytest.mark.parametrize('S,A,B,F,H,engines,replay_n', CASES)
def test_vlsac_past_the_old_width_limit(S, A, B, F, H, engines, replay_n, monkeypatch):
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    kw = dict(hidden_dim=H, feature_dim=F, extra_feature_steps=1)
    assert _plan_engine(B, F, H) == (0 if engines == 'fp32' else 1)
    a = _run('vlsac', VLSAC, S, A, B, kw, trains=2, replay_n=replay_n)
    chunked = [n for n in _stage_names(a) if CHUNKED in n]
    assert bool(chunked) == (engines == 'fp32'), chunked
    del a
    if engines == 'both':
        monkeypatch.setenv('RLREP_DISABLE', 'x3')
        a = _run('vlsac', VLSAC, S, A, B, kw, trains=2, replay_n=replay_n)
        assert any(CHUNKED in n for n in _stage_names(a))


def _full_state(agent):
    st = {k: v.numpy().copy() for k, v in agent.core.state().items()}
    st['exp_avg'] = agent.core.exp_avg.cpu().numpy().copy()
    st['exp_avg_sq'] = agent.core.exp_avg_sq.cpu().numpy().copy()
    return st


@pytest.mark.parametrize('S,A,B,F,H', IDENTITY_CASES)
def test_chunking_changes_no_bit(S, A, B, F, H, monkeypatch):
    """The chunked forward feeds its accumulators k in the order of the whole-table form: at widths both forms can run (432 is the widest that
    fits), parameters, targets and both Adam moments are EQUAL after two train() calls.  RLREP_ENABLE=nc_fwd_chunk forces the chunked form,
    which runs under a stage name of its own."""
    monkeypatch.setenv('RLREP_DISABLE', 'x3')
    outs = []
    for force in (False, True):
        if force:
            monkeypatch.setenv('RLREP_ENABLE', 'nc_fwd_chunk')
        else:
            monkeypatch.delenv('RLREP_ENABLE', raising=False)
        a = _run('vlsac', VLSAC, S, A, B, dict(hidden_dim=H, feature_dim=F, extra_feature_steps=1), trains=2)
        names = _stage_names(a)
        nc = [n for n in names if n.startswith('noise critic l1/l4') and 'dW' not in n]
        assert nc and all((CHUNKED in n) == force for n in nc), nc
        outs.append(_full_state(a))
        del a
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_default_mode_at_feature_dim_512():
    """The benchmarked mode (graph replay, device Philox, the two chains, the weight images the optimizer launch keeps) at F = 512, checked on the
    draws read back (test_default_mode._check_against_oracle)."""
    from oracle.shapes import param_shapes
    from test_default_mode import _check_against_oracle
    S, A, B, n = 17, 6, 64, 4096
    kw = dict(hidden_dim=256, feature_dim=512, extra_feature_steps=1)
    init = synth.init_like(param_shapes('vlsac', S, A, **kw), seed=99)
    _retie('vlsac', init)
    init['log_alpha'] = np.log(np.float64(0.1))
    init['critic.noise'] = np.random.RandomState(5).standard_normal(init['critic.noise'].shape).astype(np.float32)
    init['critic_target.noise'] = init['critic.noise'].copy()
    case = types.SimpleNamespace(name='vlsac_f512_synthetic', alg='vlsac', S=S, A=A, B=B, kw=kw, meta=dict(replay_n=n, bound=1.0), init=init,
                                 replay=synth.replay(S, A, n, seed=3))
    worst = _check_against_oracle(case, calls=3, expect_pipeline=True)
    print(f'vlsac F=512 default mode vs oracle: worst param rel-L2 {worst:.2e}')


def test_launcher_feature_dim_512(tmp_path):
    from rlrep_amd import main
    agent, evals = main.run(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--feature_dim', '512', '--max_timesteps', '300', '--start_timesteps', '150',
                             '--eval_freq', '150', '--batch_size', '64', '--eval_episodes', '1', '--log_root', str(tmp_path)])
    assert agent.feature_dim == 512
    rows = [json.loads(l) for l in open(os.path.join(tmp_path, 'Pendulum-v1', 'vlsac', '0', '0', 'metrics.jsonl'))]
    assert rows and all(np.isfinite(v) for r in rows for v in r.values())
    assert {'info/evaluation', 'steps_per_sec'} <= set(rows[-1]) and len(rows[-1]) > 4
    assert all(np.isfinite(v) for v in evals)
