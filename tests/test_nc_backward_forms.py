"""The weight-gradient launch of the vlsac noise critic and the two orders it can take its inner rows in (csrc/noisecritic.hip).

nc_dw_x3r_kernel (the default) steps by noise row: a step is one noise row n and 32 batch rows, its B operand the sigma block that the
producers split once per chunk, and the step's products are weighted by noise[n, k] as they are folded into the tile; one more step per chunk
multiplies A1 = sum_n dPre by the mean block.  RLREP_DISABLE=nc_dw_rows keeps nc_dw_x3_kernel, which rebuilds x = mean + sigma * noise for
every inner row.  The rounding points differ, so the two forms agree to fp32 accuracy, not bit for bit.

Every case is test_large_dims._run: synthetic parameters, graph=False, injected draws, two train() calls against the fp32 CPU oracle at 1e-4 on
metrics and per-tensor relative L2."""
import numpy as np
import pytest
import torch

from fixture_io import rel_l2      # noqa: F401  (puts tests/golden on sys.path)
import synth
from test_large_dims import _retie, _run, _Space

pytestmark = pytest.mark.gpu

VLSAC = ('rlrep_amd.agent.vlsac.vlsac_agent', 'VLSACAgent')

# S, A, B, F, H
CASES = [
    (5, 2, 5, 64, 32),          # one dW split clamped by the batch, one chunk of 5 rows; a batch one row past a 4-row dX tile; F at the engine's minimum
    (7, 3, 37, 96, 96),         # H and F no multiples of 64 (partial dW tiles, a partial dX column tile); a ragged last split
    (17, 6, 260, 256, 256),     # the headline tiling with a batch that is no multiple of the split size: 33 rows per split = a chunk of 32 and a chunk of 1
]
FORMS = ['', 'nc_dw_rows']      # RLREP_DISABLE= of the run


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', CASES)
def test_every_form_matches_the_oracle(case, form, monkeypatch):
    S, A, B, F, H = case
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    if form:
        monkeypatch.setenv('RLREP_DISABLE', form)
    else:
        monkeypatch.delenv('RLREP_DISABLE', raising=False)
    _run('vlsac', VLSAC, S, A, B, dict(hidden_dim=H, feature_dim=F, extra_feature_steps=1), trains=2)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', CASES)
def test_dw_by_noise_row_is_fp32_accurate(case, form, monkeypatch):
    """critic.l1 / l4 gradients of ONE critic step against float64, at the bar tests/test_gemm_engines.py holds the bf16x3 tiles to (2e-6 of the
    float64 result's norm).  The reference is the float64 oracle's gradient of the same step from the same parameters and draws: the whole
    chain in float64, so the bar also covers the fp32 rounding of everything upstream of the launch.  Both forms of the launch are held to it
    (tests/test_nc_backward_forms_cpu.py has the NumPy account of the n-major order).  The gradients are read where the critic group's
    optimizer launch leaves the summed split partials.  Measured on MI355X: 0.8e-7 ... 2.7e-7 in either form."""
    from oracle import make_oracle
    from oracle.agents import gather_batch
    from oracle.shapes import param_shapes
    from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
    from rlrep_amd.utils.buffer import ReplayBuffer
    S, A, B, F, H = case
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    if form:
        monkeypatch.setenv('RLREP_DISABLE', form)
    else:
        monkeypatch.delenv('RLREP_DISABLE', raising=False)
    kw = dict(hidden_dim=H, feature_dim=F, extra_feature_steps=1)
    init = synth.init_like(param_shapes('vlsac', S, A, **kw), seed=99)
    _retie('vlsac', init)
    init['log_alpha'] = np.log(np.float64(0.1))
    init['critic.noise'] = np.random.RandomState(5).standard_normal(init['critic.noise'].shape).astype(np.float32)
    init['critic_target.noise'] = init['critic.noise'].copy()
    agent = VLSACAgent(state_dim=S, action_dim=A, action_space=_Space(A), max_batch=B, graph=False, **kw)
    agent.core.load_state(init)
    data = synth.replay(S, A, 4096, seed=3)
    buf = ReplayBuffer(S, A, max_size=4096)
    buf.load(data['state'], data['action'], data['next_state'], data['reward'], data['done'])
    rs = np.random.RandomState(11)
    idx = rs.randint(0, 4096, size=B)
    eps = rs.standard_normal((B, A)).astype(np.float32)
    agent.critic_step(buf.gather(torch.as_tensor(idx, device='cuda')), eps=torch.as_tensor(eps, device='cuda'))
    o = make_oracle('vlsac', S, A, init, dtype=torch.float64, **kw)
    o.critic_step(gather_batch(data, idx, dtype=torch.float64), torch.as_tensor(eps).double())
    for name in ('critic.l1.weight', 'critic.l4.weight', 'critic.l1.bias', 'critic.l4.bias'):
        got = agent.core.view(name, 'grad').cpu().numpy().astype(np.float64)
        want = o.last_grads['critic'][name].numpy()
        e = _rel(got, want)
        print(f'{case} RLREP_DISABLE={form!r} {name}: rel {e:.3e}')
        assert e < 2e-6, (name, e)
