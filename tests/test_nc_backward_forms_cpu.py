"""CPU-only: the switch of the noise critic's weight-gradient form (csrc/noisecritic.hip nc_dw_x3r_kernel, RLREP_DISABLE=nc_dw_rows) as the
host-only layout pass sees it, and the NumPy account of the summation order the kernel takes: float32 in that order against float64."""
import ctypes as C

import pytest


def _workspace_bytes(F, H, B=256):
    from rlrep_amd import _lib
    d = _lib.Dims()
    d.alg = _lib.ALG['vlsac']
    d.state_dim, d.action_dim, d.hidden_dim, d.actor_hidden_dim = 17, 6, H, 256
    d.feature_dim, d.vae_hidden_dim, d.num_noise, d.max_batch = F, 256, 20, B
    info = _lib.LayoutInfo()
    rc = _lib.lib.rlrep_layout(C.byref(d), C.byref(info), None, 0)
    assert rc == 0, (_lib.lib.rlrep_last_error() or b'').decode()
    return int(info.workspace_bytes)


def test_python_side_parses_the_new_tokens(monkeypatch):
    from rlrep_amd.utils import switches as sw
    monkeypatch.setenv('RLREP_DISABLE', 'chain_next;nc_dw_rows')
    assert sw.off('nc_dw_rows') and sw.off('chain_next') and not sw.off('nc_dw') and not sw.off('x3')


def test_the_dw_switch_changes_no_allocation(monkeypatch):
    """nc_dw_x3r_kernel works in the slabs and the LDS of the kernel it replaces: RLREP_DISABLE=nc_dw_rows moves no byte of the workspace"""
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    full = _workspace_bytes(256, 256)
    monkeypatch.setenv('RLREP_DISABLE', 'nc_dw_rows')
    assert _workspace_bytes(256, 256) == full


def _splits(B, F, H, ntasks=2):
    """csrc/noisecritic.hip rl_nc_dw_splits"""
    tiles = ((H + 63) // 64) * ((F + 63) // 64) * ntasks
    sp = min(max((256 + tiles - 1) // tiles, 1), 16)
    return max(min(sp, (B + 7) // 8), 1)


@pytest.mark.parametrize('B,F,H', [(5, 64, 32), (37, 96, 96), (260, 256, 256), (256, 256, 256)])
def test_the_n_major_summation_order_is_fp32_accurate(B, F, H):
    """dW[j,k] = sum_b mean[b,k] A1[b,j] + sum_n noise[n,k] * sum_b sigma[b,k] dPre[b,n,j], A1 = sum_n dPre, evaluated in float32 in the order
    of nc_dw_x3r_kernel -- per split, per chunk of 32 batch rows: the chunk's products summed first, then weighted by the noise value and added
    to the running tile; A1 summed over n in float32; the splits added in split order -- against the float64 product of the same operands
    dW = sum_{b,n} dPre[b,n,j] (mean + sigma * noise)[b,n,k].  The bar is the one tests/test_gemm_engines.py holds the bf16x3 tiles to."""
    import numpy as np
    N = 20
    rs = np.random.RandomState(B + F + H)
    # operands shaped like the launch's: GH/N * elu'(U) with elu' in (0, 1], sigma = exp(clamped log-std) > 0, unit-normal noise
    dpre = (rs.standard_normal((B, 1, H)) / N * np.minimum(rs.standard_normal((B, N, H)) + 1.0, 1.0).clip(1e-3)).astype(np.float32)
    mean = rs.standard_normal((B, F)).astype(np.float32)
    sigma = np.exp(rs.uniform(-5.0, 2.0, (B, F))).astype(np.float32)
    noise = rs.standard_normal((N, F)).astype(np.float32)
    x64 = mean.astype(np.float64)[:, None, :] + sigma.astype(np.float64)[:, None, :] * noise.astype(np.float64)[None]
    want = np.einsum('bnj,bnk->jk', dpre.astype(np.float64), x64)
    splits = _splits(B, F, H)
    bs = (B + splits - 1) // splits
    total = np.zeros((H, F), np.float32)
    for sp in range(splits):
        lo, hi = min(sp * bs, B), min(sp * bs + bs, B)
        acc = np.zeros((H, F), np.float32)
        for c0 in range(lo, hi, 32):
            c1 = min(c0 + 32, hi)
            a1 = np.zeros((c1 - c0, H), np.float32)
            for n in range(N):
                d = dpre[c0:c1, n, :].T @ sigma[c0:c1]                     # float32 accumulation over the chunk's rows
                acc = (acc + noise[n][None, :] * d).astype(np.float32)
                a1 = (a1 + dpre[c0:c1, n, :]).astype(np.float32)
            acc = (acc + a1.T @ mean[c0:c1]).astype(np.float32)
        total = (total + acc).astype(np.float32) if sp else acc
    assert total.dtype == np.float32
    e = np.linalg.norm(total - want) / np.linalg.norm(want)
    print(f'B={B} F={F} H={H}: {splits} splits, n-major float32 order vs float64: rel {e:.3e}')
    assert e < 2e-6, e
