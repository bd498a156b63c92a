"""Cases, host images and float64 references of the loss heads every agent shares -- csrc/elementwise.hip policy_fwd / policy_bwd / vae_mid /
heads_vae / vae_mse / qhead_critic / qhead_actor kernels, csrc/per.hip qhead_critic_w_kernel, and the 16-row engine's epilogues that replace four
of them (csrc/gemm16_tile.h EPI_FWD_POLICY, EPI_DX_POLICYBWD, EPI_FWD_MSE, EPI_DX_REPARAM with its fused short product and mse phase) -- behind
their unit-test hook (rlrep_heads), shared by tests/test_heads_kernels.py (GPU: the launches) and tests/test_heads_kernels_cpu.py (CPU: the
hook's refusals, the form every case gets, and the error bound held against a float32 emulation, clean and with planted defects).

One launch = one Case, laid out by build(case) in ONE float32 arena as tests/replearn_cases.py lays out its own (its arena helpers are imported):
64 sentinel floats around every buffer; every output whose record has a row stride has ld > width and a sentinel row behind it; every input with a
row stride has NaN padding columns and a NaN padding row; values come from one generator seeded by the case's name.  alpha_state is one double
(two words of the arena, on a 16-byte boundary).

The operations, written once below (the _f_* functions) from the reference's formulas:

  policy forward   (agent/sac/actor.py:76-91)  t = tanh(rho), l = -5 + 3.5 (t + 1), x = mu + eps exp(l), act = tanh(x) (clamped to [lo, hi] in the
                   inference form), logp = sum_j -eps^2/2 - l - log sqrt(2 pi) - 2 (log 2 - x - softplus(-2 x))
  policy backward    g = alpha / B, h = dA (1 - y^2):  d mu = 2 g y + h,  d rho = (g (-1 + 2 y eps sigma) + h eps sigma) 3.5 (1 - t^2)
  vae_mid          (vlsac_agent.py:135-150)  l = clip(l_raw, -20, 2), z = m1 + eps exp(l1), EZ = eps exp(l1) 1[l1_raw in [-20, 2]],
                   kl = l2 - l1 + (exp(2 l1) + (m1 - m2)^2) / (2 exp(2 l2)) - 1/2 and its four gradients, scaled and masked
  heads_vae        the same on (m1 | l1_raw) = Ae We^T + be, (m2 | l2_raw) = Af Wf^T + bf
  vae_mse          (vlsac_agent.py:137-140)  d = [s_hat | r_hat] - [s' | r], gradient d scale, sums of d^2 per block
  reparam dX       (vlsac_agent.py:141-150 backward)  v = A W, G[:, :F] += v, G[:, F:] += v EZ;  A = (X Wh) 1[M > 0] (fused short product);
                   X = dmse(M Wh^T + bh) (mse phase)
  qhead critic     (sac_agent.py:112-123, vlsac_agent.py:207-226)  y = R + (1 - D) gamma (min(tq1, tq2) - alpha logp), d_h = q_h - y,
                   g_h = 2 d_h / B (x w), GE_h = g_h wc_h elu'(Ec_h), sums of (w) d_h^2 and q_h per block, td = (|d1| + |d2|) / 2
  qhead actor      (sac_agent.py:141-159, vlsac_agent.py:169-180)  GE_h = -s_h / B wc_h elu'(Ec_h), s = 1 for the arg-min head, 1/2 each on a tie;
                   sums of alpha logp - min(q1, q2) and of -logp - target_entropy per block

are evaluated through the two arithmetics of replearn_cases.py (ONE copy: imported): float64 values carrying a first-order bound of the float32
evaluation's error (class V, e = 2^-24; K-term sums 2 K e sum|a_k||b_k| in any order, fused or not; expf and logf 4 ulp assumed), and NumPy float32,
which the CPU test holds to that bound and plants defects in.  The constants log 2 and log sqrt(2 pi) are the float32 numbers the kernels and
torch's float32 arithmetic use, taken as exact.  The terms that are this family's own:

  tanhf(a)      |d tanh| <= (1 - tanh^2(max(|a| - e_a, 0))) e_a (the slope at the end of the interval nearer zero, where it is largest)
                + 2 ULP e |tanh a| + 2^-126.  ULP = 4: the ROCm installation this was written against states no figure for the device library's tanhf
                (nor for log1pf) in its headers or documents, so the project's assumption for expf / logf is extended to both.  Nothing is tuned
                to a kernel's output.
  log1pf(a)     e_a / (1 + a - e_a) + 2 ULP e |log1p a|, ULP = 4 likewise
  softplus(u)   = u > 20 ? u : log1pf(expf(u)) (torch's threshold form).  The slope is a sigmoid, <= 1: e_u carries over.  Below the threshold
                (u <= 20 + e_u): expf's error through log1p's slope 1 / (1 + e^u), plus log1pf's own.  Above it (u > 20 - e_u): the branch
                returns u for log(1 + e^u), off by log1p(e^-u) <= e^-20 = 2.1e-9 < e * 20: added.  An input within e_u of 20 gets both.  The
                two branches differ by 2.1e-9 at the threshold, so no input sits on a jump.
  alpha         (float) exp((double) log_alpha): one rounding of a double result, e |alpha|
  min(a, b)     1-Lipschitz in the maximum norm: max(e_a, e_b);  clip, |.|, relu and the clamp of the action: 1-Lipschitz, e carries over
  masks         1[l_raw in [-20, 2]], 1[M > 0], elu'(Ec), 1 - y^2 of a GIVEN y, the arg-min split: decided on values the kernel takes as given
                (exact), or on computed ones that the cases keep off the jump (below)
  partial sums  n-term sums (a block's rows, a tile's elements, the 4 waves) of terms that carry their own bounds

Discontinuities.  A bound cannot cover an input on a jump, so the cases stay off them and NOTHING is left out of a comparison: every heads_vae
case keeps each computed log_std farther from -20 and 2 than its own bound, or exactly on the edge by construction (a zero weight row with the
bias at -20 or 2, which every float32 evaluation computes exactly); every qhead_actor row is an exact tie (both heads get identical Ec rows; the
two heads share weights and bias in those cases) or has |q1 - q2| above the sum of the two bounds.  tests/test_heads_kernels_cpu.py
test_every_case_carries_the_edge_inputs checks both on the float64 reference alone, with the edge inputs each case carries (edge_report below).
A case too small to hold every edge of its kind (one row, one element) holds the first ones of the list; each kind has cases that hold all.
"""
import ctypes
import zlib

import numpy as np

from replearn_cases import GUARD, TINY, U24, V, _Arena, _B32, _B64, _block_sums, _sentinel, Built, ratios, rows_blocks, window_index, windows  # noqa: F401

ULP_TANH = ULP_LOG1P = 4
LN2 = np.float32(0.69314718055994531)
HALF_LOG_2PI = np.float32(0.91893853320467274)
SENT = float(_sentinel(1)[0])             # what an unwritten output word holds


# ------------------------------------------------------------------------------------------------------------------------------------
# arithmetic on top of _B64 / _B32
# ------------------------------------------------------------------------------------------------------------------------------------
def _val(a):
    return a.v if isinstance(a, V) else np.asarray(a)


def _cat(parts, axis):
    if isinstance(parts[0], V):
        return V(np.concatenate([p.v for p in parts], axis), np.concatenate([p.e for p in parts], axis))
    return np.concatenate(parts, axis)


class _H64(_B64):
    @staticmethod
    def tanh(a):
        r = np.tanh(a.v)
        inner = np.tanh(np.maximum(np.abs(a.v) - a.e, 0.0))
        return V(r, (1.0 - inner * inner) * a.e + 2 * ULP_TANH * U24 * np.abs(r) + TINY)

    @staticmethod
    def log1p(a):
        r = np.log1p(a.v)
        return V(r, a.e / np.maximum(1.0 + a.v - a.e, 1e-300) + 2 * ULP_LOG1P * U24 * np.abs(r))

    @staticmethod
    def softplus(u, threshold=True):
        r = np.logaddexp(0.0, u.v)
        t = _B64.exp(V(np.minimum(u.v, 60.0)))                                   # (the branch below the threshold: its own input error is e_u, added once)
        low = t.e / (1.0 + t.v) + 2 * ULP_LOG1P * U24 * np.abs(np.log1p(t.v))
        high = np.exp(-np.maximum(u.v, 0.0))
        e = u.e + np.where(u.v <= 20.0 + u.e, low, 0.0) + np.where(u.v > 20.0 - u.e, high, 0.0)
        return V(r, e + U24 * np.abs(r))

    @staticmethod
    def alpha(log_alpha):
        a = np.exp(np.float64(log_alpha))
        return V(a, U24 * a)

    @staticmethod
    def minimum(a, b):
        a, b = V.of(a), V.of(b)
        return V(np.minimum(a.v, b.v), np.maximum(a.e, b.e))

    @staticmethod
    def clip(a, lo, hi):
        return V(np.clip(a.v, lo, hi), a.e)

    @staticmethod
    def relu(a):
        return V(np.maximum(a.v, 0.0), a.e)

    @staticmethod
    def abs(a):
        return V(np.abs(a.v), a.e)


class _H32(_B32):
    @staticmethod
    def tanh(a):
        return np.tanh(a, dtype=np.float32)

    @staticmethod
    def log1p(a):
        return np.log1p(a, dtype=np.float32)

    @staticmethod
    def softplus(u, threshold=True):
        u = np.asarray(u, np.float32)
        with np.errstate(over='ignore'):
            low = np.log1p(np.exp(u, dtype=np.float32), dtype=np.float32)
        return np.where(u > np.float32(20), u, low).astype(np.float32) if threshold else low

    @staticmethod
    def alpha(log_alpha):
        return np.float32(np.exp(np.float64(log_alpha)))

    @staticmethod
    def minimum(a, b):
        return np.minimum(a, b).astype(np.float32)

    @staticmethod
    def clip(a, lo, hi):
        return np.clip(a, np.float32(lo), np.float32(hi)).astype(np.float32)

    @staticmethod
    def relu(a):
        return np.maximum(a, np.float32(0)).astype(np.float32)

    @staticmethod
    def abs(a):
        return np.abs(a).astype(np.float32)


def _linear(xp, X, W, bias=None, keep=None):
    """X [M, K] . W [N, K]^T (+ bias [N]); keep: the inner indices that enter (a planted defect)"""
    if keep is not None:
        X, W = X[:, :keep], W[:, :keep]
    y = xp.matmul_t(xp.c(X), xp.c(W))
    return y if bias is None else y + xp.c(bias)[None, :]


# ------------------------------------------------------------------------------------------------------------------------------------
# the operations (h: float32 host inputs; p: the case's parameters; defect: None or one of DEFECTS -- float32 emulation only; dbg: a dict that
# receives intermediates of the float64 evaluation for edge_report)
# ------------------------------------------------------------------------------------------------------------------------------------
def _policy_sample(xp, mu, rho, eps):
    t = xp.tanh(rho)
    l = (t + 1.0) * 3.5 + (-5.0)
    sg = xp.exp(l)
    x = mu if eps is None else mu + eps * sg
    return t, l, sg, x


def _f_policy_fwd(xp, h, p, defect=None, dbg=None):
    A = p['A']
    res = {}
    for q in range(p.get('ntasks', 1)):
        s = str(q) if q else ''
        O = _linear(xp, h['X' + s], h['W' + s], h['bias' + s]) if p['fused'] else xp.c(h['O' + s])
        if p['fused']:
            res['O' + s] = O
        mu, rho = O[:, :A], O[:, A:]
        if defect == 'rho read one column off':
            rho = xp.roll(rho, -1, 1)
        eps = xp.c(h['eps' + s]) if ('eps' + s) in h else None
        t, l, sg, x = _policy_sample(xp, mu, rho, eps)
        y = xp.tanh(x)
        res['act' + s] = xp.clip(y, p['lo'], p['hi']) if p.get('clamp') else y
        sp = xp.softplus(x * -2.0, threshold=defect != 'the softplus threshold branch removed')
        corr = ((LN2 - x) - sp) * 2.0
        e2 = (eps * eps) * -0.5 if eps is not None else 0.0
        terms = ((e2 - l) - HALF_LOG_2PI) + corr if defect == 'the sign of the tanh correction' else ((e2 - l) - HALF_LOG_2PI) - corr
        if defect == 'the last action left out of logp':
            terms = terms[:, :A - 1] if A > 1 else terms * 0.0
        if p.get('logp', True):
            res['logp' + s] = xp.sum(terms, axis=1)
        if dbg is not None:
            dbg.update({'rho' + s: _val(rho), 'x' + s: _val(x), 'l' + s: _val(l), 'y' + s: _val(y)})
    if p.get('extra'):
        res['Y'] = xp.relu(_linear(xp, h['XE'], h['WE'], h['biasE']))
    return res


def _f_policy_bwd(xp, h, p, defect=None, dbg=None):
    A = p['A']
    O = xp.c(h['O'])
    rho, eps, y = O[:, A:], xp.c(h['eps']), xp.c(h['act'])
    if defect == 'rho read one column off':
        rho = xp.roll(rho, -1, 1)
    dA = xp.matmul_t(xp.c(h['Gm']), xp.c(np.ascontiguousarray(h['Wd'].T))) if p['fused'] else xp.c(h['dA'])
    g = xp.alpha(p['log_alpha']) * np.float32(p['inv_batch'])
    t, l, sg, _ = _policy_sample(xp, None, rho, None)
    hh = dA * (1.0 - y * y)
    dmu = (g * 2.0) * y + hh
    es = eps * sg
    dl = g * ((y * 2.0) * es + (-1.0)) + hh * es
    if dbg is not None:
        dbg.update(rho=_val(rho), y=_val(y), eps=_val(eps))
    return {'G': _cat([dmu, (dl * 3.5) * (1.0 - t * t)], 1)}


def _vae_core(xp, m1, l1r, m2, l2r, eps, scale, defect=None, dbg=None):
    """vae_mid on the four heads; returns (outputs, the kl term per element)"""
    in1 = (_val(l1r) >= -20.0) & (_val(l1r) <= 2.0)
    in2 = (_val(l2r) >= -20.0) & (_val(l2r) <= 2.0)
    l1, l2 = xp.clip(l1r, -20.0, 2.0), xp.clip(l2r, -20.0, 2.0)
    es = eps * xp.exp(l1)
    v1, iv2, d = xp.exp(l1 * 2.0), xp.exp(l2 * -2.0), m1 - m2
    s = v1 + d * d
    kl = ((l2 - l1) + (s * 0.5) * iv2) - 0.5
    sc = np.float32(scale)
    if defect == 'KL scale applied twice':
        sc = sc * sc
    dm1 = (d * iv2) * sc
    gl1 = ((v1 * iv2) - 1.0) * sc
    gl2 = (1.0 - s * iv2) * sc
    out = {'Z': m1 + es, 'EZ': xp.where(in1, es, 0.0),
           'GEH': _cat([dm1, gl1 if defect == 'the clamp mask missing on a log_std gradient' else xp.where(in1, gl1, 0.0)], 1),
           'GFH': _cat([-dm1 if isinstance(dm1, V) else (-dm1).astype(np.float32), xp.where(in2, gl2, 0.0)], 1)}
    if dbg is not None:
        dbg.update(l1r=l1r, l2r=l2r, d=_val(d))
    return out, kl


def _tile_owner(B, N, tiles_c):
    return ((np.arange(B) // 16)[:, None] * tiles_c + (np.arange(N) // 16)[None, :]).reshape(-1)


def _f_vae_mid(xp, h, p, defect=None, dbg=None):
    B, F = p['B'], p['F']
    EH, FH = xp.c(h['EH']), xp.c(h['FH'])
    out, kl = _vae_core(xp, EH[:, :F], EH[:, F:], FH[:, :F], FH[:, F:], xp.c(h['eps']), p['scale'], defect, dbg)
    nblk = (B * F + 255) // 256
    out['partial'] = _block_sums(xp, [kl.reshape(-1)], np.arange(B * F) // 256, nblk)
    return out


def _f_heads_vae(xp, h, p, defect=None, dbg=None):
    B, F, K = p['B'], p['F'], p['K']
    keep = 16 * (K // 16) if defect == 'the last ragged K chunk of heads_vae dropped' else None
    EH = _linear(xp, h['Ae'], h['We'], h['be'], keep)
    FH = _linear(xp, h['Af'], h['Wf'], h['bf'], keep)
    out, kl = _vae_core(xp, EH[:, :F], EH[:, F:], FH[:, :F], FH[:, F:], xp.c(h['eps']), p['scale'], defect, dbg)
    tiles_c = (F + 15) // 16
    if p.get('pair'):                                                              # (as two products + vae_mid_kernel: its block ownership)
        out['partial'] = _block_sums(xp, [kl.reshape(-1)], np.arange(B * F) // 256, (B * F + 255) // 256)
    else:
        out['partial'] = _block_sums(xp, [kl.reshape(-1)], _tile_owner(B, F, tiles_c), ((B + 15) // 16) * tiles_c)
    if p['heads_out'] or p.get('pair'):
        out['EH'], out['FH'] = EH, FH
    return out


def _f_vae_mse(xp, h, p, defect=None, dbg=None):
    B, S = p['B'], p['S']
    pred = xp.c(h['DH']) if 'DH' in h else _linear(xp, h['X'], h['W'], h['bias'])              # (given, or the layer's product: fused form and its pair)
    tgt_r = xp.c(h['s2'][:, S - 1]) if defect == "the fused MSE's reward column compared against a state column" else xp.c(h['r'])
    ds = pred[:, :S] - xp.c(h['s2'])
    dr = pred[:, S] - tgt_r
    out = {'GDH': _cat([ds * np.float32(p['scale_s']), (dr * np.float32(p['scale_r'])).reshape(B, 1)], 1)}
    zs, zr = xp.zeros((B, 1)), xp.zeros((B, S))
    es, er = _cat([ds * ds, zs], 1).reshape(-1), _cat([zr, (dr * dr).reshape(B, 1)], 1).reshape(-1)
    if p['fused'] and not p.get('pair'):
        tiles_c = (S + 1 + 15) // 16
        out['partial'] = _block_sums(xp, [es, er], _tile_owner(B, S + 1, tiles_c), ((B + 15) // 16) * tiles_c)
    else:
        out['partial'] = _block_sums(xp, [es, er], np.arange(B * (S + 1)) // 256, (B * (S + 1) + 255) // 256)
    if p.get('pair'):
        out['DH'] = pred
    return out


def _f_reparam_dx(xp, h, p, defect=None, dbg=None):
    B, F, pre = p['B'], p['F'], p['pre']
    out = {}
    if pre == 2:
        S = p['K1'] - 1
        mse = _f_vae_mse(xp, dict(X=h['M'], W=h['Wh'], bias=h['bh'], s2=h['s2'], r=h['r']), dict(B=B, S=S, fused=True, pair=False, scale_s=p['scale_s'], scale_r=p['scale_r']), defect)
        X = mse['GDH']
        pred = _linear(xp, h['M'], h['Wh'], h['bh'])
        dsq, drq = pred[:, :S] - xp.c(h['s2']), pred[:, S] - xp.c(h['r'])
        out['X'] = X                                                                # (the squared-error sums: by row tile, one pair for all its columns)
        out['partial'] = _block_sums(xp, [xp.sum(dsq * dsq, axis=1), drq * drq], np.arange(B) // 16, (B + 15) // 16)
    else:
        X = xp.c(h['X']) if pre else None
    if pre:
        # (X carries its own error in the mse form: the K1-term dot of two bounded operands, not the product of exact inputs)
        A = xp.where(h['M'] > 0, xp.dot(X.reshape(B, -1, 1), xp.c(h['Wh'].astype(np.float64))[None, :, :], 1) if isinstance(X, V) else (X @ h['Wh']).astype(np.float32), 0.0)
        out['A'] = A
    else:
        A = xp.c(h['A'])
    if isinstance(A, V):
        Wt = np.ascontiguousarray(h['W'].T).astype(np.float64)                     # [F, K]
        v = xp.dot(A.reshape(B, 1, -1), xp.c(Wt)[None, :, :], 2)
    else:
        v = (A @ h['W']).astype(np.float32)
    G = xp.c(h['G'])
    ez = xp.c(h['EZ'])
    second = G[:, F:] + (v if defect == 'the second half of a reparameterisation store written without EZ' else v * ez)
    out['G'] = _cat([G[:, :F] + v, second], 1)
    return out


def _qhead_rows(B, nblk):
    return (np.arange(B) // 4) % nblk


def _head_dot(xp, E, w, b):
    return xp.dot(xp.c(E), xp.c(w)[None, :], 1) + xp.c(b)[0]


def _elu_grad(xp, E):
    E = xp.c(E)
    return xp.where(_val(E) > 0, 1.0, E + 1.0)


def _f_qhead_critic(xp, h, p, defect=None, dbg=None):
    B, H = p['B'], p['H']
    Et, Ec = [h['Et0'], h['Et1']], [h['Ec0'], h['Ec1']]
    if defect == 'ldE ignored' and p['ldE']:
        # rows b of head h read at base_h + b * H of the interleaved [B, 2H] images
        def wrong(a0, a1, hd):
            flat = np.concatenate([a0, a1], 1).reshape(-1)
            return np.stack([flat[hd * H + b * H: hd * H + b * H + H] for b in range(B)])
        Et, Ec = [wrong(Et[0], Et[1], 0), wrong(Et[0], Et[1], 1)], [wrong(Ec[0], Ec[1], 0), wrong(Ec[0], Ec[1], 1)]
    tq = [_head_dot(xp, Et[k], h[f'wt{k}'], h[f'bt{k}']) for k in range(2)]
    q = [_head_dot(xp, Ec[k], h[f'wc{k}'], h[f'bc{k}']) for k in range(2)]
    alpha, ib = xp.alpha(p['log_alpha']), np.float32(p['inv_batch'])
    tmin = tq[0] if defect == 'min(tq1, tq2) replaced by tq1' else xp.minimum(tq[0], tq[1])
    tv = tmin - alpha * xp.c(h['logp'])
    nd = xp.c(np.float32(1) - h['D']) if defect != '(1 - D) dropped' else xp.c(np.ones(B, np.float32))     # (1 - D of a float32 D in {0, 1}: exact)
    y = xp.c(h['R']) + (nd * np.float32(p['gamma'])) * tv
    d = [q[0] - y, q[1] - y]
    g = [(d[k] * 2.0) * ib for k in range(2)]
    w = xp.c(h['w']) if p['weighted'] else None
    if w is not None:
        g = [g[k] * w for k in range(2)]
        if defect == 'w applied twice':
            g = [g[k] * w for k in range(2)]
    nblk = rows_blocks(B)
    owner = _qhead_rows(B, nblk)
    sq = [(w * d[k]) * d[k] if w is not None else d[k] * d[k] for k in range(2)]
    out = {}
    skip = np.zeros(B, bool)
    if defect == 'rows of the second grid sweep skipped':
        skip = np.arange(B) >= 4 * nblk
        owner = np.where(skip, -1, owner)
    if p['train']:
        for k in range(2):
            ge = (g[k][:, None] * xp.c(h[f'wc{k}'])[None, :]) * _elu_grad(xp, Ec[k])
            out[f'GE{k}'] = xp.where(skip[:, None], 0.0, ge)
        out['dq'] = xp.where(np.concatenate([skip, skip]), 0.0, _cat([g[0], g[1]], 0))
    out['partial'] = _block_sums(xp, [sq[0], sq[1], q[0], q[1]], owner, nblk)
    if p['weighted']:
        td = (xp.abs(d[0]) + xp.abs(d[1]))
        out['td'] = td if defect == 'td without its 0.5' else td * 0.5
    if dbg is not None:
        dbg.update(tq0=_val(tq[0]), tq1=_val(tq[1]))
    return out


def _f_qhead_actor(xp, h, p, defect=None, dbg=None):
    B = p['B']
    Ec = [h['Ec0'], h['Ec1']]
    q = [_head_dot(xp, Ec[k], h[f'wc{k}'], h[f'bc{k}']) for k in range(2)]
    alpha, ib = xp.alpha(p['log_alpha']), np.float32(p['inv_batch'])
    q0, q1 = _val(q[0]).astype(np.float64), _val(q[1]).astype(np.float64)
    s = [np.where(q0 < q1, 1.0, np.where(q1 < q0, 0.0, 0.5)), np.where(q1 < q0, 1.0, np.where(q0 < q1, 0.0, 0.5))]
    if defect == 'the tie split given whole to head 1':
        s = [np.where(q0 <= q1, 1.0, 0.0), np.where(q1 < q0, 1.0, 0.0)]
    lp = xp.c(h['logp'])
    nblk = rows_blocks(B)
    out = {}
    for k in range(2):
        gk = xp.c((-s[k]).astype(np.float32)) * ib
        out[f'GE{k}'] = (gk[:, None] * xp.c(h[f'wc{k}'])[None, :]) * _elu_grad(xp, Ec[k])
    owner = _qhead_rows(B, nblk)
    out['partial_loss'] = _block_sums(xp, [alpha * lp - xp.minimum(q[0], q[1])], owner, nblk)
    out['partial_c'] = _block_sums(xp, [(-lp if isinstance(lp, V) else (-lp).astype(np.float32)) - np.float32(p['target_entropy'])], owner, nblk)
    if dbg is not None:
        dbg.update(q0=q[0], q1=q[1])
    return out


OPS = {'policy_fwd': _f_policy_fwd, 'policy_bwd': _f_policy_bwd, 'vae_mid': _f_vae_mid, 'heads_vae': _f_heads_vae, 'vae_mse': _f_vae_mse,
       'reparam_dx': _f_reparam_dx, 'qhead_critic': _f_qhead_critic, 'qhead_actor': _f_qhead_actor}


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
# every kernel and epilogue form the hook can launch; a fused form names the gemm16 front end its launch gets (rlrep_front_end_counts:
# fast = operands from preloaded scalars, inner % 256 == 0; fastpre = the same with the fused short product; record = gemm16_kernel)
FORMS = ('policy_fwd/kernel', 'policy_fwd/gemm16:fast', 'policy_fwd/gemm16:record',
         'policy_bwd/kernel', 'policy_bwd/gemm16:fast', 'policy_bwd/gemm16:record',
         'vae_mid/kernel', 'heads_vae/load16', 'heads_vae/load4', 'vae_mse/kernel', 'vae_mse/gemm16:fast', 'vae_mse/gemm16:record',
         'reparam_dx/plain:fast', 'reparam_dx/plain:record', 'reparam_dx/pre:fastpre', 'reparam_dx/pre:record',
         'reparam_dx/pre+mse:fastpre', 'reparam_dx/pre+mse:record',
         'qhead_critic/kernel', 'qhead_critic/weighted', 'qhead_actor/kernel')
# the stand-alone kernels no step program launches any more (the builders always take the fused form): reachable through the hook only
NEVER_PLANNED = ('vae_mid/kernel', 'vae_mse/kernel')
FRONT = {'fast': 0, 'fast4': 1, 'fastpre': 2, 'record': 3}                         # index into rlrep_front_end_counts


class Case:
    def __init__(self, name, kind, form, **p):
        self.name, self.kind, self.form = name, kind, form
        self.p = dict(p, kind=kind)

    @property
    def front(self):
        return FRONT[self.form.split(':')[1]] if ':' in self.form else None


def _pow2(n):
    return n & (n - 1) == 0


def _front(K, tiles_c, ntasks=1):
    """the front end of a gemm16 launch of the cases below (every operand on a 16-byte boundary, row strides multiples of 4 where K is)"""
    return 'fast' if K % 256 == 0 and _pow2(tiles_c) and ntasks <= 2 else 'record'


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- policy forward
    for B, A, ld in ((1, 1, 1 + 2), (5, 6, 11 + 6), (3, 9, 9 + 3), (257, 17, 17 + 3)):
        add(f'policy_fwd_{B}x{A}', 'policy_fwd', 'policy_fwd/kernel', B=B, A=A, ld_act=ld, fused=0)
    add('policy_fwd_5x6_noeps', 'policy_fwd', 'policy_fwd/kernel', B=5, A=6, ld_act=17, fused=0, eps=False)
    add('policy_fwd_5x6_nologp', 'policy_fwd', 'policy_fwd/kernel', B=5, A=6, ld_act=17, fused=0, logp=False)
    add('policy_fwd_3x9_clamp', 'policy_fwd', 'policy_fwd/kernel', B=3, A=9, ld_act=12, fused=0, clamp=1, lo=-0.5, hi=0.75)
    add('policy_fwd_257x17_clamp', 'policy_fwd', 'policy_fwd/kernel', B=257, A=17, ld_act=20, fused=0, clamp=1, lo=-0.25, hi=0.5)
    for A in (1, 6, 8):
        for B in (1, 16, 17, 37):
            for K in (4, 64, 256, 260):
                add(f'policy_fwd_fused_A{A}_B{B}_K{K}', 'policy_fwd', 'policy_fwd/gemm16:' + _front(K, 1), B=B, A=A, ld_act=A + 11, fused=1, K=K)
    for K in (64, 256):
        add(f'policy_fwd_fused2_A6_B17_K{K}', 'policy_fwd', 'policy_fwd/gemm16:' + _front(K, 1, 2), B=17, A=6, ld_act=17, fused=1, K=K, ntasks=2)
    add('policy_fwd_fused2_A8_B37_K256_extra', 'policy_fwd', 'policy_fwd/gemm16:record', B=37, A=8, ld_act=19, fused=1, K=256, ntasks=2, extra=(20, 40, 12))
    add('policy_fwd_fused_A1_B16_K260_extra', 'policy_fwd', 'policy_fwd/gemm16:record', B=16, A=1, ld_act=4, fused=1, K=260, extra=(33, 17, 64))
    # ---- policy backward
    for B, A in ((1, 1), (3, 9), (257, 17)):
        add(f'policy_bwd_{B}x{A}', 'policy_bwd', 'policy_bwd/kernel', B=B, A=A, fused=0)
    for A in (1, 6, 8, 9, 16):
        for B in (1, 17, 37):
            for K in (8, 64, 512, 260):
                add(f'policy_bwd_fused_A{A}_B{B}_K{K}', 'policy_bwd', 'policy_bwd/gemm16:' + _front(K, 1), B=B, A=A, fused=1, K=K)
    # ---- vae kinds
    for B, F in ((1, 4), (3, 20), (5, 260)):
        add(f'vae_mid_{B}x{F}', 'vae_mid', 'vae_mid/kernel', B=B, F=F)
    Bs = (1, 16, 17, 37)
    for iK, K in enumerate((4, 16, 60, 64, 256, 260, 1028)):
        for iF, F in enumerate((4, 16, 20, 36)):
            B = Bs[(iK + iF) % 4]
            add(f'heads_vae_B{B}_F{F}_K{K}', 'heads_vae', 'heads_vae/load16', B=B, F=F, K=K, lda=K + 4, heads_out=(iK + iF) % 2 == 0)
    add('heads_vae_B17_F20_K61', 'heads_vae', 'heads_vae/load4', B=17, F=20, K=61, lda=64, heads_out=True)
    add('heads_vae_B17_F20_K64_lda67', 'heads_vae', 'heads_vae/load4', B=17, F=20, K=64, lda=67, heads_out=False)
    add('heads_vae_B37_F36_K64_off1', 'heads_vae', 'heads_vae/load4', B=37, F=36, K=64, lda=68, heads_out=True, a_off=1)
    add('heads_vae_B16_F4_K260_off1', 'heads_vae', 'heads_vae/load4', B=16, F=4, K=260, lda=264, heads_out=False, a_off=1)
    for B, S in ((1, 1), (5, 17), (3, 111)):
        add(f'vae_mse_{B}x{S}', 'vae_mse', 'vae_mse/kernel', B=B, S=S, fused=0)
    for S1 in (4, 16, 17, 18, 112):
        for K in (64, 256):
            for B in (1, 17, 37):
                add(f'vae_mse_fused_S{S1 - 1}_K{K}_B{B}', 'vae_mse', 'vae_mse/gemm16:' + _front(K, (S1 + 15) // 16), B=B, S=S1 - 1, fused=1, K=K)
    Bs = (1, 17, 37)
    for iF, F in enumerate((4, 16, 20)):
        for iK, K in enumerate((64, 256, 260)):
            for pre in range(3):
                B, K1 = Bs[(iF + iK + pre) % 3], (18, 32, 5)[(iF + iK) % 3]
                tiles_c = (F + 15) // 16
                form = ('plain:' + _front(K, tiles_c), 'pre:' + ('fastpre' if K % 256 == 0 else 'record'), 'pre+mse:' + ('fastpre' if K % 256 == 0 else 'record'))[pre]
                add(f'reparam_dx_pre{pre}_F{F}_K{K}_B{B}', 'reparam_dx', 'reparam_dx/' + form, B=B, F=F, K=K, pre=pre, K1=K1)
    # ---- Q heads
    for B, H in ((1, 1), (3, 64), (5, 65), (9, 260), (517, 8)):
        for ldE in (0, 2 * H):
            for wtd in (0, 1):
                add(f'qhead_critic_{B}x{H}_ld{ldE}{"_w" if wtd else ""}', 'qhead_critic', 'qhead_critic/' + ('weighted' if wtd else 'kernel'), B=B, H=H, ldE=ldE, weighted=wtd, train=1)
            add(f'qhead_actor_{B}x{H}_ld{ldE}', 'qhead_actor', 'qhead_actor/kernel', B=B, H=H, ldE=ldE)
    add('qhead_critic_5x65_ld0_eval', 'qhead_critic', 'qhead_critic/kernel', B=5, H=65, ldE=0, weighted=0, train=0)
    add('qhead_critic_9x260_ld520_w_eval', 'qhead_critic', 'qhead_critic/weighted', B=9, H=260, ldE=520, weighted=1, train=0)
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
# The edge rows of the policy cases.  A fused case realises [mu | rho] of an edge row EXACTLY as c (12.5 ... | 10 ...): the row of X is (c, 0, 0, ...),
# column 0 of W is (12.5 ... | 10 ...), the bias is zero -- every product of the row but one is an exact zero and c * 12.5, c * 10 are exact.
# (c, eps or the x to reach through eps): rho = 10 c saturates tanh (l = 2 or -5); x = 0 and +-12.5 (tanh = +-1 in float32, 1 - y^2 = 0); x on both
# sides of -10 (softplus(-2 x) crosses its threshold 20), at -25 and at -62.5 (expf(-2 x) overflows: only the threshold branch keeps softplus finite);
# eps exactly 0 and 5
POLICY_EDGES = ((1.0, 0.0, None), (-1.0, 0.0, None), (0.0, 0.0, None), (-2.0, 0.0, None), (-5.0, 0.0, None), (1.0, 5.0, None), (0.0, None, -9.9), (0.0, None, -10.1), (-1.0, 5.0, None))
MU1, RHO1 = 12.5, 10.0


def _policy_edge_eps(c, eps, x):
    if eps is not None:
        return np.float32(eps)
    l = -5.0 + 3.5 * (np.tanh(RHO1 * c) + 1.0)
    return np.float32((x - MU1 * c) / np.exp(l))


# the edge columns of the vae kinds: (l1_raw, l2_raw, m1 == m2) -- exactly on both edges, below and above, for both nets
VAE_EDGES = ((-20.0, 2.0, True), (2.0, -20.0, False), (-25.0, 3.0, False), (3.0, -25.0, False))


def build(case):
    p, k = case.p, case.kind
    rs = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    N = lambda *s: rs.standard_normal(s).astype(np.float32)
    ar, h, sc, outs, ptr2 = _Arena(), {}, {}, [], {}

    def inp(name, data, ld=None, off=0, key=None):
        data = np.asarray(data, np.float32)
        d2 = data.reshape(1, -1) if data.ndim == 1 else data.reshape(data.shape[0], -1)
        h[key or name] = data
        return ar.add(name, d2.shape[0], d2.shape[1], ld, data=d2, off=off)

    def out(name, rows, width, ld=None, keys=None):
        o = ar.add(name, rows, width, ld)
        for key, r0, nr, c0, ncol in keys or [(name, 0, rows, 0, width)]:
            outs.append((key, name, o + r0 * (ld or width) + c0, nr, ncol, ld or width))
        return o

    def inout(name, data, ld):
        o = inp(name, data, ld)
        outs.append((name, name, o, data.shape[0], data.shape[1], ld))

    def alpha_state():
        p['log_alpha'] = float(np.float64(-0.7) + 0.3 * rs.rand())
        ar.add('alpha_state', 1, 2, raw=np.array([p['log_alpha']], np.float64).view(np.int32)[None, :])

    if k == 'policy_fwd':
        B, A, fused = p['B'], p['A'], p['fused']
        nt = p.get('ntasks', 1)
        p.setdefault('lo', 0.0), p.setdefault('hi', 0.0)
        sc.update(B=B, A=A, fused=fused, ntasks=nt, clamp=p.get('clamp', 0), lo=p['lo'], hi=p['hi'])
        for q in range(nt):
            s = str(q) if q else ''
            eps = N(B, A)
            if fused:
                K = p['K']
                X = N(B, K) * np.float32(1.0 / np.sqrt(K))
                W = N(2 * A, K)
                W[A:] *= np.float32(0.7)
                bias = N(2 * A) * np.float32(0.5)
                ne = min(B, len(POLICY_EDGES))
                W[:A, 0], W[A:, 0] = MU1, RHO1
                bias_edge = ne > 0
                if bias_edge:
                    bias[:] = 0
                for r in range(ne):
                    c, e, x = POLICY_EDGES[r]
                    X[r, :] = 0
                    X[r, 0] = c
                    eps[r, :] = _policy_edge_eps(c, e, x)
                inp('X' + s, X, K + 4), inp('W' + s, W, K + 4), inp('bias' + s, bias)
                out('O' + s, B, 2 * A)
            else:
                O = np.concatenate([N(B, A), np.float32(1.5) * N(B, A)], 1)
                flat_mu, flat_rho, flat_eps = O[:, :A].reshape(-1).copy(), O[:, A:].reshape(-1).copy(), eps.reshape(-1)
                for r in range(min(B * A, len(POLICY_EDGES))):
                    c, e, x = POLICY_EDGES[r]
                    flat_mu[r], flat_rho[r] = MU1 * c, RHO1 * c
                    flat_eps[r] = _policy_edge_eps(c, e, x) if p.get('eps', True) else 0
                O[:, :A], O[:, A:] = flat_mu.reshape(B, A), flat_rho.reshape(B, A)
                inp('O' + s, O)
            if p.get('eps', True):
                inp('eps' + s, eps)
            out('act' + s, B, A, p['ld_act'])
            if p.get('logp', True):
                out('logp' + s, 1, B)
        if p.get('extra'):
            rows, Ne, Ke = p['extra']
            inp('XE', N(rows, Ke) * np.float32(1.0 / np.sqrt(Ke)), Ke + 4), inp('WE', N(Ne, Ke), Ke + 4), inp('biasE', N(Ne))
            out('Y', rows, Ne, Ne + 3)
        if fused:
            ar.add('act_pair', B + 1, p['ld_act']), ar.add('logp_pair', 1, B)                     # (test_fused_agrees_with_the_pair: the kernel's outputs)
    elif k == 'policy_bwd':
        B, A, fused = p['B'], p['A'], p['fused']
        p['inv_batch'] = float(np.float32(1.0) / np.float32(B))
        sc.update(B=B, A=A, fused=fused, inv_batch=p['inv_batch'], ld_act=A + 5, ld_dA=A)
        O = np.concatenate([N(B, A), np.float32(1.5) * N(B, A)], 1)
        eps, act = N(B, A), np.tanh(N(B, A) * np.float32(1.5)).astype(np.float32)
        fr, fe, fy = O[:, A:].reshape(-1).copy(), eps.reshape(-1), act.reshape(-1)
        # (rho, eps, y): rho = +-10; y = +-1 exactly (1 - y^2 = 0) and 0; eps exactly 0 and 5
        edges = ((10.0, 0.0, 1.0), (-10.0, 5.0, -1.0), (0.0, 0.0, 0.0), (10.0, 5.0, 0.5), (-10.0, 0.0, -0.25))
        for r in range(min(B * A, len(edges))):
            fr[r], fe[r], fy[r] = edges[r]
        O[:, A:] = fr.reshape(B, A)
        inp('O', O), inp('eps', eps), inp('act', act, A + 5)
        alpha_state()
        if fused:
            K = p['K']
            inp('Gm', N(B, K) * np.float32(1.0 / np.sqrt(K)), K + 4, key='Gm'), inp('Wd', N(K, A), A + 3)
            ar.add('dA', B, A)                                                                      # (the pair's dX output; the fused form stores nothing there)
            ar.add('G_pair', B, 2 * A)
        else:
            inp('dA', N(B, A))
        out('G', B, 2 * A)
    elif k in ('vae_mid', 'heads_vae'):
        B, F = p['B'], p['F']
        p['scale'] = float(np.float32(1.0) / np.float32(B) / np.float32(F))
        sc.update(B=B, F=F, scale=p['scale'])
        ne = min(F, len(VAE_EDGES))
        if k == 'vae_mid':
            EH = np.concatenate([N(B, F), np.float32(-1.0) + N(B, F)], 1)
            FH = np.concatenate([N(B, F), np.float32(-1.0) + N(B, F)], 1)
            for j in range(ne):
                EH[:, F + j], FH[:, F + j] = VAE_EDGES[j][0], VAE_EDGES[j][1]
                if VAE_EDGES[j][2]:
                    FH[:, j] = EH[:, j]
            inp('EH', EH), inp('FH', FH)
            out('partial', 1, (B * F + 255) // 256)
        else:
            K = p['K']
            sc.update(K=K, lda=p['lda'])
            s = np.float32(0.4 / np.sqrt(K))
            We, Wf = N(2 * F, K) * s, N(2 * F, K) * s
            be = np.concatenate([N(F), np.float32(-1.5) + np.float32(0.5) * N(F)])
            bf = np.concatenate([N(F), np.float32(-1.5) + np.float32(0.5) * N(F)])
            for j in range(ne):
                We[F + j], Wf[F + j] = 0, 0
                be[F + j], bf[F + j] = VAE_EDGES[j][0], VAE_EDGES[j][1]
                if VAE_EDGES[j][2]:
                    We[j], Wf[j] = 0, 0
                    bf[j] = be[j]
            inp('Ae', np.maximum(N(B, K), 0), p['lda'], off=p.get('a_off', 0)), inp('Af', np.maximum(N(B, K), 0), p['lda'])
            inp('We', We), inp('be', be), inp('Wf', Wf), inp('bf', bf)
            out('partial', 1, ((B + 15) // 16) * ((F + 15) // 16))
            if p['heads_out']:
                out('EH', B, 2 * F), out('FH', B, 2 * F)
                ar.add('partial_pair', 1, (B * F + 255) // 256)
                for nm in ('Z', 'EZ'):
                    ar.add(nm + '_pair', B, F)
                for nm in ('GEH', 'GFH'):
                    ar.add(nm + '_pair', B, 2 * F)
        inp('eps', N(B, F))
        out('Z', B, F), out('EZ', B, F), out('GEH', B, 2 * F), out('GFH', B, 2 * F)
    elif k == 'vae_mse':
        B, S, fused = p['B'], p['S'], p['fused']
        p['scale_r'] = float(np.float32(1.0) / np.float32(B))
        p['scale_s'] = float(np.float32(p['scale_r']) / np.float32(S))
        sc.update(B=B, S=S, fused=fused, ld_s2=2 * S + 3, scale_s=p['scale_s'], scale_r=p['scale_r'])
        if fused:
            K = p['K']
            inp('X', np.maximum(N(B, K), 0) * np.float32(1.0 / np.sqrt(K)), K + 4), inp('W', N(S + 1, K), K + 4), inp('bias', N(S + 1))
            out('partial', 1, 2 * ((B + 15) // 16) * ((S + 1 + 15) // 16))
            ar.add('DH', B, S + 1), ar.add('GDH_pair', B, S + 1), ar.add('partial_pair', 1, 2 * ((B * (S + 1) + 255) // 256))
        else:
            inp('DH', N(B, S + 1))
            out('partial', 1, 2 * ((B * (S + 1) + 255) // 256))
        inp('s2', N(B, S), 2 * S + 3), inp('r', N(B))
        out('GDH', B, S + 1)
    elif k == 'reparam_dx':
        B, F, K, pre, K1 = p['B'], p['F'], p['K'], p['pre'], p['K1']
        sc.update(B=B, F=F, K=K, pre=pre, lda=K + 4, ldw=F + 4, ldg=2 * F + 4, ldez=F + 4)
        inp('W', N(K, F) * np.float32(1.0 / np.sqrt(K)), F + 4)
        inout('G', N(B, 2 * F), 2 * F + 4)
        inp('EZ', N(B, F), F + 4)
        if pre:
            M = np.maximum(N(B, K), 0)                                                              # (a saved ReLU output: about half of it exactly 0)
            sc.update(K1=K1, ldx=K1 + 3, ldwh=K + 4, ldm=K + 8)
            inp('Wh', N(K1, K) * np.float32(1.0 / np.sqrt(K)), K + 4), inp('M', M, K + 8)
            out('A', B, K, K + 4)
            if pre == 2:
                S = K1 - 1
                p['scale_r'] = float(np.float32(1.0) / np.float32(B))
                p['scale_s'] = float(np.float32(p['scale_r']) / np.float32(S))
                sc.update(ld_s2=2 * S + 3, scale_s=p['scale_s'], scale_r=p['scale_r'])
                inp('bh', N(K1)), inp('s2', N(B, S), 2 * S + 3), inp('r', N(B))
                out('X', B, K1, K1 + 3), out('partial', 1, 2 * ((B + 15) // 16))
            else:
                inp('X', N(B, K1), K1 + 3)
        else:
            inp('A', np.where(rs.rand(B, K) < 0.5, 0, N(B, K)).astype(np.float32), K + 4)
    elif k in ('qhead_critic', 'qhead_actor'):
        B, H, ldE = p['B'], p['H'], p['ldE']
        critic = k == 'qhead_critic'
        p['inv_batch'] = float(np.float32(1.0) / np.float32(B))
        sc.update(B=B, H=H, ldE=ldE, inv_batch=p['inv_batch'])
        s = np.float32(1.0 / np.sqrt(H))

        def elu_out(n):
            x = N(B, H)
            e = np.where(x > 0, x, np.expm1(x)).astype(np.float32)
            fl = e.reshape(-1)
            for i, v in enumerate((0.0, 0.75, -0.5)[n:] + (0.0, 0.75, -0.5)[:n]):                   # entries exactly 0, positive and negative
                if i < fl.size:
                    fl[i] = v
            return e

        def pair(name, a0, a1, is_out=False):
            """two [B, H] arrays: one buffer each (ldE = 0) or interleaved rows of one [B, 2H] buffer"""
            if ldE:
                if is_out:
                    o = ar.add(name, B, 2 * H)
                    for q in range(2):
                        outs.append((f'{name}{q}', name, o + q * H, B, H, 2 * H))
                else:
                    o = ar.add(name, B, 2 * H, data=np.concatenate([a0, a1], 1))
                    h[name + '0'], h[name + '1'] = a0, a1
                ptr2[name] = (o, o + H)
            else:
                if is_out:
                    ptr2[name] = (out(name + '0', B, H), out(name + '1', B, H))
                else:
                    ptr2[name] = (inp(name + '0', a0), inp(name + '1', a1))

        Ec0, Ec1 = elu_out(0), elu_out(1)
        wc0, wc1, bc0, bc1 = N(H) * s, N(H) * s, N(1), N(1)
        if not critic:
            wc1, bc1 = wc0.copy(), bc0.copy()                                                        # (the heads share weights: an identical Ec row is an exact tie)
            ties = [b for b in range(B) if b % 3 == 1] if B > 1 else [0]
            Ec1[ties] = Ec0[ties]
            # rows 0 and 2: head 2 clearly above head 1, then clearly below (q2 - q1 = +-0.5)
            for r, sign in ((0, 1.0), (2, -1.0)):
                if r < B and r not in ties:
                    Ec1[r] = Ec0[r] + np.float32(sign * 0.5 / np.abs(wc0).sum()) * np.sign(wc0)
        if critic:
            Et0, Et1, wt0, wt1, bt0, bt1 = elu_out(1), elu_out(2), N(H) * s, N(H) * s, N(1), N(1)
            # rows 0 and 1: tq1 = bt0 (a zero row of Et0), tq2 clearly above it, then clearly below
            for r, sign in ((0, 1.0), (1, -1.0))[:B]:
                Et0[r] = 0
                Et1[r] = np.float32(sign * (abs(float(bt0[0]) - float(bt1[0])) + 1.0) / np.abs(wt1).sum()) * np.sign(wt1)
            pair('Et', Et0, Et1)
            ptr2['wt'] = (inp('wt0', wt0), inp('wt1', wt1))
            ptr2['bt'] = (inp('bt0', bt0), inp('bt1', bt1))
        pair('Ec', Ec0, Ec1)
        ptr2['wc'] = (inp('wc0', wc0), inp('wc1', wc1))
        ptr2['bc'] = (inp('bc0', bc0), inp('bc1', bc1))
        inp('logp', N(B) * np.float32(2.0) - np.float32(3.0))
        alpha_state()
        if critic:
            p['gamma'] = float(np.float32(0.99))
            sc.update(gamma=p['gamma'], train=p['train'], weighted=p['weighted'])
            D = (rs.rand(B) < 0.3).astype(np.float32)
            D[0] = 0
            if B > 1:
                D[1] = 1
            inp('R', N(B)), inp('D', D)
            if p['weighted']:
                w = rs.rand(B).astype(np.float32)
                w[0] = 1
                if B > 1:
                    w[1] = 0
                inp('w', w), out('td', 1, B)
            if p['train']:
                pair('GE', None, None, True), out('dq', 1, 2 * B)
            else:
                ar.add('GE0', B, H), ar.add('GE1', B, H), ar.add('dq', 1, 2 * B)                      # (handed to the kernel; must stay sentinel)
                ptr2['GE'] = (None, None)
            out('partial', rows_blocks(B), 4)
        else:
            p['target_entropy'] = float(np.float32(-6.0))
            sc.update(target_entropy=p['target_entropy'])
            pair('GE', None, None, True)
            out('partial_loss', 1, rows_blocks(B)), out('partial_c', 1, rows_blocks(B))
    b = Built()
    b.arena = ar.image()
    b.off = {name: start for name, start, *_ in ar.bufs}
    if k in ('qhead_critic',) and not p['train']:
        ptr2['GE'] = (b.off['GE0'], b.off['GE1'])
    b.scalars, b.h, b.p, b.ptr2 = sc, h, p, ptr2
    b.dbg = {}
    res = OPS[k](_H64, h, p, None, b.dbg)
    b.outs = []
    for key, buf, o, rows, width, ld in outs:
        r = res[key]
        b.outs.append((key, buf, o, rows, width, ld, r.v.reshape(rows, width), r.e.reshape(rows, width)))
    assert {o[0] for o in b.outs} == set(res), (case.name, sorted(set(res)), sorted(o[0] for o in b.outs))
    b.arena.setflags(write=False)
    return b


def emulate(case, built, defect=None):
    """the float32 NumPy evaluation of the case: {output name: float32 array shaped like its window}"""
    res = OPS[case.kind](_H32, built.h, built.p, defect)
    assert all(np.asarray(v).dtype == np.float32 for v in res.values()), {k: np.asarray(v).dtype for k, v in res.items()}
    return {key: np.asarray(res[key], np.float32).reshape(rows, width) for key, _, _, rows, width, _, _, _ in built.outs}


def pair_outs(case, built):
    """outs of a fused case run as the pair it replaces (a gemm16 launch through rlrep_gemm16_table, then the stand-alone kernel): the same
    element outputs at the buffers the pair writes, with the bound of the pair's own evaluation order"""
    k, p = case.kind, built.p
    if k == 'policy_fwd':
        keys = {'act': 'act_pair', 'logp': 'logp_pair'}
        res = OPS[k](_H64, built.h, p)
    elif k == 'policy_bwd':
        keys = {'G': 'G_pair'}
        res = OPS[k](_H64, built.h, p)
    elif k == 'heads_vae':
        keys = {n: n + '_pair' for n in ('Z', 'EZ', 'GEH', 'GFH', 'partial')}
        res = OPS[k](_H64, built.h, dict(p, pair=True))
    else:
        keys = {'GDH': 'GDH_pair', 'partial': 'partial_pair'}
        res = OPS[k](_H64, built.h, dict(p, pair=True))
    outs = []
    for key, buf in keys.items():
        r = res[key]
        rows, width = (r.v.shape if r.v.ndim == 2 else (1, r.v.size))
        ld = p['ld_act'] if key == 'act' else width
        outs.append((key, buf, built.off[buf], rows, width, ld, r.v.reshape(rows, width), r.e.reshape(rows, width)))
    return outs


# ------------------------------------------------------------------------------------------------------------------------------------
# the edge inputs a case carries, from the float64 reference alone
# ------------------------------------------------------------------------------------------------------------------------------------
def edge_report(case, built):
    """(carried, required): names of the edge inputs found in the case, and of those a case of its size must carry"""
    k, p, h, d = case.kind, built.p, built.h, built.dbg
    got, need = set(), set()

    def first(names, slots):
        need.update(names[:slots] if slots < len(names) else names)

    if k == 'policy_fwd':
        names = ['rho>=10 x>=12', 'rho<=-10 x<=-12', 'x==0', 'x==-25', 'x<=-60', 'eps==5', '-10<x<-9.5', '-10.5<x<-10', 'rho<=-10 eps==5']
        rho, x = d['rho'], d['x']
        eps = h.get('eps')
        tests = [(rho >= 10) & (x >= 12), (rho <= -10) & (x <= -12), x == 0, x == -25, x <= -60,
                 None if eps is None else eps == 5, (x > -10) & (x < -9.5), (x > -10.5) & (x < -10), None if eps is None else (rho <= -10) & (eps == 5)]
        for n, t in zip(names, tests):
            if t is not None and t.any():
                got.add(n)
        if 'eps' in h:
            first(names, p['B'] if p['fused'] else p['B'] * p['A'])
            if (h['eps'] == 0).any():
                got.add('eps==0')
            need.add('eps==0')
        else:
            first(names[:5], p['B'] * p['A'])
        if p.get('clamp'):
            need.update({'beyond lo', 'beyond hi'})
            if (d['y'] < p['lo']).any():
                got.add('beyond lo')
            if (d['y'] > p['hi']).any():
                got.add('beyond hi')
        if p.get('clamp') and p['B'] * p['A'] < 2:
            need -= {'beyond lo', 'beyond hi'}
    elif k == 'policy_bwd':
        names = ['rho==10 y==1 eps==0', 'rho==-10 y==-1 eps==5', 'y==0', 'rho==10 eps==5', 'rho==-10 eps==0']
        rho, y, eps = d['rho'], d['y'], d['eps']
        tests = [(rho == 10) & (y == 1) & (eps == 0), (rho == -10) & (y == -1) & (eps == 5), y == 0, (rho == 10) & (eps == 5), (rho == -10) & (eps == 0)]
        for n, t in zip(names, tests):
            if t.any():
                got.add(n)
        first(names, p['B'] * p['A'])
    elif k in ('vae_mid', 'heads_vae'):
        l1, l2 = d['l1r'], d['l2r']
        names = ['l1==-20 l2==2 m1==m2', 'l1==2 l2==-20', 'l1<-20 l2>2', 'l1>2 l2<-20']
        tests = [(l1.v == -20) & (l2.v == 2) & (d['d'] == 0), (l1.v == 2) & (l2.v == -20), (l1.v < -20) & (l2.v > 2), (l1.v > 2) & (l2.v < -20)]
        for n, t in zip(names, tests):
            if t.any():
                got.add(n)
        first(names, p['F'])
        # no computed log_std within its own bound of a clamp edge unless it sits exactly on it
        for l in (l1, l2):
            for edge in (-20.0, 2.0):
                dist = np.abs(l.v - edge)
                assert np.all((dist == 0) | (dist > l.e)), (case.name, 'a log_std within its bound of', edge)
        need.add('every log_std off the clamp edges or exactly on one')
        got.add('every log_std off the clamp edges or exactly on one')
    elif k == 'qhead_critic':
        D, B = h['D'], p['B']
        names = ['D==0', 'D==1']
        for n, t in zip(names, [D == 0, D == 1]):
            if t.any():
                got.add(n)
        first(names, B)
        for n, t in (('tq1<tq2', d['tq0'] < d['tq1']), ('tq2<tq1', d['tq1'] < d['tq0'])):
            if t.any():
                got.add(n)
        first(['tq1<tq2', 'tq2<tq1'], B)
        E = np.concatenate([h['Ec0'].reshape(-1), h['Ec1'].reshape(-1)])
        for n, t in (('Ec>0', E > 0), ('Ec==0', E == 0), ('Ec<0', E < 0)):
            if t.any():
                got.add(n)
        need.update({'Ec==0', 'Ec>0'} | ({'Ec<0'} if E.size > 2 else set()))
        if p['weighted']:
            for n, t in (('w==1', h['w'] == 1), ('w==0', h['w'] == 0)):
                if t.any():
                    got.add(n)
            first(['w==1', 'w==0'], B)
    elif k == 'qhead_actor':
        q0, q1, B = d['q0'], d['q1'], p['B']
        tie = np.all(h['Ec0'] == h['Ec1'], axis=1)
        assert np.all(q0.v[tie] == q1.v[tie])
        gap = np.abs(q0.v - q1.v)
        assert np.all(tie | (gap > q0.e + q1.e)), (case.name, 'a row neither tied nor clear of the bounds')
        for n, t in (('tie', tie), ('q1<q2', ~tie & (q0.v < q1.v)), ('q2<q1', ~tie & (q1.v < q0.v))):
            if t.any():
                got.add(n)
        need.add('tie')
        if B >= 3:
            need.update({'q1<q2', 'q2<q1'})
        E = np.concatenate([h['Ec0'].reshape(-1), h['Ec1'].reshape(-1)])
        for n, t in (('Ec>0', E > 0), ('Ec==0', E == 0), ('Ec<0', E < 0)):
            if t.any():
                got.add(n)
        need.update({'Ec==0'} | ({'Ec>0', 'Ec<0'} if E.size > 2 else set()))
    return got, need


# ------------------------------------------------------------------------------------------------------------------------------------
# the hook's record of a case
# ------------------------------------------------------------------------------------------------------------------------------------
def record(case, built, base, form=None):
    """(args, record) of the case's rlrep_heads call on a copy of its arena at address `base` (0: a plan query that touches no memory)"""
    from rlrep_amd import _lib
    a = _lib.HeadsArgs()
    r = getattr(a, case.kind)
    p, off = built.p, built.off
    at = lambda name: base + 4 * off[name] if name in off else None
    fields = {n for n, _ in r._fields_}
    for name, v in built.scalars.items():
        if name in fields:
            setattr(r, name, v)
    if form is not None:
        r.form = ctypes.cast(form, ctypes.POINTER(ctypes.c_int32))

    def layer(l, X, ldx, W, ldw, bias, K):
        l.X, l.ldx, l.W, l.ldw, l.bias, l.K = at(X), ldx, at(W), ldw, at(bias) if bias else None, K

    k = case.kind
    if k == 'policy_fwd':
        for q in range(p.get('ntasks', 1)):
            s, t = (str(q) if q else ''), r.t[q]
            t.O, t.eps, t.act, t.ld_act, t.logp = at('O' + s), at('eps' + s), at('act' + s), p['ld_act'], at('logp' + s)
            if p['fused']:
                layer(t.l, 'X' + s, p['K'] + 4, 'W' + s, p['K'] + 4, 'bias' + s, p['K'])
        if p.get('extra'):
            rows, Ne, Ke = p['extra']
            layer(r.extra.l, 'XE', Ke + 4, 'WE', Ke + 4, 'biasE', Ke)
            r.extra.Y, r.extra.ldy, r.extra.rows, r.extra.N, r.extra.act = at('Y'), Ne + 3, rows, Ne, 1
    elif k == 'policy_bwd':
        for n in ('O', 'eps', 'act', 'dA', 'alpha_state', 'G'):
            setattr(r, n, at(n))
        if p['fused']:
            layer(r.l, 'Gm', p['K'] + 4, 'Wd', p['A'] + 3, None, p['K'])
    elif k == 'reparam_dx':
        for n in ('A', 'W', 'G', 'EZ', 'X', 'Wh', 'M', 'bh', 's2', 'r', 'partial'):
            setattr(r, n, at(n))
    elif k in ('qhead_critic', 'qhead_actor'):
        for n, (o0, o1) in built.ptr2.items():
            arr = getattr(r, n)
            arr[0], arr[1] = (base + 4 * o0 if o0 is not None else None), (base + 4 * o1 if o1 is not None else None)
        for n in ('logp', 'R', 'D', 'alpha_state', 'dq', 'partial', 'w', 'td', 'partial_loss', 'partial_c'):
            if n in fields:
                setattr(r, n, at(n))
    else:
        for n, typ in r._fields_:
            if typ is ctypes.c_void_p:
                setattr(r, n, at(n))
        if k == 'vae_mse' and p['fused']:
            r.DH = None
            layer(r.l, 'X', p['K'] + 4, 'W', p['K'] + 4, 'bias', p['K'])
    return a, r


def expected_form(case):
    """what the hook reports in form[0:2] for the case"""
    f = case.form
    if case.kind == 'heads_vae':
        return (0, 1 if f.endswith('load16') else 0)
    if case.kind == 'qhead_critic':
        return (0, 1 if f.endswith('weighted') else 0)
    if case.kind == 'reparam_dx':
        return (1, case.p['pre'])
    return (1 if 'gemm16' in f else 0, 0)


# the defects the CPU test plants in the float32 emulation, each with the case it is planted in and the output that must leave the bound
DEFECTS = (
    ('rho read one column off', 'policy_fwd_5x6', 'act'),
    ('rho read one column off', 'policy_fwd_fused_A6_B17_K64', 'logp'),
    ('rho read one column off', 'policy_bwd_3x9', 'G'),
    ('the last action left out of logp', 'policy_fwd_257x17', 'logp'),
    ('the last action left out of logp', 'policy_fwd_fused_A8_B37_K256', 'logp'),
    ('the sign of the tanh correction', 'policy_fwd_3x9', 'logp'),
    ('the softplus threshold branch removed', 'policy_fwd_5x6', 'logp'),
    ('the clamp mask missing on a log_std gradient', 'vae_mid_3x20', 'GEH'),
    ('the clamp mask missing on a log_std gradient', 'heads_vae_B16_F20_K64', 'GEH'),
    ('KL scale applied twice', 'vae_mid_5x260', 'GFH'),
    ('KL scale applied twice', 'heads_vae_B17_F16_K16', 'GEH'),
    ('(1 - D) dropped', 'qhead_critic_3x64_ld0', 'dq'),
    ('min(tq1, tq2) replaced by tq1', 'qhead_critic_9x260_ld520', 'dq'),
    ('the tie split given whole to head 1', 'qhead_actor_5x65_ld0', 'GE1'),
    ('w applied twice', 'qhead_critic_5x65_ld130_w', 'GE0'),
    ('td without its 0.5', 'qhead_critic_3x64_ld0_w', 'td'),
    ('rows of the second grid sweep skipped', 'qhead_critic_517x8_ld0', 'partial'),
    ('ldE ignored', 'qhead_critic_9x260_ld520', 'GE1'),
    ("the fused MSE's reward column compared against a state column", 'vae_mse_fused_S17_K64_B17', 'partial'),
    ("the fused MSE's reward column compared against a state column", 'vae_mse_5x17', 'GDH'),
    ('the last ragged K chunk of heads_vae dropped', 'heads_vae_B16_F4_K260', 'Z'),
    ('the last ragged K chunk of heads_vae dropped', 'heads_vae_B17_F20_K61', 'EH'),
    ('the second half of a reparameterisation store written without EZ', 'reparam_dx_pre1_F20_K256_B17', 'G'),
    ('the second half of a reparameterisation store written without EZ', 'reparam_dx_pre2_F4_K64_B37', 'G'),
)
