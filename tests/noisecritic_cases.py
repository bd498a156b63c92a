"""Cases, host images and float64 references of the vlsac noise-critic kernels (csrc/noisecritic.hip) behind their unit-test hook
(rlrep_noisecritic), shared by tests/test_noisecritic_kernels.py (GPU: the launches) and tests/test_noisecritic_kernels_cpu.py (CPU: the hook's
refusals, the form every case gets, and the error bound held against a float32 emulation, clean and with planted defects).

One launch = one Case, laid out by build(case) in ONE float32 arena as tests/replearn_cases.py lays out its own: 64 sentinel floats around every
buffer; every input with a row stride (mean | log_std through ld_ml, GH through ldgh) has ld > width with NaN padding columns and a NaN padding row
(the half of a (mean | log_std) row a kernel has no business reading is NaN as well); every output has a sentinel row behind it (G, the one output
with a stride, sentinel padding columns too); values come from one generator seeded by the case's name.

The operations (N = 20 noise rows, reference agent/vlsac/vlsac_agent.py:44-63), written once below:

  forward   sigma = exp(clip(log_std, -20, 2));  x[b,n,:] = mean[b] + sigma[b] noise[n];  U = elu(x W^T + bias);  Hm = (1/20) sum_n U;  sigma_out = sigma
  dX        dPre_h[b,n,j] = GH_h[b,j]/20 min(U_h[b,n,j] + 1, 1);  D[b,n,k] = sum_h sum_j dPre_h[b,n,j] W_h[j,k];  G[b,k] = sum_n D[b,n,k];
            G[b,F+k] = (sum_n noise[n,k] D[b,n,k]) sigma[b,k] 1[-20 <= log_std[b,k] <= 2]
  dW        gW[j,k] = sum_{b,n} dPre[b,n,j] (mean[b,k] + sigma[b,k] noise[n,k]);  gb[j] = sum_{b,n} dPre[b,n,j]      (sigma is an input)

are evaluated through the two arithmetics of replearn_cases.py (ONE copy: imported): _B64, float64 values carrying a first-order bound of the
float32 evaluation's error (e = 2^-24; K-term sums 2 K e sum|a_k||b_k| in any order; expf 4 ulp assumed), and _B32, NumPy float32, which the CPU
test holds to that bound and plants defects in.  Three terms are this family's own; each is derived here from the device code.

elu_fast (common.h: x > 0 ? x : exp2(x * 1.4426950408889634f) - 1).  For x <= 0: the constant c = fl(log2 e) and the product t = fl(x c) are one
rounding each, |t - x log2 e| <= |x| log2 e 2^-23; 2^t then differs from e^x by e^x ln 2 |t - x log2 e| <= e^x |x| 2^-23; v_exp_f32 is good to one ulp
of its result, <= e^x 2^-23; the subtraction rounds once, <= 2^-24 |y| (exact for e^x in [1/2, 1]).  Together
        |elu_fast(x) - elu(x)| <= 2^-23 e^x (1 + |x|) + 2^-24 |y|.
The product's rounding does scale with |x|, but under the factor e^x: e^x (1 + |x|) decreases from 1 at x = 0, so the supremum of the whole
expression is 1.32e-7 (near x = -0.55) -- common.h's "about 1.5e-7 absolute" holds, and the per-element form above is what the bound uses (it
goes to 2^-24 for x << 0, where the result is -1).  Results whose e^x is under 2^-126 are flushed: covered by the 2^-126 every exponential carries.
An error e_x of the pre-activation enters through the slope, e^x for x <= 0 and 1 above; within e_x of zero the slope 1 and the fast term both apply.

__expf of the bf16x3 forwards (their operand sigma; sigma_out is expf in every form): v_exp_f32 of fl(c fl(log2 e)), by the same two roundings
relative 2^-23 |c| and one ulp on top: relative 2 e (|c| + 1), up to 21 * 2^-23 at log_std = -20.

bf16x3 (x3.h).  x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m): round-to-nearest to 8 significand bits, so |x - h| <= 2^-8 |x|,
|m| <= 2^-8 (1 + 2^-8) |x|, |x - h - m| <= 2^-16 |x| and l, which has 8 bits left to hold at most 8, is exact: the split loses nothing.  Of the nine
products of two split operands six are multiplied (l h, h l, m m, m h, h m, h h); dropped are m_a l_b, l_a m_b <= 2^-24 (1 + 2^-8) |a||b| each and
l_a l_b <= 2^-32 |a||b|: <= 2.05 e |a||b| per product.  The bf16 MFMA multiplies exactly (8 x 8 bits) and accumulates in float32, which the K-term
sum term covers; a bf16x3 product therefore gets (2 K + 2.05) e sum|a_k||b_k|.  The float32 emulation of a bf16x3 form does the split and multiplies
the six kept images itself (float32 accumulation of six float32 matrix products).

dW orders.  nc_dw_kernel and nc_dw_x3_kernel sum products dPre[r,j] x[r,k] over the rows r = (b, n) of a split; nc_dw_x3r_kernel takes a split in
chunks of 32 batch rows and per chunk computes sum_n noise[n,k] (sum_b sigma[b,k] dPre[b,n,j]) + sum_b mean[b,k] A1[b,j], A1 = sum_n dPre: another
expression (its bound has |mean| + |sigma||noise| where the row order has |mean + sigma noise|), so reference bound and emulation of a case follow
the order of the kernel the case names.  Split partials are added in split order (nc_dw_fin_kernel).
"""
import ctypes
import zlib

import numpy as np

from replearn_cases import GUARD, TINY, U24, V, _B32, _B64, _sentinel, ratios, window_index  # noqa: F401  (one copy of the bound arithmetic)

NN = 20                                   # noise rows
X3_DROPPED = 2.05                         # e |a||b| of the three dropped partial products (docstring)
LOG2E = np.float32(1.4426950408889634)
SENT = float(_sentinel(1)[0])             # what an unwritten output word holds


# ------------------------------------------------------------------------------------------------------------------------------------
# arithmetic helpers on top of _B64 / _B32
# ------------------------------------------------------------------------------------------------------------------------------------
def _val(a):
    return a.v if isinstance(a, V) else a


def _T(a, *axes):
    return V(np.transpose(a.v, axes), np.transpose(a.e, axes)) if isinstance(a, V) else np.transpose(a, axes)


def _cat(parts, axis):
    if isinstance(parts[0], V):
        return V(np.concatenate([p.v for p in parts], axis), np.concatenate([p.e for p in parts], axis))
    return np.concatenate(parts, axis)


def bf16_round(x):
    """float32 -> nearest bf16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + (np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    """x3_split2 of x3.h: the three bf16 images of a float32 array, as float32 arrays"""
    x = np.asarray(x, np.float32)
    h = bf16_round(x)
    r = (x - h).astype(np.float32)
    m = bf16_round(r)
    return h, m, bf16_round((r - m).astype(np.float32))


def _mm_t(xp, a, b, x3=False, drop=None):
    """a [.., M, K] . b [N, K]^T.  x3: on the bf16x3 engines (bound: + the dropped products; emulation: split, six products; drop: one more left out)"""
    if xp is _B64:
        a, b = V.of(a), V.of(b)
        K = a.v.shape[-1]
        aa, ab = np.abs(a.v), np.abs(b.v)
        return V(a.v @ b.v.T, (2 * K + (X3_DROPPED if x3 else 0)) * U24 * (aa @ ab.T) + aa @ b.e.T + a.e @ ab.T)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if not x3:
        return (a @ b.T).astype(np.float32)
    (ah, am, al), (bh, bm, bl) = split3(a), split3(b)
    acc = None
    for i, (p, q) in enumerate(((al, bh), (ah, bl), (am, bm), (am, bh), (ah, bm), (ah, bh))):       # the kernels' order of the six MFMAs
        if i != drop:
            t = (p @ q.T).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
    return acc


def _exp_fast(xp, c):
    """__expf: v_exp_f32 of c * log2 e"""
    if xp is _B64:
        r = np.exp(c.v)
        return V(r, r * c.e + 2 * (np.abs(c.v) + 1) * U24 * r + TINY)
    with np.errstate(under='ignore'):
        return np.exp2((c * LOG2E).astype(np.float32)).astype(np.float32)


def _elu_fast(xp, x):
    if xp is _B64:
        neg = np.minimum(x.v, 0.0)
        ex = np.exp(neg)
        y = np.where(x.v > 0, x.v, np.expm1(neg))
        fast = np.where(x.v <= x.e, 2 * U24 * ex * (1 - neg) + U24 * np.abs(y) + TINY, 0.0)
        return V(y, x.e * np.where(x.v > -x.e, 1.0, ex) + fast)
    with np.errstate(under='ignore'):
        return np.where(x > 0, x, np.exp2((np.minimum(x, np.float32(0)) * LOG2E).astype(np.float32)) - np.float32(1)).astype(np.float32)


def _clip(xp, ls):
    return V(np.clip(ls.v, -20.0, 2.0)) if xp is _B64 else np.clip(ls, np.float32(-20), np.float32(2))


def _inv_n(xp):
    return xp.c(1.0) / xp.c(float(NN))


def _dpre(xp, gh, u):
    """GH/20 * min(U + 1, 1): [B, 20, H] from GH [B, H], U [B * 20, H]"""
    B, H = _val(gh).shape
    u1 = xp.c(u).reshape(B, NN, H) + 1.0
    if xp is _B32:
        u1 = u1.astype(np.float32)
    return (xp.c(gh) * _inv_n(xp))[:, None, :] * xp.where(_val(u1) < 1, u1, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# the operations (h: float32 host inputs; p: the case's parameters; defect: None or one of DEFECTS -- float32 emulation only)
# ------------------------------------------------------------------------------------------------------------------------------------
def _f_fwd(xp, h, p, defect=None):
    x3 = p['engine'] == 1
    nz = xp.c(h['noise'])
    if defect == 'noise row n read as n + 1 for one fragment':
        nz = nz.copy()
        nz[4:8] = nz[5:9]
    out = {}
    for q in range(p['ntasks']):
        B, F, H = p['B'], p['F'], p['H']
        mu, ls = xp.c(h[f'mean{q}']), xp.c(h[f'lstd{q}'])
        cl = _clip(xp, ls)
        sig = xp.exp(ls if defect == 'the clamp missing on sigma_out' else cl)
        sg = _exp_fast(xp, cl) if x3 else xp.exp(cl)
        x = mu[:, None, :] + sg[:, None, :] * nz[None, :, :]
        if defect == 'columns k >= 256 of a chunked row dropped':
            x = x.copy()
            x[:, :, 256:] = 0
        pre = _mm_t(xp, x.reshape(B * NN, F), xp.c(h[f'W{q}']), x3, drop=4 if defect == 'one dropped bf16x3 cross term too many' else
                    1 if defect == 'a second-order bf16x3 term dropped' else None) + xp.c(h[f'bias{q}'])[None, :]
        U = _elu_fast(xp, pre)
        Hm = xp.sum(U.reshape(B, NN, H), axis=1)
        if defect != '1/N left out':
            Hm = Hm * _inv_n(xp)
        out[f'Hm{q}'] = Hm
        if p['U'][q]:
            out[f'U{q}'] = U
        if p['sig'][q]:
            out[f'sigma{q}'] = sig
    return out


def _f_dx(xp, h, p, defect=None):
    B, F, H = p['B'], p['F'], p['H']
    nh = 1 if defect == 'head 1 left out of dX' else p['nheads']
    A = _cat([_dpre(xp, h[f'GH{k}'], h[f'U{k}']) for k in range(nh)], 2).reshape(B * NN, nh * H)
    Wc = np.concatenate([h[f'W{k}'] for k in range(nh)], 0)                       # [nh H, F]
    D = _mm_t(xp, A, xp.c(np.ascontiguousarray(Wc.T)), p['engine'] == 1).reshape(B, NN, F)
    ls = h['lstd']
    mask = np.ones_like(ls) if defect == 'the log_std mask missing in dX' else ((ls >= -20) & (ls <= 2)).astype(np.float32)
    Gl = xp.dot(xp.c(h['noise'])[None, :, :], D, 1) * xp.exp(_clip(xp, xp.c(ls))) * xp.c(mask)
    return {'Gm': xp.sum(D, axis=1), 'Gl': Gl}


def dw_split_rows(B, splits):
    """[(first batch row, rows)] of every split, as the bf16x3 dW kernels cut the batch"""
    bs = (B + splits - 1) // splits
    return [(min(s * bs, B), max(min(bs, B - min(s * bs, B)), 0)) for s in range(splits)]


def _f_dw(xp, h, p, defect=None, partials=None):
    """partials (a dict): receives the float32 slab / bias-slab images of the bf16x3 forms ({'slab': [tasks, splits, H, F], 'bslab': ...})"""
    B, F, H, order = p['B'], p['F'], p['H'], p['order']
    x3 = order != 'fp32'
    nz = xp.c(h['noise'])
    out = {}
    for q in range(p['ntasks']):
        dp = _dpre(xp, h[f'GH{q}'], h['U0' if defect == "dW of task 1 computed from task 0's U" else f'U{q}'])         # [B, 20, H]
        mu, sg = xp.c(h[f'mean{q}']), xp.c(h[f'sigma{q}'])
        gW = gb = None
        for b0, nbr in dw_split_rows(B, p['splits']):
            if nbr == 0:
                fill = np.float32(SENT) if defect == 'the rows of an empty split not zeroed' else np.float32(0)
                pW, pb = xp.c(np.full((H, F), fill)), xp.c(np.full(H, fill))
            elif order == 'x3r':
                pW = pb = None
                for c0 in range(0, nbr, 32):
                    nb = min(32, nbr - c0)
                    if defect == 'the last ragged chunk of a dW split dropped' and nb < 32 and c0:
                        continue
                    dc, sc, mc = dp[b0 + c0:b0 + c0 + nb], sg[b0 + c0:b0 + c0 + nb], mu[b0 + c0:b0 + c0 + nb]
                    P = _mm_t(xp, _T(dc, 1, 2, 0), _T(sc, 1, 0), True)                      # [20, H, F]: sum_b dPre[b,n,j] sigma[b,k]
                    A1 = xp.sum(dc, axis=1)                                                 # [nb, H]
                    chunk = xp.dot(nz[:, None, :], P, 0) + _mm_t(xp, _T(A1, 1, 0), _T(mc, 1, 0), True)
                    cb = xp.sum(dc.reshape(nb * NN, H), axis=0)
                    if defect == 'the bias gradient counting a clamped duplicate row' and nb < 32:
                        cb = cb + xp.sum(dc[nb - 1], axis=0) * np.float32(32 - nb)
                    pW, pb = (chunk, cb) if pW is None else (pW + chunk, pb + cb)
            else:
                d = dp[b0:b0 + nbr].reshape(nbr * NN, H)
                x = (mu[b0:b0 + nbr, None, :] + sg[b0:b0 + nbr, None, :] * nz[None, :, :]).reshape(nbr * NN, F)
                rows = nbr * NN
                keep = rows - (rows % 32 or 32) if defect == 'the last ragged chunk of a dW split dropped' and rows > 32 else rows
                pW = _mm_t(xp, _T(d[:keep], 1, 0), _T(x[:keep], 1, 0), x3)
                pb = xp.sum(d, axis=0)
                if defect == 'the bias gradient counting a clamped duplicate row' and rows % 32:
                    pb = pb + xp.sum(d[rows - 4:], axis=0) * np.float32((32 - rows % 32) // 4)
            if partials is not None:
                partials.setdefault('slab', []).append(np.asarray(_val(pW), np.float32))
                partials.setdefault('bslab', []).append(np.asarray(_val(pb), np.float32))
            gW, gb = (pW, pb) if gW is None else (gW + pW, gb + pb)
        out[f'gW{q}'], out[f'gb{q}'] = gW, gb
    return out


OPS = {'fwd': _f_fwd, 'dx': _f_dx, 'dw': _f_dw}


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, kernel, form, env=None, **p):
        self.name, self.kernel, self.form, self.env = name, kernel, form, env or {}
        self.p = dict(p, kernel=kernel)


FP32 = {'RLREP_DISABLE': 'x3'}
FP32_CHUNK = {'RLREP_DISABLE': 'x3', 'RLREP_ENABLE': 'nc_fwd_chunk'}
X3_ROWMAJOR = {'RLREP_DISABLE': 'nc_dw_rows'}

# every compiled kernel form of noisecritic.hip in the default library
FORMS = ([f'nc_fwd_kernel<{g},{w}>' for g in (1, 2, 4) for w in (8, 4)] + [f'nc_fwd_chunk_kernel<{g},8>' for g in (1, 2, 4)] +
         ['nc_fwd_x3_kernel<1>', 'nc_fwd_x3q_kernel', 'nc_dx_kernel<true>', 'nc_dx_kernel<false>', 'nc_dx_x3_kernel',
          'nc_dw_kernel<false>', 'nc_dw_kernel<true>', 'nc_dw_x3_kernel+nc_dw_fin_kernel', 'nc_dw_x3r_kernel+nc_dw_fin_kernel'])
# ... and the ones rl_nc_fwd_plan never selects (g2 is 1 or 2, rl_nc_fwd_cols() is 128): reached here by the hook's overrides only
NEVER_PLANNED = ['nc_fwd_kernel<4,8>', 'nc_fwd_chunk_kernel<4,8>', 'nc_fwd_kernel<1,4>', 'nc_fwd_kernel<2,4>', 'nc_fwd_kernel<4,4>']

# variety of a forward case, by position: (tasks, U given per task, sigma_out given per task, ld_ml - 2 F, w3 images per task)
_FWD_MIX = ((1, (1,), (1,), 0), (3, (1, 0, 1), (0, 0, 1), 8), (4, (1, 1, 1, 1), (1, 0, 0, 0), 4), (2, (0, 0), (0, 0), 0))


def _cases():
    c = []

    def fwd(name, form, env, B, F, H, mix, g2=0, cols=0, w3=None, **kw):
        nt, U, sig, pad = mix
        c.append(Case(name, 'fwd', form, env, B=B, F=F, H=H, ntasks=nt, U=U, sig=sig, ldpad=pad, g2=g2, cols=cols, w3=w3 or (0,) * nt,
                      engine=1 if 'x3' in form else 0, **kw))

    # fp32 forward, whole table: one row past every row group (B = 5 / 9 / 17 at 4 / 8 / 16 rows), a wave with no column (H = 3), a partial last
    # column tile at 64 and at 128 (H = 70, 129, 130), F from one K step to the widest whole table
    for g2 in (1, 2, 4):
        for cols in (128, 64):
            shapes = ((1, 4, 3), (5, 20, 70), (9, 256, 129), (17, 432, 130)) if g2 < 4 else ((1, 4, 3), (9, 20, 129), (5, 96, 70), (17, 256, 130))
            for i, (B, F, H) in enumerate(shapes):
                fwd(f'fwd_g{g2}_c{cols}_{B}x{F}x{H}', f'nc_fwd_kernel<{g2},{cols // 16}>', FP32, B, F, H, _FWD_MIX[i], g2, cols)
    # K-chunked: a ragged last chunk (260, 436), the row end on a chunk boundary (512), one K step into a third chunk (516)
    for g2, B in ((1, 5), (2, 9), (4, 17)):
        for i, F in enumerate((260, 436, 512, 516)):
            fwd(f'fwd_chunk_g{g2}_{B}x{F}', f'nc_fwd_chunk_kernel<{g2},8>', FP32_CHUNK if F == 260 else FP32, B, F, (70, 130)[i & 1], _FWD_MIX[(i + g2) % 4], g2, 128)
    # ... and widths both forms run: the outputs must agree bit for bit (twin: the whole-table launch of the same arena)
    for g2, B, F, H in ((1, 5, 96, 70), (2, 9, 432, 130), (4, 17, 96, 129)):
        fwd(f'fwd_chunk_twin_g{g2}_{B}x{F}x{H}', f'nc_fwd_chunk_kernel<{g2},8>', FP32_CHUNK, B, F, H, _FWD_MIX[2], g2, 128, twin=FP32)
    # bf16x3 forward: 64 columns (two-role kernel) and 128 (32x32x16 kernel) by override; with weight images, without, and mixed
    for cols, form in ((64, 'nc_fwd_x3_kernel<1>'), (128, 'nc_fwd_x3q_kernel')):
        fwd(f'fwd_x3_c{cols}_1x64x5', form, None, 1, 64, 5, (2, (1, 1), (1, 0), 0), 0, cols, w3=(1, 1))
        fwd(f'fwd_x3_c{cols}_7x96x64', form, None, 7, 96, 64, (4, (1, 0, 1, 1), (0, 1, 0, 0), 8), 0, cols)
        fwd(f'fwd_x3_c{cols}_9x288x130', form, None, 9, 288, 130, (2, (1, 1), (0, 1), 4), 0, cols, w3=(1, 0))
    # ... and the 128-column kernel once by the planner's own rule: tasks * ceil(B / 8) * ceil(H / 128) = 4 * 64 * 1 >= 256
    fwd('fwd_x3_planner_505x64x5', 'nc_fwd_x3q_kernel', None, 505, 64, 5, (4, (1, 0, 0, 1), (0, 0, 1, 0), 0), 0, 0, w3=(1, 1, 1, 1))

    def dx(form, env, B, F, H, nh):
        c.append(Case(f'dx_{"x3" if "x3" in form else "vec" if "true" in form else "scalar"}{"_off" if env else ""}_{B}x{F}x{H}_h{nh}', 'dx', form, env,
                      B=B, F=F, H=H, nheads=nh, engine=1 if 'x3' in form else 0))
    # dX: a partial column tile (F = 4, 68), one and two heads; H = 30 is the 4-byte kernel, 100 the 16-byte one by H % 32, 32 / 96 bf16x3
    for B, F, H, nh in ((1, 4, 32, 1), (5, 68, 96, 2), (5, 128, 32, 2)):
        dx('nc_dx_x3_kernel', None, B, F, H, nh)
    for B, F, H, nh in ((5, 68, 100, 2), (1, 128, 100, 1)):
        dx('nc_dx_kernel<true>', None, B, F, H, nh)
    for B, F, H, nh in ((5, 4, 32, 2), (5, 68, 96, 1)):
        dx('nc_dx_kernel<true>', FP32, B, F, H, nh)
    for B, F, H, nh in ((5, 68, 30, 2), (1, 4, 30, 1), (5, 128, 30, 1)):
        dx('nc_dx_kernel<false>', None, B, F, H, nh)

    def dw(order, B, F, H, nt, splits=0, lean=0):
        form = {'fp32': f'nc_dw_kernel<{"true" if lean else "false"}>', 'x3': 'nc_dw_x3_kernel+nc_dw_fin_kernel', 'x3r': 'nc_dw_x3r_kernel+nc_dw_fin_kernel'}[order]
        env = {'fp32': FP32, 'x3': X3_ROWMAJOR, 'x3r': None}[order]
        c.append(Case(f'dw_{order}{"_lean" if lean else ""}_{B}x{F}x{H}_t{nt}{f"_s{splits}" if splits else ""}', 'dw', form, env,
                      B=B, F=F, H=H, ntasks=nt, order=order, splits_arg=splits, lean=lean))
    for lean in (0, 1):
        for i, (B, F, H) in enumerate(((1, 4, 3), (5, 36, 20), (37, 96, 96))):
            dw('fp32', B, F, H, 1 + (i + lean) % 2, lean=lean)
    # bf16x3, both orders: splits clamped by the batch (5 rows: one split); a split without rows (B = 3 in 4 splits: it zero-fills its slab);
    # a ragged batch over planner splits; chunks of 32, 32 and 2 batch rows in one split; 33 rows per split (a chunk of 32 and a chunk of 1)
    for order in ('x3', 'x3r'):
        dw(order, 5, 64, 32, 1)
        dw(order, 3, 64, 64, 2, splits=4)
        dw(order, 37, 96, 96, 2)
        dw(order, 66, 68, 70, 1, splits=1)
        dw(order, 260, 256, 256, 2)
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------------------------
# host-only plan queries (no GPU call), under the switches in force
# ------------------------------------------------------------------------------------------------------------------------------------
def _i32s(n):
    return [ctypes.c_int32(-1) for _ in range(n)]


def fwd_plan(ntasks, B, F, H):
    """(engine, g2, cols) of rl_nc_fwd_plan for tasks of one shape on aligned buffers"""
    from rlrep_amd import _lib
    o = _i32s(3)
    assert _lib.lib.rlrep_nc_fwd_plan(ntasks, B, F, H, *[ctypes.byref(x) for x in o]) == 0
    return o[0].value, o[1].value // 4, o[2].value


def nc_forms(ntasks, B, F, H, g2=1):
    """(K-chunked, dW splits) of rl_nc_fwd_chunked / rl_nc_dw_splits"""
    from rlrep_amd import _lib
    o = _i32s(2)
    assert _lib.lib.rlrep_nc_forms(ntasks, B, F, H, g2, ctypes.byref(o[0]), ctypes.byref(o[1])) == 0
    return o[0].value, o[1].value


def w3_bytes(H, F):
    from rlrep_amd import _lib
    return int(_lib.lib.rlrep_nc_w3_bytes(H, F))


def dw_splits(case):
    """split count of a dW case: the caller's, or the planner's (1 on the fp32 engine, which has no splits)"""
    p = case.p
    if p['order'] == 'fp32':
        return 1
    return p['splits_arg'] or nc_forms(p['ntasks'], p['B'], p['F'], p['H'])[1]


def expected_form(case):
    """(kernel name, the hook's form array) the case must get under the switches in force; dX: None (its engine rule has no host-only query:
    the GPU test reads it from the hook)"""
    p = case.p
    if case.kernel == 'fwd':
        engine, g2, cols = fwd_plan(p['ntasks'], p['B'], p['F'], p['H'])
        g2, cols = p['g2'] or g2, p['cols'] or cols
        chunked = int(engine == 0 and nc_forms(p['ntasks'], p['B'], p['F'], p['H'], g2)[0] != 0)
        name = ('nc_fwd_x3q_kernel' if cols == 128 else 'nc_fwd_x3_kernel<1>') if engine else f'nc_fwd_{"chunk_" if chunked else ""}kernel<{g2},{cols // 16}>'
        return name, (engine, g2, cols, chunked)
    if case.kernel == 'dw':
        import os
        off = os.environ.get('RLREP_DISABLE', '').split(',')
        engine, rows = int('x3' not in off), int('nc_dw_rows' not in off)
        splits = p['splits_arg'] or nc_forms(p['ntasks'], p['B'], p['F'], p['H'])[1]          # (resolved, and ignored, on the fp32 engine too)
        if not engine:
            return f'nc_dw_kernel<{"true" if p["lean"] else "false"}>', (0, p['lean'], splits, 0)
        return f'nc_dw_x3{"r" if rows else ""}_kernel+nc_dw_fin_kernel', (1, p['lean'], splits, rows)
    return None


def dx_form_name(form):
    engine, vec = form
    return 'nc_dx_x3_kernel' if engine else f'nc_dx_kernel<{"true" if vec else "false"}>'


# ------------------------------------------------------------------------------------------------------------------------------------
# arena
# ------------------------------------------------------------------------------------------------------------------------------------
class Built:
    """arena: float32 host image of the launch's one allocation (read-only once built);  off[name]: float offset of a buffer's first element;
    ld[name]: its row stride;  h: the float32 inputs;  p: the case's parameters (with the resolved split count);
    outs: [(output name, buffer, float offset of the window, rows, width, ld, want (float64), bound (float64))];
    raw: [(buffer, float offset, floats)] of the windows without a reference of their own (weight-image scratch, split slabs)"""


class _Arena:
    def __init__(self):
        self.cur, self.bufs = 0, []

    def add(self, name, rows, width, ld=None, data=None, pad_row=False, nan_pad=False):
        ld = ld or width
        total = rows + (1 if pad_row else 0)
        start = (self.cur + GUARD + 3) // 4 * 4
        self.cur = start + total * ld
        self.bufs.append((name, start, rows, width, ld, total, data, nan_pad))
        return start

    def image(self):
        arena = _sentinel(self.cur + GUARD + 4)
        for name, start, rows, width, ld, total, data, nan_pad in self.bufs:
            if data is not None:
                view = arena[start:start + total * ld].reshape(total, ld)
                if nan_pad:
                    view[:] = np.nan
                view[:rows, :width] = data
        return arena


def _edges(rs, ls):
    """log_std below -20, above 2, exactly -20 and exactly 2, each at least once (a 1 x 4 matrix is nothing else)"""
    flat = ls.reshape(-1)
    pos = rs.choice(flat.size, min(flat.size, 8), replace=False)
    for i, v in enumerate((-25.5, 3.25, -20.0, 2.0, -20.000002, 2.0000002, -31.0, 7.5)[:pos.size]):
        flat[pos[i]] = np.float32(v)


def _plant_u(rs, U):
    """elu outputs as a backward kernel finds them: positive, exactly 0, exactly -1 (a pre-activation below -30) and within 1e-6 of -1"""
    flat = U.reshape(-1)
    pos = rs.choice(flat.size, min(flat.size, 12), replace=False)
    for i, v in enumerate((0.0, -1.0, -1.0 + 2.0 ** -21, -0.999999, 0.0, -1.0, 2.5, -1.0 + 2.0 ** -24, -0.9999995, 1e-30, -1e-30, 0.0)[:pos.size]):
        flat[pos[i]] = np.float32(v)


def build(case):
    p, k = dict(case.p), case.kernel
    rs = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    Nrm = lambda *s: rs.standard_normal(s).astype(np.float32)
    ar, h, outs, raw = _Arena(), {}, [], []
    B, F, H = p['B'], p['F'], p['H']
    ld = {}

    def inp(name, data, ldv=None):
        data = np.asarray(data, np.float32)
        d2 = data.reshape(1, -1) if data.ndim == 1 else data
        h[name] = data
        ld[name] = ldv or d2.shape[1]
        return ar.add(name, d2.shape[0], d2.shape[1], ldv, data=d2, pad_row=bool(ldv and ldv > d2.shape[1]), nan_pad=bool(ldv and ldv > d2.shape[1]))

    def hh(name, mean, lstd, pad):
        """a (mean | log_std) block as the feature net's head writes it: lstd = mean + F in rows of ld_ml floats.  None: that half is NaN."""
        both = np.full((B, 2 * F), np.nan, np.float32)
        if mean is not None:
            both[:, :F] = mean
            h['mean' + name] = mean
        if lstd is not None:
            both[:, F:] = lstd
            h['lstd' + name] = lstd
        ld['hh' + name] = 2 * F + pad
        return ar.add('hh' + name, B, 2 * F, 2 * F + pad, data=both, pad_row=pad > 0, nan_pad=pad > 0)

    def out(name, rows, width, ldv=None, keys=None):
        o = ar.add(name, rows, width, ldv, pad_row=True)
        for key, c0, ncol in keys or [(name, 0, width)]:
            outs.append((key, name, o + c0, rows, ncol, ldv or width))
        return o

    def lstd_of():
        ls = (0.5 * Nrm(B, F) - 1.0).astype(np.float32)
        _edges(rs, ls)
        return ls

    def u_of():
        pre = (1.5 * Nrm(B * NN, H)).astype(np.float32)
        U = np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0))).astype(np.float32)
        _plant_u(rs, U)
        return U

    def gh_of():
        g = Nrm(B, H)
        if B >= 2:
            g[rs.randint(B)] = 0.0                    # a zero row
        return g

    inp('noise', Nrm(NN, F))
    if k == 'fwd':
        scale = np.float32(1.0 / np.sqrt(F))
        for q in range(p['ntasks']):
            hh(str(q), Nrm(B, F), lstd_of(), p['ldpad'])
            W, bias = (Nrm(H, F) * scale).astype(np.float32), (0.5 * Nrm(H)).astype(np.float32)
            if H >= 3:
                W[0], bias[0] = 0.0, 0.0                                            # pre-activation exactly 0: U = 0, Hm = 0
                W[1] *= np.float32(0.25)
                bias[1] = np.float32(-40.0) - np.abs(Nrm(1))[0]                      # pre-activation below -30: U = -1 to the last bit
            inp(f'W{q}', W), inp(f'bias{q}', bias)
            out(f'Hm{q}', B, H)
            if p['U'][q]:
                out(f'U{q}', B * NN, H)
            if p['sig'][q]:
                out(f'sigma{q}', B, F)
            if p['w3'][q]:
                nfl = w3_bytes(H, F) // 4
                raw.append((f'w3{q}', ar.add(f'w3{q}', 1, nfl), nfl))
    elif k == 'dx':
        for hd in range(p['nheads']):
            inp(f'GH{hd}', gh_of(), (H + 3) // 4 * 4 + 4), inp(f'U{hd}', u_of()), inp(f'W{hd}', (Nrm(H, F) * np.float32(1.0 / np.sqrt(H))).astype(np.float32))
        hh('', None, lstd_of(), 4)
        out('G', B, 2 * F, 2 * F + 8, keys=[('Gm', 0, F), ('Gl', F, F)])
    elif k == 'dw':
        p['splits'] = dw_splits(case)
        for q in range(p['ntasks']):
            inp(f'U{q}', u_of()), inp(f'GH{q}', gh_of(), (H + 3) // 4 * 4 + 4)
            hh(str(q), Nrm(B, F), None, 8 if q == 0 else 0)
            with np.errstate(under='ignore'):
                inp(f'sigma{q}', np.exp(np.clip(lstd_of(), np.float32(-20), np.float32(2))).astype(np.float32))
            out(f'gW{q}', H, F), out(f'gb{q}', 1, H)
        sp = max(p['splits'], 1)
        for name, n in (('slab', p['ntasks'] * sp * H * F), ('bslab', p['ntasks'] * sp * H)):
            o = ar.add(name, 1, n)
            if p['order'] != 'fp32':
                raw.append((name, o, n))
    b = Built()
    b.arena = ar.image()
    b.off = {name: start for name, start, *_ in ar.bufs}
    b.ld, b.h, b.p, b.raw = ld, h, p, raw
    res = OPS[k](_B64, h, p)
    b.outs = [(key, buf, o, rows, width, ldv, res[key].v.reshape(rows, width), res[key].e.reshape(rows, width)) for key, buf, o, rows, width, ldv in outs]
    assert {o[0] for o in b.outs} == set(res), (case.name, set(res))
    b.arena.setflags(write=False)
    return b


def windows(built):
    """bool mask of the arena: True inside the output windows (scratch and slabs included)"""
    m = np.zeros(built.arena.size, bool)
    for key, buf, o, rows, width, ldv, _, _ in built.outs:
        m[window_index(o, rows, width, ldv)] = True
    for _, o, n in built.raw:
        m[o:o + n] = True
    return m


def emulate(case, built, defect=None, partials=None):
    """the float32 NumPy evaluation of the case in its kernel's own order: {output name: float32 array shaped like its window}"""
    kw = {'partials': partials} if case.kernel == 'dw' else {}
    res = OPS[case.kernel](_B32, built.h, built.p, defect, **kw)
    assert all(np.asarray(v).dtype == np.float32 for v in res.values()), {k: np.asarray(v).dtype for k, v in res.items()}
    return {key: np.asarray(res[key], np.float32).reshape(rows, width) for key, _, _, rows, width, _, _, _ in built.outs}


def w3_image(W):
    """the bf16x3 images of W [H, F] in the layout of x3.h:27 -- [F / 32 steps][3 images][rows][4 groups of 8 k][8 bf16] -- as uint16"""
    H, F = W.shape
    img = np.zeros((F // 32, 3, H, 4, 8), np.uint16)
    for i, part in enumerate(split3(W)):
        img[:, i] = (part.view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(H, F // 32, 4, 8).transpose(1, 0, 2, 3)
    return img.reshape(-1)


# the defects the CPU test plants in the float32 emulation: (defect, case, the output that must leave its bound)
DEFECTS = (
    ('noise row n read as n + 1 for one fragment', 'fwd_g1_c128_5x20x70', 'Hm0'),
    ('noise row n read as n + 1 for one fragment', 'fwd_x3_c128_9x288x130', 'U0'),
    ('1/N left out', 'fwd_g2_c128_9x256x129', 'Hm0'),
    ('columns k >= 256 of a chunked row dropped', 'fwd_chunk_g1_5x260', 'Hm0'),
    ('the clamp missing on sigma_out', 'fwd_g1_c128_1x4x3', 'sigma0'),
    ('the log_std mask missing in dX', 'dx_x3_5x68x96_h2', 'Gl'),
    ('head 1 left out of dX', 'dx_vec_5x68x100_h2', 'Gm'),
    ('the last ragged chunk of a dW split dropped', 'dw_x3r_66x68x70_t1_s1', 'gW0'),
    ('the last ragged chunk of a dW split dropped', 'dw_x3_66x68x70_t1_s1', 'gW0'),
    ('the rows of an empty split not zeroed', 'dw_x3r_3x64x64_t2_s4', 'gW0'),
    ('the bias gradient counting a clamped duplicate row', 'dw_x3r_66x68x70_t1_s1', 'gb0'),
    ('the bias gradient counting a clamped duplicate row', 'dw_x3_66x68x70_t1_s1', 'gb0'),
    ("dW of task 1 computed from task 0's U", 'dw_x3r_37x96x96_t2', 'gW1'),
    ('one dropped bf16x3 cross term too many', 'fwd_x3_c64_7x96x64', 'U0'),
)
# a defect the bound does NOT catch at these depths, kept on record (docs/history/noisecritic_kernels.md): the h l product, 2^-16 relative
UNCAUGHT = (('a second-order bf16x3 term dropped', 'fwd_x3_c64_7x96x64', 'U0'),)
