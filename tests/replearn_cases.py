"""Cases, host images and float64 references of the representation-loss kernels (csrc/replearn.hip) behind their unit-test hook
(rlrep_replearn), shared by tests/test_replearn_kernels.py (GPU: the launches) and tests/test_replearn_kernels_cpu.py (CPU: the hook's
refusals, the dispatch plan, and the error bound held against a float32 emulation, clean and with planted defects).

One launch = one Case.  build(case) lays every input and output out in ONE float32 arena:

  * every buffer has at least GUARD = 64 sentinel floats (a finite bit pattern, 0xC0DExxxx) before and after it;
  * outputs whose record has a row stride get ld > width and one sentinel row behind the last row;
  * inputs with a row stride carry NaN in their padding columns and in one padding row, so that a clamped or masked read that leaks padding
    into a result makes it non-finite;
  * values are drawn per case from one generator (seeded by the case's name): no constants, no two elements alike.

Reference and bound.  Every kernel's operation is written ONCE below (the _f_* functions), from the formulas of the reference agents -- ctrlsac's
cross entropy of phi mu'^T against the identity plus 0.5 mse(theta(phi), r); spedersac's -2 diag(phi mu'^T) / B + sum((phi_r mu_r^T)(phi_r mu_r^T)^T)
/ B^2 + 0.5 mse; diffsrsac's perturbation sqrt(ab) s' + sqrt(1 - ab) eps, target -(pert - sqrt(ab) s'), score = phi . U, diff = target - (1 - ab)
sigma score, loss sum(diff^2) / B and its gradients; get_reg_term of the diffsrsac critic -- and evaluated through one of two arithmetics:

  * _B64: float64 values that carry a first-order bound of the float32 evaluation's error with them (class V), e = 2^-24:
        input                exact (a float32 number)
        a + b, a - b         e_a + e_b + e |result|
        a * b                |a| e_b + |b| e_a + e |result|
        a / b                e_a / |b| + |a| e_b / b^2 + e |result|
        sqrt(a)              e_a / (2 sqrt a) + e |result|                       (correctly rounded)
        K-term dot / sum     2 K e sum_k |a_k| |b_k| + sum_k (|a_k| e_bk + |b_k| e_ak)   (the project's form: any order, fma or not)
        exp(a)               exp(a) e_a + 2 ULP e exp(a) + 2^-126                (ULP units in the last place, one ulp <= 2 e |x|; results under
                                                                                  the smallest normal number may be flushed to zero)
        log(a)               e_a / a + 2 ULP e |log a|
    ULP = 4 for expf and for logf: the ROCm installation this was written against ships no document that states a figure for the device
    functions, so four units each are ASSUMED here.  The row maximum subtracted inside the log-sum-exp is exact in this model: the identity
    lse = m + log sum exp(S - m) holds for ANY shift m, and the kernel's m is one of its own float32 scores.
    So the linear outputs (column sums; c, d and the rhat dot products; spectral gradients; perturbed states and targets; score_s, dphi_z, dU;
    regulariser sums) get 2 K e sum |a_k| |b_k| plus e times the magnitude of every later operation's result, and dS of both InfoNCE forms gets
    the error of lse (ncols-term sum of expf, one logf) carried through expf.  Per-block partial sums are n-term sums of row terms that carry
    their own bounds.
  * _B32: NumPy float32 (pairwise sums: another order than any kernel's).  The CPU test holds it to the bound above, and plants defects in it.
"""
import zlib

import numpy as np

U24 = 2.0 ** -24
TINY = 2.0 ** -126
ULP_EXP = ULP_LOG = 4
GUARD = 64
NUM_NOISES = 50          # entries of the alpha-bar table the diffsrsac cases draw from


# ------------------------------------------------------------------------------------------------------------------------------------
# the two arithmetics
# ------------------------------------------------------------------------------------------------------------------------------------
class V:
    """float64 value(s) with a first-order bound of the error a float32 evaluation of the same expression may have"""
    __slots__ = ('v', 'e')
    __array_priority__ = 100

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) + e

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    @staticmethod
    def _r(v, e):
        return V(v, e + U24 * np.abs(v))

    def __add__(a, b):
        b = V.of(b)
        return V._r(a.v + b.v, a.e + b.e)

    __radd__ = __add__

    def __sub__(a, b):
        b = V.of(b)
        return V._r(a.v - b.v, a.e + b.e)

    def __rsub__(a, b):
        return V.of(b) - a

    def __neg__(a):
        return V(-a.v, a.e)

    def __mul__(a, b):
        b = V.of(b)
        return V._r(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e)

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = V.of(b)
        return V._r(a.v / b.v, a.e / np.abs(b.v) + np.abs(a.v) * b.e / (b.v * b.v))

    def __rtruediv__(a, b):
        return V.of(b) / a

    def __getitem__(a, k):
        return V(a.v[k], a.e[k])

    @property
    def shape(a):
        return a.v.shape

    def reshape(a, *s):
        return V(a.v.reshape(*s), a.e.reshape(*s))


class _B64:
    name = 'float64 + bound'

    @staticmethod
    def c(x):
        return V(np.asarray(x, np.float64))

    @staticmethod
    def exp(a):
        r = np.exp(a.v)
        return V(r, r * a.e + 2 * ULP_EXP * U24 * r + TINY)

    @staticmethod
    def log(a):
        r = np.log(a.v)
        return V(r, a.e / a.v + 2 * ULP_LOG * U24 * np.abs(r))

    @staticmethod
    def sqrt(a):
        r = np.sqrt(a.v)
        return V._r(r, a.e / (2 * np.maximum(r, 1e-300)))

    @staticmethod
    def dot(a, b, axis):
        a, b = V.of(a), V.of(b)
        K = np.broadcast(a.v, b.v).shape[axis]
        aa, ab = np.abs(a.v), np.abs(b.v)
        return V((a.v * b.v).sum(axis), 2 * K * U24 * (aa * ab).sum(axis) + (aa * b.e + ab * a.e).sum(axis))

    @staticmethod
    def matmul_t(a, b):
        """a [M, K] . b [N, K]^T of exact inputs"""
        K = a.v.shape[1]
        return V(a.v @ b.v.T, 2 * K * U24 * (np.abs(a.v) @ np.abs(b.v).T))

    @staticmethod
    def sum(a, axis=None):
        K = a.v.size if axis is None else a.v.shape[axis]
        return V(a.v.sum(axis), a.e.sum(axis) + 2 * K * U24 * np.abs(a.v).sum(axis))

    @staticmethod
    def rowmax(a):
        return V(a.v.max(axis=1, keepdims=True))          # exact: see the module docstring

    @staticmethod
    def zeros(shape):
        return V(np.zeros(shape))

    @staticmethod
    def put(dst, key, src):
        src = V.of(src)
        dst.v[key] = src.v
        dst.e[key] = src.e

    @staticmethod
    def where(m, a, b):
        a, b = V.of(a), V.of(b)
        return V(np.where(m, a.v, b.v), np.where(m, a.e, b.e))

    @staticmethod
    def roll(a, n, axis):
        return V(np.roll(a.v, n, axis), np.roll(a.e, n, axis))


class _B32:
    name = 'float32'
    f = np.float32

    @staticmethod
    def c(x):
        return np.asarray(x, np.float32)

    @staticmethod
    def exp(a):
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            return np.exp(a, dtype=np.float32)

    @staticmethod
    def log(a):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.log(a, dtype=np.float32)

    @staticmethod
    def sqrt(a):
        return np.sqrt(a, dtype=np.float32)

    @staticmethod
    def dot(a, b, axis):
        return (np.asarray(a, np.float32) * np.asarray(b, np.float32)).sum(axis, dtype=np.float32)

    @staticmethod
    def matmul_t(a, b):
        return (a @ b.T).astype(np.float32)

    @staticmethod
    def sum(a, axis=None):
        with np.errstate(invalid='ignore', over='ignore'):
            return np.asarray(a.sum(axis, dtype=np.float32), np.float32)

    @staticmethod
    def rowmax(a):
        return a.max(axis=1, keepdims=True)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, np.float32)

    @staticmethod
    def put(dst, key, src):
        dst[key] = src

    @staticmethod
    def where(m, a, b):
        return np.where(m, a, b).astype(np.float32)

    @staticmethod
    def roll(a, n, axis):
        return np.roll(a, n, axis)


def _f32(x):
    return np.float32(x)


def rows_blocks(B):
    """blocks of the one-wave-per-row kernels (the builder's qhead_blocks): row i belongs to block (i // 4) % rows_blocks(B)"""
    return min((B + 3) // 4, 128)


def _block_sums(xp, terms, owner, nblk):
    """[nblk, len(terms)]: per block the sum of every row term over exactly the rows the block owns"""
    out = xp.zeros((nblk, len(terms)))
    for blk in range(nblk):
        rows = np.nonzero(owner == blk)[0]
        for q, t in enumerate(terms):
            if rows.size:
                xp.put(out, (blk, q), xp.sum(t[rows]))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the operations (h: float32 host inputs; p: the case's parameters; defect: None, or one of DEFECTS planted -- float32 emulation only)
# ------------------------------------------------------------------------------------------------------------------------------------
def _f_infonce(xp, h, p, defect=None):
    B, NC, ib = p['B'], p['ncols'], _f32(p['inv_batch'])
    fused = p['kernel'] == 'score_infonce' and not p.get('pair')          # (pair: the same product through the GEMM + InfoNCE pair: its row ownership)
    S = xp.matmul_t(xp.c(h['Z']), xp.c(h['ZM'])) if 'ZM' in h else xp.c(h['S'])
    ii = np.arange(B)
    di = p['diag_off'] + ii
    if defect == 'diagonal one column off':
        di = np.minimum(di + 1, NC - 1)
    if defect == 'diag_off ignored':
        di = ii
    mx = xp.rowmax(S)
    if defect == 'no maximum subtraction':
        mx = mx * 0
    t = xp.exp(S - mx)
    if defect == 'one lane stride left out of a row sum':
        t = xp.where((np.arange(NC) % 64 == 5)[None, :], 0.0, t)
    lse = mx[:, 0] + xp.log(xp.sum(t, axis=1))
    eye = np.zeros((B, NC), np.float32)
    eye[ii, di] = 1.0
    dS = (xp.exp(S - lse[:, None]) - eye) * ib
    if 'Z' in h:
        rh = xp.dot(xp.c(h['Z']), xp.c(h['theta_w'])[None, :], 1) + xp.c(h['theta_b'])[0]
    else:
        rh = xp.c(h['rhat'])
    dr = rh - xp.c(h['r'])
    drhat = dr * ib
    if defect == 'inv_batch applied twice':
        dS, drhat = dS * ib, drhat * ib
    nblk = (B + 15) // 16 if fused else rows_blocks(B)
    owner = ii // 16 if fused else (ii // 4) % nblk
    terms = [lse - S[ii, di], dr * dr]
    if defect == 'rows of the second grid sweep skipped' and not fused:
        skip = ii >= 4 * nblk
        dS = xp.where(skip[:, None], S, dS)
        drhat = xp.where(skip, 0.0, drhat)
        owner = np.where(skip, -1, owner)
    return {'S': dS, 'drhat': drhat, 'partial': _block_sums(xp, terms, owner, nblk)}


def _f_colsum(xp, h, p, defect=None):
    def one(X, w, rows):
        X = xp.c(X[:rows])
        return xp.sum(X, axis=0) if w is None else xp.dot(xp.c(w[:rows])[:, None], X, 0)
    out = {'out': one(h['X'], h.get('w'), p['rows'])}
    if 'X2' in h:
        rows2 = min(p['rows'], p['rows2']) if defect == 'second column-sum set with the first set\'s row count' else p['rows2']
        out['out2'] = one(h['X2'], h.get('w2'), rows2)
        if 'w2' in h:
            out['outb2'] = xp.sum(xp.c(h['w2'][:rows2])).reshape(1)
    return out


def _f_speder_rows(xp, h, p, defect=None):
    B, ib = p['B'], _f32(p['inv_batch'])
    phi = xp.c(h['phi'])
    c = xp.dot(xp.c(h['mu_r']), xp.c(h['phibar'])[None, :], 1)
    d = xp.dot(phi, xp.c(h['mu']), 1)
    dr = (xp.dot(phi, xp.c(h['theta_w'])[None, :], 1) + xp.c(h['theta_b'])[0]) - xp.c(h['r'])
    nblk = rows_blocks(B)
    return {'c': c, 'drhat': dr * ib, 'partial': _block_sums(xp, [d, c * c, dr * dr], (np.arange(B) // 4) % nblk, nblk)}


def _f_speder_grads(xp, h, p, defect=None):
    B, F, ib = p['B'], p['F'], xp.c(_f32(p['inv_batch']))
    k1, k2 = ib * -2.0, (ib * ib) * 2.0
    if defect == 'inv_batch applied twice':
        k1 = k1 * ib
    phi, mu = xp.c(h['phi']), xp.c(h['mu'])
    ones = np.ones((B, 1), np.float32)
    g = {'Gphi_1': mu * k1 + xp.c(h['drhat'])[:, None] * xp.c(h['theta_w'])[None, :], 'Gmu_1': phi * k1,
         'Gphi_2': (xp.c(h['v']) * k2)[None, :] * ones, 'Gmu_2': (xp.c(h['c']) * k2)[:, None] * xp.c(h['phibar'])[None, :]}
    if defect == 'rows of the second grid sweep skipped':
        e = (np.arange(B)[:, None] * F + np.arange(F)[None, :]) >= 2048 * 256
        g = {k: xp.where(e, 0.0, v) for k, v in g.items()}
    return g


def _f_perturb(xp, h, p, defect=None):
    ab = xp.c(h['alphabars'][h['idx']])[:, None]
    sq = xp.sqrt(ab)
    x = xp.c(h['s2'])
    pert = sq * x + xp.sqrt(1.0 - ab) * xp.c(h['eps'])
    return {'XN_s': pert, 'XN_a': ab, 'TGT': -(pert - sq * x)}


def _f_score(xp, h, p, defect=None):
    B, F, S, ib = p['B'], p['F'], p['S'], _f32(p['inv_batch'])
    U, phi = xp.c(h['U']), xp.c(h['PHI'])                                        # [B, F, S], [B, F]
    score = xp.dot(phi[:, :, None], U, 1)                                        # [B, S]
    coef = (1.0 - xp.c(h['alphabars'][h['idx']])) * _f32(p['sigma'])
    diff = xp.c(h['TGT']) - coef[:, None] * score
    dsc = ((coef * -2.0)[:, None] * diff) * ib
    if defect == 'inv_batch applied twice':
        dsc = dsc * ib
    keep = slice(None)
    if defect == 'last partial column chunk left out':
        keep = slice(0, 64 * (S // 64))
    sq = diff * diff
    part = xp.sum(sq[:, keep], axis=1)
    gphi = xp.dot(dsc[:, None, keep], U[:, :, keep], 2)                          # [B, F]
    if defect == 'dU from phi of the neighbouring row':
        phi = xp.roll(phi, -1, 1)
    return {'U': phi[:, :, None] * dsc[:, None, :], 'GPHI': gphi, 'partial': part}


def _f_reg_stats(xp, h, p, defect=None):
    B, H, lam = p['B'], p['H'], _f32(p['lambda'])
    nbc, nbr = (H * H + 1023) // 1024, (B + 3) // 4
    n, d = xp.c(_f32(B)), xp.c(_f32(H))
    a = 1.0 / ((n - 1.0) * n)
    out = xp.zeros((4 * (nbc + nbr),))
    for k in range(4):
        C = xp.c(h[f'C{k}'])
        for blk in range(nbc):
            e = C[blk * 1024:(blk + 1) * 1024]
            xp.put(out, k * nbc + blk, (xp.sum(e * e) * a) * lam)
        x = xp.c(h[f'X{k}'])
        s = xp.dot(x, x, 1)                                                      # |x_row|^2
        v = -(a * s * s) - (s * 2.0) / (n * d)
        for blk in range(nbr):
            r = xp.sum(v[4 * blk:4 * blk + 4])
            if k == 0 and blk == 0:
                r = r + 4.0 / d                                                  # part3 of the four (net, head) pairs
            xp.put(out, 4 * nbc + k * nbr + blk, r * lam)
    return {'partial': out}


def _f_copy2(xp, h, p, defect=None):
    out = {'d1': xp.c(h['src'])}
    if p['d2']:
        out['d2'] = xp.c(h['src'])
    return out


OPS = {'infonce': _f_infonce, 'score_infonce': _f_infonce, 'colsum': _f_colsum, 'speder_rows': _f_speder_rows, 'speder_grads': _f_speder_grads,
       'perturb': _f_perturb, 'score': _f_score, 'reg_stats': _f_reg_stats, 'copy2': _f_copy2}


# ------------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, kernel, env=None, form=None, **p):
        self.name, self.kernel, self.env, self.form = name, kernel, env or {}, form
        self.p = dict(p, kernel=kernel)


ENV = {'ch32': {'RLREP_ENABLE': 'score_ch=32'}, 'ch128': {'RLREP_ENABLE': 'score_ch=128'}, 'ch0': {'RLREP_ENABLE': 'score_ch=0'},
       'nosmall': {'RLREP_DISABLE': 'score_small'}}
# (form, S, F, switches, floats by which U is moved off a 16-byte boundary)
SCORE_SHAPES = (
    [('LDS64', S, F, None, 0) for S, F in ((4, 3), (64, 17), (76, 20), (132, 256))] +
    [(f, S, F, e, 0) for f, e in (('LDS32', 'ch32'), ('LDS128', 'ch128')) for S, F in ((36, 20), (132, 256))] +
    [('SMALL1', S, F, None, 0) for S, F in ((1, 3), (5, 8), (17, 256), (31, 200))] + [('SMALL1', 8, 8, None, 1)] +
    [('SMALL2', 17, 257, None, 0), ('SMALL2', 8, 512, None, 0), ('SMALL4', 5, 513, None, 0), ('SMALL4', 32, 1024, None, 0)] +
    [('VEC', S, F, None, 0) for S, F in ((36, 257), (132, 260), (512, 300))] + [('VEC', 376, 20, 'ch0', 0)] +
    [('ROWS', S, F, None, 0) for S, F in ((33, 8), (111, 70))] +
    [('ROWS', 516, 9, 'ch0', 0),            # (S % 4 == 0 and F <= 256 is the LDS form's; with the two-pass kernels selected S > 512 is past the 16-byte kernel)
     ('ROWS', 17, 40, 'nosmall', 0), ('ROWS', 5, 1025, None, 0), ('ROWS', 36, 20, None, 1)])
# (S, F) of the suite's diffsrsac fixtures and the kernel each gets today (S = 17 and 5 are no multiples of 4: a thread per row; Humanoid's 376: LDS)
FIXTURE_FORMS = (((17, 256), 'SMALL1'), ((5, 8), 'SMALL1'), ((376, 256), 'LDS64'))


def plan(S, F, aligned=1):
    """the name of the kernel a score-matching launch gets under the switches in force (rlrep_diffsr_score_plan: host only)"""
    import ctypes
    from rlrep_amd import _lib
    form = ctypes.c_int32(-1)
    assert _lib.lib.rlrep_diffsr_score_plan(S, F, aligned, ctypes.byref(form)) == 0
    return _lib.SCORE_FORM[form.value]


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    for B, NC, off in ((1, 1, 0), (5, 5, 0), (67, 67, 0), (33, 66, 33), (515, 515, 0)):
        add(f'infonce_rhat_{B}x{NC}+{off}', 'infonce', B=B, ncols=NC, diag_off=off, F=0)
        for F in (8, 100):
            add(f'infonce_theta{F}_{B}x{NC}+{off}', 'infonce', B=B, ncols=NC, diag_off=off, F=F)
    for F in (64, 192):
        for B, NC, off in ((16, 16, 0), (23, 23, 0), (23, 33, 10), (100, 200, 100), (256, 256, 0)):
            add(f'fused_F{F}_{B}x{NC}+{off}', 'score_infonce', B=B, ncols=NC, diag_off=off, F=F)
    for rows in (1, 63, 64, 513, 1030):
        for F in (1, 16, 17, 50):
            for w in (False, True):
                add(f'colsum_{rows}x{F}{"_w" if w else ""}', 'colsum', rows=rows, F=F, w=w, two=False)
                add(f'colsum2_{rows}x{F}{"_w" if w else ""}', 'colsum', rows=rows, F=F, w=w, two=True, rows2=rows + 7)
    for B in (1, 6, 515):
        for F in (8, 64, 100):
            add(f'speder_rows_{B}x{F}', 'speder_rows', B=B, F=F)
    for B, F in ((3, 8), (1030, 512)):
        add(f'speder_grads_{B}x{F}', 'speder_grads', B=B, F=F)
    for B, S in ((1, 5), (19, 17), (1400, 376)):
        add(f'perturb_{B}x{S}', 'perturb', B=B, S=S)
    for form, S, F, e, uoff in SCORE_SHAPES:
        for B in (1, 3):
            add(f'score_{form}_S{S}_F{F}_B{B}{"_" + e if e else ""}{"_uoff" if uoff else ""}', 'score', env=ENV[e] if e else None, form=form,
                B=B, S=S, F=F, u_off=uoff)
    for B, H in ((2, 8), (5, 33), (9, 70)):
        add(f'reg_stats_{B}x{H}', 'reg_stats', B=B, H=H)
    for n in (1, 1025, 600001):
        for d2 in (False, True):
            add(f'copy2_{n}{"_d2" if d2 else ""}', 'copy2', n=n, d2=d2)
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------------------------
# arena
# ------------------------------------------------------------------------------------------------------------------------------------
def _sentinel(n, salt=0):
    """n floats of a recognisable finite bit pattern (0xC0DExxxx: about -6.9)"""
    return (np.uint32(0xC0DE0000) + ((np.arange(n, dtype=np.uint32) * np.uint32(7) + np.uint32(salt)) & np.uint32(0xffff))).view(np.float32)


class Built:
    """arena: float32 host image of the launch's one allocation (read-only once built);  off[name]: float offset of a buffer's first element;
    ld[name]: its row stride;  scalars: the record's integer / float fields;  h: the float32 inputs;
    outs: [(output name, buffer, float offset of the window, rows, width, ld, want (float64), bound (float64))]"""


class _Arena:
    def __init__(self):
        self.cur, self.bufs = 0, []

    def add(self, name, rows, width, ld=None, data=None, off=0, raw=None):
        ld = ld or width
        total_rows = rows + (1 if ld > width else 0)
        start = (self.cur + GUARD + 3) // 4 * 4 + off
        self.cur = start + total_rows * ld
        self.bufs.append((name, start, rows, width, ld, total_rows, data, raw))
        return start

    def image(self):
        arena = _sentinel(self.cur + GUARD + 4)
        for name, start, rows, width, ld, total_rows, data, raw in self.bufs:
            view = arena[start:start + total_rows * ld].reshape(total_rows, ld)
            if raw is not None:
                view.view(np.int32)[:rows, :width] = raw
            elif data is not None:
                if ld > width and name != 'S':             # an input's padding: NaN (S is an output too: its padding stays sentinel)
                    view[:] = np.nan
                view[:rows, :width] = data
        return arena


def build(case):
    p, k = case.p, case.kernel
    rs = np.random.RandomState(zlib.crc32(case.name.encode()) & 0x7fffffff)
    N = lambda *s: rs.standard_normal(s).astype(np.float32)
    ar, h, sc, outs = _Arena(), {}, {}, []

    def inp(name, data, ld=None, off=0, key=None):
        data = np.asarray(data, np.float32)
        d2 = data.reshape(1, -1) if data.ndim == 1 else data.reshape(data.shape[0], -1)
        h[key or name] = data
        return ar.add(name, d2.shape[0], d2.shape[1], ld, data=d2, off=off)

    def out(name, rows, width, ld=None, keys=None):
        """keys: [(result name, first row, rows, first column, columns)] of the windows inside the buffer (default: the whole of it)"""
        o = ar.add(name, rows, width, ld)
        for key, r0, nr, c0, ncol in keys or [(name, 0, rows, 0, width)]:
            outs.append((key, name, o + r0 * (ld or width) + c0, nr, ncol, ld or width))
        return o

    if k in ('infonce', 'score_infonce'):
        B, NC, F = p['B'], p['ncols'], p['F']
        p['inv_batch'] = float(np.float32(1.0) / np.float32(B))
        ldS = NC + 5
        sc.update(B=B, ncols=NC, diag_off=p['diag_off'], ldS=ldS, inv_batch=p['inv_batch'])
        if k == 'infonce':
            S = (3 * N(B, NC)).astype(np.float32)
            if B >= 5:
                hot = rs.choice(NC, min(3, NC), replace=False)           # one row with entries up to +100, one row entirely at -100
                S[1, hot] = np.float32(100) - np.abs(N(hot.size))
                S[3, :] = np.float32(-100)
            h['S'] = S
            ar.add('S', B, NC, ldS, data=S)
            outs.append(('S', 'S', ar.bufs[-1][1], B, NC, ldS))
        else:
            out('S', B, NC, ldS)
        if F:
            ldZ = F + 4
            scale = np.float32(1.0 / np.sqrt(F))
            inp('Z', 3 * N(B, F) * scale if k == 'score_infonce' else N(B, F), ldZ)
            inp('theta_w', N(F) * scale)
            inp('theta_b', N(1))
            sc.update(ldZ=ldZ, F=F)
            if k == 'score_infonce':
                inp('ZM', N(NC, F), F + 8)
                sc['ldZM'] = F + 8
        else:
            inp('rhat', N(B))
        inp('r', N(B))
        out('drhat', 1, B)
        nblk = (B + 15) // 16 if k == 'score_infonce' else rows_blocks(B)
        out('partial', nblk, 2)
        if k == 'score_infonce':
            ar.add('partial_pair', rows_blocks(B), 2)                    # the pair form's partials (test_fused_agrees_with_the_pair)
    elif k == 'colsum':
        rows, F = p['rows'], p['F']
        sc.update(rows=rows, F=F, ldX=F + 3)
        inp('X', N(rows, F), F + 3)
        if p['w']:
            inp('w', N(rows))
        out('out', 1, F)
        if p['two']:
            sc.update(rows2=p['rows2'], ldX2=F + 6)
            inp('X2', N(p['rows2'], F), F + 6)
            out('out2', 1, F)
            if p['w']:
                inp('w2', N(p['rows2']))
                out('outb2', 1, 1)
    elif k == 'speder_rows':
        B, F = p['B'], p['F']
        p['inv_batch'] = float(np.float32(1.0) / np.float32(B))
        sc.update(B=B, F=F, inv_batch=p['inv_batch'])
        s = np.float32(1.0 / np.sqrt(F))
        for nm in ('phi', 'mu', 'mu_r'):
            inp(nm, N(B, F))
        inp('phibar', N(F) * s), inp('theta_w', N(F) * s), inp('theta_b', N(1)), inp('r', N(B))
        out('c', 1, B), out('drhat', 1, B), out('partial', rows_blocks(B), 3)
    elif k == 'speder_grads':
        B, F = p['B'], p['F']
        p['inv_batch'] = float(np.float32(1.0) / np.float32(B))
        sc.update(B=B, F=F, inv_batch=p['inv_batch'])
        inp('phi', N(B, F)), inp('mu', N(B, F)), inp('c', N(B)), inp('drhat', N(B)), inp('phibar', N(F)), inp('v', N(F)), inp('theta_w', N(F))
        out('Gphi', 2 * B, F, keys=[('Gphi_1', 0, B, 0, F), ('Gphi_2', B, B, 0, F)])
        out('Gmu', 2 * B, F, keys=[('Gmu_1', 0, B, 0, F), ('Gmu_2', B, B, 0, F)])
    elif k in ('perturb', 'score'):
        B, S = p['B'], p['S']
        betas = np.linspace(1e-4, 0.02, NUM_NOISES) * (1 + 0.01 * rs.standard_normal(NUM_NOISES))
        inp('alphabars', np.cumprod(1.0 - betas).astype(np.float32))
        idx = rs.choice(NUM_NOISES, B, replace=B > NUM_NOISES).astype(np.int32)            # (distinct per sample where the table allows)
        if k == 'perturb' and B >= 2:
            idx[0], idx[-1] = 0, NUM_NOISES - 1                         # the first and the last entry of the table
        if k == 'perturb' and B == 1:
            idx[0] = NUM_NOISES - 1
        h['idx'] = idx
        ar.add('idx', 1, B, raw=idx[None, :])
        if k == 'perturb':
            sc.update(B=B, S=S, ld_s2=2 * S + 3)
            inp('s2', N(B, S), 2 * S + 3), inp('eps', N(B, S))
            out('XN', B, S + 1, keys=[('XN_s', 0, B, 0, S), ('XN_a', 0, B, S, 1)])
            out('TGT', B, S)
        else:
            F = p['F']
            p['sigma'], p['inv_batch'] = float(np.float32(0.7 + 0.1 * rs.rand())), float(np.float32(1.0) / np.float32(B))
            sc.update(B=B, F=F, S=S, sigma=p['sigma'], inv_batch=p['inv_batch'])
            U = (N(B, F, S) * np.float32(1.0 / np.sqrt(F)))
            h['U'] = U
            o = ar.add('U', B, F * S, data=U.reshape(B, F * S), off=p['u_off'])
            outs.append(('U', 'U', o, B, F * S, F * S))
            inp('PHI', N(B, F)), inp('TGT', N(B, S))
            out('GPHI', B, F), out('partial', 1, B)
    elif k == 'reg_stats':
        B, H = p['B'], p['H']
        p['lambda'] = float(np.float32(0.3 + 0.1 * rs.rand()))
        sc.update(B=B, H=H, lam=p['lambda'])
        for q in range(4):
            inp(f'X{q}', N(B, H) * np.float32(1.0 / np.sqrt(H)))
            inp(f'C{q}', N(H * H) * np.float32(1.0 / np.sqrt(H)))
        out('partial', 1, 4 * ((H * H + 1023) // 1024 + (B + 3) // 4))
    elif k == 'copy2':
        n = p['n']
        sc['n'] = n
        inp('src', N(n))
        out('d1', 1, n)
        if p['d2']:
            out('d2', 1, n)
    b = Built()
    b.arena = ar.image()
    b.off = {name: start for name, start, *_ in ar.bufs}
    b.scalars, b.h, b.p = sc, h, p
    res = OPS[k](_B64, h, p)
    b.outs = []
    for key, buf, o, rows, width, ld in outs:
        r = res[key]
        b.outs.append((key, buf, o, rows, width, ld, r.v.reshape(rows, width), r.e.reshape(rows, width)))
    assert {o[0] for o in b.outs} == set(res), (case.name, set(res))
    b.arena.setflags(write=False)
    return b


def pair_outs(built):
    """outs of a fused case run as the pair it replaces -- S = Z ZM^T by a GEMM launch into the S window, then the InfoNCE kernel on it with Z / theta
    given: the same dS and drhat, and the per-block partials of the pair's row ownership in the `partial_pair` buffer"""
    res = OPS['infonce'](_B64, built.h, dict(built.p, pair=True))
    B = built.p['B']
    outs = [o for o in built.outs if o[0] in ('S', 'drhat')]
    return outs + [('partial', 'partial_pair', built.off['partial_pair'], rows_blocks(B), 2, 2, res['partial'].v, res['partial'].e)]


def window_index(o, rows, width, ld):
    return o + np.arange(rows)[:, None] * ld + np.arange(width)[None, :]


def windows(built, outs=None):
    """bool mask of the arena: True inside the output windows (of `outs`, default the case's own)"""
    m = np.zeros(built.arena.size, bool)
    for key, buf, o, rows, width, ld, _, _ in outs or built.outs:
        m[window_index(o, rows, width, ld)] = True
    return m


def emulate(case, built, defect=None):
    """the float32 NumPy evaluation of the case: {output name: float32 array shaped like its window}"""
    res = OPS[case.kernel](_B32, built.h, built.p, defect)
    assert all(np.asarray(v).dtype == np.float32 for v in res.values()), {k: np.asarray(v).dtype for k, v in res.items()}
    return {key: np.asarray(res[key], np.float32).reshape(rows, width) for key, _, _, rows, width, _, _, _ in built.outs}


def ratios(built, got, outs=None):
    """{output name: (relative L2, worst |error| / bound)} of `got` ({name: array}) against the float64 reference; a non-finite element counts as
    an infinite ratio"""
    out = {}
    for key, _, _, _, _, _, want, bound in outs or built.outs:
        g = np.asarray(got[key], np.float64)
        with np.errstate(invalid='ignore'):
            err = np.abs(g - want)
        err = np.where(np.isfinite(g), err, np.inf)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
        rel = float(np.linalg.norm(np.where(np.isfinite(g), g - want, np.inf)) / max(np.linalg.norm(want), 1e-30))
        out[key] = (rel, float(q.max()))
    return out


# the defects the CPU test plants in the float32 emulation, each with the case it is planted in
DEFECTS = (
    ('diagonal one column off', 'infonce_rhat_67x67+0'),
    ('diagonal one column off', 'fused_F64_256x256+0'),
    ('diag_off ignored', 'infonce_rhat_33x66+33'),
    ('no maximum subtraction', 'infonce_rhat_67x67+0'),
    ('one lane stride left out of a row sum', 'infonce_rhat_515x515+0'),
    ('last partial column chunk left out', 'score_LDS64_S76_F20_B3'),
    ('rows of the second grid sweep skipped', 'infonce_rhat_515x515+0'),
    ('rows of the second grid sweep skipped', 'speder_grads_1030x512'),
    ('dU from phi of the neighbouring row', 'score_LDS64_S132_F256_B3'),
    ('inv_batch applied twice', 'infonce_theta100_67x67+0'),
    ('inv_batch applied twice', 'speder_grads_3x8'),
    ('inv_batch applied twice', 'score_VEC_S36_F257_B3'),
    ("second column-sum set with the first set's row count", 'colsum2_513x17_w'),
)
