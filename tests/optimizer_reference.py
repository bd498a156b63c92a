"""Float64 reference of one optimizer step (Adam + Polyak + the fp64 temperature update) with PER-ELEMENT rounding bounds.

What is held to it: every element that the optimizer launches (csrc/elementwise.hip adam_kernel / adam_l1_kernel) or the weight-gradient
epilogues (FLAG_ADAM, csrc/gemm16_tile.h) write, through `adam_elem` (csrc/common.h) with the scalars of `adam_scalars` / `bump_group`.

The reference
-------------
Hyper-parameters are the float32 values of the group record (include/rlrep.h's float hyper-parameters) widened to double -- 1 - float32(0.999),
not 0.001 -- and the step is the record's bumped counter:

    m* = m0 + (1 - b1) (g - m0)
    v* = b2 v0 + (1 - b2) g^2
    d* = sqrt(v*) / sqrt(1 - b2^step) + eps
    u* = m* / d*
    p* = p0 - lr / (1 - b1^step) u*
    t* = tau p1 + (1 - tau) t0                 (p1: the parameter the DEVICE wrote)

all evaluated in float64 (rounding 1.1e-16: eight orders below the bounds).

The bounds
----------
e = 2^-24 is the unit roundoff of float32 round-to-nearest: fl(x) = x (1 + d), |d| <= e, for every operation adam_elem performs (each one an
explicit __f*_rn), and for each conversion of a double scalar to float (w1, w2, nss, bc2s, omt).  Second-order terms (e^2) are absorbed by the
slack between the counted coefficient and the stated one.  A floor of 2^-149 (the smallest subnormal) is added to each bound; magnitudes under
test stay normal.

m1 = fl(fl(w1) * fl(g - m0) + m0)                                   [fma: one rounding]
    The product term carries 2 e (w1, the subtraction) on (1 - b1) |g - m0| <= |g| + |m0|, the final rounding 1 e on |m*| <= |g| + |m0|:
        |m1 - m*| <= 3 e (|m0| + |g|)   ->  stated 4 e (|m0| + |g|).

v1 = fl(fl(fl(w2) * g) * g + fl(v0 * b2))                           [mul, mul, fma]
    Every term is non-negative, so relative errors add on v*: w2, w2 * g and the fma on the first term (3 e), the product and the fma on the
    second (2 e):
        |v1 - v*| <= 3 e v*             ->  stated 4 e v*.

p1 = fl(fl(nss) * fl(m1 / denom) + p0),  denom = fl(fl(fl(sqrt(v1)) / fl(bc2s)) + eps)
    sqrt(v1) = sqrt(v*) (1 + 1.5 e) [half of v's 3 e]; its rounding 1 e; bc2s 1 e; the quotient 1 e: 4.5 e on the first term of d*, which is at
    most d* (eps > 0 is exact); the sum 1 e: denom = d* (1 + 5.5 e).  The quotient m1 / denom: m's absolute error over d*, plus 5.5 e + 1 e on
    u*.  nss 1 e more: 7.5 e on u*.  The final fma rounds once, 1 e on |p*|:
        |p1 - p*| <= 1 e |p*| + |lr / (1 - b1^step)| (3 e (|m0| + |g|) / d* + 7.5 e |u*|)
                                        ->  stated 2 e |p*| + |lr / (1 - b1^step)| (4 e (|m0| + |g|) / d* + 8 e |u*|).

t1 = fl(tau * p1 + fl(fl(1 - tau) * t0))                            [mul, fma; the stand-alone polyak_kernel may also round tau * p1]
    omt and its product 2 e on |(1 - tau) t0| <= |t0|, at most 1 e on |tau p1| (unfused form), the sum 1 e on |t*| <= |tau p1| + |t0|:
        |t1 - t*| <= 2 e |tau p1| + 3 e |t0|   ->  stated 3 e (|tau p1| + |t0|).

The temperature (FIN_ALPHA, csrc/kparams.h) is float64 Adam on a scalar; check_temperature() recovers its gradient from the first moment and
holds the second moment and log_alpha to 1e-12 relative (double rounding is 1.1e-16; the recovery of g from m costs a cancellation of at most
(|m1| + b1 |m0|) / ((1 - b1) |g|) roundoffs, about ten for moments the size of the gradient).
"""
import numpy as np

EPS = 2.0 ** -24
FLOOR = 2.0 ** -149
QUANTITIES = ('m', 'v', 'p', 't')


def record(cfg_row):
    """(step, lr, b1, b2, eps, tau) of one optimizer group record (float32[22]: word 0 the int32 step, words 1..5 the hyper-parameters as the
    device holds them), the hyper-parameters widened to double."""
    row = np.ascontiguousarray(np.asarray(cfg_row, dtype=np.float32))
    step = int(row[:1].view(np.int32)[0])
    lr, b1, b2, eps, tau = (float(x) for x in row[1:6].astype(np.float64))
    return step, lr, b1, b2, eps, tau


def expected(p0, g, m0, v0, t0, lr, b1, b2, eps, tau, step):
    """Float64 Adam (+ Polyak of the reference's own p*) -> dict m, v, d, u, p, t, step_size.  Scalars may be Python floats or float32 scalars;
    they are used as doubles."""
    p0, g, m0, v0 = (np.asarray(x, dtype=np.float64) for x in (p0, g, m0, v0))
    lr, b1, b2, eps, tau = float(lr), float(b1), float(b2), float(eps), float(tau)
    st = float(step)
    m = m0 + (1.0 - b1) * (g - m0)
    v = b2 * v0 + (1.0 - b2) * g * g
    d = np.sqrt(v) / np.sqrt(1.0 - b2 ** st) + eps
    u = m / d
    step_size = lr / (1.0 - b1 ** st)
    p = p0 - step_size * u
    out = dict(m=m, v=v, d=d, u=u, p=p, step_size=step_size)
    if t0 is not None:
        out['t'] = polyak_expected(p, t0, tau)
    return out


def polyak_expected(p1, t0, tau):
    tau = float(tau)
    return tau * np.asarray(p1, dtype=np.float64) + (1.0 - tau) * np.asarray(t0, dtype=np.float64)


def bounds(ex, g, m0):
    """Per-element bounds on |device - expected| for m, v, p (module docstring)."""
    g, m0 = np.abs(np.asarray(g, dtype=np.float64)), np.abs(np.asarray(m0, dtype=np.float64))
    bm = 4.0 * EPS * (m0 + g) + FLOOR
    bv = 4.0 * EPS * ex['v'] + FLOOR
    bp = 2.0 * EPS * np.abs(ex['p']) + abs(ex['step_size']) * (4.0 * EPS * (m0 + g) / ex['d'] + 8.0 * EPS * np.abs(ex['u'])) + FLOOR
    return dict(m=bm, v=bv, p=bp)


def polyak_bound(p1, t0, tau):
    return 3.0 * EPS * (np.abs(float(tau) * np.asarray(p1, dtype=np.float64)) + np.abs(np.asarray(t0, dtype=np.float64))) + FLOOR


def _worst(err, bound):
    r = err / bound
    r = np.where(np.isfinite(r), r, np.inf)          # a NaN / inf the device wrote is a failure, not a skipped element
    if r.size == 0:
        return 0.0, -1
    i = int(np.argmax(r))
    return float(r[i]), i


def check_elements(p0, g, m0, v0, p1, m1, v1, cfg):
    """Ratios error / bound of m, v, p for flat arrays; cfg = (step, lr, b1, b2, eps, tau).  -> {q: (worst ratio, index)}"""
    step, lr, b1, b2, eps, tau = cfg
    ex = expected(p0, g, m0, v0, None, lr, b1, b2, eps, tau, step)
    bd = bounds(ex, g, m0)
    out = {}
    for q, got in (('m', m1), ('v', v1), ('p', p1)):
        out[q] = _worst(np.abs(np.asarray(got, dtype=np.float64) - ex[q]), bd[q])
    return out


def check_polyak(p1, t0, t1, tau):
    """Ratio error / bound of a Polyak update from the parameter values the device wrote.  -> (worst ratio, index)"""
    return _worst(np.abs(np.asarray(t1, dtype=np.float64) - polyak_expected(p1, t0, tau)), polyak_bound(p1, t0, tau))


def check_group(before, after, grads, cfg_row, slice, polyak_map, polyak_on):
    """One optimizer step of a whole group slice.

    before / after: dicts of the whole arenas as float32 NumPy arrays: 'params', 'targets', 'exp_avg', 'exp_avg_sq'
    grads:          the gradient arena after the step (what the device left there: plain gradients, epilogue gradients, summed split partials)
    cfg_row:        the group's record AFTER the step (float32[22], step already bumped)
    slice:          (offset, n) of the group in the parameter arena
    polyak_map:     [(parameter offset, target offset, n)] of the twins this step averages (absolute arena offsets)
    polyak_on:      whether the step's Polyak gate was open; closed: the twins' targets must be bit-identical

    -> {'m' | 'v' | 'p' | 't': (worst error / bound, arena index of that element)}; indices of 't' are target-arena indices."""
    off, n = int(slice[0]), int(slice[1])
    s = np.s_[off:off + n]
    cfg = record(cfg_row)
    out = check_elements(before['params'][s], np.asarray(grads)[s], before['exp_avg'][s], before['exp_avg_sq'][s],
                         after['params'][s], after['exp_avg'][s], after['exp_avg_sq'][s], cfg)
    out = {q: (r, off + i) for q, (r, i) in out.items()}
    worst_t = (0.0, -1)
    for po, to, cnt in polyak_map:
        po, to, cnt = int(po), int(to), int(cnt)
        t0, t1 = before['targets'][to:to + cnt], after['targets'][to:to + cnt]
        if polyak_on:
            r, i = check_polyak(after['params'][po:po + cnt], t0, t1, cfg[5])
        else:
            diff = t0.view(np.uint32) != t1.view(np.uint32)
            r, i = (np.inf, int(np.argmax(diff))) if diff.any() else (0.0, -1)
        if r > worst_t[0]:
            worst_t = (r, to + i)
    out['t'] = worst_t
    return out


def twin_map(descs, prefixes, target_arena=1):
    """[(parameter offset, target offset, n)] for every trainable tensor `x.rest` with x in `prefixes` that has a twin `x_target.rest` in the
    target arena.  descs: HipCore.descs, name -> (arena, group, offset, rows, cols)."""
    out = []
    for name, (arena, _group, off, rows, cols) in descs.items():
        head, _, rest = name.partition('.')
        if arena == target_arena or head not in prefixes or name.endswith('noise'):
            continue
        twin = descs.get(head + '_target.' + rest)
        if twin is None or twin[0] != target_arena:
            continue
        assert twin[3] * twin[4] == rows * cols, name
        out.append((off, twin[2], rows * cols))
    return out


def mask_of(total, ranges):
    """bool[total], True inside any (offset, n)."""
    mk = np.zeros(int(total), dtype=bool)
    for off, n in ranges:
        mk[int(off):int(off) + int(n)] = True
    return mk


def bit_identical_outside(before, after, mask):
    """Index of the first element outside `mask` whose bits changed, or -1."""
    diff = (np.asarray(before).view(np.uint32) != np.asarray(after).view(np.uint32)) & ~mask
    return int(np.argmax(diff)) if diff.any() else -1


def temperature_expected(alpha0, g, lr, b1, b2, eps):
    """float64 Adam of the scalar log_alpha on gradient g: alpha0 = (log_alpha, m, v, step) -> the next record."""
    la, m, v, st = (float(x) for x in alpha0)
    lr, b1, b2, eps = float(lr), float(b1), float(b2), float(eps)
    st += 1.0
    m = m + (1.0 - b1) * (g - m)
    v = v * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** st) + eps
    la = la - (lr / (1.0 - b1 ** st)) * (m / denom)
    return np.array([la, m, v, st], dtype=np.float64)


def check_temperature(alpha0, alpha1, lr, b1, b2, eps, rtol=1e-12):
    """From the record alone: g recovered from the first moment, then v1 and log_alpha1 against float64 Adam on that g.
    -> dict(g=, v=relative error, log_alpha=relative error, step_ok=bool, ok=bool)"""
    a0, a1 = np.asarray(alpha0, dtype=np.float64), np.asarray(alpha1, dtype=np.float64)
    b1d = float(b1)
    g = (a1[1] - b1d * a0[1]) / (1.0 - b1d)
    want = temperature_expected(a0, g, lr, b1, b2, eps)
    rel = lambda x, y: abs(x - y) / max(abs(y), 1e-300)
    ev, ela = rel(a1[2], want[2]), rel(a1[0], want[0])
    step_ok = a1[3] == a0[3] + 1.0
    return dict(g=float(g), v=ev, log_alpha=ela, step_ok=bool(step_ok), ok=bool(step_ok and ev <= rtol and ela <= rtol and np.isfinite(a1).all()))


# ---- adam_elem in NumPy float32 (every operation rounded to float32; the fma as a float64 product-sum rounded once) -------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def scalars_f32(lr, b1, b2, eps, tau, step, bias_step=None):
    """adam_scalars (csrc/common.h): doubles from the float32 record values, rounded to float32 once."""
    lr, b1, b2, eps, tau = (float(np.float32(x)) for x in (lr, b1, b2, eps, tau))
    st = float(step if bias_step is None else bias_step)
    return dict(nss=np.float32(-(lr / (1.0 - b1 ** st))), bc2s=np.float32(np.sqrt(1.0 - b2 ** st)), w1=np.float32(1.0 - b1), w2=np.float32(1.0 - b2),
                b2=np.float32(b2), eps=np.float32(eps), tau=np.float32(tau), omt=np.float32(1.0 - tau))


def emulate(p0, g, m0, v0, t0, sc, mutation=None):
    """adam_elem on float32 arrays -> (p1, m1, v1, t1).  `mutation` plants one of the defects the bounds must reject:
    'sqrt_eps_inside' (sqrt(v + eps)), 'tau_swapped', 'polyak_old_p'; the others ('skip4', 'bias_step') are planted by the caller."""
    p0, g, m0, v0 = _f32(p0), _f32(g), _f32(m0), _f32(v0)
    with np.errstate(all='ignore'):
        m1 = _fma(sc['w1'], (g - m0).astype(np.float32), m0)
        v1 = (v0 * sc['b2']).astype(np.float32)
        v1 = _fma((sc['w2'] * g).astype(np.float32), g, v1)
        if mutation == 'sqrt_eps_inside':
            denom = (np.sqrt((v1 + sc['eps']).astype(np.float32)).astype(np.float32) / sc['bc2s']).astype(np.float32)
        else:
            denom = ((np.sqrt(v1).astype(np.float32) / sc['bc2s']).astype(np.float32) + sc['eps']).astype(np.float32)
        p1 = _fma(sc['nss'], (m1 / denom).astype(np.float32), p0)
        t1 = None
        if t0 is not None:
            t0 = _f32(t0)
            src = p0 if mutation == 'polyak_old_p' else p1
            tau, omt = (sc['omt'], sc['tau']) if mutation == 'tau_swapped' else (sc['tau'], sc['omt'])
            t1 = _fma(tau, src, (omt * t0).astype(np.float32))
    return p1, m1, v1, t1


# ---- planted values shared by the CPU test of the bounds and the GPU test of the split entry points --------------------------------------------
def _log_uniform(rs, n, lo, hi, zero_frac, signed):
    x = np.exp(rs.uniform(np.log(lo), np.log(hi), size=n))
    if signed:
        x *= rs.choice([-1.0, 1.0], size=n)
    x[rs.rand(n) < zero_frac] = 0.0
    return x.astype(np.float32)


def wide_range(n, seed, p_zero):
    """|g|, |m| log-uniform in [1e-12, 1e4] with both signs, v in {0} u [1e-20, 1e6], exact zeros mixed in separately (so that every
    combination of zero / non-zero g, m, v occurs); p0 all-zero or random; targets random.  All magnitudes normal."""
    rs = np.random.RandomState(seed)
    g = _log_uniform(rs, n, 1e-12, 1e4, 0.1, True)
    m = _log_uniform(rs, n, 1e-12, 1e4, 0.1, True)
    v = _log_uniform(rs, n, 1e-20, 1e6, 0.1, False)
    p = np.zeros(n, np.float32) if p_zero else (0.05 * rs.standard_normal(n)).astype(np.float32)
    t = (0.05 * rs.standard_normal(n)).astype(np.float32)
    return p, g, m, v, t


def realistic(n, seed):
    rs = np.random.RandomState(seed)
    p = (0.05 * rs.standard_normal(n)).astype(np.float32)
    g = (1e-3 * rs.standard_normal(n)).astype(np.float32)
    m = (1e-3 * rs.standard_normal(n)).astype(np.float32)
    v = (1e-6 * rs.uniform(0.2, 2.0, size=n)).astype(np.float32)
    t = (p + 1e-3 * rs.standard_normal(n)).astype(np.float32)
    return p, g, m, v, t
