"""Cases, host buffers and float64 references of the 16-row tile engine's table hook (rlrep_gemm16_table), shared by
tests/test_gemm16_engine.py (GPU: the launches) and tests/test_gemm16_hook_cpu.py (CPU: the error bound and the hook's refusals).

One launch = one Case = a table of tasks.  build(case) lays every operand and output of the launch out in ONE float32 arena (the fast
front ends need all operands within 16 GiB of one base):

  * operands sit in matrices with a padded row stride and GUARD extra rows, the padding filled with NaN -- a masked load that leaks one
    padded element into a sum makes the result non-finite;
  * outputs (C, and out2 where the epilogue has one) sit in matrices with ldc > Cn and GUARD extra rows, everything outside the R x Cn
    window filled with a sentinel bit pattern -- a stray store lands in the guard (never outside the allocation) and is seen as a changed bit.

The reference of every task is the same operation in float64 NumPy on the float32 operands.  Per-element bound (forward and dX with no
activation or ReLU, and dW):
    |got - want| <= 2 K 2^-24 (|A| |B|^T |scale| + |bias| + |C0| + |r1u| |r1v|)
i.e. the worst case of a K-term fp32 fma sum in any order (K u sum |a||b|, u = 2^-24), doubled for the epilogue's roundings; the rank-1 term
of a dX task is one more addend of the epilogue and enters like the bias.  The bias gradient (a K-term sum of operand A's entries): 2 K 2^-24 sum |A|.
ELU / tanh / sin outputs are held to the relative-L2 bar only (the device transcendentals' error is not derived anywhere in the project)."""
import numpy as np

ACT = {'none': 0, 'relu': 1, 'elu': 2, 'sin': 3, 'tanh': 4}
MODE = {'fwd': (0, 0, 0), 'dx': (0, 1, 1), 'dw': (1, 1, 3)}          # la, lb, epi
GUARD = 16
U24 = 2.0 ** -24


def act_f(x, a):
    if a == 'relu':
        return np.maximum(x, 0)
    if a == 'elu':
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    if a == 'sin':
        return np.sin(x)
    if a == 'tanh':
        return np.tanh(x)
    return x


def dact_f(aux, a):
    if a == 'relu':
        return (aux > 0).astype(aux.dtype)
    if a == 'elu':
        return np.where(aux > 0, 1.0, aux + 1.0).astype(aux.dtype)
    if a == 'sin':
        return np.cos(aux)
    if a == 'tanh':
        return 1.0 - aux * aux
    return np.ones_like(aux)


def T(mode, R, Cn, K, act='none', accum=False, bias=True, biasgrad=None, r1=False, scale=1.0, lda=None, ldb=None, a_off=0, b_off=0,
      a_guard=GUARD, b_guard=GUARD):
    """One task: R x Cn output, inner length K.  mode 'fwd': A [R, K], B [Cn, K]; 'dx': A [R, K], B [K, Cn]; 'dw': A [K, R], B [K, Cn].
    lda / ldb: row strides (default: the row length + 4, rounded up to a multiple of 4 floats: 16-byte regular); a_off / b_off: floats by
    which the operand's first element is moved off a 16-byte boundary."""
    return dict(mode=mode, R=R, Cn=Cn, K=K, act=act, accum=accum, bias=bias, biasgrad=(mode == 'dw') if biasgrad is None else biasgrad,
                r1=r1, scale=scale, lda=lda, ldb=ldb, a_off=a_off, b_off=b_off, a_guard=a_guard, b_guard=b_guard)


class Case:
    def __init__(self, name, tasks, front, nf=1, duo_split=0, nf2=1):
        self.name, self.tasks, self.front, self.nf, self.duo_split, self.nf2 = name, tasks, front, nf, duo_split, nf2
        self.la, self.lb, _ = MODE[tasks[0]['mode']]


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # ---- record front end: K neither <= 64 nor a multiple of 256 ----
    for m in ('fwd', 'dx', 'dw'):
        add(f'rec_{m}_37x24x100', [T(m, 37, 24, 100)], 'record')
        add(f'rec_{m}_100x256x136', [T(m, 100, 256, 136)], 'record')
    for a in ('relu', 'elu', 'sin', 'tanh'):
        add(f'rec_fwd_{a}', [T('fwd', 37, 24, 100, act=a)], 'record')
        add(f'rec_dx_{a}', [T('dx', 37, 24, 100, act=a)], 'record')
    add('rec_dx_accum', [T('dx', 37, 24, 100, accum=True)], 'record')
    add('rec_dx_relu_accum', [T('dx', 37, 24, 100, act='relu', accum=True)], 'record')
    add('rec_dw_accum', [T('dw', 37, 24, 100, accum=True)], 'record')
    add('rec_dw_no_biasgrad', [T('dw', 37, 24, 100, biasgrad=False)], 'record')
    add('rec_dw_biasgrad_9_column_tiles', [T('dw', 37, 136, 100)], 'record')
    add('rec_fwd_no_bias', [T('fwd', 37, 24, 100, bias=False)], 'record')
    add('rec_dx_rank1_scale', [T('dx', 37, 24, 100, r1=True, scale=0.5)], 'record')
    add('rec_dx_rank1_scale_elu_accum', [T('dx', 37, 24, 100, r1=True, scale=0.5, act='elu', accum=True)], 'record')
    # scalar-load variants (VA / VB = false): a row stride that is no multiple of 4, a pointer one float off a 16-byte boundary
    add('rec_fwd_lda101', [T('fwd', 37, 24, 100, lda=101)], 'record')
    add('rec_fwd_a_off1', [T('fwd', 37, 24, 100, a_off=1)], 'record')
    add('rec_fwd_ldb101_a_regular', [T('fwd', 37, 24, 100, ldb=101)], 'record')            # A 16-byte regular, B not: the all-scalar instantiation
    add('rec_fwd_b_off1_a_regular', [T('fwd', 37, 24, 100, act='relu', b_off=1)], 'record')
    add('rec_dx_lda101', [T('dx', 37, 24, 100, lda=101, act='relu')], 'record')
    add('rec_dx_a_off1', [T('dx', 37, 24, 100, a_off=1)], 'record')
    add('rec_dx_ldb29_b_off1', [T('dx', 37, 24, 100, ldb=29, b_off=1)], 'record')
    add('rec_dw_odd_strides', [T('dw', 37, 24, 100, lda=41, ldb=29, a_off=1, b_off=1)], 'record')
    # ---- fast, K % 256 == 0, one task ----
    for a in ('elu', 'relu', 'none', 'tanh'):
        add(f'fast_fwd_{a}_100x256x256', [T('fwd', 100, 256, 256, act=a)], 'fast')
    for a in ('none', 'relu', 'elu', 'sin', 'tanh'):
        add(f'fast_dx_{a}_100x256x512', [T('dx', 100, 256, 512, act=a)], 'fast')
        add(f'fast_dx_{a}_accum_100x256x512', [T('dx', 100, 256, 512, act=a, accum=True)], 'fast')
    add('fast_fwd_R8', [T('fwd', 8, 256, 256, act='relu')], 'fast')
    add('fast_dx_R8', [T('dx', 8, 256, 256)], 'fast')
    add('k256_fwd_Cn40_three_column_tiles', [T('fwd', 100, 40, 256, act='relu')], 'record')
    add('fast_fwd_Cn24_half_empty_tile', [T('fwd', 100, 24, 256, act='relu')], 'fast')
    add('fast_dx_Cn24_half_empty_tile', [T('dx', 100, 24, 256)], 'fast')
    # ---- fast, K <= 64, row x row forward (the first layers) ----
    add('short_K17_elu', [T('fwd', 100, 256, 17, act='elu', lda=17, ldb=17)], 'fast')
    add('short_K23_relu', [T('fwd', 100, 256, 23, act='relu', lda=23, ldb=23)], 'fast')
    add('short_K40_elu', [T('fwd', 100, 256, 40, act='elu', lda=40, ldb=40)], 'fast')
    add('short_K40_relu_a_off1', [T('fwd', 100, 256, 40, act='relu', lda=40, ldb=40, a_off=1)], 'fast')
    add('short_K64_relu_aligned', [T('fwd', 100, 256, 64, act='relu', lda=64, ldb=64)], 'fast')
    add('short_mixed_acts', [T('fwd', 100, 256, 17, act='elu', lda=17, ldb=17), T('fwd', 100, 256, 23, act='relu', lda=23, ldb=23)], 'fast')
    add('short_K17_none_is_record', [T('fwd', 100, 256, 17, lda=17, ldb=17)], 'record')      # (no short instantiation without an activation)
    # ---- two-task fast launches of different shapes ----
    add('fast2_256_then_512', [T('fwd', 100, 256, 256, act='elu'), T('fwd', 100, 512, 256, act='elu')], 'fast')
    add('fast2_512_then_256', [T('fwd', 100, 512, 256, act='elu'), T('fwd', 100, 256, 256, act='elu')], 'fast')
    add('fast2_dx_mixed_rows', [T('dx', 100, 256, 256, act='relu'), T('dx', 37, 64, 512, act='relu')], 'fast')
    add('two_tasks_one_K136_is_record', [T('fwd', 100, 256, 256, act='elu'), T('fwd', 100, 256, 136, act='elu')], 'record')
    # ---- fast4: three / four tasks of one shape ----
    for n in (3, 4):
        add(f'fast4_fwd_elu_{n}', [T('fwd', 100, 256, 256, act='elu') for _ in range(n)], 'fast4')
        add(f'fast4_dx_{n}', [T('dx', 100, 256, 256, act='elu' if n == 3 else 'none') for _ in range(n)], 'fast4')
    add('four_tasks_one_other_Cn_is_record', [T('fwd', 100, 256, 256, act='elu') for _ in range(3)] + [T('fwd', 100, 240, 256, act='elu')], 'record')
    # ---- NF = 2 and 4 ----
    for nf in (2, 4):
        for m in ('fwd', 'dx', 'dw'):
            add(f'nf{nf}_{m}_100x520x256', [T(m, 100, 520, 256, act='relu' if m == 'fwd' else 'none')], 'record', nf=nf)
    add('nf2_fwd_100x512x256', [T('fwd', 100, 512, 256, act='elu')], 'fast', nf=2)
    add('nf2_dx_100x512x256', [T('dx', 100, 512, 256, act='relu')], 'fast', nf=2)
    add('nf4_fwd_100x512x256', [T('fwd', 100, 512, 256, act='relu')], 'record', nf=4)
    add('nf4_dx_100x512x256', [T('dx', 100, 512, 256, accum=True)], 'record', nf=4)
    # the weight-gradient launch of a step: eight tasks of mixed shapes at NF = 4 (234 tiles: dealt to the XCDs, 234 % 8 = 2)
    add('nf4_dw_8_tasks', [T('dw', R, Cn, 100) for R, Cn in ((256, 17), (256, 256), (256, 256), (1, 256), (256, 23), (256, 256), (12, 256), (24, 40))],
        'record', nf=4)
    add('nf2_dw_3_tasks_accum', [T('dw', 100, 72, 136, accum=True), T('dw', 17, 520, 100), T('dw', 256, 17, 37)], 'record', nf=2)
    # ---- XCD run dealing: >= 64 tiles, total % 8 != 0 ----
    add('xcd_dw_65_tiles', [T('dw', 80, 208, 100)], 'record')
    add('xcd_dw_107_tiles_3_tasks', [T('dw', 48, 100, 100), T('dw', 64, 136, 72), T('dw', 80, 150, 100, accum=True)], 'record')
    # ---- packed-argument guards: a row stride that does not fit 16 bits ----
    add('lda_65540', [T('fwd', 16, 256, 256, act='relu', lda=65540, a_guard=0)], 'record')
    add('ldb_65540', [T('fwd', 100, 16, 256, act='relu', ldb=65540, b_guard=0)], 'record')
    # ---- duo: dX-form and weight-gradient-form tasks in one launch ----
    for nf2 in (1, 4):
        add(f'duo_nf2_{nf2}_aligned', [T('dx', 100, 64, 256, act='relu'), T('dw', 64, 256, 100)], 'record', duo_split=1, nf2=nf2)
        add(f'duo_nf2_{nf2}_a_off1', [T('dx', 100, 64, 256, a_off=1), T('dw', 64, 256, 100, accum=True)], 'record', duo_split=1, nf2=nf2)
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
XCD_CASES = ['nf4_dw_8_tasks', 'nf2_dw_100x520x256', 'xcd_dw_65_tiles', 'xcd_dw_107_tiles_3_tasks']          # (234, 119, 65 and 107 tiles)


def _sentinel(n, salt):
    """n floats of a recognisable finite bit pattern (0xC0DExxxx: about -6.9)"""
    return (np.uint32(0xC0DE0000) + ((np.arange(n, dtype=np.uint32) * np.uint32(7) + np.uint32(salt)) & np.uint32(0xffff))).view(np.float32)


class _Arena:
    def __init__(self):
        self.cur, self.fills = 0, []

    def place(self, n, off=0):
        start = (self.cur + 3) // 4 * 4 + off
        self.cur = start + n
        return start


class Built:
    """arena: float32 host image of the launch's one allocation; tasks: per task a dict of offsets / strides (floats from the arena's start),
    `outs`: [(name, offset, rows_total, ld, R, Cn, want64, bound64 or None)]"""


def build(case, seed=0):
    rs = np.random.RandomState(1000 + seed + sum(map(ord, case.name)))
    ar = _Arena()
    lay, data = [], []
    for t in case.tasks:
        la, lb, epi = MODE[t['mode']]
        R, Cn, K = t['R'], t['Cn'], t['K']
        ash = (K, R) if la else (R, K)
        bsh = (K, Cn) if lb else (Cn, K)
        lda = t['lda'] or (ash[1] + 4 + 3) // 4 * 4
        ldb = t['ldb'] or (bsh[1] + 4 + 3) // 4 * 4
        assert lda >= ash[1] and ldb >= bsh[1]
        ldc = Cn + 8
        d = dict(t)
        d.update(la=la, lb=lb, epi=epi, lda=lda, ldb=ldb, ldc=ldc, ash=ash, bsh=bsh,
                 a_rows=ash[0] + t['a_guard'], b_rows=bsh[0] + t['b_guard'])
        d['a'] = ar.place(d['a_rows'] * lda, t['a_off'])
        d['b'] = ar.place(d['b_rows'] * ldb, t['b_off'])
        d['c'] = ar.place((R + GUARD) * ldc)
        d['bias_o'] = ar.place(Cn + GUARD) if (epi == 0 and t['bias']) else None
        d['aux_o'] = ar.place((R + GUARD) * ldc) if epi == 1 else None           # (aux shares C's shape and stride)
        d['out2_o'] = ar.place((R + GUARD) * ldc) if (epi == 0 and t['act'] == 'sin') else ar.place(R + GUARD) if (epi == 3 and t['biasgrad']) else None
        d['r1u_o'] = ar.place(R + GUARD) if t['r1'] else None
        d['r1v_o'] = ar.place(Cn + GUARD) if t['r1'] else None
        lay.append(d)
    arena = np.full(ar.cur + 4, np.nan, np.float32)
    out = Built()
    out.tasks, out.outs = lay, []
    for q, d in enumerate(lay):
        R, Cn, K = d['R'], d['Cn'], d['K']
        A = (rs.standard_normal(d['ash']) / np.sqrt(K)).astype(np.float32)      # keeps outputs O(1)
        Bm = rs.standard_normal(d['bsh']).astype(np.float32)
        C0 = rs.standard_normal((R, Cn)).astype(np.float32)
        va = arena[d['a']:d['a'] + d['a_rows'] * d['lda']].reshape(d['a_rows'], d['lda'])
        va[:d['ash'][0], :d['ash'][1]] = A
        vb = arena[d['b']:d['b'] + d['b_rows'] * d['ldb']].reshape(d['b_rows'], d['ldb'])
        vb[:d['bsh'][0], :d['bsh'][1]] = Bm
        n = (R + GUARD) * d['ldc']
        arena[d['c']:d['c'] + n] = _sentinel(n, 11 * q)
        arena[d['c']:d['c'] + n].reshape(R + GUARD, d['ldc'])[:R, :Cn] = C0
        d['A'], d['B'], d['C0'] = (A.T if d['la'] else A), (Bm.T if d['lb'] else Bm), C0          # as [R, K], [Cn, K]
        d['bias_v'] = d['aux_v'] = d['r1u_v'] = d['r1v_v'] = None
        if d['bias_o'] is not None:
            d['bias_v'] = rs.standard_normal(Cn).astype(np.float32)
            arena[d['bias_o']:d['bias_o'] + Cn] = d['bias_v']
        if d['aux_o'] is not None:
            d['aux_v'] = rs.standard_normal((R, Cn)).astype(np.float32)
            arena[d['aux_o']:d['aux_o'] + n].reshape(R + GUARD, d['ldc'])[:R, :Cn] = d['aux_v']
        if d['r1u_o'] is not None:
            d['r1u_v'], d['r1v_v'] = rs.standard_normal(R).astype(np.float32), rs.standard_normal(Cn).astype(np.float32)
            arena[d['r1u_o']:d['r1u_o'] + R] = d['r1u_v']
            arena[d['r1v_o']:d['r1v_o'] + Cn] = d['r1v_v']
        if d['out2_o'] is not None:
            n2 = n if d['epi'] == 0 else R + GUARD
            arena[d['out2_o']:d['out2_o'] + n2] = _sentinel(n2, 11 * q + 5)
        want, bound, want2, bound2 = evaluate(d, np.float64)
        out.outs.append((f'task {q} C', q, d['c'], R + GUARD, d['ldc'], R, Cn, want, bound))
        if want2 is not None:
            if d['epi'] == 0:
                out.outs.append((f'task {q} out2', q, d['out2_o'], R + GUARD, d['ldc'], R, Cn, want2, bound2))
            else:
                out.outs.append((f'task {q} bias gradient', q, d['out2_o'], 1, R + GUARD, 1, R, want2[None, :], bound2[None, :]))
    out.arena = arena
    return out


def evaluate(d, dt):
    """The task's operation in NumPy at precision dt (float64: the reference; float32: the CPU check of the bound).
    Returns (C, bound or None, second output or None, its bound or None); the bounds always in float64."""
    K, act = d['K'], d['act']
    A, B, C0 = d['A'].astype(dt), d['B'].astype(dt), d['C0'].astype(dt)
    sc = dt(d['scale'])
    prod = (A @ B.T) * sc
    mag = (np.abs(d['A'].astype(np.float64)) @ np.abs(d['B'].astype(np.float64)).T) * abs(float(d['scale']))
    want2 = bound2 = None
    if d['epi'] == 0:
        pre = prod + (d['bias_v'].astype(dt) if d['bias_v'] is not None else dt(0))
        want = act_f(pre, act)
        if d['bias_v'] is not None:
            mag = mag + np.abs(d['bias_v'].astype(np.float64))
        if act == 'sin':
            want2, bound2 = pre, 2 * K * U24 * mag
    elif d['epi'] == 1:
        g = prod
        if d['r1u_v'] is not None:
            g = g + np.outer(d['r1u_v'].astype(dt), d['r1v_v'].astype(dt))
            mag = mag + np.outer(np.abs(d['r1u_v'].astype(np.float64)), np.abs(d['r1v_v'].astype(np.float64)))
        want = g * dact_f(d['aux_v'].astype(dt), act)
        if d['accum']:
            want = want + C0
            mag = mag + np.abs(d['C0'].astype(np.float64))
    else:
        want = prod + (C0 if d['accum'] else dt(0))
        if d['accum']:
            mag = mag + np.abs(d['C0'].astype(np.float64))
        if d['biasgrad']:
            want2, bound2 = A.sum(axis=1), 2 * K * U24 * np.abs(d['A'].astype(np.float64)).sum(axis=1)
    bound = 2 * K * U24 * mag if (d['epi'] == 3 or act in ('none', 'relu')) else None
    return want, bound, want2, bound2
