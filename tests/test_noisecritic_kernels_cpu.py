"""CPU side of the noise-critic kernels' unit tests (tests/test_noisecritic_kernels.py runs the launches): the hook (rlrep_noisecritic) refuses bad
records before any GPU call; the host-only plan queries (rlrep_nc_fwd_plan, rlrep_nc_forms) name the form every case expects, and every compiled
form has a case; the per-element error bound of tests/noisecritic_cases.py holds for a float32 NumPy emulation of every case in its kernel's own
order (the bf16x3 forms with the split and the six kept products); and that bound trips on each planted defect."""
import ctypes as C

import numpy as np
import pytest

import noisecritic_cases as nc

RLREP_ERR_ARG = -1
PTR = 4096              # 16-byte aligned, never dereferenced: every call below is refused before a launch


def _good(kernel):
    """a record of `kernel` the hook would launch: every pointer set, small consistent extents"""
    from rlrep_amd import _lib
    a = _lib.NoisecriticArgs()
    r = getattr(a, kernel)
    if kernel == 'fwd':
        r.ntasks = 2
        for t in r.t[:2]:
            for name, typ in t._fields_:
                if typ is C.c_void_p:
                    setattr(t, name, PTR)
            t.B, t.F, t.H, t.ld_ml = 8, 64, 16, 128
    elif kernel == 'dx':
        r.GH[0] = r.GH[1] = r.U[0] = r.U[1] = r.W[0] = r.W[1] = r.noise = r.lstd = r.G = PTR
        r.B, r.F, r.H, r.nheads, r.ldgh, r.ld_l, r.ldg = 8, 64, 32, 2, 32, 128, 128
    else:
        r.ntasks, r.slab, r.bslab, r.slab_floats, r.bslab_floats = 2, PTR, PTR, 2 * 16 * 16 * 64, 2 * 16 * 16
        for t in r.t:
            for name, typ in t._fields_:
                if typ is C.c_void_p:
                    setattr(t, name, PTR)
            t.B, t.F, t.H, t.ldgh, t.ld_ml = 8, 64, 16, 16, 128
    return a, r


def _t(q, **kw):
    return ('t', q, kw)


REFUSALS = [
    # (what, kernel, environment, fields of the record, (task, fields of a task) ...)
    ('fwd: no tasks', 'fwd', {}, dict(ntasks=0)), ('fwd: five tasks', 'fwd', {}, dict(ntasks=5)), ('fwd: g2 3', 'fwd', {}, dict(g2=3)), ('fwd: cols 32', 'fwd', {}, dict(cols=32)),
    ('fwd: null mean', 'fwd', {}, {}, _t(0, mean=None)), ('fwd: null lstd', 'fwd', {}, {}, _t(1, lstd=None)), ('fwd: null noise', 'fwd', {}, {}, _t(0, noise=None)),
    ('fwd: null W', 'fwd', {}, {}, _t(0, W=None)), ('fwd: null bias', 'fwd', {}, {}, _t(1, bias=None)), ('fwd: null Hm', 'fwd', {}, {}, _t(0, Hm=None)),
    ('fwd: B 0', 'fwd', {}, {}, _t(0, B=0), _t(1, B=0)), ('fwd: F -4', 'fwd', {}, {}, _t(0, F=-4), _t(1, F=-4)), ('fwd: H 0', 'fwd', {}, {}, _t(1, H=0)),
    ('fwd: F % 4', 'fwd', {}, {}, _t(0, F=66), _t(1, F=66)), ('fwd: ld_ml below F', 'fwd', {}, {}, _t(0, ld_ml=60)), ('fwd: ld_ml % 4', 'fwd', {}, {}, _t(1, ld_ml=130)),
    ('fwd: mean off 16 bytes', 'fwd', {}, {}, _t(0, mean=PTR + 4)), ('fwd: lstd off 16 bytes', 'fwd', {}, {}, _t(0, lstd=PTR + 8)),
    ('fwd: noise off 16 bytes', 'fwd', {}, {}, _t(1, noise=PTR + 12)), ('fwd: sigma_out off 16 bytes', 'fwd', {}, {}, _t(1, sigma_out=PTR + 4)),
    ('fwd: tasks differ in F', 'fwd', {}, {}, _t(1, F=96)), ('fwd: bf16x3 tasks differ in B', 'fwd', {}, {}, _t(1, B=9)), ('fwd: bf16x3 tasks differ in H', 'fwd', {}, {}, _t(1, H=17)),
    ('fwd: g2 1 on bf16x3', 'fwd', {}, dict(g2=1)), ('fwd: g2 4 on bf16x3', 'fwd', {}, dict(g2=4)),
    ('fwd: chunked with cols 64', 'fwd', {'RLREP_DISABLE': 'x3'}, dict(cols=64), _t(0, F=512, ld_ml=1024), _t(1, F=512, ld_ml=1024)),
    ('fwd: chunked by the switch with cols 64', 'fwd', {'RLREP_DISABLE': 'x3', 'RLREP_ENABLE': 'nc_fwd_chunk'}, dict(cols=64)),
    ('fwd: w3 with F % 32', 'fwd', {}, {}, _t(0, F=80, ld_ml=160), _t(1, F=80, ld_ml=160)), ('fwd: w3 off 16 bytes', 'fwd', {}, {}, _t(0, w3=PTR + 8)),
    ('fwd: w3 with W off 16 bytes', 'fwd', {}, {}, _t(1, W=PTR + 4)),
    ('dx: no heads', 'dx', {}, dict(nheads=0)), ('dx: three heads', 'dx', {}, dict(nheads=3)), ('dx: null GH of head 1', 'dx', {}, dict(GH=(PTR, None))),
    ('dx: null U', 'dx', {}, dict(U=(None, PTR))), ('dx: null W of head 1', 'dx', {}, dict(W=(PTR, None))), ('dx: null noise', 'dx', {}, dict(noise=None)),
    ('dx: null lstd', 'dx', {}, dict(lstd=None)), ('dx: null G', 'dx', {}, dict(G=None)), ('dx: B 0', 'dx', {}, dict(B=0)), ('dx: F 0', 'dx', {}, dict(F=0)),
    ('dx: H -1', 'dx', {}, dict(H=-1)), ('dx: F % 4', 'dx', {}, dict(F=62)), ('dx: ldgh below H', 'dx', {}, dict(ldgh=28)), ('dx: ldgh % 4', 'dx', {}, dict(ldgh=34)),
    ('dx: ld_l below F', 'dx', {}, dict(ld_l=60)), ('dx: ldg below 2 F', 'dx', {}, dict(ldg=124)), ('dx: ldg % 4', 'dx', {}, dict(ldg=130)),
    ('dx: lstd off 16 bytes', 'dx', {}, dict(lstd=PTR + 4)), ('dx: noise off 16 bytes', 'dx', {}, dict(noise=PTR + 8)),
    ('dw: no tasks', 'dw', {}, dict(ntasks=0)), ('dw: three tasks', 'dw', {}, dict(ntasks=3)), ('dw: lean 2', 'dw', {}, dict(lean=2)), ('dw: splits 17', 'dw', {}, dict(splits=17)),
    ('dw: splits -1', 'dw', {}, dict(splits=-1)), ('dw: null U', 'dw', {}, {}, _t(0, U=None)), ('dw: null GH', 'dw', {}, {}, _t(1, GH=None)), ('dw: null mean', 'dw', {}, {}, _t(0, mean=None)),
    ('dw: null sigma', 'dw', {}, {}, _t(0, sigma=None)), ('dw: null noise', 'dw', {}, {}, _t(1, noise=None)), ('dw: null gW', 'dw', {}, {}, _t(1, gW=None)),
    ('dw: null gb', 'dw', {}, {}, _t(0, gb=None)), ('dw: B 0', 'dw', {}, {}, _t(0, B=0), _t(1, B=0)), ('dw: H 0', 'dw', {}, {}, _t(0, H=0), _t(1, H=0)),
    ('dw: F % 4', 'dw', {}, {}, _t(0, F=62), _t(1, F=62)), ('dw: ldgh below H', 'dw', {}, {}, _t(0, ldgh=12)), ('dw: ld_ml % 4', 'dw', {}, {}, _t(1, ld_ml=129)),
    ('dw: mean off 16 bytes', 'dw', {}, {}, _t(0, mean=PTR + 4)), ('dw: sigma off 16 bytes', 'dw', {}, {}, _t(1, sigma=PTR + 8)), ('dw: noise off 16 bytes', 'dw', {}, {}, _t(0, noise=PTR + 4)),
    ('dw: tasks differ in B', 'dw', {}, {}, _t(1, B=9)), ('dw: tasks differ in F', 'dw', {}, {}, _t(1, F=68)), ('dw: tasks differ in H', 'dw', {}, {}, _t(1, H=12)),
    ('dw: fp32 tasks differ in B', 'dw', {'RLREP_DISABLE': 'x3'}, {}, _t(1, B=9)),
    ('dw: bf16x3 without a slab', 'dw', {}, dict(slab=None)), ('dw: bf16x3 without a bias slab', 'dw', {}, dict(bslab=None)),
    ('dw: slab too small for 16 splits', 'dw', {}, dict(splits=16, slab_floats=2 * 16 * 16 * 64 - 1)), ('dw: bias slab too small', 'dw', {}, dict(bslab_floats=2 * 16 - 1)),
]


@pytest.mark.parametrize('what,kernel,env,kw,tasks', [(r[0], r[1], r[2], r[3], r[4:]) for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_hook_refuses(what, kernel, env, kw, tasks, monkeypatch):
    """No GPU is needed: a refusal happens before any GPU call, rl_nc_init() included (this test runs where there is none)."""
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, r = _good(kernel)
    form = (C.c_int32 * 4)(-7, -7, -7, -7)
    r.form = C.cast(form, C.POINTER(C.c_int32))
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(r, k)[i] = x
        else:
            setattr(r, k, v)
    for _, q, tk in tasks:
        for k, v in tk.items():
            setattr(r.t[q], k, v)
    assert _lib.lib.rlrep_noisecritic(_lib.NC_KERNEL[kernel], C.byref(a), None) == RLREP_ERR_ARG, what
    msg = _lib.lib.rlrep_last_error()
    assert msg and msg.startswith(b'noisecritic:'), (what, msg)


def test_hook_refuses_unknown_kernels_and_a_null_record_and_the_abi_is_unchanged():
    from rlrep_amd import _lib
    a, _ = _good('dx')
    for kernel in (-1, 3, 1000):
        assert _lib.lib.rlrep_noisecritic(kernel, C.byref(a), None) == RLREP_ERR_ARG and _lib.lib.rlrep_last_error().startswith(b'noisecritic:')
    assert _lib.lib.rlrep_noisecritic(0, None, None) == RLREP_ERR_ARG and _lib.lib.rlrep_last_error().startswith(b'noisecritic:')
    assert _lib.lib.rlrep_abi_version() == 4                                # additive
    o = C.c_int32()
    assert _lib.lib.rlrep_nc_forms(0, 8, 64, 64, 1, C.byref(o), None) == RLREP_ERR_ARG
    assert _lib.lib.rlrep_nc_forms(1, 8, 64, 64, 3, C.byref(o), None) == RLREP_ERR_ARG
    assert _lib.lib.rlrep_nc_w3_bytes(0, 64) == 0 and _lib.lib.rlrep_nc_w3_bytes(64, -1) == 0
    assert _lib.lib.rlrep_nc_w3_bytes(5, 64) >= 3 * 2 * 5 * 64 + 56 and _lib.lib.rlrep_nc_w3_bytes(5, 64) % 16 == 0


def test_every_compiled_form_has_a_case_and_the_never_planned_ones_are_the_overrides(monkeypatch):
    assert {c.form for c in nc.CASES} == set(nc.FORMS)
    assert set(nc.NEVER_PLANNED) < set(nc.FORMS)
    # what rl_nc_fwd_plan can return, over a sweep of shapes and both engines' switches: g2 in {1, 2}, 128 columns on fp32 (64 on bf16x3 only)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    seen = set()
    for off in ('', 'x3'):
        monkeypatch.setenv('RLREP_DISABLE', off)
        for nt in (1, 2, 3, 4):
            for B in (1, 5, 64, 256, 1024, 4096):
                for F in (4, 20, 64, 96, 256, 432, 512):
                    for H in (3, 64, 130, 256, 1024):
                        seen.add(nc.fwd_plan(nt, B, F, H))
    assert {(e, g) for e, g, _ in seen} == {(0, 1), (0, 2), (1, 2)} and {c for e, _, c in seen if e == 0} == {128} and {c for e, _, c in seen if e == 1} == {64, 128}


@pytest.mark.parametrize('name', [c.name for c in nc.CASES if c.kernel != 'dx'])
def test_plan_names_the_form_of_every_case(name, monkeypatch):
    case = nc.BY_NAME[name]
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    got, form = nc.expected_form(case)
    assert got == case.form, (name, got, form)
    if case.p.get('twin'):
        for k in ('RLREP_ENABLE', 'RLREP_DISABLE'):
            monkeypatch.delenv(k, raising=False)
        for k, v in case.p['twin'].items():
            monkeypatch.setenv(k, v)
        assert nc.expected_form(case)[0] == case.form.replace('chunk_', ''), name


def test_the_dw_cases_cut_the_batch_as_their_comments_say():
    s = {c.name: nc.dw_splits(c) for c in nc.CASES if c.kernel == 'dw'}
    assert s['dw_x3r_5x64x32_t1'] == 1 and s['dw_x3_3x64x64_t2_s4'] == 4 and s['dw_x3r_66x68x70_t1_s1'] == 1
    assert nc.dw_split_rows(3, 4) == [(0, 1), (1, 1), (2, 1), (3, 0)]                                   # the fourth split has no rows
    assert s['dw_x3r_37x96x96_t2'] == 5 and nc.dw_split_rows(37, 5)[-1] == (32, 5)
    assert s['dw_x3r_260x256x256_t2'] == 8 and nc.dw_split_rows(260, 8)[0] == (0, 33) and nc.dw_split_rows(260, 8)[-1] == (231, 29)


def test_the_bf16_split_is_exact_and_the_dropped_products_are_inside_their_term():
    rs = np.random.RandomState(5)
    x = (rs.standard_normal(20000) * np.exp(rs.uniform(-20, 20, 20000))).astype(np.float32)
    y = (rs.standard_normal(20000) * np.exp(rs.uniform(-20, 20, 20000))).astype(np.float32)
    (xh, xm, xl), (yh, ym, yl) = nc.split3(x), nc.split3(y)
    assert np.array_equal(xh.astype(np.float64) + xm + xl, x.astype(np.float64))
    for part in (xh, xm, xl):
        assert not (part.view(np.uint32) & np.uint32(0xffff)).any()                                   # bf16 values
    dropped = np.abs(xm.astype(np.float64) * yl) + np.abs(xl.astype(np.float64) * ym) + np.abs(xl.astype(np.float64) * yl)
    assert np.all(dropped <= nc.X3_DROPPED * nc.U24 * np.abs(x.astype(np.float64) * y))


def test_elu_fast_error_term_covers_the_float32_evaluation():
    """the docstring's 2^-23 e^x (1 + |x|) + 2^-24 |y| against exp2 of the rounded product in float32, over (-100, 0]; its supremum is under 1.5e-7"""
    x = -np.concatenate([np.linspace(0, 100, 200001), np.logspace(-30, 2, 20001)]).astype(np.float32)
    got = nc._elu_fast(nc._B32, x).astype(np.float64)
    want = nc._elu_fast(nc._B64, nc.V(x.astype(np.float64)))
    assert np.all(np.abs(got - want.v) <= want.e)
    assert 1.3e-7 < want.e.max() < 1.5e-7


_worst = {}


@pytest.mark.parametrize('name', [c.name for c in nc.CASES])
def test_float32_emulation_stays_inside_the_error_bound(name):
    """Every case's float32 NumPy emulation, in its kernel's order and with the bf16x3 split where the form has one, before the kernels are held to
    the same bound.  Prints the worst ratio per form (pytest -s)."""
    case = nc.BY_NAME[name]
    built = nc.build(case)
    for key, (rel, ratio) in nc.ratios(built, nc.emulate(case, built)).items():
        assert ratio < 1, (name, key, ratio)
        assert rel < 1e-5, (name, key, rel)
        k = (case.form, key.rstrip('0123'))
        _worst[k] = max(_worst.get(k, 0.0), ratio)
    print(f'noisecritic {name}: float32 emulation, worst |err|/bound so far per output of {case.form}: '
          + ', '.join(f'{k[1]} {v:.3f}' for k, v in sorted(_worst.items()) if k[0] == case.form))


def test_every_case_carries_the_edge_inputs():
    """log_std below -20, above 2 and exactly at both; elu outputs positive, exactly 0 and within 1e-6 of -1 (forward: pre-activations on both
    sides of 0 and below -30); a zero row of GH wherever the batch has two rows"""
    for case in nc.CASES:
        if case.p['B'] * case.p['F'] * case.p['H'] > 5000000:
            continue                                                        # (the same generators; the large arenas are built by their own tests)
        b = nc.build(case)
        if case.kernel in ('fwd', 'dx'):
            for k, ls in b.h.items():
                if k.startswith('lstd'):
                    assert (ls < -20).any() and (ls > 2).any() and (ls == -20).any() and (ls == 2).any(), (case.name, k)
        if case.kernel == 'fwd' and case.p['H'] >= 3:
            for q in range(case.p['ntasks']):
                x = b.h[f'mean{q}'][:, None, :].astype(np.float64) + np.exp(np.clip(b.h[f'lstd{q}'], -20, 2).astype(np.float64))[:, None, :] * b.h['noise'][None]
                pre = x @ b.h[f'W{q}'].T.astype(np.float64) + b.h[f'bias{q}']
                assert (pre > 0).any() and (pre < 0).any() and (pre == 0).any() and (pre < -30).any(), case.name
        if case.kernel in ('dx', 'dw'):
            for k, u in b.h.items():
                if k.startswith('U'):
                    assert (u > 0).any() and (u == 0).any() and (u == -1).any() and ((u > -1) & (u < -1 + 1e-6)).any(), (case.name, k)
                if k.startswith('GH') and case.p['B'] >= 2:
                    assert (np.abs(u).sum(1) == 0).any(), (case.name, k)
        if case.kernel == 'dw':
            for k, s in b.h.items():
                if k.startswith('sigma'):
                    assert (s == np.exp(np.float32(2))).any() and (s < 3e-9).any(), (case.name, k)


@pytest.mark.parametrize('defect,name,key', nc.DEFECTS, ids=[f'{d} in {n}' for d, n, _ in nc.DEFECTS])
def test_the_bound_catches_a_planted_defect(defect, name, key):
    """relative L2 alone need not trip (printed); some element of the named output must leave its bound"""
    case = nc.BY_NAME[name]
    built = nc.build(case)
    clean = nc.ratios(built, nc.emulate(case, built))
    assert max(q for _, q in clean.values()) < 1
    bad = nc.ratios(built, nc.emulate(case, built, defect))
    print(f'noisecritic defect "{defect}" in {name}: ' + ', '.join(f'{k}: rel-L2 {r:.2e} ratio {q:.3g}' for k, (r, q) in bad.items() if q != clean[k][1]))
    assert bad[key][1] > 1, (defect, name, bad)


@pytest.mark.parametrize('defect,name,key', nc.UNCAUGHT, ids=[f'{d} in {n}' for d, n, _ in nc.UNCAUGHT])
def test_what_the_bound_does_not_catch_stays_on_record(defect, name, key):
    """the h l product of a bf16x3 pair is 2^-16 of the product: left out, the result moves, but stays inside a bound built on 2 K e sum|a||b|"""
    case = nc.BY_NAME[name]
    built = nc.build(case)
    clean, bad = nc.emulate(case, built), nc.emulate(case, built, defect)
    assert not np.array_equal(clean[key], bad[key])
    r = nc.ratios(built, bad)[key]
    print(f'noisecritic defect "{defect}" in {name}: {key}: rel-L2 {r[0]:.2e} ratio {r[1]:.3g} (not caught)')
