"""CPU side of the representation-loss kernels' unit tests (tests/test_replearn_kernels.py runs the launches): the hook (rlrep_replearn) refuses
bad records before any GPU call; the score-matching dispatch (rlrep_diffsr_score_plan) names the kernel every case expects; the per-element
error bound of tests/replearn_cases.py holds for a float32 NumPy evaluation of every case; and that bound trips on each planted defect."""
import ctypes as C

import numpy as np
import pytest

import replearn_cases as rc

RLREP_ERR_ARG = -1
PTR = 4096              # 16-byte aligned, never dereferenced: every call below is refused before a launch


def _good(kernel):
    """a record of `kernel` the hook would launch: every pointer set, small consistent extents"""
    from rlrep_amd import _lib
    a = _lib.ReplearnArgs()
    r = getattr(a, {'score_infonce': 'infonce'}.get(kernel, kernel))
    for name, typ in r._fields_:
        if typ is C.c_void_p:
            setattr(r, name, PTR)
    if kernel in ('infonce', 'score_infonce'):
        r.B, r.ncols, r.ldS, r.diag_off, r.inv_batch, r.F, r.ldZ, r.ldZM = 8, 16, 16, 8, 0.125, 64, 64, 64
        if kernel == 'infonce':
            r.ZM = None
    elif kernel == 'colsum':
        r.rows, r.F, r.ldX, r.rows2, r.ldX2 = 8, 16, 16, 8, 16
    elif kernel in ('speder_rows', 'speder_grads'):
        r.B, r.F, r.inv_batch = 8, 16, 0.125
    elif kernel == 'perturb':
        r.B, r.S, r.ld_s2 = 8, 16, 16
    elif kernel == 'score':
        r.B, r.F, r.S, r.sigma, r.inv_batch = 2, 16, 16, 1.0, 0.5
    elif kernel == 'reg_stats':
        for k in range(4):
            r.X[k] = r.C[k] = PTR
        r.B, r.H, r.lam = 4, 8, 0.5
    elif kernel == 'copy2':
        r.n = 8
    return a, r


REFUSALS = [
    # (what, kernel, fields to set)
    ('null S', 'infonce', dict(S=None)), ('null r', 'infonce', dict(r=None)), ('null drhat', 'infonce', dict(drhat=None)),
    ('null partial', 'infonce', dict(partial=None)), ('neither rhat nor Z', 'infonce', dict(rhat=None, Z=None)),
    ('Z without theta_w', 'infonce', dict(theta_w=None)), ('Z without theta_b', 'infonce', dict(theta_b=None)),
    ('ZM on the pair form', 'infonce', dict(ZM=PTR)),
    ('no rows', 'infonce', dict(B=0)), ('negative columns', 'infonce', dict(ncols=-1)), ('ldS below ncols', 'infonce', dict(ldS=15)),
    ('ldZ below F', 'infonce', dict(ldZ=63)), ('F 0 with Z', 'infonce', dict(F=0)),
    ('negative diag_off', 'infonce', dict(diag_off=-1)), ('diagonal past the last column', 'infonce', dict(diag_off=9)),
    ('fused: null ZM', 'score_infonce', dict(ZM=None)), ('fused: null Z', 'score_infonce', dict(Z=None)), ('fused: null theta_w', 'score_infonce', dict(theta_w=None)),
    ('fused: F % 64', 'score_infonce', dict(F=96, ldZ=96, ldZM=96)), ('fused: 257 columns', 'score_infonce', dict(ncols=257, ldS=260)),
    ('fused: ldZ % 4', 'score_infonce', dict(ldZ=66)), ('fused: ldZM % 4', 'score_infonce', dict(ldZM=65)),
    ('fused: Z off 16 bytes', 'score_infonce', dict(Z=PTR + 4)), ('fused: ZM off 16 bytes', 'score_infonce', dict(ZM=PTR + 8)),
    ('fused: theta_w off 16 bytes', 'score_infonce', dict(theta_w=PTR + 12)),
    ('fused: negative diag_off', 'score_infonce', dict(diag_off=-3)), ('fused: diagonal past the last column', 'score_infonce', dict(diag_off=9)),
    ('fused: ldZM below F', 'score_infonce', dict(ldZM=60)),
    ('colsum: null X', 'colsum', dict(X=None)), ('colsum: null out', 'colsum', dict(out=None)), ('colsum: no rows', 'colsum', dict(rows=0)),
    ('colsum: F 0', 'colsum', dict(F=0)), ('colsum: ldX below F', 'colsum', dict(ldX=15)), ('colsum: second set without out2', 'colsum', dict(out2=None)),
    ('colsum: rows2 0', 'colsum', dict(rows2=0)), ('colsum: ldX2 below F', 'colsum', dict(ldX2=8)),
    ('rows: null phibar', 'speder_rows', dict(phibar=None)), ('rows: null c', 'speder_rows', dict(c=None)), ('rows: B 0', 'speder_rows', dict(B=0)),
    ('rows: F -1', 'speder_rows', dict(F=-1)),
    ('grads: null Gmu', 'speder_grads', dict(Gmu=None)), ('grads: null v', 'speder_grads', dict(v=None)), ('grads: F 0', 'speder_grads', dict(F=0)),
    ('perturb: null idx', 'perturb', dict(idx=None)), ('perturb: null TGT', 'perturb', dict(TGT=None)), ('perturb: S 0', 'perturb', dict(S=0)),
    ('perturb: ld_s2 below S', 'perturb', dict(ld_s2=15)),
    ('score: null U', 'score', dict(U=None)), ('score: null GPHI', 'score', dict(GPHI=None)), ('score: B 0', 'score', dict(B=0)), ('score: F 0', 'score', dict(F=0)),
    ('score: S 0', 'score', dict(S=0)),
    ('score: row kernel over 64 KB of LDS', 'score', dict(S=3277, F=8)), ('score: row kernel over 64 KB of LDS, S % 4 == 0', 'score', dict(S=4000, F=300)),
    ('reg: B 1', 'reg_stats', dict(B=1)), ('reg: B 0', 'reg_stats', dict(B=0)), ('reg: H 0', 'reg_stats', dict(H=0)), ('reg: null partial', 'reg_stats', dict(partial=None)),
    ('copy2: null src', 'copy2', dict(src=None)), ('copy2: null d1', 'copy2', dict(d1=None)), ('copy2: n 0', 'copy2', dict(n=0)),
]


@pytest.mark.parametrize('what,kernel,kw', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_hook_refuses(what, kernel, kw, monkeypatch):
    """No GPU is needed: a refusal happens before any GPU call (this test runs where there is none)."""
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    a, r = _good(kernel)
    for k, v in kw.items():
        setattr(r, k, v)
    assert _lib.lib.rlrep_replearn(_lib.RL_KERNEL[kernel], C.byref(a), None) == RLREP_ERR_ARG, what
    msg = _lib.lib.rlrep_last_error()
    assert msg and b'replearn' in msg, (what, msg)


def test_hook_refuses_null_matrices_of_the_regulariser_and_unknown_kernels():
    from rlrep_amd import _lib
    for field in ('X', 'C'):
        for k in range(4):
            a, r = _good('reg_stats')
            getattr(r, field)[k] = None
            assert _lib.lib.rlrep_replearn(_lib.RL_KERNEL['reg_stats'], C.byref(a), None) == RLREP_ERR_ARG and b'replearn' in _lib.lib.rlrep_last_error()
    a, _ = _good('copy2')
    for kernel in (-1, 9, 1000):
        assert _lib.lib.rlrep_replearn(kernel, C.byref(a), None) == RLREP_ERR_ARG and b'replearn' in _lib.lib.rlrep_last_error()
    assert _lib.lib.rlrep_replearn(0, None, None) == RLREP_ERR_ARG and b'replearn' in _lib.lib.rlrep_last_error()
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_every_form_and_every_kernel_has_a_case():
    from rlrep_amd import _lib
    assert {c.form for c in rc.CASES if c.kernel == 'score'} == set(_lib.SCORE_FORM)
    assert {c.kernel for c in rc.CASES} == set(_lib.RL_KERNEL)


@pytest.mark.parametrize('form,S,F,env,uoff', rc.SCORE_SHAPES, ids=[f'{f}_S{S}_F{F}_{e}_{u}' for f, S, F, e, u in rc.SCORE_SHAPES])
def test_plan_names_the_form_of_every_case(form, S, F, env, uoff, monkeypatch):
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    for k, v in (rc.ENV[env] if env else {}).items():
        monkeypatch.setenv(k, v)
    assert rc.plan(S, F, 0 if uoff else 1) == form


def test_plan_of_the_fixture_shapes_and_its_refusals(monkeypatch):
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    for (S, F), form in rc.FIXTURE_FORMS:
        assert rc.plan(S, F) == form, (S, F)
    form = C.c_int32(-1)
    assert _lib.lib.rlrep_diffsr_score_plan(0, 8, 1, C.byref(form)) == RLREP_ERR_ARG
    assert _lib.lib.rlrep_diffsr_score_plan(8, -1, 1, C.byref(form)) == RLREP_ERR_ARG
    assert _lib.lib.rlrep_diffsr_score_plan(8, 8, 1, None) == RLREP_ERR_ARG


_worst = {}


@pytest.mark.parametrize('name', [c.name for c in rc.CASES])
def test_float32_numpy_stays_inside_the_error_bound(name):
    """The bound is meant to hold for ANY correct float32 evaluation: NumPy's (another summation order than any kernel's) at every case the GPU
    tests run, before the kernels are held to it.  Prints the worst ratio per kernel at the end of the kernel's cases (pytest -s)."""
    case = rc.BY_NAME[name]
    built = rc.build(case)
    for key, (rel, ratio) in rc.ratios(built, rc.emulate(case, built)).items():
        assert ratio < 1, (name, key, ratio)
        assert rel < 1e-5, (name, key, rel)
        _worst[case.kernel, key] = max(_worst.get((case.kernel, key), 0.0), ratio)
    print(f'replearn {name}: float32 emulation, worst |err|/bound so far per output of {case.kernel}: '
          + ', '.join(f'{k[1]} {v:.3f}' for k, v in sorted(_worst.items()) if k[0] == case.kernel))


@pytest.mark.parametrize('defect,name', rc.DEFECTS, ids=[f'{d} in {n}' for d, n in rc.DEFECTS])
def test_the_bound_catches_a_planted_defect(defect, name):
    """relative L2 alone need not trip (printed); some element's |error| / bound must exceed 1"""
    case = rc.BY_NAME[name]
    built = rc.build(case)
    clean = rc.ratios(built, rc.emulate(case, built))
    assert max(q for _, q in clean.values()) < 1
    bad = rc.ratios(built, rc.emulate(case, built, defect))
    worst = max(q for _, q in bad.values())
    print(f'replearn defect "{defect}" in {name}: ' + ', '.join(f'{k}: rel-L2 {r:.2e} ratio {q:.3g}' for k, (r, q) in bad.items()))
    assert worst > 1, (defect, name, bad)
