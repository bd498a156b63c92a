"""CPU side of the loss heads' unit tests (tests/test_heads_kernels.py runs the launches): the hook (rlrep_heads) refuses bad records before any
GPU call; the host-only plan (rlrep_heads_plan, rlrep_heads_partials) accepts every case's record, names the form the case expects and sizes its
partial buffers; every kernel and epilogue form has a case; every case carries the edge inputs of its kind and stays off the discontinuities; the
per-element error bound of tests/heads_cases.py holds for a float32 NumPy emulation of every case; and that bound trips on each planted defect."""
import ctypes as C

import numpy as np
import pytest

import heads_cases as hc

RLREP_ERR_ARG = -1
BASE = 1 << 20          # 16-byte aligned, never dereferenced: no call below launches anything

_built = {}


def _build(name):
    if name not in _built:
        _built[name] = hc.build(hc.BY_NAME[name])
    return _built[name]


def _set(r, path, value):
    """r.t0.l.X = value, r.Et1 = value (element 1 of the array Et), ..."""
    *head, last = path.split('.')
    for part in head:
        r = getattr(r, part) if hasattr(r, part) else getattr(r, part[:-1])[int(part[-1])]
    if hasattr(r, last):
        setattr(r, last, value)
    else:
        getattr(r, last[:-1])[int(last[-1])] = value


PF, PFF, PFX = 'policy_fwd_5x6', 'policy_fwd_fused2_A6_B17_K64', 'policy_fwd_fused_A1_B16_K260_extra'
PB, PBF = 'policy_bwd_3x9', 'policy_bwd_fused_A16_B17_K64'
VM, HV, MS, MSF = 'vae_mid_3x20', 'heads_vae_B16_F20_K64', 'vae_mse_5x17', 'vae_mse_fused_S17_K64_B17'
R0, R1, R2 = 'reparam_dx_pre0_F16_K64_B17', 'reparam_dx_pre1_F16_K64_B37', 'reparam_dx_pre2_F16_K64_B1'
QC, QW, QA = 'qhead_critic_3x64_ld0', 'qhead_critic_5x65_ld130_w', 'qhead_actor_5x65_ld130'
REFUSALS = [
    # (what, the case whose record is spoiled, fields to set)
    ('fwd: fused 2', PF, {'fused': 2}), ('fwd: B 0', PF, {'B': 0}), ('fwd: A -1', PF, {'A': -1}), ('fwd: null O', PF, {'t0.O': None}),
    ('fwd: null act', PF, {'t0.act': None}), ('fwd: ld_act below A', PF, {'t0.ld_act': 5}), ('fwd: O off 4 bytes', PF, {'t0.O': BASE + 2}),
    ('fwd: logp off 4 bytes', PF, {'t0.logp': BASE + 1}),
    ('fwd fused: no tasks', PFF, {'ntasks': 0}), ('fwd fused: three tasks', PFF, {'ntasks': 3}), ('fwd fused: 2 A = 18', PFF, {'A': 9}),
    ('fwd fused: clamp', PFF, {'clamp': 1}), ('fwd fused: null eps of task 1', PFF, {'t1.eps': None}), ('fwd fused: null X', PFF, {'t0.l.X': None}),
    ('fwd fused: null W of task 1', PFF, {'t1.l.W': None}), ('fwd fused: null bias', PFF, {'t0.l.bias': None}), ('fwd fused: K 0', PFF, {'t0.l.K': 0}),
    ('fwd fused: ldx below K', PFF, {'t1.l.ldx': 63}), ('fwd fused: ldw below K', PFF, {'t0.l.ldw': 60}), ('fwd fused: ld_act below A', PFF, {'t1.ld_act': 5}),
    ('fwd fused: X off 4 bytes', PFF, {'t0.l.X': BASE + 3}),
    ('fwd extra: rows 0', PFX, {'extra.rows': 0}), ('fwd extra: N 0', PFX, {'extra.N': 0}), ('fwd extra: null Y', PFX, {'extra.Y': None}),
    ('fwd extra: ldy below N', PFX, {'extra.ldy': 16}), ('fwd extra: sin', PFX, {'extra.act': 3}), ('fwd extra: activation 5', PFX, {'extra.act': 5}),
    ('fwd extra: null W', PFX, {'extra.l.W': None}), ('fwd extra: ldx below K', PFX, {'extra.l.ldx': 63}),
    ('bwd: fused -1', PB, {'fused': -1}), ('bwd: null O', PB, {'O': None}), ('bwd: null eps', PB, {'eps': None}), ('bwd: null act', PB, {'act': None}),
    ('bwd: null alpha_state', PB, {'alpha_state': None}), ('bwd: null G', PB, {'G': None}), ('bwd: null dA', PB, {'dA': None}), ('bwd: ld_dA below A', PB, {'ld_dA': 8}),
    ('bwd: ld_act below A', PB, {'ld_act': 8}), ('bwd: alpha_state off 8 bytes', PB, {'alpha_state': BASE + 4}), ('bwd: B 0', PB, {'B': 0}), ('bwd: A 0', PB, {'A': 0}),
    ('bwd fused: A 17', PBF, {'A': 17}), ('bwd fused: null X', PBF, {'l.X': None}), ('bwd fused: null W', PBF, {'l.W': None}), ('bwd fused: ldw below A', PBF, {'l.ldw': 15}),
    ('bwd fused: K -1', PBF, {'l.K': -1}), ('bwd fused: ldx below K', PBF, {'l.ldx': 60}),
    ('vae_mid: null EH', VM, {'EH': None}), ('vae_mid: null eps', VM, {'eps': None}), ('vae_mid: null partial', VM, {'partial': None}), ('vae_mid: B 0', VM, {'B': 0}),
    ('vae_mid: F 0', VM, {'F': 0}), ('vae_mid: GFH off 4 bytes', VM, {'GFH': BASE + 2}),
    ('heads_vae: null Ae', HV, {'Ae': None}), ('heads_vae: null bf', HV, {'bf': None}), ('heads_vae: null eps', HV, {'eps': None}), ('heads_vae: null Z', HV, {'Z': None}),
    ('heads_vae: K 0', HV, {'K': 0}), ('heads_vae: F -2', HV, {'F': -2}), ('heads_vae: lda below K', HV, {'lda': 63}), ('heads_vae: EH off 4 bytes', HV, {'EH': BASE + 1}),
    ('mse: fused 3', MS, {'fused': 3}), ('mse: null DH', MS, {'DH': None}), ('mse: null s2', MS, {'s2': None}), ('mse: null r', MS, {'r': None}), ('mse: null GDH', MS, {'GDH': None}),
    ('mse: null partial', MS, {'partial': None}), ('mse: ld_s2 below S', MS, {'ld_s2': 16}), ('mse: S 0', MS, {'S': 0}), ('mse: B -3', MS, {'B': -3}),
    ('mse: fused without a layer', MS, {'fused': 1}),
    ('mse fused: null W', MSF, {'l.W': None}), ('mse fused: null bias', MSF, {'l.bias': None}), ('mse fused: ldw below K', MSF, {'l.ldw': 63}), ('mse fused: K 0', MSF, {'l.K': 0}),
    ('reparam: pre 3', R0, {'pre': 3}), ('reparam: null A', R0, {'A': None}), ('reparam: null W', R0, {'W': None}), ('reparam: null G', R0, {'G': None}), ('reparam: null EZ', R0, {'EZ': None}),
    ('reparam: lda below K', R0, {'lda': 60}), ('reparam: ldw below F', R0, {'ldw': 15}), ('reparam: ldg below 2 F', R0, {'ldg': 31}), ('reparam: ldez below F', R0, {'ldez': 12}),
    ('reparam: F 0', R0, {'F': 0}), ('reparam: K 0', R0, {'K': 0}), ('reparam: B 0', R0, {'B': 0}),
    ('reparam pre: null X', R1, {'X': None}), ('reparam pre: null Wh', R1, {'Wh': None}), ('reparam pre: null M', R1, {'M': None}), ('reparam pre: K1 33', R1, {'K1': 33, 'ldx': 40}),
    ('reparam pre: K1 0', R1, {'K1': 0}), ('reparam pre: ldx below K1', R1, {'ldx': 4}), ('reparam pre: ldwh below K', R1, {'ldwh': 60}), ('reparam pre: ldm below K', R1, {'ldm': 63}),
    ('reparam mse: null bh', R2, {'bh': None}), ('reparam mse: null s2', R2, {'s2': None}), ('reparam mse: null r', R2, {'r': None}), ('reparam mse: null partial', R2, {'partial': None}),
    ('reparam mse: K % 4', R2, {'K': 62}), ('reparam mse: ldm % 4', R2, {'ldm': 70}), ('reparam mse: ldwh % 4', R2, {'ldwh': 66}), ('reparam mse: M off 16 bytes', R2, {'M': BASE + 4}),
    ('reparam mse: Wh off 16 bytes', R2, {'Wh': BASE + 8}), ('reparam mse: K1 1', R2, {'K1': 1}), ('reparam mse: ld_s2 below S', R2, {'ld_s2': 3}),
    ('critic: null Et of head 1', QC, {'Et1': None}), ('critic: null wc', QC, {'wc0': None}), ('critic: null bt', QC, {'bt1': None}), ('critic: null GE while training', QC, {'GE0': None}),
    ('critic: null dq while training', QC, {'dq': None}), ('critic: null logp', QC, {'logp': None}), ('critic: null R', QC, {'R': None}), ('critic: null D', QC, {'D': None}),
    ('critic: null partial', QC, {'partial': None}), ('critic: null alpha_state', QC, {'alpha_state': None}), ('critic: alpha_state off 8 bytes', QC, {'alpha_state': BASE + 12}),
    ('critic: ldE below H', QC, {'ldE': 63}), ('critic: B 0', QC, {'B': 0}), ('critic: H 0', QC, {'H': 0}), ('critic: weighted without w', QC, {'weighted': 1}),
    ('critic: weighted, null td', QW, {'td': None}), ('critic: weighted, null w', QW, {'w': None}), ('critic: weighted, ldE below H', QW, {'ldE': 64}),
    ('actor: null Ec', QA, {'Ec0': None}), ('actor: null bc', QA, {'bc1': None}), ('actor: null GE', QA, {'GE1': None}), ('actor: null logp', QA, {'logp': None}),
    ('actor: null partial_loss', QA, {'partial_loss': None}), ('actor: null partial_c', QA, {'partial_c': None}), ('actor: ldE below H', QA, {'ldE': 64}),
    ('actor: null alpha_state', QA, {'alpha_state': None}), ('actor: alpha_state off 8 bytes', QA, {'alpha_state': BASE + 4}), ('actor: B 0', QA, {'B': 0}),
]


@pytest.mark.parametrize('what,name,kw', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_hook_refuses(what, name, kw, monkeypatch):
    """No GPU is needed: a refusal happens before any GPU call (this test runs where there is none).  The unspoiled record is accepted."""
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    case = hc.BY_NAME[name]
    a, r = hc.record(case, _build(name), BASE)
    assert _lib.lib.rlrep_heads_plan(_lib.HD_KIND[case.kind], C.byref(a)) == 0, _lib.lib.rlrep_last_error()
    for k, v in kw.items():
        _set(r, k, v)
    assert _lib.lib.rlrep_heads(_lib.HD_KIND[case.kind], C.byref(a), None) == RLREP_ERR_ARG, what
    msg = _lib.lib.rlrep_last_error()
    assert msg and msg.startswith(b'heads:'), (what, msg)
    assert _lib.lib.rlrep_heads_plan(_lib.HD_KIND[case.kind], C.byref(a)) == RLREP_ERR_ARG, what


def test_hook_refuses_unknown_kinds_and_a_null_record_and_the_abi_is_unchanged():
    from rlrep_amd import _lib
    a, _ = hc.record(hc.BY_NAME[VM], _build(VM), BASE)
    for kind in (-1, 8, 1000):
        assert _lib.lib.rlrep_heads(kind, C.byref(a), None) == RLREP_ERR_ARG and _lib.lib.rlrep_last_error().startswith(b'heads:')
        assert _lib.lib.rlrep_heads_partials(kind, 0, 8, 8) == 0
    assert _lib.lib.rlrep_heads(0, None, None) == RLREP_ERR_ARG and _lib.lib.rlrep_last_error().startswith(b'heads:')
    assert _lib.lib.rlrep_heads_partials(_lib.HD_KIND['vae_mid'], 0, 0, 8) == 0 and _lib.lib.rlrep_heads_partials(_lib.HD_KIND['vae_mse'], 1, 8, 0) == 0
    assert _lib.lib.rlrep_abi_version() == 4                                # additive


def test_every_kernel_and_every_form_has_a_case():
    from rlrep_amd import _lib
    assert {c.form for c in hc.CASES} == set(hc.FORMS), set(hc.FORMS) ^ {c.form for c in hc.CASES}
    assert {c.kind for c in hc.CASES} == set(_lib.HD_KIND)
    assert set(hc.NEVER_PLANNED) < set(hc.FORMS)
    assert all(c.form.split('/')[0] == c.kind for c in hc.CASES)
    # both heads_vae loader copies by every trigger of the 4-byte one; both policy-backward instantiations; every reparameterisation launch form
    load4 = [c.p for c in hc.CASES if c.form == 'heads_vae/load4']
    assert any(p['K'] % 4 for p in load4) and any(p['lda'] % 4 and not p['K'] % 4 for p in load4) and any(p.get('a_off') and not p['K'] % 4 and not p['lda'] % 4 for p in load4)
    assert {c.p['A'] for c in hc.CASES if c.form == 'policy_bwd/gemm16:fast'} == {1, 6, 8, 9, 16} == {c.p['A'] for c in hc.CASES if c.form == 'policy_bwd/gemm16:record'}
    assert any(c.p.get('ntasks') == 2 and c.p.get('extra') for c in hc.CASES) and any(c.p.get('ntasks') == 2 and not c.p.get('extra') for c in hc.CASES)
    assert any(c.kind == 'qhead_critic' and not c.p['train'] for c in hc.CASES)
    assert any(c.kind == 'policy_fwd' and c.p.get('eps') is False for c in hc.CASES) and any(c.kind == 'policy_fwd' and c.p.get('logp') is False for c in hc.CASES)


def expected_fused(case):
    return 'gemm16' in case.form or case.kind == 'reparam_dx'


@pytest.mark.parametrize('name', [c.name for c in hc.CASES])
def test_plan_accepts_the_case_and_names_its_form(name, monkeypatch):
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    case, built = hc.BY_NAME[name], _build(name)
    form = (C.c_int32 * 2)(-7, -7)
    a, r = hc.record(case, built, BASE, form)
    assert _lib.lib.rlrep_heads_plan(_lib.HD_KIND[case.kind], C.byref(a)) == 0, _lib.lib.rlrep_last_error()
    assert tuple(form) == hc.expected_form(case), (name, tuple(form))
    # the partial buffers of the case have the size the hook's own count gives
    p = built.p
    n = {'vae_mid': p.get('F'), 'heads_vae': p.get('F'), 'vae_mse': p.get('S')}.get(case.kind, 0)
    count = _lib.lib.rlrep_heads_partials(_lib.HD_KIND[case.kind], 1 if expected_fused(case) else 0, p['B'], n or 0)
    sizes = {key: rows * width for key, _, _, rows, width, _, _, _ in built.outs if key.startswith('partial')}
    if case.kind in ('policy_fwd', 'policy_bwd') or (case.kind == 'reparam_dx' and p['pre'] < 2):
        assert count == 0 or not sizes
    else:
        assert sizes and all(v == count for v in sizes.values()), (name, sizes, count)


@pytest.mark.parametrize('name', [c.name for c in hc.CASES])
def test_every_case_carries_the_edge_inputs(name):
    """On the float64 reference alone: the edge inputs of the case's kind (heads_cases.edge_report; a case too small for all of them carries the
    first ones), every computed log_std of heads_vae off the clamp edges by more than its bound or exactly on one, every qhead_actor row an
    exact tie or clear of the two bounds (both asserted inside edge_report).  Nothing is excluded from a comparison."""
    got, need = hc.edge_report(hc.BY_NAME[name], _build(name))
    assert need <= got, (name, sorted(need - got))


def test_each_kind_has_cases_that_carry_every_edge():
    full = {}
    for c in hc.CASES:
        got, _ = hc.edge_report(c, _build(c.name))
        full.setdefault(c.form, set()).update(got)
    for form, got in full.items():
        kind = form.split('/')[0]
        if kind == 'policy_fwd':
            assert {'rho>=10 x>=12', 'rho<=-10 x<=-12', 'x==0', 'x==-25', 'x<=-60', 'eps==5', 'eps==0', '-10<x<-9.5', '-10.5<x<-10'} <= got, (form, got)
        elif kind == 'policy_bwd':
            assert len(got) == 5, (form, got)
        elif kind in ('vae_mid', 'heads_vae'):
            assert len(got) == 5, (form, got)
        elif kind == 'qhead_critic':
            assert {'D==0', 'D==1', 'tq1<tq2', 'tq2<tq1', 'Ec>0', 'Ec==0', 'Ec<0'} <= got and ('weighted' not in form or {'w==0', 'w==1'} <= got), (form, got)
        elif kind == 'qhead_actor':
            assert {'tie', 'q1<q2', 'q2<q1', 'Ec>0', 'Ec==0', 'Ec<0'} <= got, (form, got)
    assert any(c.kind == 'policy_fwd' and c.p.get('clamp') for c in hc.CASES)


_worst = {}


@pytest.mark.parametrize('name', [c.name for c in hc.CASES])
def test_float32_numpy_stays_inside_the_error_bound(name):
    """The bound is meant to hold for ANY correct float32 evaluation: NumPy's (another summation order than any kernel's; the fused forms as the
    product followed by the epilogue) at every case the GPU tests run, before the kernels are held to it.  Prints the worst ratio per output (pytest -s)."""
    case, built = hc.BY_NAME[name], _build(name)
    for key, (rel, ratio) in hc.ratios(built, hc.emulate(case, built)).items():
        assert ratio < 1, (name, key, ratio)
        assert rel < 1e-5, (name, key, rel)
        k = (case.form, key.rstrip('01'))
        _worst[k] = max(_worst.get(k, 0.0), ratio)
    print(f'heads {name}: float32 emulation, worst |err|/bound so far per output of {case.form}: '
          + ', '.join(f'{k[1]} {v:.3f}' for k, v in sorted(_worst.items()) if k[0] == case.form))


@pytest.mark.parametrize('defect,name,key', hc.DEFECTS, ids=[f'{d} in {n}' for d, n, _ in hc.DEFECTS])
def test_the_bound_catches_a_planted_defect(defect, name, key):
    """relative L2 alone need not trip (printed); the named output's worst |error| / bound must exceed 1"""
    case, built = hc.BY_NAME[name], _build(name)
    clean = hc.ratios(built, hc.emulate(case, built))
    assert max(q for _, q in clean.values()) < 1
    with np.errstate(all='ignore'):
        bad = hc.ratios(built, hc.emulate(case, built, defect))
    print(f'heads defect "{defect}" in {name}: ' + ', '.join(f'{k}: rel-L2 {r:.2e} ratio {q:.3g}' for k, (r, q) in bad.items()))
    assert bad[key][1] > 1, (defect, name, bad)
    if defect == 'the softplus threshold branch removed':
        assert not np.all(np.isfinite(hc.emulate(case, built, defect)['logp'])) and np.all(np.isfinite(hc.emulate(case, built)['logp']))


def test_every_defect_of_the_list_is_planted():
    assert {d for d, _, _ in hc.DEFECTS} >= {
        'rho read one column off', 'the last action left out of logp', 'the sign of the tanh correction', 'the softplus threshold branch removed',
        'the clamp mask missing on a log_std gradient', 'KL scale applied twice', '(1 - D) dropped', 'min(tq1, tq2) replaced by tq1',
        'the tie split given whole to head 1', 'w applied twice', 'td without its 0.5', 'rows of the second grid sweep skipped', 'ldE ignored',
        "the fused MSE's reward column compared against a state column", 'the last ragged K chunk of heads_vae dropped',
        'the second half of a reparameterisation store written without EZ'}
