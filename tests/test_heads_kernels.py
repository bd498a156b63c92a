"""GPU unit tests of the loss heads every agent shares, through their hook (rlrep_heads): the policy forward and backward, vae_mid, heads_vae (both
loader copies), vae_mse, the critic head plain and weighted, the actor head -- and the gemm16 epilogues that replace four of them (policy forward
with one or two policy tasks and an extra plain task, policy backward on the fast front end and on the record one, decoder heads + mse, the
reparameterisation dX plain, with the fused short product and with the mse phase) -- one launch per case against the same operation in float64
NumPy (tests/heads_cases.py), at the smallest shapes at which each form can still go wrong.

Per case: the hook reports the form the case names, and a fused launch took the gemm16 front end it names (rlrep_front_end_counts around the
call); every word of the allocation outside the output windows is bit-unchanged (64 sentinel floats around every buffer, ld > width, a sentinel
row after the last, NaN input padding; train = 0: GE and dq stay sentinel); every output is finite; every output array is within 1e-5 relative L2;
every output ELEMENT is within the first-order bound derived in heads_cases.py, the per-block partial sums included; and a second launch on a
fresh copy of the arena gives bit-identical outputs.

Across forms: every fused case agrees with the pair of launches it replaces within the sum of the two bounds; heads_vae's 16-byte and 4-byte loader
copies are bit-identical on the same values; the weighted critic head with w = 1 is bit-identical to the plain one (per.hip's claim).

Every case prints its worst relative L2 and its worst |error| / bound (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import heads_cases as hc

pytestmark = pytest.mark.gpu

_built = {}
_worst = {}


def _build(name):
    """host image and float64 references of a case: computed once, shared by every test that runs the case, never modified"""
    if name not in _built:
        _built[name] = hc.build(hc.BY_NAME[name])
    return _built[name]


def _device(built, shift=0):
    """a fresh device copy of the arena, `shift` floats off the allocation's start; (tensor, address of the arena's word 0)"""
    dev = torch.empty(built.arena.size + shift, dtype=torch.float32, device='cuda')
    dev[shift:].copy_(torch.from_numpy(built.arena.copy()))
    return dev, dev.data_ptr() + 4 * shift


def _call(case, a, front=None, form=None):
    from rlrep_amd import _lib
    torch.cuda.synchronize()
    f0 = _lib.front_end_counts()
    try:
        _lib.check(_lib.lib.rlrep_heads(_lib.HD_KIND[case.kind], C.byref(a), torch.cuda.current_stream().cuda_stream), 'heads ' + case.name)
        torch.cuda.synchronize()
    except RuntimeError as e:
        # a refused record is a failed test; an error of the GPU ends the session: nothing more is launched on a device that has faulted
        if str(e).find('heads:') >= 0 and str(e).find('launch failed') < 0:
            raise
        pytest.exit(f'GPU error in {case.name}: {e}', returncode=3)
    f1 = _lib.front_end_counts()
    took = [f1[k] - f0[k] for k in ('fast', 'fast4', 'fastpre', 'record')]                     # (in the order of heads_cases.FRONT)
    if front is not None:
        assert took == [1 if q == front else 0 for q in range(4)], f'{case.name}: gemm16 front ends taken {took}, the case names {case.form}'
    else:
        assert took == [0, 0, 0, 0], (case.name, took)
    if form is not None:
        assert tuple(form) == hc.expected_form(case), (case.name, tuple(form))


def _launch(case, built, shift=0, expect=True):
    """One launch of the case on a fresh device copy of its arena; returns the arena after."""
    dev, base = _device(built, shift)
    form = (C.c_int32 * 2)(-7, -7)
    a, r = hc.record(case, built, base, form)
    _call(case, a, case.front if expect else None, form if expect else None)
    return dev[shift:].cpu().numpy()


def _verify(case, built, after, outs=None, guards=True):
    """Every check on the arena a launch left behind; returns (worst relative L2, worst |error| / bound)."""
    outs = outs or built.outs
    if guards:
        changed = (after.view(np.uint32) != built.arena.view(np.uint32)) & ~hc.windows(built, outs)
        assert not changed.any(), f'{case.name}: {int(changed.sum())} words outside the output windows changed, first at float offset {int(np.argmax(changed))} (buffers at {built.off})'
    got = {key: after[hc.window_index(o, rows, width, ld)] for key, _, o, rows, width, ld, _, _ in outs}
    res = hc.ratios(built, got, outs)
    for key, _, _, _, _, _, want, bound in outs:
        g = got[key].astype(np.float64)
        err = np.abs(g - want)
        rr, cc = np.unravel_index(np.argmax(np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf)), err.shape)
        where = f'{case.name} {key}: worst element (row {rr}, col {cc}) got {g[rr, cc]!r} want {want[rr, cc]!r} bound {bound[rr, cc]:.3e}'
        rel, ratio = res[key]
        print(f'heads {case.name} {key}: rel-L2 {rel:.2e} |err|/bound {ratio:.3f}')
        assert np.all(np.isfinite(g)), 'non-finite output (a clamped load leaked input padding?) ' + where
        assert rel < 1e-5, f'relative L2 {rel:.3e} ' + where
        assert ratio <= 1, f'|error| / bound = {ratio:.3f} ' + where
        k = (case.form if guards else case.form + ' as the pair', key.rstrip('01'))
        _worst[k] = max(_worst.get(k, 0.0), ratio)
    return max(r for r, _ in res.values()), max(q for _, q in res.values())


def _clean_env(monkeypatch):
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)


@pytest.mark.parametrize('name', [c.name for c in hc.CASES])
def test_kernel_against_float64(name, monkeypatch):
    case, built = hc.BY_NAME[name], _build(name)
    _clean_env(monkeypatch)
    after = _launch(case, built)
    rel, ratio = _verify(case, built, after)
    again = _launch(case, built)
    same = np.array_equal(after.view(np.uint32), again.view(np.uint32))
    print(f'heads {name}: form={case.form} worst rel-L2 {rel:.2e} worst |err|/bound {ratio:.3f} rerun {"bit-identical" if same else "DIFFERS"}; '
          f'worst per output of {case.form} so far: ' + ', '.join(f'{k[1]} {v:.3f}' for k, v in sorted(_worst.items()) if k[0] == case.form))
    assert same, f'{name}: a second launch on a fresh copy of the arena changes {int((after.view(np.uint32) != again.view(np.uint32)).sum())} words'


def _gemm16(la, lb, tasks):
    from rlrep_amd import _lib
    arr = (_lib.Gemm16Task * len(tasks))()
    for s, d in zip(arr, tasks):
        s.scale = 1.0
        for k, v in d.items():
            setattr(s, k, v)
    _lib.check(_lib.lib.rlrep_gemm16_table(la, lb, 1, arr, len(tasks), 0, 1, 0, torch.cuda.current_stream().cuda_stream), 'gemm16_table')


PAIRED = [c.name for c in hc.CASES if 'gemm16' in c.form and c.p.get('ntasks', 1) == 1 and not c.p.get('extra')] + \
         [c.name for c in hc.CASES if c.kind == 'heads_vae' and c.p['heads_out']]


@pytest.mark.parametrize('name', PAIRED)
def test_fused_agrees_with_the_pair(name, monkeypatch):
    """The launches a fused form replaces -- the layer's product through rlrep_gemm16_table, then the stand-alone kernel on what it left: gemm16
    forward + policy_fwd_kernel; gemm16 dX + policy_bwd_kernel; two gemm16 forwards + vae_mid_kernel against heads_vae_kernel; gemm16 forward +
    vae_mse_kernel -- are held to the bound of their own evaluation, and the fused launch agrees with them within the sum of the two bounds,
    element by element (the partial sums have another ownership in the two forms and are held to their own reference only)."""
    from rlrep_amd import _lib
    case, built = hc.BY_NAME[name], _build(name)
    _clean_env(monkeypatch)
    p, off = built.p, built.off
    dev, base = _device(built)
    at = lambda n: base + 4 * off[n]
    a, r = hc.record(case, built, base)
    kernel = hc.Case(name + ' (pair)', case.kind, case.kind + '/kernel')
    if case.kind == 'policy_fwd':
        _gemm16(0, 0, [dict(a=at('X'), b=at('W'), c=at('O'), lda=p['K'] + 4, ldb=p['K'] + 4, ldc=2 * p['A'], rows=p['B'], cols=2 * p['A'], inner=p['K'], bias=at('bias'))])
        r.fused, r.t[0].act, r.t[0].logp = 0, at('act_pair'), at('logp_pair')
    elif case.kind == 'policy_bwd':
        _gemm16(0, 1, [dict(a=at('Gm'), b=at('Wd'), c=at('dA'), lda=p['K'] + 4, ldb=p['A'] + 3, ldc=p['A'], rows=p['B'], cols=p['A'], inner=p['K'], epi=1)])
        r.fused, r.G = 0, at('G_pair')
    elif case.kind == 'heads_vae':
        B, F, K = p['B'], p['F'], p['K']
        _gemm16(0, 0, [dict(a=at('A' + n), b=at('W' + n), c=at(n.upper() + 'H'), lda=p['lda'], ldb=K, ldc=2 * F, rows=B, cols=2 * F, inner=K, bias=at('b' + n)) for n in ('e', 'f')])
        kernel = hc.Case(name + ' (pair)', 'vae_mid', 'vae_mid/kernel')
        a = _lib.HeadsArgs()
        r = a.vae_mid
        r.EH, r.FH, r.eps, r.B, r.F, r.scale = at('EH'), at('FH'), at('eps'), B, F, p['scale']
        for n in ('Z', 'EZ', 'GEH', 'GFH', 'partial'):
            setattr(r, n, at(n + '_pair'))
    else:
        _gemm16(0, 0, [dict(a=at('X'), b=at('W'), c=at('DH'), lda=p['K'] + 4, ldb=p['K'] + 4, ldc=p['S'] + 1, rows=p['B'], cols=p['S'] + 1, inner=p['K'], bias=at('bias'))])
        r.fused, r.DH, r.GDH, r.partial = 0, at('DH'), at('GDH_pair'), at('partial_pair')
    _call(kernel, a)
    pair = dev.cpu().numpy()
    outs = hc.pair_outs(case, built)
    rel, ratio = _verify(case, built, pair, outs, guards=False)
    fused = _launch(case, built)
    own = {o[0]: o for o in built.outs}
    worst = 0.0
    for key, _, o, rows, width, ld, _, bound in outs:
        if key == 'partial':
            continue
        _, _, fo, _, _, fld, _, fbound = own[key]
        q = np.abs(pair[hc.window_index(o, rows, width, ld)].astype(np.float64) - fused[hc.window_index(fo, rows, width, fld)].astype(np.float64)) / np.maximum(bound + fbound, 1e-300)
        worst = max(worst, float(q.max()))
    print(f'heads {name} as the pair it replaces: worst rel-L2 {rel:.2e} worst |err|/bound {ratio:.3f}; |pair - fused| / (sum of the bounds) {worst:.3f}')
    assert worst <= 1


@pytest.mark.parametrize('name', [c.name for c in hc.CASES if c.form == 'heads_vae/load16' and c.p['K'] in (4, 64, 260, 1028)])
def test_heads_vae_loader_copies_are_bit_identical(name, monkeypatch):
    """the same values one float off the allocation's 16-byte boundary: every operand pointer misaligned, the 4-byte loader copy, the same bits"""
    case, built = hc.BY_NAME[name], _build(name)
    _clean_env(monkeypatch)
    wide = _launch(case, built)
    dev, base = _device(built, 1)
    form = (C.c_int32 * 2)(-7, -7)
    a, _ = hc.record(case, built, base, form)
    _call(case, a)
    assert tuple(form) == (0, 0), (name, tuple(form))
    narrow = dev[1:].cpu().numpy()
    diff = wide.view(np.uint32) != narrow.view(np.uint32)
    assert not diff.any(), f'{name}: {int(diff.sum())} words differ between the loader copies, first at float offset {int(np.argmax(diff))}'


@pytest.mark.parametrize('name', [c.name for c in hc.CASES if c.form == 'qhead_critic/kernel'])
def test_weighted_critic_head_with_unit_weights_is_the_plain_one(name, monkeypatch):
    """per.hip: with d_h = q_h - y, g_h = (2 d_h inv_batch) w in this order, so that w = 1 is the identity: GE, dq and the partials bit for bit"""
    case, built = hc.BY_NAME[name], _build(name)
    _clean_env(monkeypatch)
    plain = _launch(case, built)
    dev, base = _device(built)
    a, r = hc.record(case, built, base)
    ones, td = torch.ones(built.p['B'], dtype=torch.float32, device='cuda'), torch.zeros(built.p['B'], dtype=torch.float32, device='cuda')
    r.weighted, r.w, r.td = 1, ones.data_ptr(), td.data_ptr()
    _call(hc.Case(name + ' (w = 1)', 'qhead_critic', 'qhead_critic/weighted'), a)
    weighted = dev.cpu().numpy()
    diff = plain.view(np.uint32) != weighted.view(np.uint32)
    assert not diff.any(), f'{name}: {int(diff.sum())} words differ with w = 1, first at float offset {int(np.argmax(diff))} (buffers at {built.off})'
    assert torch.isfinite(td).all()


@pytest.fixture(scope='module', autouse=True)
def _print_the_worst_ratios():
    """after the module's last test: the worst |error| / bound per form and output over the cases that ran (pytest -s; docs/history/head_kernels.md)"""
    yield
    for (form, key), v in sorted(_worst.items()):
        print(f'heads worst |err|/bound: {form:34s} {key:14s} {v:.3f}')
