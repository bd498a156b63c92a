"""GPU unit tests of the vlsac noise-critic kernels (csrc/noisecritic.hip) through their hook (rlrep_noisecritic): every compiled form of the first
layer's forward (fp32 whole-table and K-chunked at 1 / 2 / 4 row groups and 64 / 128 columns, the two bf16x3 kernels with and without weight
images), of dX (16-byte, 4-byte, bf16x3; one and two heads) and of dW (fp32 full and lean; bf16x3 by row and by noise row, with the finishing
launch) -- one launch per case against the same operation in float64 NumPy (tests/noisecritic_cases.py), at the smallest shapes at which each
code path can still go wrong.

Per case: the form the hook launched is the one the case names; every word of the allocation outside the output windows is bit-unchanged (64
sentinel floats around every buffer, sentinel rows behind the outputs, NaN input padding); every output is finite; every output array is within
1e-5 relative L2 (the project's bar for its fp32 and bf16x3 engines); every output ELEMENT is within the first-order bound derived in
noisecritic_cases.py; a second launch on a fresh copy of the arena is bit-identical.  Besides: the weight images the hook's producer launch
left in the scratch are bit-equal to a NumPy construction of the documented layout; gW and gb of the bf16x3 dW forms are bit-equal to the sum of
their slab partials in split order; and the K-chunked forward agrees bit for bit with the whole-table one where both run.

Every case prints its worst relative L2 and its worst |error| / bound (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import noisecritic_cases as nc

pytestmark = pytest.mark.gpu

_built = {}
_worst = {}


def _build(name):
    """host image and float64 references of a case: computed once, shared by every test that runs the case, never modified"""
    if name not in _built:
        _built[name] = nc.build(nc.BY_NAME[name])
    return _built[name]


def _record(case, built, base):
    """the hook's record of the case on a device copy of its arena at `base`, and the array that receives the launched form"""
    from rlrep_amd import _lib
    p, at = built.p, lambda name, plus=0: base + 4 * (built.off[name] + plus)
    a = _lib.NoisecriticArgs()
    r = getattr(a, case.kernel)
    form = (C.c_int32 * 4)(-1, -1, -1, -1)
    r.form = C.cast(form, C.POINTER(C.c_int32))
    if case.kernel == 'fwd':
        r.ntasks, r.g2, r.cols = p['ntasks'], p['g2'], p['cols']
        for q in range(p['ntasks']):
            t = r.t[q]
            t.mean, t.lstd, t.ld_ml, t.noise, t.W, t.bias, t.Hm = at(f'hh{q}'), at(f'hh{q}', p['F']), built.ld[f'hh{q}'], at('noise'), at(f'W{q}'), at(f'bias{q}'), at(f'Hm{q}')
            t.U = at(f'U{q}') if p['U'][q] else None
            t.sigma_out = at(f'sigma{q}') if p['sig'][q] else None
            t.w3 = at(f'w3{q}') if p['w3'][q] else None
            t.B, t.F, t.H = p['B'], p['F'], p['H']
    elif case.kernel == 'dx':
        for k in range(p['nheads']):
            r.GH[k], r.U[k], r.W[k] = at(f'GH{k}'), at(f'U{k}'), at(f'W{k}')
        r.ldgh, r.noise, r.lstd, r.ld_l, r.G, r.ldg = built.ld['GH0'], at('noise'), at('hh', p['F']), built.ld['hh'], at('G'), 2 * p['F'] + 8
        r.B, r.F, r.H, r.nheads = p['B'], p['F'], p['H'], p['nheads']
    else:
        r.ntasks, r.lean, r.splits = p['ntasks'], p['lean'], p['splits_arg']
        n = p['ntasks'] * max(p['splits'], 1) * p['H']
        r.slab, r.slab_floats, r.bslab, r.bslab_floats = at('slab'), n * p['F'], at('bslab'), n
        for q in range(p['ntasks']):
            t = r.t[q]
            t.U, t.GH, t.ldgh, t.mean, t.sigma, t.ld_ml, t.noise, t.gW, t.gb = (at(f'U{q}'), at(f'GH{q}'), built.ld[f'GH{q}'], at(f'hh{q}'), at(f'sigma{q}'),
                                                                               built.ld[f'hh{q}'], at('noise'), at(f'gW{q}'), at(f'gb{q}'))
            t.B, t.F, t.H = p['B'], p['F'], p['H']
    return a, form


def _launch(case, built):
    """One launch of the case on a fresh device copy of its arena; returns (the arena after, the form the hook launched)."""
    from rlrep_amd import _lib
    dev = torch.from_numpy(built.arena.copy()).cuda()
    a, form = _record(case, built, dev.data_ptr())
    torch.cuda.synchronize()
    _lib.check(_lib.lib.rlrep_noisecritic(_lib.NC_KERNEL[case.kernel], C.byref(a), torch.cuda.current_stream().cuda_stream), 'noisecritic ' + case.name)
    torch.cuda.synchronize()
    return dev.cpu().numpy(), tuple(form)


def _verify(case, built, after):
    """Every check on the arena a launch left behind; returns (worst relative L2, worst |error| / bound)."""
    changed = (after.view(np.uint32) != built.arena.view(np.uint32)) & ~nc.windows(built)
    assert not changed.any(), f'{case.name}: {int(changed.sum())} words outside the output windows changed, first at float offset {int(np.argmax(changed))} (buffers at {built.off})'
    got = {key: after[nc.window_index(o, rows, width, ld)] for key, _, o, rows, width, ld, _, _ in built.outs}
    res = nc.ratios(built, got)
    for key, _, _, _, _, _, want, bound in built.outs:
        g = got[key].astype(np.float64)
        err = np.abs(g - want)
        rr, cc = np.unravel_index(np.argmax(np.where(np.isfinite(err), err / np.maximum(bound, 1e-300), np.inf)), err.shape)
        where = f'{case.name} {key}: worst element (row {rr}, col {cc}) got {g[rr, cc]!r} want {want[rr, cc]!r} bound {bound[rr, cc]:.3e}'
        assert np.all(np.isfinite(g)), 'non-finite output (a clamped load leaked input padding?) ' + where
        rel, ratio = res[key]
        print(f'noisecritic {case.name} {key}: rel-L2 {rel:.2e} |err|/bound {ratio:.3f}')
        assert rel < 1e-5, f'relative L2 {rel:.3e} ' + where
        assert ratio <= 1, f'|error| / bound = {ratio:.3f} ' + where
        k = (case.form, key.rstrip('0123'))
        _worst[k] = max(_worst.get(k, 0.0), ratio)
    return max(r for r, _ in res.values()), max(q for _, q in res.values())


def _set_env(monkeypatch, env):
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize('name', [c.name for c in nc.CASES])
def test_kernel_against_float64(name, monkeypatch):
    case, built = nc.BY_NAME[name], _build(name)
    _set_env(monkeypatch, case.env)
    after, form = _launch(case, built)
    if case.kernel == 'dx':
        assert nc.dx_form_name(form[:2]) == case.form, (name, form)
    else:
        want_name, want_form = nc.expected_form(case)
        assert want_name == case.form and form == want_form, (name, want_name, form, want_form)
    rel, ratio = _verify(case, built, after)
    p = built.p
    for q in range(p['ntasks'] if case.kernel == 'fwd' else 0):
        if p['w3'][q]:              # the images the producer launch left in the scratch: the layout documented at x3.h:27, bit for bit
            o = built.off[f'w3{q}']
            want = nc.w3_image(built.h[f'W{q}'])
            got = after[o:o + want.size // 2].view(np.uint16)
            assert np.array_equal(got, want), f'{name}: {int((got != want).sum())} of {want.size} bf16 words of the weight images of task {q} differ'
    if case.kernel == 'dw' and p['order'] != 'fp32':
        # gW / gb are the slab partials added in split order, bit for bit (a float32 chain; no atomics, no other order)
        H, F, S = p['H'], p['F'], p['splits']
        slab = after[built.off['slab']:built.off['slab'] + p['ntasks'] * S * H * F].reshape(p['ntasks'], S, H, F)
        bslab = after[built.off['bslab']:built.off['bslab'] + p['ntasks'] * S * H].reshape(p['ntasks'], S, H)
        for q in range(p['ntasks']):
            w, b = slab[q, 0].copy(), bslab[q, 0].copy()
            for s in range(1, S):
                w, b = w + slab[q, s], b + bslab[q, s]
            gW = after[built.off[f'gW{q}']:built.off[f'gW{q}'] + H * F].reshape(H, F)
            gb = after[built.off[f'gb{q}']:built.off[f'gb{q}'] + H]
            assert np.array_equal(gW.view(np.uint32), w.view(np.uint32)) and np.array_equal(gb.view(np.uint32), b.view(np.uint32)), f'{name}: task {q} is not the sum of its {S} slabs'
            for s, (_, nbr) in enumerate(nc.dw_split_rows(p['B'], S)):
                if nbr == 0:
                    assert not slab[q, s].any() and not bslab[q, s].any(), f'{name}: split {s} has no rows and did not zero its slab'
    again, _ = _launch(case, built)
    stable = np.ones(after.size, bool)                     # (the producer's table entry behind the weight images holds device addresses)
    for buf, o, n in built.raw:
        if buf.startswith('w3'):
            stable[o + 3 * p['H'] * p['F'] // 2:o + n] = False
    same = np.array_equal(after.view(np.uint32)[stable], again.view(np.uint32)[stable])
    twin = ''
    if p.get('twin'):
        _set_env(monkeypatch, p['twin'])
        whole, wform = _launch(case, built)
        assert wform[3] == 0 and form[3] == 1, (name, form, wform)
        diff = int((after.view(np.uint32) != whole.view(np.uint32)).sum())
        twin = f' whole-table form: {"bit-identical" if diff == 0 else f"{diff} words DIFFER"};'
        assert diff == 0, f'{name}: the K-chunked and the whole-table forward differ in {diff} words'
    print(f'noisecritic {name}: form={case.form} {form} worst rel-L2 {rel:.2e} worst |err|/bound {ratio:.3f} rerun {"bit-identical" if same else "DIFFERS"};{twin} '
          f'worst per output of {case.form} so far: ' + ', '.join(f'{k[1]} {v:.3f}' for k, v in sorted(_worst.items()) if k[0] == case.form))
    assert same, f'{name}: a second launch on a fresh copy of the arena changes {int(((after.view(np.uint32) != again.view(np.uint32)) & stable).sum())} words'
