"""GPU unit tests of the representation-loss kernels (csrc/replearn.hip) through their hook (rlrep_replearn): ctrlsac's InfoNCE on given scores and
with the score matrix in the same launch, the weighted column sum (one and two sets), spedersac's spectral rows and gradients, diffsrsac's
perturbation, every launch form of its score matching (LDS chunks of 32 / 64 / 128, a thread per row with 1 / 2 / 4 rows, the 16-byte two-pass
kernel, the lanes-over-columns kernel), the regulariser statistics and copy2 -- one launch per case against the same operation in float64 NumPy
(tests/replearn_cases.py), at the smallest shapes at which each code path can still go wrong.

Per case: the score-matching form is the one the case names (rlrep_diffsr_score_plan under the case's switches, asked with the alignment of the
pointer actually passed); every word of the allocation outside the output windows is bit-unchanged (64 sentinel floats around every buffer,
ld > width, a sentinel row after the last, NaN input padding); every output is finite; every output array is within 1e-5 relative L2 (the bar
test_gemm_engines.py and test_gemm16_engine.py hold fp32 engines to); every output ELEMENT is within the first-order bound derived in
replearn_cases.py -- the per-block partial sums included, each against the reference's sum over exactly the rows that block owns; and a second
launch on a fresh copy of the arena gives bit-identical outputs (the kernels' file header promises determinism).

Every case prints its worst relative L2 and its worst |error| / bound (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import replearn_cases as rc

pytestmark = pytest.mark.gpu

_built = {}
_worst = {}


def _build(name):
    """host image and float64 references of a case: computed once, shared by every test that runs the case, never modified"""
    if name not in _built:
        _built[name] = rc.build(rc.BY_NAME[name])
    return _built[name]


def _record(case, built, base, **over):
    """the hook's record of the case on a device copy of its arena at `base`"""
    from rlrep_amd import _lib
    a = _lib.ReplearnArgs()
    r = getattr(a, {'score_infonce': 'infonce'}.get(case.kernel, case.kernel))
    fields = {n for n, _ in r._fields_}
    for name, off in built.off.items():
        if name in fields:
            setattr(r, name, base + 4 * off)
    if case.kernel == 'reg_stats':
        for k in range(4):
            r.X[k], r.C[k] = base + 4 * built.off[f'X{k}'], base + 4 * built.off[f'C{k}']
    for name, v in built.scalars.items():
        setattr(r, name, v)
    for name, v in over.items():
        setattr(r, name, v)
    return a, r


def _launch(case, built, pair=False):
    """One launch of the case on a fresh device copy of its arena; returns the arena after.  pair: a fused case as GEMM + InfoNCE."""
    from rlrep_amd import _lib
    dev = torch.from_numpy(built.arena.copy()).cuda()
    base = dev.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    if pair:
        a, r = _record(case, built, base, ZM=None, ldZM=0, partial=base + 4 * built.off['partial_pair'])
        s = built.scalars
        _lib.check(_lib.lib.rlrep_gemm(0, 0, 0, base + 4 * built.off['Z'], s['ldZ'], base + 4 * built.off['ZM'], s['ldZM'], base + 4 * built.off['S'], s['ldS'],
                                       s['B'], s['ncols'], s['F'], 0, 0, 0, None, None, 0, None, 0, 0, None, 0, st), 'gemm')
        kernel = 'infonce'
    else:
        a, r = _record(case, built, base)
        kernel = case.kernel
    if case.kernel == 'score':
        aligned = (r.U & 15) == 0
        assert aligned == (built.p['u_off'] == 0)
        assert rc.plan(built.p['S'], built.p['F'], int(aligned)) == case.form, (case.name, 'launch form')
    _lib.check(_lib.lib.rlrep_replearn(_lib.RL_KERNEL[kernel], C.byref(a), st), 'replearn ' + case.name)
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def _verify(case, built, after, outs=None):
    """Every check on the arena a launch left behind; returns (worst relative L2, worst |error| / bound)."""
    outs = outs or built.outs
    changed = (after.view(np.uint32) != built.arena.view(np.uint32)) & ~rc.windows(built, outs)
    assert not changed.any(), f'{case.name}: {int(changed.sum())} words outside the output windows changed, first at float offset {int(np.argmax(changed))} (buffers at {built.off})'
    got = {key: after[rc.window_index(o, rows, width, ld)] for key, _, o, rows, width, ld, _, _ in outs}
    res = rc.ratios(built, got, outs)
    for key, _, _, _, _, _, want, bound in outs:
        g = got[key].astype(np.float64)
        err = np.abs(g - want)
        rr, cc = np.unravel_index(np.argmax(np.where(np.isfinite(err), err, np.inf)), err.shape)
        where = f'{case.name} {key}: worst element (row {rr}, col {cc}) got {g[rr, cc]!r} want {want[rr, cc]!r} bound {bound[rr, cc]:.3e}'
        assert np.all(np.isfinite(g)), 'non-finite output (a clamped load leaked input padding?) ' + where
        rel, ratio = res[key]
        print(f'replearn {case.name} {key}: rel-L2 {rel:.2e} |err|/bound {ratio:.3f}')
        assert rel < 1e-5, f'relative L2 {rel:.3e} ' + where
        assert ratio <= 1, f'|error| / bound = {ratio:.3f} ' + where
        _worst[case.kernel, key] = max(_worst.get((case.kernel, key), 0.0), ratio)
    return max(r for r, _ in res.values()), max(q for _, q in res.values())


@pytest.mark.parametrize('name', [c.name for c in rc.CASES])
def test_kernel_against_float64(name, monkeypatch):
    case, built = rc.BY_NAME[name], _build(name)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    after = _launch(case, built)
    rel, ratio = _verify(case, built, after)
    again = _launch(case, built)
    same = np.array_equal(after.view(np.uint32), again.view(np.uint32))
    print(f'replearn {name}: kernel={case.kernel}{" form=" + case.form if case.form else ""} worst rel-L2 {rel:.2e} worst |err|/bound {ratio:.3f} '
          f'rerun {"bit-identical" if same else "DIFFERS"}; worst per output of {case.kernel} so far: '
          + ', '.join(f'{k[1]} {v:.3f}' for k, v in sorted(_worst.items()) if k[0] == case.kernel))
    assert same, f'{name}: a second launch on a fresh copy of the arena changes {int((after.view(np.uint32) != again.view(np.uint32)).sum())} words'


@pytest.mark.parametrize('name', [c.name for c in rc.CASES if c.kernel == 'score_infonce'])
def test_fused_agrees_with_the_pair(name, monkeypatch):
    """the product through the GEMM engine into S, then the InfoNCE kernel with Z / theta given: the same dS, drhat and (by the pair's row ownership)
    partials, held to the bound the fused launch is held to -- so the two forms agree within twice that bound, element by element"""
    case, built = rc.BY_NAME[name], _build(name)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    outs = rc.pair_outs(built)
    after = _launch(case, built, pair=True)
    rel, ratio = _verify(case, built, after, outs)
    fused = _launch(case, built)
    worst = 0.0
    for key, _, o, rows, width, ld, _, bound in outs[:2]:
        idx = rc.window_index(o, rows, width, ld)
        q = np.abs(after[idx].astype(np.float64) - fused[idx].astype(np.float64)) / (2 * bound)
        worst = max(worst, float(q.max()))
    print(f'replearn {name} as GEMM + infonce: worst rel-L2 {rel:.2e} worst |err|/bound {ratio:.3f}; |pair - fused| / (2 bound) {worst:.3f}')
    assert worst <= 1
