"""GPU unit tests of the 16-row tile engine (csrc/gemm16.hip, gemm16_tile.h) through its table hook (rlrep_gemm16_table): every front end
(record, fast, fast4, duo), every tile width (NF = 1 / 2 / 4), multi-task directories, the XCD dealing of weight-gradient tiles and the
packed-argument guards, on partial row and column tiles -- against the same operation in float64 NumPy (tests/gemm16_cases.py).

Per output: relative L2 < 1e-5 (the bar tests/test_gemm_engines.py holds the fp32 engines to); for forward / dX with no activation or ReLU
and for dW also the per-element bound 2 K 2^-24 (|A| |B|^T + |bias| + |C0|) derived in gemm16_cases.py; every word of the allocation outside
the R x Cn output windows bit-unchanged (sentinel guards behind ldc > Cn and after row R; NaN operand padding); all outputs finite; and the
front end each case names is the one it got (rlrep_front_end_counts around the call), so no case is vacuous.

Every case prints its worst relative L2 and its worst |error| / bound (pytest -s)."""
import numpy as np
import pytest
import torch

import gemm16_cases as gc

pytestmark = pytest.mark.gpu

_built = {}


def _build(name):
    """host image and float64 references of a case: computed once, shared by every test that runs the case, never modified"""
    if name not in _built:
        _built[name] = gc.build(gc.BY_NAME[name])
        _built[name].arena.setflags(write=False)
    return _built[name]


def _launch(case, built):
    """One launch of the case's table on a fresh device copy of its arena.  Returns (arena after, front-end count differences)."""
    from rlrep_amd import _lib
    dev = torch.from_numpy(built.arena.copy()).cuda()
    base = dev.data_ptr()
    at = lambda o: None if o is None else base + 4 * o
    arr = (_lib.Gemm16Task * len(built.tasks))()
    for s, d in zip(arr, built.tasks):
        s.a, s.b, s.c = at(d['a']), at(d['b']), at(d['c'])
        s.lda, s.ldb, s.ldc, s.rows, s.cols, s.inner = d['lda'], d['ldb'], d['ldc'], d['R'], d['Cn'], d['K']
        s.epi, s.act, s.flags = d['epi'], gc.ACT[d['act']], (1 if d['accum'] else 0) | (2 if d['biasgrad'] else 0)
        s.bias, s.aux, s.ldaux, s.out2 = at(d['bias_o']), at(d['aux_o']), d['ldc'], at(d['out2_o'])
        s.r1u, s.r1v, s.scale = at(d['r1u_o']), at(d['r1v_o']), d['scale']
    torch.cuda.synchronize()
    f0 = _lib.front_end_counts()
    rc = _lib.lib.rlrep_gemm16_table(case.la, case.lb, case.nf, arr, len(built.tasks), case.duo_split, case.nf2, 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'gemm16_table')
    torch.cuda.synchronize()
    f1 = _lib.front_end_counts()
    return dev.cpu().numpy(), {k: f1[k] - f0[k] for k in f1}


def _only(front):
    return {k: int(k == front) for k in ('fast', 'fast4', 'fastpre', 'record')}


def _verify(case, built, after):
    """Every check on the arena a launch left behind; returns (worst relative L2, worst |error| / bound)."""
    nfs = [1 if (case.duo_split and q < case.duo_split) else case.nf2 if case.duo_split else case.nf for q in range(len(built.tasks))]
    window = np.zeros(after.size, bool)
    worst_rel, worst_ratio = 0.0, 0.0
    for what, q, off, rows, ld, R, Cn, want, bound in built.outs:
        idx = (off + np.arange(rows)[:, None] * ld + np.arange(ld)[None, :])[:R, :Cn]
        window[idx] = True
        got = after[idx].astype(np.float64)
        err = np.abs(got - want)
        r, c = np.unravel_index(np.argmax(np.where(np.isfinite(err), err, np.inf)), err.shape)
        where = f'{case.name} {what}: worst element (row {r}, col {c}) = tile (tr {r // 16}, tc {c // (16 * nfs[q])}) of NF {nfs[q]}, got {got[r, c]!r} want {want[r, c]!r}'
        assert np.all(np.isfinite(got)), 'non-finite output (a masked load leaked operand padding?) ' + where
        rel = float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
        worst_rel = max(worst_rel, rel)
        assert rel < 1e-5, f'relative L2 {rel:.3e} ' + where
        if bound is not None:
            ratio = float(np.max(err / np.maximum(bound, 1e-300)))
            worst_ratio = max(worst_ratio, ratio)
            assert np.all(err <= bound), f'|error| / bound = {ratio:.3f} ' + where
    changed = (after.view(np.uint32) != built.arena.view(np.uint32)) & ~window
    assert not changed.any(), f'{case.name}: {int(changed.sum())} words outside the output windows changed, first at float offset {int(np.argmax(changed))}'
    return worst_rel, worst_ratio


@pytest.mark.parametrize('name', [c.name for c in gc.CASES])
def test_table_against_float64(name, monkeypatch):
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    case, built = gc.BY_NAME[name], _build(name)
    after, fe = _launch(case, built)
    assert fe == _only(case.front), (name, 'front end', fe, 'expected', case.front)
    rel, ratio = _verify(case, built, after)
    print(f'gemm16 {name}: front={case.front} nf={case.nf2 if case.duo_split else case.nf}{" duo" if case.duo_split else ""} tasks={len(built.tasks)} '
          f'worst rel-L2 {rel:.2e} worst |err|/bound {ratio:.3f}')


@pytest.mark.parametrize('name', [c.name for c in gc.CASES if c.front in ('fast', 'fast4')])
def test_front_ends_are_bit_identical(name, monkeypatch):
    """gemm16.hip's contract for RLREP_DISABLE=gemm16_fast (every launch on the record front end) and =gemm16_spec (no compiled-in epilogues):
    bit-identical results -- here on partial row tiles, for every fast / fast4 case; and a rerun of the same launch is bit-identical too."""
    case, built = gc.BY_NAME[name], _build(name)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    ref, fe = _launch(case, built)
    assert fe == _only(case.front), (name, fe)
    again, fe = _launch(case, built)
    assert fe == _only(case.front) and np.array_equal(ref.view(np.uint32), again.view(np.uint32)), (name, 'rerun', fe)
    for off in ('gemm16_fast', 'gemm16_spec'):
        monkeypatch.setenv('RLREP_DISABLE', off)
        got, fe = _launch(case, built)
        assert fe == _only('record'), (name, off, fe)
        diff = got.view(np.uint32) != ref.view(np.uint32)
        assert not diff.any(), f'{name}: RLREP_DISABLE={off} changes {int(diff.sum())} words, first at float offset {int(np.argmax(diff))}'
    _verify(case, built, got)


@pytest.mark.parametrize('name', gc.XCD_CASES)
def test_xcd_dealing_changes_no_bit(name, monkeypatch):
    """weight-gradient launches of >= 64 tiles with total % 8 != 0: the tiles dealt to the XCDs as contiguous runs (gemm16_kernel, hdr bit 1)
    against launch order (RLREP_DISABLE=dw_xcd) -- the same tiles on other workgroups, so every output bit must agree (and every tile is right:
    test_table_against_float64 runs these cases too)."""
    case, built = gc.BY_NAME[name], _build(name)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    dealt, _ = _launch(case, built)
    _verify(case, built, dealt)
    monkeypatch.setenv('RLREP_DISABLE', 'dw_xcd')
    plain, fe = _launch(case, built)
    assert fe == _only('record')
    _verify(case, built, plain)
    assert np.array_equal(dealt.view(np.uint32), plain.view(np.uint32)), name


def test_gemm_engine_0_is_unchanged_by_the_hook():
    """rlrep_gemm(engine 0) and the hook run the same launch: same bits for the same task"""
    from rlrep_amd import _lib
    case, built = gc.BY_NAME['rec_fwd_relu'], _build('rec_fwd_relu')
    ref, _ = _launch(case, built)
    d = built.tasks[0]
    dev = torch.from_numpy(built.arena.copy()).cuda()
    at = lambda o: dev.data_ptr() + 4 * o
    rc = _lib.lib.rlrep_gemm(0, 0, 0, at(d['a']), d['lda'], at(d['b']), d['ldb'], at(d['c']), d['ldc'], d['R'], d['Cn'], d['K'], 0, gc.ACT['relu'], 0,
                             at(d['bias_o']), None, 0, None, 0, 0, None, 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'gemm')
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), ref.view(np.uint32))
