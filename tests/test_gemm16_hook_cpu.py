"""CPU side of the 16-row tile engine's unit tests (tests/test_gemm16_engine.py runs the launches): the table hook refuses bad arguments before
any GPU call, and the per-element error bound the GPU tests rely on holds for a float32 NumPy evaluation of every case."""
import numpy as np
import pytest

import gemm16_cases as gc


def _task(**kw):
    from rlrep_amd import _lib
    t = _lib.Gemm16Task()
    t.a = t.b = t.c = 4096              # never dereferenced: every call below is refused before a launch
    t.lda = t.ldb = t.ldc = 16
    t.rows = t.cols = t.inner = 16
    t.scale = 1.0
    for k, v in kw.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize('what,nf,ntasks,kw', [
    ('no task', 1, 0, {}), ('nine tasks', 1, 9, {}), ('negative task count', 1, -1, {}),
    ('nf 3', 3, 1, {}), ('nf 0', 0, 1, {}), ('nf 8', 8, 1, {}),
    ('null a', 1, 1, dict(a=None)), ('null b', 1, 1, dict(b=None)), ('null c', 1, 1, dict(c=None)),
    ('null c in the second task', 1, 2, dict(c=None)),
    ('no rows', 1, 1, dict(rows=0)), ('negative columns', 1, 1, dict(cols=-3)), ('no inner length', 1, 1, dict(inner=0)),
    ('reparameterisation epilogue', 1, 1, dict(epi=2)), ('mse epilogue', 1, 1, dict(epi=4)), ('negative epilogue', 1, 1, dict(epi=-1)),
])
def test_table_hook_refuses_bad_arguments(what, nf, ntasks, kw):
    """No GPU is needed: a refusal happens before any GPU call (this test runs where there is none)."""
    from rlrep_amd import _lib
    n = max(ntasks, 1)
    arr = (_lib.Gemm16Task * 9)(*[_task() for _ in range(9)])
    arr[min(n, 9) - 1] = _task(**kw)
    rc = _lib.lib.rlrep_gemm16_table(0, 0, nf, arr, ntasks, 0, 1, 0, None)
    assert rc < 0, what
    msg = _lib.lib.rlrep_last_error()
    assert msg and b'gemm16_table' in msg, (what, msg)


def test_table_hook_refuses_a_null_table():
    from rlrep_amd import _lib
    assert _lib.lib.rlrep_gemm16_table(0, 0, 1, None, 1, 0, 1, 0, None) < 0 and _lib.lib.rlrep_last_error()


@pytest.mark.parametrize('name', [c.name for c in gc.CASES])
def test_float32_numpy_stays_inside_the_error_bound(name):
    """The bound 2 K 2^-24 (|A| |B|^T + |bias| + |C0|) is meant to hold for ANY correct fp32 evaluation: check it on NumPy's own float32 product
    (another summation order than the kernel's) at every shape the GPU tests use, before they rely on it."""
    built = gc.build(gc.BY_NAME[name])
    checked = 0
    for d in built.tasks:
        want, bound, want2, bound2 = gc.evaluate(d, np.float64)
        got, _, got2, _ = gc.evaluate(d, np.float32)
        for g, w, b in ((got, want, bound), (got2, want2, bound2)):
            if b is None:
                continue
            assert g.dtype == np.float32
            err = np.abs(g.astype(np.float64) - w)
            assert np.all(err <= b), (name, float(np.max(err / np.maximum(b, 1e-300))))
            checked += 1
    assert checked or all(d['act'] in ('elu', 'tanh', 'sin') for d in built.tasks)
