"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, written as DIR/<name>.npy so that two builds can be
compared output for output (same arguments, same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_keeps_small_outputs_whole_and_samples_large_ones_the_same_way_every_time(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    small = {'info.loss': np.asarray(0.25, np.float64), 'state.w': rng.standard_normal((8, 4)).astype(np.float32)}
    d = bench.dump_outputs(small, str(tmp_path / 'a'), limit=1 << 10)
    assert d['files'] == 2 and d['sampled'] == [] and d['bytes'] == 8 + 8 * 4 * 4
    for k, v in small.items():
        got = np.load(tmp_path / 'a' / f'{k}.npy')
        assert got.dtype == v.dtype and np.array_equal(got, v), k

    big = dict(small, **{'state.big': rng.standard_normal(4096).astype(np.float32), 'state.a/b': rng.standard_normal(3000)})
    limit = 4 << 10
    runs = [bench.dump_outputs(big, str(tmp_path / r), limit=limit) for r in ('b', 'c')]
    assert runs[0]['sampled'] == ['state.big', 'state.a/b'] and runs[0]['bytes'] <= limit
    for name, f in (('info.loss', 'info.loss'), ('state.w', 'state.w'), ('state.big', 'state.big'), ('state.a/b', 'state.a_b')):
        b, c = np.load(tmp_path / 'b' / f'{f}.npy'), np.load(tmp_path / 'c' / f'{f}.npy')
        assert b.dtype == big[name].dtype and np.array_equal(b, c), name
        if name in runs[0]['sampled']:
            assert b.nbytes == limit // len(big) and np.isin(b, big[name]).all()
        else:
            assert np.array_equal(b, big[name])
    assert sum(p.stat().st_size for p in (tmp_path / 'b').iterdir()) <= limit + 128 * len(big)       # (+ the .npy headers)


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """The driver's workload over a short protocol: exactly --steps timed train() calls, and the dump holds the metric dict and every
    parameter / target tensor of the agent (finite)."""
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '2', '--no-extra-warmup', '--no-cpu',
                        '--quick', '--no-profile', '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert d['steps'] == 4 and d['ms_per_step'] > 0
    assert d['total_train_calls'] == 2 + 4 + 1          # warm-up, timed window, and the one call whose metrics are checked for finiteness
    names = {p.name[:-len('.npy')] for p in out.iterdir()}
    assert d['dump_outputs']['files'] == len(names) and d['dump_outputs']['sampled'] == []
    assert {'info.vae_loss', 'info.q1_loss', 'info.actor_loss', 'info.alpha', 'state.log_alpha'} <= names
    assert sum(n.startswith('state.') for n in names) > 20
    for p in out.iterdir():
        a = np.load(p)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), p.name
