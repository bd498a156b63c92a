"""vlsac train() rate against feature_dim, measured (profiles/vlsac_feature_dims.txt).  Not a bench.py workload: bench.py measures F = 256.

HalfCheetah dimensions (S = 17, A = 6), B = 256, H = 256, extra_feature_steps = 3, the default mode (graph replay, device Philox, two chains), and the
timing loop of bench.py: 300 untimed calls, then five windows of 500 train() calls, the median window.  Every arm runs in a process of its own (the
library is chosen when the package is imported: RLREP_LIB), one after the other, alternated where two builds are compared.

  1. F = 256 on a build of the PARENT commit (--parent-lib: the same ABI, built from the parent's csrc/ with OUTNAME=...) and on this build, alternated;
     the bar for "did not move" is the spread between the repeats of the parent arm itself.
  2. train()/s at F = 512 and F = 1024 (absolute figures: nothing ran at these widths before).
  3. one `rocprofv3 --kernel-trace --stats` run at F = 512: per-launch times of the nc_* kernels beside those of F = 256 in
     profiles/r06_vlsac_halfcheetah_f256_b256_kernel_stats.csv.
  4. the K-chunked fp32 forward against the whole-table form at F = 432 (RLREP_DISABLE=x3, without / with RLREP_ENABLE=nc_fwd_chunk): microseconds per
     launch of the two forward stages, each replayed from a graph of 50 launches (the method of tools/stage_times.py).

usage: python tools/vlsac_widths.py [--parent-lib PATH] [--out profiles/vlsac_feature_dims.txt] [--sections 1,2,3,4] [--repeats 3]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')]
S, A, B, H = 17, 6, 256, 256
WINDOW, WINDOWS, WARM = 500, 5, 300
R06 = os.path.join(ROOT, 'profiles', 'r06_vlsac_halfcheetah_f256_b256_kernel_stats.csv')


# ---- child: one agent, one process ------------------------------------------------------------------------------------------------------------
def _agent(F):
    import torch
    import bench
    torch.manual_seed(0)
    agent = bench.make_agent('vlsac', S, A, B, dict(hidden_dim=H, feature_dim=F, extra_feature_steps=3))
    buf, _ = bench.synth_buffer(S, A, 0)
    return agent, buf


def child_rate(F, quick):
    import time
    import numpy as np
    import torch
    agent, buf = _agent(F)
    for _ in range(20 if quick else WARM):
        agent.train(buf, B)
    agent.flush()
    torch.cuda.synchronize()
    rates, calls = [], 20 if quick else 0
    for _ in range(1 if quick else WINDOWS):
        t0 = time.perf_counter()
        for _ in range(WINDOW):
            info = agent.train(buf, B)
        agent.flush()
        torch.cuda.synchronize()
        rates.append(WINDOW / (time.perf_counter() - t0))
        calls += WINDOW
    assert all(np.isfinite(float(v)) for v in info.values())
    print(json.dumps({'F': F, 'windows': [round(r, 1) for r in rates], 'median': round(float(np.median(rates)), 1), 'train_calls': calls,
                      'graph': bool(agent.use_graph)}))


def child_stage(F):
    """microseconds per launch of the noise-critic forward stages of the critic and actor programs"""
    import torch
    agent, buf = _agent(F)
    for _ in range(20):
        agent.train(buf, B)
    agent.flush()
    torch.cuda.synchronize()
    core, out = agent.core, {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for p in (2, 4):
        for i, n in enumerate(core.stages(p)):
            if not n.startswith('noise critic l1/l4'):
                continue
            for _ in range(10):
                core.run_stage(p, i)
            torch.cuda.synchronize()
            g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.graph(g, stream=s):
                for _ in range(50):
                    core.run_stage(p, i)
            for _ in range(20):
                g.replay()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(8):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[n] = round(e0.elapsed_time(e1) * 1e3 / 400, 2)
    print(json.dumps({'F': F, 'stage_us': out}))


# ---- parent: the arms, one process each -------------------------------------------------------------------------------------------------------
def _spawn(args, lib=None, disable=None, enable=None, prefix=(), timeout=600):
    env = dict(os.environ)
    for k in ('RLREP_LIB', 'RLREP_DISABLE', 'RLREP_ENABLE'):
        env.pop(k, None)
    if lib:
        env['RLREP_LIB'] = lib
    if disable:
        env['RLREP_DISABLE'] = disable
    if enable:
        env['RLREP_ENABLE'] = enable
    r = subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=env, cwd=ROOT, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f'arm {args} (lib={lib}, disable={disable}, enable={enable}) ended with {r.returncode}: nothing further is started\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


def _stats(path):
    rows = {}
    with open(path) as f:
        for row in csv.DictReader(ln for ln in f if not ln.startswith('#')):
            rows[row['Name']] = (int(row['Calls']), float(row['AverageNs']))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', choices=['rate', 'stage'])
    ap.add_argument('--F', type=int, default=256)
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vlsac_feature_dims.txt'))
    ap.add_argument('--sections', default='1,2,3,4')
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    if a.child == 'rate':
        return child_rate(a.F, a.quick)
    if a.child == 'stage':
        return child_stage(a.F)
    sections = {int(x) for x in a.sections.split(',') if x}
    L = ['vlsac train() rate against feature_dim (tools/vlsac_widths.py)',
         f'HalfCheetah dims S={S} A={A}, B={B}, H={H}, extra_feature_steps=3, default mode; {WARM} untimed calls, then {WINDOWS} windows of {WINDOW} train() calls;',
         'a figure is the median window of ONE process unless it says otherwise.', '']

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(L) + '\n')

    if 1 in sections:
        L.append('1. F = 256: the parent commit\'s library against this build, alternated (one process per figure)')
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            L.append('   skipped: no --parent-lib given')
        else:
            par, cur = [], []
            for _ in range(a.repeats):
                par.append(_spawn(['--child', 'rate', '--F', '256'], lib=os.path.abspath(a.parent_lib))['median'])
                cur.append(_spawn(['--child', 'rate', '--F', '256'])['median'])
            med = lambda v: sorted(v)[len(v) // 2]
            L += [f'   parent     : {par} train()/s   median {med(par)}   spread (max - min) {max(par) - min(par):.1f} = {100 * (max(par) - min(par)) / med(par):.2f} %',
                  f'   this build : {cur} train()/s   median {med(cur)}   spread (max - min) {max(cur) - min(cur):.1f}',
                  f'   this build - parent (medians): {med(cur) - med(par):+.1f} train()/s = {100 * (med(cur) - med(par)) / med(par):+.2f} %;  bar: the parent arm\'s own spread']
        L.append('')
        flush()
    if 2 in sections:
        L.append('2. wider feature_dim on this build (absolute; nothing to compare with; ONE process each)')
        for F in (256, 512, 1024):
            d = _spawn(['--child', 'rate', '--F', str(F)])
            L.append(f'   F = {F:4d}: median {d["median"]} train()/s   windows {d["windows"]}')
        L.append('')
        flush()
    if 3 in sections:
        L.append('3. nc_* kernels, average ns per launch: F = 512 (ONE rocprofv3 --kernel-trace --stats run of this build, 520 train() calls) beside F = 256 (profiles/' + os.path.basename(R06) + ')')
        with tempfile.TemporaryDirectory() as td:
            _spawn(['--child', 'rate', '--F', '512', '--quick'], prefix=['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', td, '--'])
            found = glob.glob(os.path.join(td, '**', '*kernel_stats.csv'), recursive=True)
            new = _stats(found[0]) if found else {}
        old = _stats(R06) if os.path.exists(R06) else {}
        if not new:
            L.append('   no kernel_stats.csv came out of the profiler run')
        for name in sorted(n for n in new if 'nc_' in n):
            short = name.split('(')[0].replace('void ', '')
            o = old.get(name)
            L.append(f'   {short:28s} F=512: {new[name][1] / 1e3:8.2f} us x {new[name][0]:5d} launches    F=256: ' + (f'{o[1] / 1e3:8.2f} us x {o[0]:5d}' if o else '   (not in that run)'))
        L.append('')
        flush()
    if 4 in sections:
        L.append('4. fp32 forward at F = 432 (RLREP_DISABLE=x3), us per launch: whole table in LDS | K-chunked (RLREP_ENABLE=nc_fwd_chunk).  ONE process each; no bar (a fallback form)')
        whole = _spawn(['--child', 'stage', '--F', '432'], disable='x3')['stage_us']
        chunk = _spawn(['--child', 'stage', '--F', '432'], disable='x3', enable='nc_fwd_chunk')['stage_us']
        by_base = {n.replace(' [K-chunked]', ''): (n, u) for n, u in chunk.items()}          # (the chunked stage carries a suffix of its own)
        for n0, u0 in sorted(whole.items()):
            n1, u1 = by_base[n0]
            assert n1 != n0, 'the forced run did not take the chunked form'
            L.append(f'   {n0:36s} {u0:8.2f} us | {u1:8.2f} us  ({100 * (u1 - u0) / u0:+.1f} %)')
        L.append('')
        flush()
    print('\n'.join(L))


if __name__ == '__main__':
    main()
