"""What prioritized replay costs: train()/s of sac with a plain and with a prioritized buffer, the three new launches alone,
and per_add behind add_device.  Writes profiles/per_replay.txt (and prints it).

    python tools/per_rate.py                                   # every table of this tree
    python tools/per_rate.py --parent DIR                      # ... and the plain-buffer rate of another checkout (built), alternated with this one

train:    sac_halfcheetah_b256 and sac_pendulum_b64 (bench.py's dimensions), graph train() on a ring filled with synthetic rows: a plain
          ReplayBuffer and a PrioritizedReplayBuffer at ring sizes 65 536 and 10^6.  One agent per arm (an agent keeps one captured graph),
          all arms of a workload in ONE process, alternated; the ratio to the plain arm of the same ring size is the finding.
parent:   the plain arms alone, in child processes (one at a time) that import the package of --parent DIR and of this tree in turn: the same
          graph with the same launch count, so the two must agree within the spread of the repeats.
launches: per_sample (drawing and given-indices mode), the gather (rlrep_replay_sample) and per_update alone: a hipGraph of --chain launches
          of the one kernel on one stream, host clock around a replay and a synchronise, per launch.
add:      add_device on a plain and on a prioritized ring at N = 256 / 4096 / 65 536 (each call followed by a synchronise), and per_add alone
          as in `launches`.  The bound: per_add at N = 65 536 stays below the add_device launch it follows.

Every figure: --warmup calls, then the median (and the sorted values) of --windows windows of --calls calls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {'sac_halfcheetah_b256': (17, 6, 256), 'sac_pendulum_b64': (3, 1, 64)}
RINGS = (65536, 1000000)


def _setup(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    return np, torch


class _Space(object):
    def __init__(self, np, A):
        self.low, self.high = -np.ones(A, np.float32), np.ones(A, np.float32)


def _agent(np, torch, S, A, B):
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    torch.manual_seed(0)
    return SACAgent(S, A, _Space(np, A), max_batch=B, seed=0, hidden_dim=256)


def _filled(np, cls, S, A, n, **kw):
    rng = np.random.default_rng(n)
    buf = cls(S, A, max_size=n, **kw)
    buf.load(rng.normal(size=(n, S)).astype(np.float32), rng.uniform(-1, 1, size=(n, A)).astype(np.float32), rng.normal(size=(n, S)).astype(np.float32),
             rng.normal(size=n).astype(np.float32), (rng.random(n) < 0.01).astype(np.float32))
    return buf


def _windows(torch, arms, warmup, calls, windows):
    """{arm: sorted us per call of each window}, arms alternated inside every window round"""
    for f in arms.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(windows):
        for k, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
            us[k].append(1e6 * (time.perf_counter() - t0) / calls)
    return {k: sorted(v) for k, v in us.items()}


def _fmt(v):
    return f'{statistics.median(v):8.2f} us ({", ".join(f"{u:.2f}" for u in v)})'


def _rate(v):
    return 1e6 / statistics.median(v)


def plain_rates(args, root):
    """{workload: sorted us per train() of each window} with a plain 65 536-row ring, importing the package under `root` (a child process's job)"""
    np, torch = _setup(root)
    from rlrep_amd.utils.buffer import ReplayBuffer
    out = {}
    for wl, (S, A, B) in WORKLOADS.items():
        agent, buf = _agent(np, torch, S, A, B), _filled(np, ReplayBuffer, S, A, RINGS[0])
        out[wl] = _windows(torch, {'plain': lambda: agent.train(buf, B)}, args.warmup, args.calls, args.windows)['plain']
        out[wl + '/launches'] = agent._graph_launches
    return out


def parent_table(args, say):
    """plain-buffer train()/s of --parent and of this tree, in child processes run one after the other, --repeats times each, alternated"""
    rows = {}
    for rep in range(args.repeats):
        for name, root in (('parent', os.path.abspath(args.parent)), ('this', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, '--warmup', str(args.warmup), '--calls', str(args.calls), '--windows', str(args.windows)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
            rows.setdefault(name, []).append(json.loads(res.stdout.strip().splitlines()[-1]))
    for wl in WORKLOADS:
        for name in ('parent', 'this'):
            meds = [_rate(r[wl]) for r in rows[name]]
            say(f'{wl} plain ring {RINGS[0]} [{name:6s}] {rows[name][0][wl + "/launches"]} launches: {statistics.median(meds):9.0f} train()/s, process medians '
                f'{", ".join(f"{m:.0f}" for m in meds)} (spread {100 * (max(meds) - min(meds)) / statistics.median(meds):.1f} %)')
        a, b = statistics.median([_rate(r[wl]) for r in rows['this']]), statistics.median([_rate(r[wl]) for r in rows['parent']])
        say(f'{wl}: this tree / parent = {a / b:.3f}')


def train_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer, ReplayBuffer
    for wl, (S, A, B) in WORKLOADS.items():
        arms, agents = {}, {}
        for n in RINGS:
            for kind, cls in (('plain', ReplayBuffer), ('prioritized', PrioritizedReplayBuffer)):
                agent, buf = _agent(np, torch, S, A, B), _filled(np, cls, S, A, n)
                agents[(kind, n)] = agent
                arms[(kind, n)] = lambda agent=agent, buf=buf: agent.train(buf, B)
        us = _windows(torch, arms, args.warmup, args.calls, args.windows)
        for n in RINGS:
            p, q = us[('plain', n)], us[('prioritized', n)]
            say(f'{wl} ring {n:7d} plain       ({agents[("plain", n)]._graph_launches} launches): {_fmt(p)} per train() = {_rate(p):8.0f} train()/s')
            say(f'{wl} ring {n:7d} prioritized ({agents[("prioritized", n)]._graph_launches} launches): {_fmt(q)} per train() = {_rate(q):8.0f} train()/s; '
                f'{_rate(q) / _rate(p):.3f} x plain, +{statistics.median(q) - statistics.median(p):.2f} us per train()')
        del arms, agents


def _chain(torch, fn, n):
    """a hipGraph of n launches of fn on one stream -> its replay"""
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        for _ in range(n):
            fn()
    return g.replay


def launches_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer
    K = args.chain
    for wl, (S, A, B) in WORKLOADS.items():
        agent = _agent(np, torch, S, A, B)
        for n in RINGS:
            buf = _filled(np, PrioritizedReplayBuffer, S, A, n)
            agent.train(buf, B)                                  # sizes the programs for B, leaves |TD| in the workspace and moved priorities in the tree
            torch.cuda.synchronize()
            idx, w = buf.draw_buffers(B)
            given = idx.cpu().numpy()
            arms = {'per_sample (draw)': _chain(torch, lambda: buf.draw(B, 1, 3 << 40, core=agent.core), K),
                    'per_sample (given)': _chain(torch, lambda: _given(buf, agent, B), K),
                    'gather': _chain(torch, lambda: _gather(agent, buf, idx, B), K),
                    'per_update': _chain(torch, lambda: buf.update(B, core=agent.core), K)}
            buf.draw(B, 0, 0, core=agent.core, given=given)
            us = _windows(torch, arms, args.warmup, max(1, args.calls // K), args.windows)
            for k, v in us.items():
                say(f'{wl} B = {B:3d} ring {n:7d} (tree {buf.P.bit_length() - 1} levels) {k:18s}: {_fmt([u / K for u in v])} per launch (chain of {K})')


def _given(buf, agent, B):
    import ctypes as C
    from rlrep_amd._lib import lib, check
    import torch
    idx, w = buf.draw_buffers(B)
    check(lib.rlrep_per_sample(agent.core.h, C.c_void_p(buf.tree.data_ptr()), buf.P, C.c_void_p(buf._scal.data_ptr()), C.c_void_p(idx.data_ptr()),
                               C.c_void_p(w.data_ptr()), B, 1, 0, 0, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'per_sample')


def _gather(agent, buf, idx, B):
    import ctypes as C
    from rlrep_amd._lib import lib, check
    import torch
    check(lib.rlrep_replay_sample(agent.core.h, 0, C.c_void_p(buf.ring.data_ptr()), C.c_void_p(idx.data_ptr()), B,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'replay_sample')


def add_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer, ReplayBuffer
    S, A, ring = 3, 1, 1000000
    gen = torch.Generator(device='cuda').manual_seed(0)
    sync = torch.cuda.current_stream().synchronize
    K = max(2, args.chain // 4)
    for N in (256, 4096, 65536):
        cols = [torch.randn(N, S, device='cuda', generator=gen), torch.randn(N, A, device='cuda', generator=gen), torch.randn(N, S, device='cuda', generator=gen),
                torch.randn(N, device='cuda', generator=gen), torch.zeros(N, device='cuda')]
        plain, per = ReplayBuffer(S, A, max_size=ring), PrioritizedReplayBuffer(S, A, max_size=ring)

        def add(buf):
            buf.add_device(*cols)
            sync()
        alone = _chain(torch, lambda: per._per_add(per.ptr, N), K)
        us = _windows(torch, {'plain': lambda: add(plain), 'prioritized': lambda: add(per)}, args.warmup, args.calls, args.windows)
        ua = _windows(torch, {'alone': alone}, max(1, args.warmup // K), max(1, args.calls // K), args.windows)['alone']
        p, q = statistics.median(us['plain']), statistics.median(us['prioritized'])
        say(f'add_device N = {N:5d} into a ring of {ring} rows (call + synchronise): plain {_fmt(us["plain"])}; prioritized {_fmt(us["prioritized"])}; '
            f'+{q - p:.2f} us = {q / p:.2f} x')
        say(f'per_add    N = {N:5d} alone (chain of {K}): {_fmt([u / K for u in ua])} per launch')
    big = PrioritizedReplayBuffer(S, A, max_size=ring)
    whole = _windows(torch, {'load': lambda: (big._per_add(0, ring), sync())}, 2, 5, args.windows)['load']
    say(f'per_add    N = {ring} (the whole ring, as load() issues it; call + synchronise): {_fmt(whole)}')


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='train,launches,add')
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain-buffer train()/s is measured beside this tree\'s')
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'per_replay.txt'))
    p.add_argument('--warmup', type=int, default=200)
    p.add_argument('--calls', type=int, default=2000)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--chain', type=int, default=64)
    args = p.parse_args(argv)
    if args.child:
        print(json.dumps(plain_rates(args, args.child)))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.parent:                      # (children first: this process has not opened the GPU yet)
        say(f'# plain-buffer train()/s, child processes alternated ({args.repeats} each): {args.warmup} warm-up calls, median of {args.windows} windows of {args.calls} calls')
        parent_table(args, say)
    np, torch = _setup(ROOT)
    say(f'# {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per arm, median (sorted windows) of {args.windows} windows of {args.calls} calls, '
        'arms alternated in one process')
    only = args.only.split(',')
    if 'train' in only:
        train_table(args, say)
    if 'launches' in only:
        launches_table(args, say)
    if 'add' in only:
        add_table(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
