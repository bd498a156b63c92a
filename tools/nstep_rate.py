"""What n-step replay costs: train()/s of sac with a plain and with an n-step ring, single agent and seed group, the gather
alone, and the plain-buffer rate against another checkout.  Writes profiles/nstep_replay.txt (and prints it).

    python tools/nstep_rate.py                                   # every table of this tree
    python tools/nstep_rate.py --parent DIR                      # ... and the plain-buffer rate of another checkout (built), alternated with this one

parent:   sac_halfcheetah_b256 and sac_pendulum_b64 (bench.py's dimensions), graph train() on a plain 65 536-row ring, in child processes (one
          at a time) that import the package of --parent DIR and of this tree in turn: the same graph with the same launch count, so the two
          must agree within the spread of the repeats.
train:    the same workloads on a ring of 65 536 rows of synthetic trajectories (episodes of 200 steps): a plain ReplayBuffer against
          n_step = 3 and 5, one agent per arm, all arms of a workload in ONE process, alternated; then an R = 4 seed group the same way.
gather:   rlrep_replay_gather_nstep alone at S = 3, 17 and 376 (B = 256; n = 1, the plain copy, 3 and 5): a hipGraph of
          --chain launches of the one kernel on one stream, host clock around a replay and a synchronise, per launch.

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
RING = 65536
NS = (3, 5)


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


def _trajectory_rows(np, S, A, n, seed, episode=200):
    """n rows of one environment: s of a row is s' of the row before it, except at the first row of an episode"""
    rng = np.random.default_rng(seed)
    s2 = rng.normal(size=(n, S)).astype(np.float32)
    s = np.empty_like(s2)
    s[1:] = s2[:-1]
    starts = np.arange(0, n, episode)
    s[starts] = rng.normal(size=(len(starts), S)).astype(np.float32)
    return (s, rng.uniform(-1, 1, size=(n, A)).astype(np.float32), s2, rng.normal(size=n).astype(np.float32), np.zeros(n, np.float32))


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
    """{workload: sorted us per train() of each window} with a plain ring, importing the package under `root` (a child process's job)"""
    np, torch = _setup(root)
    from rlrep_amd.utils.buffer import ReplayBuffer
    out = {}
    for wl, (S, A, B) in WORKLOADS.items():
        agent, buf = _agent(np, torch, S, A, B), ReplayBuffer(S, A, max_size=RING)
        buf.load(*_trajectory_rows(np, S, A, RING, 1))
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
            say(f'{wl} plain ring {RING} [{name:6s}] {rows[name][0][wl + "/launches"]} launches: {statistics.median(meds):9.0f} train()/s, process medians '
                f'{", ".join(f"{m:.0f}" for m in meds)} (spread {100 * (max(meds) - min(meds)) / statistics.median(meds):.1f} %)')
        a, b = statistics.median([_rate(r[wl]) for r in rows['this']]), statistics.median([_rate(r[wl]) for r in rows['parent']])
        say(f'{wl}: this tree / parent = {a / b:.3f}')


def train_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import ReplayBuffer
    for wl, (S, A, B) in WORKLOADS.items():
        rows = _trajectory_rows(np, S, A, RING, 1)
        arms, agents = {}, {}
        for n in (1,) + NS:
            agent, buf = _agent(np, torch, S, A, B), ReplayBuffer(S, A, max_size=RING, n_step=n)
            buf.load(*rows)
            agents[n] = agent
            arms[n] = lambda agent=agent, buf=buf: agent.train(buf, B)
        us = _windows(torch, arms, args.warmup, args.calls, args.windows)
        p = us[1]
        say(f'{wl} single agent, ring {RING} plain      ({agents[1]._graph_launches} launches): {_fmt(p)} per train() = {_rate(p):8.0f} train()/s')
        for n in NS:
            q = us[n]
            say(f'{wl} single agent, ring {RING} n_step = {n} ({agents[n]._graph_launches} launches): {_fmt(q)} per train() = {_rate(q):8.0f} train()/s; '
                f'{_rate(q) / _rate(p):.3f} x plain, +{statistics.median(q) - statistics.median(p):.2f} us per train()')
        del arms, agents


def group_table(args, say, R=4):
    np, torch = _setup(ROOT)
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    for wl, (S, A, B) in WORKLOADS.items():
        arms, groups = {}, {}
        for n in (1,) + NS:
            g = SACSeedBatch(list(range(R)), S, A, _Space(np, A), max_batch=B, hidden_dim=256)
            gb = ReplayBufferGroup(R, S, A, max_size=RING, n_step=n)
            for r in range(R):
                gb.load(r, *_trajectory_rows(np, S, A, RING, 10 + r))
            groups[n] = g
            arms[n] = lambda g=g, gb=gb: g.train(gb, B)
        us = _windows(torch, arms, args.warmup, args.calls, args.windows)
        p = us[1]
        say(f'{wl} group R = {R}, rings {RING} plain      ({groups[1]._graph_launches} launches): {_fmt(p)} per train() = {_rate(p):8.0f} train()/s')
        for n in NS:
            q = us[n]
            say(f'{wl} group R = {R}, rings {RING} n_step = {n} ({groups[n]._graph_launches} launches): {_fmt(q)} per train() = {_rate(q):8.0f} train()/s; '
                f'{_rate(q) / _rate(p):.3f} x plain, +{statistics.median(q) - statistics.median(p):.2f} us per train()')
        del arms, groups


def _chain(torch, fn, n):
    """a hipGraph of n launches of fn on one stream -> its replay"""
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        for _ in range(n):
            fn()
    return g.replay


def gather_table(args, say, B=256, A=6):
    import ctypes as C
    np, torch = _setup(ROOT)
    from rlrep_amd._lib import lib, check
    from rlrep_amd.utils.buffer import ReplayBuffer
    K = args.chain
    for S in (3, 17, 376):
        buf = ReplayBuffer(S, A, max_size=RING)
        buf.load(*_trajectory_rows(np, S, A, RING, 2))
        size_dev = buf.size_dev()
        idx = torch.from_numpy(np.random.default_rng(3).integers(0, RING, size=B).astype(np.int32)).cuda()
        xe = torch.empty(B, 2 * S + A, device='cuda')
        xf, xf2, xfpi = (torch.zeros(B, S + A, device='cuda') for _ in range(3))
        r, d = torch.empty(B, device='cuda'), torch.empty(B, device='cuda')
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def gather(n):
            check(lib.rlrep_replay_gather_nstep(ptr(buf.ring), ptr(idx), B, S, A, RING, ptr(size_dev), n, 1, 0.99, ptr(xe), ptr(xf), ptr(xf2), ptr(xfpi), ptr(r),
                                                ptr(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'replay_gather_nstep')
        arms = {f'n = {n}': _chain(torch, lambda n=n: gather(n), K) for n in (1,) + NS}
        us = _windows(torch, arms, max(1, args.warmup // K), max(1, args.calls // K), args.windows)
        for k, v in us.items():
            say(f'gather S = {S:3d} A = {A} B = {B} ring {RING} {k:11s}: {_fmt([u / K for u in v])} per launch (chain of {K})')


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='train,group,gather')
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain-buffer train()/s is measured beside this tree\'s')
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nstep_replay.txt'))
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
    if 'group' in only:
        group_table(args, say)
    if 'gather' in only:
        gather_table(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
