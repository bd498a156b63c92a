"""What prioritized replay costs a sac SEED GROUP: train()/s of a group on a plain and on a prioritized buffer group, the
group against separate prioritized agents, and the three group launches alone.  Writes profiles/per_group.txt (and prints it).  The helpers
(windows, chains, formatting) are tools/per_rate.py's.

    python tools/per_group_rate.py                             # every table of this tree
    python tools/per_group_rate.py --parent DIR                # ... and the plain group rate of another checkout (built), alternated with this one

parent:   a plain ReplayBufferGroup, R = 4 and 8, sac_halfcheetah_b256, in child processes (one at a time) that import the package of --parent
          DIR and of this tree in turn: the same graph with the same launch count, so the two must agree within the spread of the processes.
train:    R = 4 / 8 / 16 members, sac_pendulum_b64 and sac_halfcheetah_b256, rings of 65 536 rows (R = 4: also 10^6): a plain and a prioritized
          buffer group, one group per arm, all arms of a row in ONE process, alternated.
separate: R = 4 in one group against four SACAgents called one after the other, both on prioritized and on plain buffers.
launches: per_add_grp (N = 256 and 65 536 rows), per_sample_grp (alone, and with the gather launch behind it) and per_update_grp alone at R = 1 / 4 / 16, as chains in a
          hipGraph, and the add_device call per_add_grp follows.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from per_rate import WORKLOADS, _Space, _agent, _chain, _fmt, _rate, _setup, _windows  # noqa: E402


def _group(np, torch, S, A, B, R):
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    return SACSeedBatch(list(range(R)), S, A, _Space(np, A), max_batch=B, hidden_dim=256)


def _rows(np, S, A, n):
    rng = np.random.default_rng(n)
    return (rng.normal(size=(n, S)).astype(np.float32), rng.uniform(-1, 1, size=(n, A)).astype(np.float32), rng.normal(size=(n, S)).astype(np.float32),
            rng.normal(size=n).astype(np.float32), (rng.random(n) < 0.01).astype(np.float32))


def _filled_group(cls, rows, S, A, n, R):
    buf = cls(R, S, A, max_size=n)
    for r in range(R):                    # (the same rows in every ring: the members differ by their seeds)
        buf.load(r, *rows)
    return buf


def plain_rates(args, root):
    """{R: sorted us per train() of each window} of a plain group, importing the package under `root` (a child process's job)"""
    np, torch = _setup(root)
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    S, A, B = WORKLOADS['sac_halfcheetah_b256']
    rows, out = _rows(np, S, A, 65536), {}
    for R in (4, 8):
        g, buf = _group(np, torch, S, A, B, R), _filled_group(ReplayBufferGroup, rows, S, A, 65536, R)
        out[str(R)] = _windows(torch, {'plain': lambda: g.train(buf, B)}, args.warmup, args.calls, args.windows)['plain']
        out[f'{R}/launches'] = g._graph_launches
    return out


def parent_table(args, say):
    res = {}
    for rep in range(args.repeats):
        for name, root in (('parent', os.path.abspath(args.parent)), ('this', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, '--warmup', str(args.warmup), '--calls', str(args.calls), '--windows', str(args.windows)]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
            res.setdefault(name, []).append(json.loads(out.stdout.strip().splitlines()[-1]))
    for R in ('4', '8'):
        for name in ('parent', 'this'):
            meds = [_rate(r[R]) for r in res[name]]
            say(f'sac_halfcheetah_b256 plain group R = {R} ring 65536 [{name:6s}] {res[name][0][R + "/launches"]} launches: {statistics.median(meds):9.0f} train()/s, '
                f'process medians {", ".join(f"{m:.0f}" for m in meds)} (spread {100 * (max(meds) - min(meds)) / statistics.median(meds):.1f} %)')
        a, b = statistics.median([_rate(r[R]) for r in res['this']]), statistics.median([_rate(r[R]) for r in res['parent']])
        say(f'R = {R}: this tree / parent = {a / b:.3f}')


def train_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup, ReplayBufferGroup
    for wl, (S, A, B) in WORKLOADS.items():
        for R, n in ((4, 65536), (8, 65536), (16, 65536), (4, 1000000)):
            rows = _rows(np, S, A, n)
            arms, groups = {}, {}
            for kind, cls in (('plain', ReplayBufferGroup), ('prioritized', PrioritizedReplayBufferGroup)):
                g, buf = _group(np, torch, S, A, B, R), _filled_group(cls, rows, S, A, n, R)
                groups[kind] = g
                arms[kind] = lambda g=g, buf=buf: g.train(buf, B)
            us = _windows(torch, arms, args.warmup, args.calls, args.windows)
            p, q = us['plain'], us['prioritized']
            say(f'{wl} R = {R:2d} ring {n:7d} plain       ({groups["plain"]._graph_launches} launches): {_fmt(p)} per train() = {_rate(p):8.0f} train()/s')
            say(f'{wl} R = {R:2d} ring {n:7d} prioritized ({groups["prioritized"]._graph_launches} launches): {_fmt(q)} per train() = {_rate(q):8.0f} train()/s; '
                f'{_rate(q) / _rate(p):.3f} x plain, +{statistics.median(q) - statistics.median(p):.2f} us per train()')
            del arms, groups, rows
            torch.cuda.empty_cache()


def separate_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import PrioritizedReplayBuffer, ReplayBuffer
    from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup, ReplayBufferGroup
    R, n = 4, 65536
    for wl, (S, A, B) in WORKLOADS.items():
        rows, arms = _rows(np, S, A, n), {}
        for kind, gcls, cls in (('plain', ReplayBufferGroup, ReplayBuffer), ('prioritized', PrioritizedReplayBufferGroup, PrioritizedReplayBuffer)):
            g, gb = _group(np, torch, S, A, B, R), _filled_group(gcls, rows, S, A, n, R)
            agents = [_agent(np, torch, S, A, B) for _ in range(R)]
            bufs = []
            for _ in range(R):
                b = cls(S, A, max_size=n)
                b.load(*rows)
                bufs.append(b)
            arms[(kind, 'group')] = lambda g=g, gb=gb: g.train(gb, B)
            arms[(kind, 'separate')] = lambda agents=agents, bufs=bufs: [a.train(b, B) for a, b in zip(agents, bufs)]
        us = _windows(torch, arms, args.warmup, max(1, args.calls // 2), args.windows)
        for kind in ('plain', 'prioritized'):
            gq, sq = us[(kind, 'group')], us[(kind, 'separate')]
            say(f'{wl} R = 4 {kind:11s}: one group {_fmt(gq)} per train() of all members; four agents {_fmt(sq)} per round of four train(); '
                f'group = {statistics.median(sq) / statistics.median(gq):.2f} x the separate agents')
        del arms


def launches_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup
    K = args.chain
    S, A, B = WORKLOADS['sac_halfcheetah_b256']
    n = 65536
    rows = _rows(np, S, A, n)
    gen = torch.Generator(device='cuda').manual_seed(0)
    sync = torch.cuda.current_stream().synchronize
    for R in (1, 4, 16):
        g, gb = _group(np, torch, S, A, B, R), _filled_group(PrioritizedReplayBufferGroup, rows, S, A, n, R)
        g.train(gb, B)                    # sizes the programs for B, leaves |TD| in the workspaces and moved priorities in the trees
        torch.cuda.synchronize()
        arms = {'per_sample_grp (draw + gather)': _chain(torch, lambda: gb.draw(B, 3 << 40, core=g.core, use_counter=True, gather=True), K),
                'per_sample_grp (draw)': _chain(torch, lambda: gb.draw(B, 3 << 40, core=g.core, use_counter=True), K),
                'per_update_grp': _chain(torch, lambda: gb.update(B, core=g.core), K),
                'per_add_grp N = 256': _chain(torch, lambda: gb._per_add(gb.ptr, 256), K),
                'per_add_grp N = 65536': _chain(torch, lambda: gb._per_add(gb.ptr, n), K)}
        us = _windows(torch, arms, max(1, args.warmup // K), max(1, args.calls // K), args.windows)
        for k, v in us.items():
            say(f'R = {R:2d} B = {B} ring {n} (trees of {gb.P.bit_length() - 1} levels) {k:31s}: {_fmt([u / K for u in v])} per launch (chain of {K})')
        for N in (256, n):
            cols = [torch.randn(R, N, S, device='cuda', generator=gen), torch.randn(R, N, A, device='cuda', generator=gen), torch.randn(R, N, S, device='cuda', generator=gen),
                    torch.randn(R, N, device='cuda', generator=gen), torch.zeros(R, N, device='cuda')]
            from rlrep_amd.utils.buffer_group import ReplayBufferGroup
            plain = ReplayBufferGroup(R, S, A, max_size=n)
            ua = _windows(torch, {'plain': lambda: (plain.add_device(*cols), sync()), 'prioritized': lambda: (gb.add_device(*cols), sync())},
                          20, max(20, args.calls // 20), args.windows)
            say(f'R = {R:2d} add_device N = {N:5d} (call + synchronise): plain {_fmt(ua["plain"])}; prioritized {_fmt(ua["prioritized"])}; '
                f'+{statistics.median(ua["prioritized"]) - statistics.median(ua["plain"]):.2f} us')
            del cols, plain
        del g, gb, arms
        torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='train,separate,launches')
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain group train()/s is measured beside this tree\'s')
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'per_group.txt'))
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
        say(f'# plain group train()/s, child processes alternated ({args.repeats} each): {args.warmup} warm-up calls, median of {args.windows} windows of {args.calls} calls')
        parent_table(args, say)
    np, torch = _setup(ROOT)
    say(f'# {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per arm, median (sorted windows) of {args.windows} windows of {args.calls} calls, '
        'arms alternated in one process')
    only = args.only.split(',')
    if 'train' in only:
        train_table(args, say)
    if 'separate' in only:
        separate_table(args, say)
    if 'launches' in only:
        launches_table(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
