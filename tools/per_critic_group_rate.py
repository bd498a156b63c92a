"""What prioritized critic replay costs a ctrlsac SEED GROUP: the rates the change must leave alone against another checkout,
train()/s of a group on a plain ReplayBufferGroup and on a CriticPrioritizedReplayBufferGroup, the group against separate prioritized agents,
and the fused group launch beside the two launches it replaces.  Writes profiles/per_critic_group.txt (and prints it).  The helpers (windows,
chains, formatting) are tools/per_rate.py's.

    python tools/per_critic_group_rate.py                      # every table of this tree
    python tools/per_critic_group_rate.py --parent DIR         # ... and the untouched rates of another checkout (built), alternated with this one

parent:   a ctrlsac group (ctrlsac_halfcheetah_f256_b256, R = 4) on a plain ReplayBufferGroup and a sac group (sac_halfcheetah_b256, R = 4) on a
          PrioritizedReplayBufferGroup, rings of 65 536 rows, in child processes (one at a time) that import the package of --parent DIR and of
          this tree in turn: the same graphs with the same launch counts, so the two must agree within the spread of the processes.
train:    ctrlsac_halfcheetah_f256_b256 (F = 256, B = 256), R = 4 / 8 / 16, rings of 65 536 rows: a plain and a critic-prioritized buffer group,
          one group per arm, both arms of a row in ONE process, alternated; the difference in us per train() is the finding.
separate: R = 4 in one group against four CTRLSACAgent(pipeline=False) called one after the other, on critic-prioritized and on plain buffers.
fused:    rlrep_group_per_sample_fill on a ctrlsac group against rlrep_group_per_sample with its gather (two launches, a sac group of the same
          S, A, B and R), each as a hipGraph of --chain repetitions, R = 4 and 16, (S, A) = (17, 6), B = 256; per repetition.

Every figure: --warmup calls, then the median (and the sorted values) of --windows windows of --calls calls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from per_rate import _Space, _chain, _fmt, _rate, _setup, _windows  # noqa: E402

S, A, B, RING = 17, 6, 256, 65536
CTRL_KW = dict(hidden_dim=256, feature_dim=256, extra_feature_steps=3)          # bench.py ctrlsac_halfcheetah_f256_b256
PER_STREAM = 3 << 40


def _rows(np, n):
    rng = np.random.default_rng(n)
    return (rng.normal(size=(n, S)).astype(np.float32), rng.uniform(-1, 1, size=(n, A)).astype(np.float32), rng.normal(size=(n, S)).astype(np.float32),
            rng.normal(size=n).astype(np.float32), (rng.random(n) < 0.01).astype(np.float32))


def _ctrl_group(np, R):
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    return CTRLSACSeedBatch(list(range(R)), S, A, _Space(np, A), max_batch=B, **CTRL_KW)


def _sac_group(np, R):
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    return SACSeedBatch(list(range(R)), S, A, _Space(np, A), max_batch=B, hidden_dim=256)


def _filled_group(cls, rows, R):
    buf = cls(R, S, A, max_size=RING)
    for r in range(R):                    # (the same rows in every ring: the members differ by their seeds)
        buf.load(r, *rows)
    return buf


def untouched_rates(args, root):
    """{arm: sorted us per train() of each window} of the two groups this change must leave alone, importing the package under `root` (a
    child process's job)"""
    np, torch = _setup(root)
    from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup, ReplayBufferGroup
    rows, out = _rows(np, RING), {}
    for arm, g, buf in (('ctrlsac plain group', _ctrl_group(np, 4), _filled_group(ReplayBufferGroup, rows, 4)),
                        ('sac prioritized group', _sac_group(np, 4), _filled_group(PrioritizedReplayBufferGroup, rows, 4))):
        out[arm] = _windows(torch, {arm: lambda: g.train(buf, B)}, args.warmup, args.calls, args.windows)[arm]
        out[arm + '/launches'] = g._graph_launches
    return out


def parent_table(args, say):
    res = {}
    for rep in range(args.repeats):
        for name, root in (('parent', os.path.abspath(args.parent)), ('this', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, '--warmup', str(args.warmup), '--calls', str(args.calls), '--windows', str(args.windows)]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300)
            res.setdefault(name, []).append(json.loads(out.stdout.strip().splitlines()[-1]))
    for arm in ('ctrlsac plain group', 'sac prioritized group'):
        for name in ('parent', 'this'):
            meds = [_rate(r[arm]) for r in res[name]]
            say(f'{arm} R = 4 ring {RING} [{name:6s}] {res[name][0][arm + "/launches"]} launches: {statistics.median(meds):9.0f} train()/s, '
                f'process medians {", ".join(f"{m:.0f}" for m in meds)} (spread {100 * (max(meds) - min(meds)) / statistics.median(meds):.1f} %)')
        a, b = statistics.median([_rate(r[arm]) for r in res['this']]), statistics.median([_rate(r[arm]) for r in res['parent']])
        say(f'{arm}: this tree / parent = {a / b:.3f}')


def train_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup, ReplayBufferGroup
    rows = _rows(np, RING)
    for R in (4, 8, 16):
        arms, groups = {}, {}
        for kind, cls in (('plain', ReplayBufferGroup), ('prioritized critic', CriticPrioritizedReplayBufferGroup)):
            g, buf = _ctrl_group(np, R), _filled_group(cls, rows, R)
            groups[kind] = g
            arms[kind] = lambda g=g, buf=buf: g.train(buf, B)
        us = _windows(torch, arms, args.warmup, args.calls, args.windows)
        p, q = us['plain'], us['prioritized critic']
        say(f'ctrlsac_halfcheetah_f256_b256 R = {R:2d} ring {RING} plain              ({groups["plain"]._graph_launches} launches): {_fmt(p)} per train() = '
            f'{_rate(p):8.0f} train()/s')
        say(f'ctrlsac_halfcheetah_f256_b256 R = {R:2d} ring {RING} prioritized critic ({groups["prioritized critic"]._graph_launches} launches): {_fmt(q)} per train() = '
            f'{_rate(q):8.0f} train()/s; {_rate(q) / _rate(p):.3f} x plain, {statistics.median(q) - statistics.median(p):+.2f} us per train()')
        del arms, groups
        torch.cuda.empty_cache()


def separate_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer, ReplayBuffer
    from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup, ReplayBufferGroup
    R, rows, arms = 4, _rows(np, RING), {}
    for kind, gcls, cls in (('plain', ReplayBufferGroup, ReplayBuffer), ('prioritized critic', CriticPrioritizedReplayBufferGroup, CriticPrioritizedReplayBuffer)):
        g, gb = _ctrl_group(np, R), _filled_group(gcls, rows, R)
        agents, bufs = [], []
        for r in range(R):
            torch.manual_seed(r)
            agents.append(CTRLSACAgent(S, A, _Space(np, A), max_batch=B, seed=r, pipeline=False, **CTRL_KW))
            b = cls(S, A, max_size=RING)
            b.load(*rows)
            bufs.append(b)
        arms[(kind, 'group')] = lambda g=g, gb=gb: g.train(gb, B)
        arms[(kind, 'separate')] = lambda agents=agents, bufs=bufs: [a.train(b, B) for a, b in zip(agents, bufs)]
    us = _windows(torch, arms, args.warmup, max(1, args.calls // 2), args.windows)
    for kind in ('plain', 'prioritized critic'):
        gq, sq = us[(kind, 'group')], us[(kind, 'separate')]
        say(f'ctrlsac_halfcheetah_f256_b256 R = 4 {kind:18s}: one group {_fmt(gq)} per train() of all members; four agents {_fmt(sq)} per round of four '
            f'train(); group = {statistics.median(sq) / statistics.median(gq):.2f} x the separate agents')


def fused_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd._lib import lib, check
    from rlrep_amd.utils.buffer_group import CriticPrioritizedReplayBufferGroup, PrioritizedReplayBufferGroup
    K, rows = args.chain, _rows(np, RING)
    leaves = (1.0 + 99.0 * np.random.default_rng(5).random(RING)).astype(np.float32)
    for R in (4, 16):
        cg, sgp = _ctrl_group(np, R), _sac_group(np, R)
        cb, sb = _filled_group(CriticPrioritizedReplayBufferGroup, rows, R), _filled_group(PrioritizedReplayBufferGroup, rows, R)
        for r in range(R):
            cb.set_priorities(r, leaves, 100.0)
            sb.set_priorities(r, leaves, 100.0)
        for g in (cg, sgp):
            check(lib.rlrep_group_prepare(g.core.h, B), 'group_prepare')          # (sizes the slots for B outside the captures)
        arms = {'fused launch': _chain(torch, lambda: cb.draw_fill(cg.core, B, PER_STREAM, use_counter=True), K),
                'sample + gather': _chain(torch, lambda: sb.draw(B, PER_STREAM, core=sgp.core, use_counter=True, gather=True), K)}
        us = _windows(torch, arms, max(1, args.warmup // K), max(1, args.calls // K), args.windows)
        f, p = [u / K for u in us['fused launch']], [u / K for u in us['sample + gather']]
        say(f'fused R = {R:2d} (S, A) = ({S}, {A}) B = {B} ring {RING}: fused group launch {_fmt(f)}, per_sample_grp + per_gather_grp {_fmt(p)} per repetition '
            f'(chains of {K}); fused / pair = {statistics.median(f) / statistics.median(p):.3f}')
        del arms, cg, sgp, cb, sb
        torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='train,separate,fused')
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: the rates this change must leave alone are measured beside this tree\'s')
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'per_critic_group.txt'))
    p.add_argument('--warmup', type=int, default=200)
    p.add_argument('--calls', type=int, default=1000)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--chain', type=int, default=64)
    args = p.parse_args(argv)
    if args.child:
        print(json.dumps(untouched_rates(args, args.child)))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.parent:                      # (children first: this process has not opened the GPU yet)
        say(f'# untouched rates, child processes alternated ({args.repeats} each): {args.warmup} warm-up calls, median of {args.windows} windows of {args.calls} calls')
        parent_table(args, say)
    np, torch = _setup(ROOT)
    say(f'# {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per arm, median (sorted windows) of {args.windows} windows of {args.calls} calls, '
        'arms alternated in one process')
    only = args.only.split(',')
    if 'train' in only:
        train_table(args, say)
    if 'separate' in only:
        separate_table(args, say)
    if 'fused' in only:
        fused_table(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
