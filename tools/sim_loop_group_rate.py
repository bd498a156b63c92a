"""What one iteration of the one-graph simulator loop costs for a SEED GROUP (SeedBatchMixin.iterate_sim, SimLoopGroup,
FusedSimGroup) -- the sibling of tools/fused_sim_rate.py, same protocol.

    python tools/sim_loop_group_rate.py                         # profiles/sim_loop_group.txt
    python tools/sim_loop_group_rate.py --parent DIR            # ... and the plain train() rates of another (built) checkout, alternated with this one

sac, Pendulum-v1, hidden 256, B = --batch, past warm-up.  For every R of --members and every N of --envs four arms run in ONE process,
alternated:
    group_app   group iterate_sim on a FusedSimGroup, fused-append form (act launch, step-and-append launch, train())
    group_sep   the same with SimLoopGroup(fused_append=False): observation copy, act launch, step launch, append launch, train()
    train       the bare group train() replay
    singles     R single agents, each with its own SimLoop + FusedSim (fused-append), iterated in turn
--warmup calls per arm, --windows windows of --calls calls each, every window closed by a device synchronisation around a host clock; medians
and sorted windows are printed, then iterate_sim - train() of both forms and the ratio group_app : singles.
--parent: the plain single-agent train()/s and the plain group train()/s (R = --parent-members) of the parent's build and of this one, in
child processes run one after the other, --repeats times each, alternated, and which build goes first alternates from one repeat to the next
(with the parent's process always first this build read 0.1 to 1.6 % slower, with the order alternating it did not: docs/history/
sim_loop_group.md); the spread of each build's process medians is printed, and the verdict reads the difference against the PARENT build's
own run-to-run spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = 100000
S, A, BOUND = 3, 1, 2.0
EPS_GREEDY = 0.01


def _setup(root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, 'tools'))
    import numpy as np
    import torch
    return np, torch


class _Space(object):
    def __init__(self, np):
        self.low, self.high = -BOUND * np.ones(A, np.float32), BOUND * np.ones(A, np.float32)


def _single(np, torch, B, seed=0):
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    torch.manual_seed(seed)
    return SACAgent(S, A, _Space(np), max_batch=B, seed=seed, hidden_dim=256)


def _group(np, R, B):
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    return SACSeedBatch(list(range(R)), S, A, _Space(np), max_batch=B, hidden_dim=256)


def _filled_group_rings(torch, R, N):
    """rings that N-row appends have filled, for the bare train()"""
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    bufs = ReplayBufferGroup(R, S, A, max_size=RING)
    gen = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)  # noqa: E731
    for _ in range(4):
        bufs.add_device(rnd(R, N, S), rnd(R, N, A), rnd(R, N, S), rnd(R, N), torch.zeros(R, N, device='cuda'))
    return bufs


class GroupLoop(object):
    """main.py's _fused_sim_group_loop body past warm-up: R members x N FusedSimGroup environments"""

    def __init__(self, np, R, N, B, fused_append):
        from rlrep_amd.envs.fused_sim import FusedSimGroup
        from rlrep_amd.envs.sim_loop import SimLoopGroup
        from rlrep_amd.utils.buffer_group import ReplayBufferGroup
        self.B = B
        self.agent = _group(np, R, B)
        self.replay = ReplayBufferGroup(R, S, A, max_size=RING)
        self.env = FusedSimGroup('Pendulum-v1', R, N, 'cuda', seeds=list(range(R)), group=self.agent)
        self.env.reset()
        self.loop = SimLoopGroup(self.agent, self.env, eps_greedy=EPS_GREEDY, start_timesteps=0, fused_append=fused_append)

    def __call__(self):
        self.agent.iterate_sim(self.loop, self.replay, self.B)


class GroupTrain(object):
    def __init__(self, np, torch, R, N, B):
        self.B = B
        self.agent = _group(np, R, B)
        self.replay = _filled_group_rings(torch, R, N)

    def __call__(self):
        self.agent.train(self.replay, self.B)


class Singles(object):
    """R single agents, each with a SimLoop + FusedSim of its own (fused-append), iterated in turn"""

    def __init__(self, np, torch, R, N, B):
        from rlrep_amd.envs.fused_sim import FusedSim
        from rlrep_amd.envs.sim_loop import SimLoop
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.B, self.members = B, []
        for r in range(R):
            agent = _single(np, torch, B, seed=r)
            env = FusedSim('Pendulum-v1', N, 'cuda', seed=r)
            env.reset()
            self.members.append((agent, SimLoop(agent, env, eps_greedy=EPS_GREEDY, start_timesteps=0), ReplayBuffer(S, A, max_size=RING)))

    def __call__(self):
        for agent, loop, replay in self.members:
            agent.iterate_sim(loop, replay, self.B)


def _rate(v):
    return 1e6 / statistics.median(v)


def plain_rates(args, root):
    """{arm: sorted us per train() of each window} of the untouched paths, importing the package under `root` (a child process's job)"""
    np, torch = _setup(root)
    from host_envs_rate import _windows
    from rlrep_amd.utils.buffer import ReplayBuffer
    R, N = args.parent_members, 256
    agent, buf = _single(np, torch, args.batch), ReplayBuffer(S, A, max_size=RING)
    gen = torch.Generator(device='cuda').manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)  # noqa: E731
    for _ in range(4):
        buf.add_device(rnd(N, S), rnd(N, A), rnd(N, S), rnd(N), torch.zeros(N, device='cuda'))
    grp = GroupTrain(np, torch, R, N, args.batch)
    out = _windows({'single': lambda: agent.train(buf, args.batch), 'group': grp}, args.warmup, args.calls, args.windows)
    out['single/launches'], out['group/launches'] = agent._graph_launches, grp.agent._graph_launches
    return out


def parent_table(args, say):
    rows = {}
    for rep in range(args.repeats):
        pair = (('parent', os.path.abspath(args.parent)), ('this', ROOT))
        for name, root in (pair if rep % 2 == 0 else pair[::-1]):          # (who goes first alternates: neither build always follows an idle GPU)
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, '--warmup', '200', '--calls', '2000', '--windows', str(args.windows),
                   '--batch', str(args.batch), '--parent-members', str(args.parent_members)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
            rows.setdefault(name, []).append(json.loads(res.stdout.strip().splitlines()[-1]))
    for arm, what in (('single', 'plain single-agent train()'), ('group', f'plain group train(), R = {args.parent_members}')):
        spread = {}
        for name in ('parent', 'this'):
            meds = [_rate(r[arm]) for r in rows[name]]
            spread[name] = 100 * (max(meds) - min(meds)) / statistics.median(meds)
            say(f'{what} [{name:6s}] {rows[name][0][arm + "/launches"]} launches: {statistics.median(meds):9.0f} train()/s, process medians '
                f'{", ".join(f"{m:.0f}" for m in meds)} (spread {spread[name]:.2f} %)')
        a, b = statistics.median([_rate(r[arm]) for r in rows['this']]), statistics.median([_rate(r[arm]) for r in rows['parent']])
        d = 100 * (a / b - 1)
        say(f'{what}: this tree / parent = {a / b:.4f} ({d:+.2f} %); run-to-run spread of the parent build {spread["parent"]:.2f} %, of this build '
            f'{spread["this"]:.2f} %: {"within" if abs(d) <= spread["parent"] else "OUTSIDE"} the spread of the parent build'
            + ('' if abs(d) <= spread['parent'] else f' ({"within" if abs(d) <= spread["this"] else "outside"} that of this build)'))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--members', default='4,8,16')
    p.add_argument('--envs', default='256,4096')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=50)
    p.add_argument('--calls', type=int, default=300)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain train() rates are measured beside this tree\'s')
    p.add_argument('--parent-members', type=int, default=8)
    p.add_argument('--repeats', type=int, default=2)
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sim_loop_group.txt'))
    args = p.parse_args(argv)
    if args.child:
        print(json.dumps(plain_rates(args, args.child)))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.parent:                     # (children first: this process has not opened the GPU yet)
        say(f'# untouched paths, child processes alternated ({args.repeats} each): 200 warm-up calls, median of {args.windows} windows of 2000 calls')
        parent_table(args, say)
    np, torch = _setup(ROOT)
    from host_envs_rate import _fmt, _windows
    say(f'# {torch.cuda.get_device_name(0)}; sac Pendulum-v1, hidden 256, B = {args.batch}; {args.warmup} warm-up calls per arm, median (sorted windows) of '
        f'{args.windows} windows of {args.calls} iterations, arms alternated in one process; us per iteration (of all R members)')
    ints = lambda s: [int(v) for v in s.split(',') if v]  # noqa: E731
    for R in ints(args.members):
        for N in ints(args.envs):
            arms = {'group_app': GroupLoop(np, R, N, args.batch, True), 'group_sep': GroupLoop(np, R, N, args.batch, False),
                    'train': GroupTrain(np, torch, R, N, args.batch), 'singles': Singles(np, torch, R, N, args.batch)}
            us = _windows(arms, args.warmup, args.calls, args.windows)
            med = {k: statistics.median(v) for k, v in us.items()}
            tag = f'R = {R:2d} N = {N:5d}'
            say(f'{tag} a) group iterate_sim, FusedSimGroup, fused-append ({arms["group_app"].agent._sim_launches} library launches): {_fmt(us["group_app"])} = '
                f'{R * N * 1e6 / med["group_app"]:11.0f} environment steps/s')
            say(f'{tag} b) group iterate_sim, separate route ({arms["group_sep"].agent._sim_launches} library launches): {_fmt(us["group_sep"])}')
            say(f'{tag} c) bare group train() replay ({arms["train"].agent._graph_launches} library launches): {_fmt(us["train"])}')
            say(f'{tag} d) {R} single agents, SimLoop + FusedSim each, in turn: {_fmt(us["singles"])}')
            say(f'{tag} iterate_sim - train(): fused-append {med["group_app"] - med["train"]:.1f} us; separate {med["group_sep"] - med["train"]:.1f} us; '
                f'a) : d) = {med["group_app"] / med["singles"]:.3f} (the group is {"FASTER" if max(us["group_app"]) < min(us["singles"]) else "not faster"} by more than '
                'the spread of the windows)')
            del arms
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
