"""What one iteration of the one-graph simulator loop costs with a simulator kind compiled at RUN TIME (envs/fused_sim.py CustomFusedSim,
csrc/sim_jit.h) against the built-in fused kind -- tools/fused_sim_rate.py's protocol with one more arm.

    python tools/sim_kind_jit_rate.py                           # profiles/sim_kind_jit.txt
    python tools/sim_kind_jit_rate.py --parent DIR              # ... and the plain train() rate of another (built) checkout, alternated with this one

sac, hidden 256, B = --batch, N = --envs environments, past warm-up, the fused-append form (act launch, step-and-append launch, train()).  For
every N three arms run in ONE process, alternated: `built_in` is iterate_sim on FusedSim('Pendulum-v1'), `jit` the same on the example kind
envs/kinds/pendulum.h compiled at run time, `train` the bare train() replay.  Then the example point mass (S = 4, A = 2) at --pm-envs beside the
train() of its dimensions.  --warmup calls per arm, --windows windows of --calls calls each, every window closed by a device synchronisation
around a host clock; medians and sorted windows are printed.  No ratio is fixed in advance: the yardstick is the built-in arm of the same run,
and "equal within the spread" means that the two arms' windows overlap.  The compile time of both examples (rlrep_sim_kind_compile: hiprtc,
the module load, the attribute queries) and kernel_info() of both are printed with it.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from host_envs_rate import _fmt, _windows  # noqa: E402
from act_device_rate import _sac  # noqa: E402
from sim_loop_rate import RING, TrainOnly  # noqa: E402
from fused_sim_rate import FusedLoop  # noqa: E402


class JitLoop(object):
    """main.py's _fused_sim_loop body past warm-up on N CustomFusedSim environments of a compiled kind"""

    def __init__(self, kind, N, B, eps_greedy):
        from rlrep_amd.envs.fused_sim import CustomFusedSim
        from rlrep_amd.envs.sim_loop import SimLoop
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.N, self.B = N, B
        self.env = CustomFusedSim(kind, N, 'cuda', seed=0)
        S, A = self.env.state_dim, self.env.action_dim
        self.agent = _sac(S, A, B, self.env.action_range[1])
        self.replay = ReplayBuffer(S, A, max_size=RING)
        self.env.reset()
        self.loop = SimLoop(self.agent, self.env, eps_greedy=eps_greedy, start_timesteps=0)
        assert self.loop.fused_append

    def __call__(self):
        self.agent.iterate_sim(self.loop, self.replay, self.B)


class TrainAt(TrainOnly):
    """TrainOnly at other dimensions"""

    def __init__(self, S, A, N, B):
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.B = B
        self.agent = _sac(S, A, B, 1.0)
        self.replay = ReplayBuffer(S, A, max_size=RING)
        gen = torch.Generator(device='cuda').manual_seed(0)
        rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)  # noqa: E731
        for _ in range(4):
            self.replay.add_device(rnd(N, S), rnd(N, A), rnd(N, S), rnd(N), torch.zeros(N, device='cuda'))


def _overlap(a, b):
    return not (max(a) < min(b) or max(b) < min(a))


def main(argv=None):
    from act_device_rate import EPS_GREEDY
    p = argparse.ArgumentParser()
    p.add_argument('--envs', default='256,4096')
    p.add_argument('--pm-envs', default='4096')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=50)
    p.add_argument('--calls', type=int, default=300)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain train()/s is measured beside this tree\'s')
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sim_kind_jit.txt'))
    args = p.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.parent:                     # (children first: this process has not opened the GPU yet)
        import nstep_rate
        pa = argparse.Namespace(parent=args.parent, repeats=args.repeats, warmup=200, calls=2000, windows=5)
        say(f'# plain-buffer train()/s, child processes alternated ({pa.repeats} each): {pa.warmup} warm-up calls, median of {pa.windows} windows of {pa.calls} calls')
        nstep_rate.parent_table(pa, say)
    from rlrep_amd.envs.fused_sim import SimKind, example_kind
    torch.zeros(1, device='cuda')       # (the context exists before the first compile is timed)
    kinds = {}
    for which in ('pendulum', 'point_mass', 'pendulum', 'point_mass'):     # (the second round: the compiler's own start-up is paid)
        t0 = time.perf_counter()
        k = SimKind(example_kind(which))
        say(f'# rlrep_sim_kind_compile {which} ({"first" if which not in kinds else "again"}): {1e3 * (time.perf_counter() - t0):.0f} ms')
        kinds[which] = k
    for which, k in kinds.items():
        say(f'# kernel_info {which}: ' + '; '.join(f'{n} {v["regs"]} registers, {v["scratch_bytes"]} B scratch, {v["lds_bytes"]} B LDS' for n, v in k.info().items()))
    say(f'# {torch.cuda.get_device_name(0)}; sac, hidden 256, B = {args.batch}; {args.warmup} warm-up calls per arm, median (sorted windows) of '
        f'{args.windows} windows of {args.calls} iterations, arms alternated in one process; us per iteration; fused-append form')
    ints = lambda s: [int(v) for v in s.split(',') if v]  # noqa: E731
    for N in ints(args.envs):
        arms = {'built_in': FusedLoop('Pendulum-v1', N, args.batch, EPS_GREEDY, True), 'jit': JitLoop(kinds['pendulum'], N, args.batch, EPS_GREEDY),
                'train': TrainOnly(N, args.batch)}
        us = _windows(arms, args.warmup, args.calls, args.windows)
        med = {k: statistics.median(v) for k, v in us.items()}
        say(f'Pendulum-v1 N = {N:5d} iterate_sim, built-in FusedSim ({arms["built_in"].agent._sim_launches} library launches): {_fmt(us["built_in"])} = '
            f'{N * 1e6 / med["built_in"]:11.0f} environment steps/s')
        say(f'Pendulum-v1 N = {N:5d} iterate_sim, kinds/pendulum.h compiled at run time ({arms["jit"].agent._sim_launches} library launches): {_fmt(us["jit"])} = '
            f'{N * 1e6 / med["jit"]:11.0f} environment steps/s')
        say(f'Pendulum-v1 N = {N:5d} bare train() replay ({arms["train"].agent._graph_launches} library launches): {_fmt(us["train"])}')
        say(f'Pendulum-v1 N = {N:5d} jit / built-in = {med["jit"] / med["built_in"]:.3f}; iterate_sim - train(): built-in {med["built_in"] - med["train"]:.1f} us, jit '
            f'{med["jit"] - med["train"]:.1f} us; the two arms\' windows overlap: {"yes" if _overlap(us["jit"], us["built_in"]) else "NO"}')
        del arms
    for N in ints(args.pm_envs):
        arms = {'jit': JitLoop(kinds['point_mass'], N, args.batch, EPS_GREEDY), 'train': TrainAt(4, 2, N, args.batch)}
        us = _windows(arms, args.warmup, args.calls, args.windows)
        med = {k: statistics.median(v) for k, v in us.items()}
        say(f'point mass  N = {N:5d} iterate_sim, kinds/point_mass.h compiled at run time ({arms["jit"].agent._sim_launches} library launches): {_fmt(us["jit"])} = '
            f'{N * 1e6 / med["jit"]:11.0f} environment steps/s')
        say(f'point mass  N = {N:5d} bare train() replay ({arms["train"].agent._graph_launches} library launches): {_fmt(us["train"])}; iterate_sim - train() = '
            f'{med["jit"] - med["train"]:.1f} us; episodes finished {int(arms["jit"].env.episodes.sum())}')
        del arms
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
