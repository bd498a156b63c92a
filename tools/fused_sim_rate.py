"""What one iteration of the one-graph simulator loop costs with a FUSED simulator (envs/fused_sim.py) against the arms of
tools/sim_loop_rate.py -- the sibling of that tool, same protocol.

    python tools/fused_sim_rate.py                              # profiles/fused_sim.txt
    python tools/fused_sim_rate.py --parent DIR                 # ... and the plain train() rate of another (built) checkout, alternated with this one

sac, hidden 256, B = --batch, N = --envs environments, past warm-up.  For every N five arms run in ONE process, alternated: `eager`, `graph`
and `train` are sim_loop_rate.py's (the eager loop body of --torch-envs, iterate_sim on a TorchPendulum(capturable=True), the bare train()
replay); `fused_sep` is iterate_sim on a FusedPendulum with SimLoop(fused_append=False) -- observation copy, act launch, step launch, append
launch -- and `fused_app` the same with the step-and-append launch: act launch, step-and-append launch.  Then MountainCarContinuous-v0 at
--mc-envs: the two fused arms and train().  --warmup calls per arm, --windows windows of --calls calls each, every window closed by a device
synchronisation around a host clock; medians and sorted windows are printed.  "beats by more than the spread": the slower arm's fastest
window is slower than the faster arm's slowest window.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from host_envs_rate import _fmt, _windows  # noqa: E402
from act_device_rate import TorchLoop, _sac  # noqa: E402
from sim_loop_rate import RING, GraphLoop, TrainOnly  # noqa: E402

DIMS = {'Pendulum-v1': (3, 1, 2.0), 'MountainCarContinuous-v0': (2, 1, 1.0)}


class FusedLoop(object):
    """main.py's _fused_sim_loop body past warm-up on N FusedSim environments of `env_name`"""

    def __init__(self, env_name, N, B, eps_greedy, fused_append):
        from rlrep_amd.envs.fused_sim import FusedSim
        from rlrep_amd.envs.sim_loop import SimLoop
        from rlrep_amd.utils.buffer import ReplayBuffer
        S, A, bound = DIMS[env_name]
        self.N, self.B = N, B
        self.agent = _sac(S, A, B, bound)
        self.replay = ReplayBuffer(S, A, max_size=RING)
        self.env = FusedSim(env_name, N, 'cuda', seed=0)
        self.env.reset()
        self.loop = SimLoop(self.agent, self.env, eps_greedy=eps_greedy, start_timesteps=0, fused_append=fused_append)

    def __call__(self):
        self.agent.iterate_sim(self.loop, self.replay, self.B)


class TrainDims(TrainOnly):
    """TrainOnly at other dimensions"""

    def __init__(self, env_name, N, B):
        from rlrep_amd.utils.buffer import ReplayBuffer
        S, A, bound = DIMS[env_name]
        self.B = B
        self.agent = _sac(S, A, B, bound)
        self.replay = ReplayBuffer(S, A, max_size=RING)
        gen = torch.Generator(device='cuda').manual_seed(0)
        rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)  # noqa: E731
        for _ in range(4):
            self.replay.add_device(rnd(N, S), rnd(N, A), rnd(N, S), rnd(N), torch.zeros(N, device='cuda'))


def _beats(fast, slow):
    """`fast` beats `slow` by more than the spread of their own windows (sorted us per window)"""
    return max(fast) < min(slow)


def main(argv=None):
    from act_device_rate import EPS_GREEDY
    p = argparse.ArgumentParser()
    p.add_argument('--envs', default='256,4096')
    p.add_argument('--mc-envs', default='4096')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=50)
    p.add_argument('--calls', type=int, default=300)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain train()/s is measured beside this tree\'s')
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fused_sim.txt'))
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
    say(f'# {torch.cuda.get_device_name(0)}; sac, hidden 256, B = {args.batch}; {args.warmup} warm-up calls per arm, median (sorted windows) of '
        f'{args.windows} windows of {args.calls} iterations, arms alternated in one process; us per iteration')
    ok = True
    ints = lambda s: [int(v) for v in s.split(',') if v]  # noqa: E731
    for N in ints(args.envs):
        arms = {'eager': TorchLoop(N, args.batch), 'graph': GraphLoop(N, args.batch, EPS_GREEDY),
                'fused_sep': FusedLoop('Pendulum-v1', N, args.batch, EPS_GREEDY, False), 'fused_app': FusedLoop('Pendulum-v1', N, args.batch, EPS_GREEDY, True),
                'train': TrainOnly(N, args.batch)}
        us = _windows(arms, args.warmup, args.calls, args.windows)
        med = {k: statistics.median(v) for k, v in us.items()}
        t = med['train']
        say(f'Pendulum-v1 N = {N:5d} eager loop body (act_device, torch mix, step, add_device, train()): {_fmt(us["eager"])}')
        say(f'Pendulum-v1 N = {N:5d} iterate_sim, TorchPendulum(capturable=True) ({arms["graph"].agent._sim_launches} library launches): {_fmt(us["graph"])}')
        say(f'Pendulum-v1 N = {N:5d} iterate_sim, FusedSim, separate form ({arms["fused_sep"].agent._sim_launches} library launches): {_fmt(us["fused_sep"])} = '
            f'{N * 1e6 / med["fused_sep"]:11.0f} environment steps/s')
        say(f'Pendulum-v1 N = {N:5d} iterate_sim, FusedSim, fused-append form ({arms["fused_app"].agent._sim_launches} library launches): {_fmt(us["fused_app"])} = '
            f'{N * 1e6 / med["fused_app"]:11.0f} environment steps/s')
        say(f'Pendulum-v1 N = {N:5d} bare train() replay ({arms["train"].agent._graph_launches} library launches): {_fmt(us["train"])}')
        say(f'Pendulum-v1 N = {N:5d} iterate_sim - train(): torch simulator {med["graph"] - t:.1f} us; separate form {med["fused_sep"] - t:.1f} us; fused-append form '
            f'{med["fused_app"] - t:.1f} us; eager - train() = {med["eager"] - t:.1f} us')
        say(f'Pendulum-v1 N = {N:5d} torch-simulator graph / separate = {med["graph"] / med["fused_sep"]:.2f}; / fused-append = {med["graph"] / med["fused_app"]:.2f}; eager / '
            f'separate = {med["eager"] / med["fused_sep"]:.2f}; / fused-append = {med["eager"] / med["fused_app"]:.2f}; separate / fused-append = '
            f'{med["fused_sep"] / med["fused_app"]:.3f}')
        checks = {f'{a} beats the torch-simulator graph': _beats(us[a], us['graph']) for a in ('fused_sep', 'fused_app')}
        if N >= 4096:
            checks.update({f'{a} beats the eager loop': _beats(us[a], us['eager']) for a in ('fused_sep', 'fused_app')})
        checks['(reported either way) fused_app beats fused_sep'] = _beats(us['fused_app'], us['fused_sep'])
        for what, v in checks.items():
            say(f'Pendulum-v1 N = {N:5d} by more than the spread of the windows: {what}: {"yes" if v else "NO"}')
            ok = ok and (v or what.startswith('('))
        del arms
    for N in ints(args.mc_envs):
        name = 'MountainCarContinuous-v0'
        arms = {'fused_sep': FusedLoop(name, N, args.batch, EPS_GREEDY, False), 'fused_app': FusedLoop(name, N, args.batch, EPS_GREEDY, True),
                'train': TrainDims(name, N, args.batch)}
        us = _windows(arms, args.warmup, args.calls, args.windows)
        med = {k: statistics.median(v) for k, v in us.items()}
        say(f'{name} N = {N:5d} iterate_sim, FusedSim, separate form ({arms["fused_sep"].agent._sim_launches} library launches): {_fmt(us["fused_sep"])}')
        say(f'{name} N = {N:5d} iterate_sim, FusedSim, fused-append form ({arms["fused_app"].agent._sim_launches} library launches): {_fmt(us["fused_app"])}')
        say(f'{name} N = {N:5d} bare train() replay ({arms["train"].agent._graph_launches} library launches): {_fmt(us["train"])}')
        say(f'{name} N = {N:5d} iterate_sim - train(): separate form {med["fused_sep"] - med["train"]:.1f} us; fused-append form {med["fused_app"] - med["train"]:.1f} us; '
            f'separate / fused-append = {med["fused_sep"] / med["fused_app"]:.3f}; episodes finished {int(arms["fused_app"].env.episodes.sum())}')
        del arms
    say(f'# condition (both fused arms beat the torch-simulator graph at every N and the eager loop at N >= 4096): {"met" if ok else "NOT met"}')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
