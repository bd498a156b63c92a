"""What one iteration of the torch-simulator loop costs as ONE graph replay (`SACAgent.iterate_sim`) against the eager loop body of
main.py --torch-envs (act_device, the torch exploration mix, TorchPendulum.step, add_device, train()) and against the bare train() replay.

    python tools/sim_loop_rate.py                               # profiles/sim_loop.txt
    python tools/sim_loop_rate.py --parent DIR                  # ... and the plain train() rate of another (built) checkout, alternated with this one

sac at Pendulum dims, hidden 256, B = --batch, N = --envs environments, past warm-up.  For every N three arms run in ONE process,
alternated: `eager` is _torch_envs_loop's body (tools/act_device_rate.py TorchLoop), `graph` one iterate_sim on a
TorchPendulum(capturable=True), `train` the bare train() on a ring filled beforehand.  Nothing inside an arm waits for the device; every
window closes with a device synchronisation around a host clock: --warmup calls per arm, then --windows windows of --calls calls each;
medians and sorted windows are printed.  --parent: nstep_rate.py's child processes (plain-buffer train()/s of the other checkout and of this
one, alternated), to show that train() itself has not moved.
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

RING = 100000


class GraphLoop(object):
    """main.py's _sim_graph_loop body past warm-up on N capturable TorchPendulum environments"""

    def __init__(self, N, B, eps_greedy):
        from rlrep_amd.envs.sim_loop import SimLoop
        from rlrep_amd.envs.torch_pendulum import TorchPendulum
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.N, self.B = N, B
        self.agent = _sac(3, 1, B, 2.0)
        self.replay = ReplayBuffer(3, 1, max_size=RING)
        self.env = TorchPendulum(N, 'cuda', seed=0, capturable=True)
        self.env.reset()
        self.loop = SimLoop(self.agent, self.env, eps_greedy=eps_greedy, start_timesteps=0)

    def __call__(self):
        self.agent.iterate_sim(self.loop, self.replay, self.B)


class TrainOnly(object):
    """the bare train() replay on a ring that N-row appends have filled"""

    def __init__(self, N, B):
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.B = B
        self.agent = _sac(3, 1, B, 2.0)
        self.replay = ReplayBuffer(3, 1, max_size=RING)
        gen = torch.Generator(device='cuda').manual_seed(0)
        rnd = lambda *shape: torch.randn(*shape, device='cuda', generator=gen)  # noqa: E731
        for _ in range(4):
            self.replay.add_device(rnd(N, 3), rnd(N, 1), rnd(N, 3), rnd(N), torch.zeros(N, device='cuda'))

    def __call__(self):
        self.agent.train(self.replay, self.B)


def main(argv=None):
    from act_device_rate import EPS_GREEDY
    p = argparse.ArgumentParser()
    p.add_argument('--envs', default='256,4096')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=50)
    p.add_argument('--calls', type=int, default=300)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain train()/s is measured beside this tree\'s')
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sim_loop.txt'))
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
    say(f'# {torch.cuda.get_device_name(0)}; sac Pendulum-v1 dims, hidden 256, B = {args.batch}; {args.warmup} warm-up calls per arm, median (sorted '
        f'windows) of {args.windows} windows of {args.calls} iterations, arms alternated in one process; us per iteration')
    for N in [int(v) for v in args.envs.split(',') if v]:
        arms = {'eager': TorchLoop(N, args.batch), 'graph': GraphLoop(N, args.batch, EPS_GREEDY), 'train': TrainOnly(N, args.batch)}
        us = _windows(arms, args.warmup, args.calls, args.windows)
        e, g, t = (statistics.median(us[k]) for k in ('eager', 'graph', 'train'))
        say(f'N = {N:5d} eager loop body (act_device, torch mix, step, add_device, train()): {_fmt(us["eager"])} = {N * 1e6 / e:11.0f} environment steps/s')
        say(f'N = {N:5d} iterate_sim, one graph replay ({arms["graph"].agent._sim_launches} library launches): {_fmt(us["graph"])} = {N * 1e6 / g:11.0f} environment steps/s')
        say(f'N = {N:5d} bare train() replay ({arms["train"].agent._graph_launches} library launches): {_fmt(us["train"])}')
        say(f'N = {N:5d} eager / iterate_sim = {e / g:.2f}; iterate_sim - train() = {g - t:.1f} us; eager - train() = {e - t:.1f} us')
        del arms
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
