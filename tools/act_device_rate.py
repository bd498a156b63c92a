"""What acting on a device-resident observation batch costs: one `act_device([N, S])` launch against the routes that existed before it, and
the loop of main.py at --torch-envs 256 / 4096 against --host-envs 256.

    python tools/act_device_rate.py                    # both tables
    python tools/act_device_rate.py --only act --rows 16,256,4096,65536

act:  sac at Pendulum dims (S = 3, A = 1) and HalfCheetah dims (S = 17, A = 6), hidden 256, explore on: us per call of `select_actions([N, S])`
      for every N of --select-rows (host rows in pinned buffers, one workgroup per row), of `core.actor_forward` at N = 256 = max_batch (the
      six-launch route on a device batch, with a noise tensor made beforehand), and of `act_device([N, S])` on a device tensor for every N of
      --rows.  Every call is followed by a stream synchronisation, in every arm.
loop: environment steps per second past warm-up, sac B = --batch: --torch-envs N is _torch_envs_loop's body (act_device, TorchPendulum.step,
      add_device, ONE train; nothing in it waits for the device, the window's closing synchronisation does), --host-envs E is
      _host_envs_loop's (select_actions, E NumPy steps, add_batch, ONE train).

All arms of a table run in ONE process, alternated: --warmup calls per arm, then --windows windows of --calls calls each, host wall clock
around a device synchronisation; the median and the sorted windows are printed.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from host_envs_rate import DIMS, EPS_GREEDY, HostLoop, _Space, _fmt, _windows  # noqa: E402


def _sac(S, A, B, bound=1.0):
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    torch.manual_seed(0)
    return SACAgent(S, A, _Space(A, bound), max_batch=B, seed=0, hidden_dim=256)


def act_table(args, rows, select_rows):
    sync = torch.cuda.current_stream().synchronize
    for name, (S, A) in DIMS.items():
        agent = _sac(S, A, 256)
        gen = torch.Generator(device='cuda').manual_seed(0)
        dev = {N: torch.randn(N, S, device='cuda', generator=gen) for N in set(rows) | {256}}
        out = {N: torch.empty(N, A, device='cuda') for N in dev}
        host = {N: np.random.RandomState(N).randn(N, S).astype(np.float32) for N in select_rows}
        eps = torch.randn(256, A, device='cuda', generator=gen)
        lo, hi = agent.action_range

        def forward():
            agent.core.actor_forward(dev[256], eps, lo, hi, out=out[256])
            sync()

        def act(N):
            agent.act_device(dev[N], explore=True, out=out[N])
            sync()
        arms = {('select', N): (lambda N=N: agent.select_actions(host[N], explore=True)) for N in select_rows}
        arms['forward'] = forward
        arms.update({('act', N): (lambda N=N: act(N)) for N in rows})
        us = _windows(arms, args.warmup, args.calls, args.windows)
        for N in select_rows:
            print(f'sac {name} (S = {S}, A = {A}) select_actions N = {N:5d}: {_fmt(us[("select", N)])}', flush=True)
        fwd = statistics.median(us['forward'])
        print(f'sac {name} core.actor_forward N =   256 (six launches): {_fmt(us["forward"])}')
        for N in rows:
            med = statistics.median(us[('act', N)])
            ref = statistics.median(us[('select', N)]) if N in select_rows else None
            print(f'sac {name} act_device N = {N:5d} ({(N + 15) // 16:4d} workgroups): {_fmt(us[("act", N)])}; {1e3 * med / N:8.1f} ns per row'
                  + (f'; {med / ref:.2f} x select_actions' if ref else '') + (f'; {med / fwd:.2f} x actor_forward' if N == 256 else ''), flush=True)
        del agent


class TorchLoop(object):
    """main.py's _torch_envs_loop body past warm-up on N TorchPendulum environments"""

    def __init__(self, N, B):
        from rlrep_amd.envs.torch_pendulum import TorchPendulum
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.N, self.B = N, B
        self.agent = _sac(3, 1, B, 2.0)
        self.replay = ReplayBuffer(3, 1, max_size=100000)
        self.env = TorchPendulum(N, 'cuda', seed=0)
        self.gen = torch.Generator(device='cuda').manual_seed(0)
        self.obs = self.env.reset()

    def __call__(self):
        N = self.N
        lo, hi = self.agent.action_range
        uniform = lo + (hi - lo) * torch.rand(N, 1, dtype=torch.float32, device='cuda', generator=self.gen)
        pick = torch.rand(N, 1, dtype=torch.float32, device='cuda', generator=self.gen) < EPS_GREEDY
        actions = torch.where(pick, uniform, self.agent.act_device(self.obs, explore=True))
        nexts, rewards, dones = self.env.step(actions)
        self.replay.add_device(self.obs, actions, nexts, rewards, dones)
        self.obs = self.env.obs
        self.agent.train(self.replay, self.B)


def loop_table(args, torch_envs, host_envs):
    arms = {('torch', N): TorchLoop(N, args.batch) for N in torch_envs}
    arms.update({('host', E): HostLoop(E, args.batch) for E in host_envs})
    us = _windows(arms, args.warmup, args.loop_calls, args.windows)
    for (kind, N), v in us.items():
        med = statistics.median(v)
        print(f'sac Pendulum-v1 B = {args.batch} loop --{kind}-envs {N:5d}: {_fmt(v)} per iteration = {N * 1e6 / med:11.0f} environment steps/s, '
              f'{1e6 / med:7.0f} train()/s', flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='act,loop')
    p.add_argument('--rows', default='16,256,4096,65536', help='N of the act_device arms')
    p.add_argument('--select-rows', default='16,64,256', help='N of the select_actions arms')
    p.add_argument('--torch-envs', default='256,4096')
    p.add_argument('--host-envs', default='256')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=50)
    p.add_argument('--calls', type=int, default=300)
    p.add_argument('--loop-calls', type=int, default=300)
    p.add_argument('--windows', type=int, default=5)
    args = p.parse_args(argv)
    ints = lambda s: [int(v) for v in s.split(',') if v]  # noqa: E731
    print(f'# {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per arm, median (sorted windows) of {args.windows} windows of {args.calls} '
          f'calls, arms alternated in one process; every act arm synchronises its stream after every call', flush=True)
    only = args.only.split(',')
    if 'act' in only:
        act_table(args, ints(args.rows), ints(args.select_rows))
    if 'loop' in only:
        loop_table(args, ints(args.torch_envs), ints(args.host_envs))


if __name__ == '__main__':
    main()
