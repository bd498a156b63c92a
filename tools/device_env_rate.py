"""Iterations/s of a seed group's environment loop on the host against the device loop, and one evaluation by either.

    python tools/device_env_rate.py --alg sac --members 4,8,16
    python tools/device_env_rate.py --alg ctrlsac --members 4,8,16
    python tools/device_env_rate.py --alg sac --env MountainCarContinuous-v0 --calls 300

Host loop: the body of main.py run_seeds past warm-up -- group select_action (one launch, one synchronisation), R NumPy environment steps (--env: Pendulum-v1 or MountainCarContinuous-v0) and
the epsilon-greedy draws in a Python loop, ReplayBufferGroup.add, train().  Device loop: SeedBatchMixin.iterate (rlrep_amd/envs/device.py):
one graph replay.  Both on groups of the same seeds and shapes (sac: hidden 256; ctrlsac: F = 256, hidden 256; the environment's dims, B = 64), in ONE
process, arms alternated: --warmup iterations per arm, then --windows windows of --calls iterations each, host wall clock around a device
synchronisation; median and min .. max of the windows.  Also the group's bare train() (the floor of either loop) in the same alternation.
Evaluation: util.eval_policy per member (as run_seeds scores) against SeedBatchMixin.evaluate, --eval-episodes episodes, median of --eval-repeats.

    python tools/device_env_rate.py --single --alg vlsac --batch 256 --calls 300

--single: ONE agent of --alg (sac, vlsac, ctrlsac, spedersac, diffsrsac; widths 256) instead of a group.  Host loop: the body of main.py run()
past warm-up (select_action, NumPy step, ReplayBuffer.add, train() in the form the agent picks).  Device loop: SACAgent.iterate.  Bare train():
the ONE-GRAPH train() (an agent built with pipeline=False) on a ring a device loop filled.  The same alternation and windows; one evaluation
by util.eval_policy against SACAgent.evaluate.

    python tools/device_env_rate.py --alg sac --members 4 --num-envs 1,4,16,64
    python tools/device_env_rate.py --single --alg vlsac --batch 256 --num-envs 1,4,16,64 --calls 300

--num-envs E1,E2,...: the device loop with E environments per member / agent (DeviceEnvGroup / DeviceEnv num_envs) for every E of the list and
the bare train(), arms alternated in the same windows: us per iterate, iterate - train(), environment steps per second per member (E per
iterate) and the spread of the windows.  No host loop and no evaluation in this form.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EPS_GREEDY = 0.01


ENV = 'Pendulum-v1'          # --env


def _dims():
    from rlrep_amd import envs
    e = envs.make(ENV)
    return e.observation_space.shape[0], e.action_space.shape[0], e.action_space, e._max_episode_steps


def _group(alg, seeds, B):
    S, A, space, _ = _dims()
    if alg == 'sac':
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
        return SACSeedBatch(seeds, S, A, space, max_batch=B, hidden_dim=256)
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    return CTRLSACSeedBatch(seeds, S, A, space, max_batch=B, hidden_dim=256, feature_dim=256, extra_feature_steps=3)


class HostLoop(object):
    """run_seeds' loop body (main.py), all members live, past warm-up"""

    def __init__(self, alg, seeds, B):
        from rlrep_amd import envs
        from rlrep_amd.utils.buffer_group import ReplayBufferGroup
        self.R, self.B = len(seeds), B
        self.agent = _group(alg, seeds, B)
        S, A, space, self.limit = _dims()
        self.replay = ReplayBufferGroup(self.R, S, A, max_size=100000)
        self.envs = [envs.make(ENV) for _ in seeds]
        for s, e in zip(seeds, self.envs):
            e.seed(s)
        self.rngs = [np.random.RandomState(s) for s in seeds]
        self.states = np.stack([np.asarray(e.reset(), np.float32) for e in self.envs])
        self.ep_steps = np.zeros(self.R, np.int64)
        self.lo, self.hi = np.float32(space.low[0]), np.float32(space.high[0])

    def step(self):
        R = self.R
        self.ep_steps += 1
        greedy = self.agent.select_action(self.states, explore=True)
        actions = np.zeros((R, 1), np.float32)
        for r in range(R):
            actions[r] = self.rngs[r].uniform(self.lo, self.hi) if self.rngs[r].uniform(0, 1) < EPS_GREEDY else greedy[r]
        nexts, rewards, dones = np.zeros_like(self.states), np.zeros(R, np.float32), np.zeros(R, np.float32)
        resets = []
        for r, e in enumerate(self.envs):
            ns, rew, done, _ = e.step(actions[r])
            nexts[r], rewards[r] = ns, rew
            dones[r] = float(done) if self.ep_steps[r] < self.limit else 0.0
            if done:
                resets.append(r)
        self.replay.add(self.states, actions, nexts, rewards, dones)
        self.states = nexts.copy()
        for r in resets:
            self.states[r] = self.envs[r].reset()
            self.ep_steps[r] = 0
        self.agent.train(self.replay, self.B)


class DeviceLoop(object):
    def __init__(self, alg, seeds, B, num_envs=1):
        from rlrep_amd.envs.device import device_class
        from rlrep_amd.utils.buffer_group import ReplayBufferGroup
        self.R, self.B = len(seeds), B
        self.agent = _group(alg, seeds, B)
        S, A, _, _ = _dims()
        self.replay = ReplayBufferGroup(self.R, S, A, max_size=100000)
        self.env = device_class(ENV)(self.agent, eps_greedy=EPS_GREEDY, start_timesteps=0, num_envs=num_envs)

    def step(self):
        self.agent.iterate(self.env, self.replay, self.B)


class TrainOnly(object):
    """the group's bare train() on a ring a device loop filled: what either loop cannot go below"""

    def __init__(self, alg, seeds, B):
        d = DeviceLoop(alg, seeds, B)
        for _ in range(256):
            d.agent.iterate(d.env, d.replay, B, train=False)
        self.agent, self.replay, self.B = d.agent, d.replay, B

    def step(self):
        self.agent.train(self.replay, self.B)


def _single(alg, B, **extra):
    S, A, space, _ = _dims()
    kw = dict(max_batch=B, seed=0, hidden_dim=256)
    if alg == 'sac':
        from rlrep_amd.agent.sac.sac_agent import SACAgent as cls
    elif alg == 'vlsac':
        from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent as cls
        kw.update(feature_dim=256, extra_feature_steps=3)
    elif alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent as cls
        kw.update(feature_dim=256, extra_feature_steps=3)
    elif alg == 'spedersac':
        from rlrep_amd.agent.spedersac.spedersac_agent import SPEDERSACAgent as cls
        kw.update(phi_and_mu_lr=1e-5, phi_hidden_dim=256, phi_hidden_depth=1, mu_hidden_dim=256, mu_hidden_depth=0, critic_and_actor_lr=3e-4,
                  critic_and_actor_hidden_dim=256, feature_dim=256, extra_feature_steps=5)
    else:
        from rlrep_amd.agent.diffsrsac.diffsrsac_agent import DIFFSRSACAgent as cls
        kw.update(feature_dim=256, extra_feature_steps=3)
    kw.update(extra)
    torch.manual_seed(0)
    return cls(S, A, space, **kw)


class SingleHostLoop(object):
    """run()'s loop body (main.py), past warm-up"""

    def __init__(self, alg, B):
        from rlrep_amd import envs
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.B = B
        self.agent = _single(alg, B)
        S, A, space, self.limit = _dims()
        self.replay = ReplayBuffer(S, A, max_size=100000)
        self.env = envs.make(ENV)
        self.env.seed(0)
        self.rng = np.random.RandomState(0)
        self.space = space
        self.state, self.ep_steps = self.env.reset(), 0

    def step(self):
        self.ep_steps += 1
        if self.rng.uniform(0, 1) < EPS_GREEDY:
            action = self.space.sample()
        else:
            action = self.agent.select_action(self.state, explore=True)
        nxt, rew, done, _ = self.env.step(action)
        self.replay.add(self.state, action, nxt, rew, float(done) if self.ep_steps < self.limit else 0)
        self.state = nxt
        self.agent.train(self.replay, self.B)
        if done:
            self.state, self.ep_steps = self.env.reset(), 0


class SingleDeviceLoop(object):
    def __init__(self, alg, B, num_envs=1, **extra):
        from rlrep_amd.envs.device import single_device_class
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.B = B
        self.agent = _single(alg, B, **extra)
        S, A, _, _ = _dims()
        self.replay = ReplayBuffer(S, A, max_size=100000)
        self.env = single_device_class(ENV)(self.agent, eps_greedy=EPS_GREEDY, start_timesteps=0, num_envs=num_envs)

    def step(self):
        self.agent.iterate(self.env, self.replay, self.B)


class SingleTrainOnly(object):
    """the agent's bare ONE-GRAPH train() on a ring a device loop filled: what iterate() adds its step launch to"""

    def __init__(self, alg, B):
        d = SingleDeviceLoop(alg, B, pipeline=False)
        for _ in range(256):
            d.agent.iterate(d.env, d.replay, B, train=False)
        self.agent, self.replay, self.B = d.agent, d.replay, B

    def step(self):
        self.agent.train(self.replay, self.B)


def single_main(args):
    from rlrep_amd.utils import util
    from rlrep_amd import envs
    alg, B = args.alg, args.batch
    print(f'# {torch.cuda.get_device_name(0)}; single agent, {alg} {ENV} B = {B}; {args.warmup} warm-up iterations, median (min .. max) of '
          f'{args.windows} windows of {args.calls} iterations, arms alternated in one process')
    arms = {'host': SingleHostLoop(alg, B), 'device': SingleDeviceLoop(alg, B), 'train': SingleTrainOnly(alg, B)}
    rates = _windows(arms, args.warmup, args.calls, args.windows)
    med = {k: statistics.median(v) for k, v in rates.items()}
    for k in ('host', 'device', 'train'):
        what = {'host': 'host loop  (select_action, NumPy step, add, train)', 'device': 'device loop (iterate: one graph replay)      ',
                'train': 'bare one-graph train()                       '}[k]
        us = sorted(1e6 / r for r in rates[k])
        print(f'{alg} single {what}: {med[k]:9.1f} iterations/s ({min(rates[k]):.1f} .. {max(rates[k]):.1f}) = {1e6 / med[k]:7.1f} us '
              f'(windows {", ".join(f"{u:.1f}" for u in us)})')
    print(f'{alg} single iterate / host loop: {med["device"] / med["host"]:.2f}x; iterate period - train() period: '
          f'{1e6 / med["device"] - 1e6 / med["train"]:.1f} us; iterate graph: {arms["device"].agent._iter_launches} launches')
    host, dev = arms['host'], arms['device']
    ev = envs.make(ENV)
    th, td = [], []
    for _ in range(args.eval_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        util.eval_policy(host.agent, ev, args.eval_episodes)
        th.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.agent.evaluate(dev.env, args.eval_episodes)
        td.append(time.perf_counter() - t0)
    mh, md = statistics.median(th), statistics.median(td)
    print(f'{alg} single one evaluation ({args.eval_episodes} episodes): util.eval_policy {1e3 * mh:.1f} ms, evaluate {1e3 * md:.2f} ms ({mh / md:.0f}x)', flush=True)


def num_envs_main(args):
    """--num-envs: iterate at every E of the list against the bare train(), one table per group size (or for the single agent)"""
    Es = [int(v) for v in args.num_envs.split(',')]
    alg, B = args.alg, args.batch
    print(f'# {torch.cuda.get_device_name(0)}; {alg} {ENV} B = {B}; {args.warmup} warm-up iterations, median (min .. max) of '
          f'{args.windows} windows of {args.calls} iterations, arms alternated in one process')
    for R in ([None] if args.single else [int(v) for v in args.members.split(',')]):
        if R is None:
            arms = {'train': SingleTrainOnly(alg, B)}
            arms.update({E: SingleDeviceLoop(alg, B, num_envs=E) for E in Es})
            tag = f'{alg} single'
        else:
            seeds = list(range(R))
            arms = {'train': TrainOnly(alg, seeds, B)}
            arms.update({E: DeviceLoop(alg, seeds, B, num_envs=E) for E in Es})
            tag = f'{alg} R={R:2d}'
        rates = _windows(arms, args.warmup, args.calls, args.windows)
        us = {k: sorted(1e6 / r for r in v) for k, v in rates.items()}
        med = {k: statistics.median(v) for k, v in us.items()}
        print(f'{tag} bare {"one-graph " if R is None else ""}train(): {med["train"]:8.1f} us (windows {", ".join(f"{u:.1f}" for u in us["train"])})')
        for E in Es:
            print(f'{tag} num_envs {E:2d}: iterate {med[E]:8.1f} us (windows {", ".join(f"{u:.1f}" for u in us[E])}); iterate - train() '
                  f'{med[E] - med["train"]:6.1f} us; {E * 1e6 / med[E]:9.0f} environment steps/s per member; graph: '
                  f'{arms[E].agent._iter_launches} launches, step grid {E} x {R or 1} workgroups', flush=True)
        del arms


def _windows(arms, warmup, calls, windows):
    for a in arms.values():
        for _ in range(warmup):
            a.step()
    torch.cuda.synchronize()
    rates = {k: [] for k in arms}
    for _ in range(windows):
        for k, a in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                a.step()
            torch.cuda.synchronize()
            rates[k].append(calls / (time.perf_counter() - t0))
    return rates


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--alg', default='sac', choices=['sac', 'ctrlsac', 'vlsac', 'spedersac', 'diffsrsac'])
    p.add_argument('--single', action='store_true', help='one agent (any --alg) instead of a seed group')
    p.add_argument('--members', default='4,8,16')
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=300)
    p.add_argument('--calls', type=int, default=400)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--eval-episodes', type=int, default=10)
    p.add_argument('--eval-repeats', type=int, default=3)
    p.add_argument('--env', default='Pendulum-v1', choices=['Pendulum-v1', 'MountainCarContinuous-v0'])
    p.add_argument('--num-envs', default=None, help='comma-separated environments per member / agent: the device loop at each against the bare train()')
    args = p.parse_args(argv)
    global ENV
    ENV = args.env
    if args.num_envs is not None:
        if not args.single and args.alg not in ('sac', 'ctrlsac'):
            raise SystemExit(f'--alg {args.alg}: seed groups are built for sac and ctrlsac (give --single)')
        return num_envs_main(args)
    if args.single:
        return single_main(args)
    if args.alg not in ('sac', 'ctrlsac'):
        raise SystemExit(f'--alg {args.alg}: seed groups are built for sac and ctrlsac (give --single)')
    from rlrep_amd.utils import util
    from rlrep_amd.main import _MemberPolicy
    from rlrep_amd import envs
    print(f'# {torch.cuda.get_device_name(0)}; {args.alg} {ENV} B = {args.batch}; {args.warmup} warm-up iterations, median (min .. max) of '
          f'{args.windows} windows of {args.calls} iterations, arms alternated in one process')
    for R in [int(v) for v in args.members.split(',')]:
        seeds = list(range(R))
        arms = {'host': HostLoop(args.alg, seeds, args.batch), 'device': DeviceLoop(args.alg, seeds, args.batch),
                'train': TrainOnly(args.alg, seeds, args.batch)}
        rates = _windows(arms, args.warmup, args.calls, args.windows)
        med = {k: statistics.median(v) for k, v in rates.items()}
        for k in ('host', 'device', 'train'):
            what = {'host': 'host loop  (select_action, NumPy step, add, train)', 'device': 'device loop (iterate: one graph replay)      ',
                    'train': 'bare train() of the group                    '}[k]
            print(f'{args.alg} R={R:2d} {what}: {med[k]:9.1f} iterations/s ({min(rates[k]):.1f} .. {max(rates[k]):.1f}) = {1e6 / med[k]:7.1f} us')
        print(f'{args.alg} R={R:2d} iterate / host loop: {med["device"] / med["host"]:.2f}x; iterate period - train() period: '
              f'{1e6 / med["device"] - 1e6 / med["train"]:.1f} us')
        # one evaluation of every member
        host, dev = arms['host'], arms['device']
        policies = [_MemberPolicy(host.agent, r) for r in range(R)]
        evals = [envs.make(ENV) for _ in seeds]
        th, td = [], []
        for _ in range(args.eval_repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for r in range(R):
                util.eval_policy(policies[r], evals[r], args.eval_episodes)
            th.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dev.agent.evaluate(dev.env, args.eval_episodes)
            td.append(time.perf_counter() - t0)
        mh, md = statistics.median(th), statistics.median(td)
        print(f'{args.alg} R={R:2d} one evaluation ({args.eval_episodes} episodes x {R} members): util.eval_policy {1e3 * mh:.1f} ms, evaluate {1e3 * md:.2f} ms '
              f'({mh / md:.0f}x)', flush=True)
        del arms, host, dev, policies


if __name__ == '__main__':
    main()
