"""What acting for E host environments costs: one `select_actions(E)` launch against `select_action` and against E of them, and the host loop
of main.py at --host-envs 1, 4, 16.

    python tools/host_envs_rate.py                    # all three tables
    python tools/host_envs_rate.py --only act --rows 1,4,16,64,256

act:   sac at Pendulum dims (S = 3, A = 1) and HalfCheetah dims (S = 17, A = 6), hidden 256, with and without `explore`: us per call of
       `select_action` (the baseline: the existing entry point, in the same process), of E x `select_action`, and of `select_actions([E, S])`
       for every E of --rows.  Every call includes its stream synchronisation, as the environment loop pays it.
group: the sac seed group of --members members at Pendulum dims: `select_action([R, S])`, E x that, `select_actions([R, E, S])`, explore on.
loop:  environment steps per second of main.py's loop body past warm-up, sac B = --batch on the NumPy Pendulum: --host-envs 1 is run()'s body
       (select_action, step, add, train), --host-envs E > 1 is _host_envs_loop's (select_actions, E steps, add_batch, ONE train).

All arms of a table run in ONE process, alternated: --warmup calls per arm, then --windows windows of --calls calls each, host wall clock
around a device synchronisation; the median and the sorted windows are printed.
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
DIMS = {'pendulum': (3, 1), 'halfcheetah': (17, 6)}


class _Space(object):
    def __init__(self, A, bound):
        self.low, self.high = -bound * np.ones(A, np.float32), bound * np.ones(A, np.float32)


def _sac(S, A, B=64, bound=1.0):
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    torch.manual_seed(0)
    return SACAgent(S, A, _Space(A, bound), max_batch=B, seed=0, hidden_dim=256)


def _windows(arms, warmup, calls, windows):
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
    return f'{statistics.median(v):8.1f} us ({", ".join(f"{u:.1f}" for u in v)})'


def act_table(args, rows):
    for name, (S, A) in DIMS.items():
        agent = _sac(S, A)
        rng = np.random.RandomState(0)
        obs = {E: rng.randn(E, S).astype(np.float32) for E in rows}
        for explore in (False, True):
            arms = {'single': lambda: agent.select_action(obs[rows[0]][0], explore=explore)}
            for E in rows:
                arms[('loop', E)] = lambda E=E: [agent.select_action(o, explore=explore) for o in obs[E]]
                arms[('vec', E)] = lambda E=E: agent.select_actions(obs[E], explore=explore)
            us = _windows(arms, args.warmup, args.calls, args.windows)
            base = statistics.median(us['single'])
            print(f'sac {name} (S = {S}, A = {A}) explore={int(explore)} select_action: {_fmt(us["single"])}')
            for E in rows:
                loop, vec = statistics.median(us[('loop', E)]), statistics.median(us[('vec', E)])
                print(f'sac {name} explore={int(explore)} E = {E:3d}: E x select_action {_fmt(us[("loop", E)])}; select_actions {_fmt(us[("vec", E)])}; '
                      f'= {vec / base:.2f} x one select_action, {loop / vec:.1f}x faster than E calls, {vec / E:.2f} us per row', flush=True)
        del agent


def group_table(args, rows):
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    R, (S, A) = args.members, DIMS['pendulum']
    grp = SACSeedBatch(list(range(R)), S, A, _Space(A, 2.0), max_batch=64, hidden_dim=256)
    rng = np.random.RandomState(0)
    obs = {E: rng.randn(R, E, S).astype(np.float32) for E in rows}
    arms = {'single': lambda: grp.select_action(obs[rows[0]][:, 0], explore=True)}
    for E in rows:
        arms[('loop', E)] = lambda E=E: [grp.select_action(obs[E][:, e], explore=True) for e in range(E)]
        arms[('vec', E)] = lambda E=E: grp.select_actions(obs[E], explore=True)
    us = _windows(arms, args.warmup, args.calls, args.windows)
    base = statistics.median(us['single'])
    print(f'sac group R = {R} pendulum explore=1 select_action([R, S]): {_fmt(us["single"])}')
    for E in rows:
        loop, vec = statistics.median(us[('loop', E)]), statistics.median(us[('vec', E)])
        print(f'sac group R = {R} E = {E:3d}: E x select_action {_fmt(us[("loop", E)])}; select_actions {_fmt(us[("vec", E)])}; '
              f'= {vec / base:.2f} x one select_action, {loop / vec:.1f}x faster than E calls, grid {E} x {R} workgroups', flush=True)


class HostLoop(object):
    """main.py's loop body past warm-up on E NumPy Pendulums: run()'s for E = 1, _host_envs_loop's for E > 1"""

    def __init__(self, E, B):
        from rlrep_amd import envs
        from rlrep_amd.utils.buffer import ReplayBuffer
        self.E, self.B = E, B
        self.agent = _sac(3, 1, B, 2.0)
        self.replay = ReplayBuffer(3, 1, max_size=100000)
        self.envs = [envs.make('Pendulum-v1') for _ in range(E)]
        for i, e in enumerate(self.envs):
            e.seed(i)
        self.rng = np.random.RandomState(0)
        self.limit = self.envs[0]._max_episode_steps
        self.states = np.stack([np.asarray(e.reset(), np.float32) for e in self.envs])
        self.ep_steps = np.zeros(E, np.int64)

    def __call__(self):
        if self.E == 1:
            return self._one()
        E = self.E
        self.ep_steps += 1
        greedy = self.agent.select_actions(self.states, explore=True)
        actions = np.zeros((E, 1), np.float32)
        for i, e in enumerate(self.envs):
            actions[i] = e.action_space.sample() if self.rng.uniform(0, 1) < EPS_GREEDY else greedy[i]
        nexts, rewards, dones = np.zeros_like(self.states), np.zeros(E, np.float32), np.zeros(E, np.float32)
        resets = []
        for i, e in enumerate(self.envs):
            nexts[i], reward, done, _ = e.step(actions[i])
            rewards[i] = reward
            dones[i] = float(done) if self.ep_steps[i] < self.limit else 0.0
            if done:
                resets.append(i)
        self.replay.add_batch(self.states, actions, nexts, rewards, dones)
        self.states = nexts
        for i in resets:
            self.states[i] = self.envs[i].reset()
            self.ep_steps[i] = 0
        self.agent.train(self.replay, self.B)

    def _one(self):
        env = self.envs[0]
        self.ep_steps[0] += 1
        state = self.states[0]
        if self.rng.uniform(0, 1) < EPS_GREEDY:
            action = env.action_space.sample()
        else:
            action = self.agent.select_action(state, explore=True)
        nxt, rew, done, _ = env.step(action)
        self.replay.add(state, action, nxt, rew, float(done) if self.ep_steps[0] < self.limit else 0)
        self.states[0] = nxt
        self.agent.train(self.replay, self.B)
        if done:
            self.states[0], self.ep_steps[0] = env.reset(), 0


def loop_table(args, Es):
    arms = {E: HostLoop(E, args.batch) for E in Es}
    us = _windows(arms, args.warmup, args.calls, args.windows)
    for E in Es:
        med = statistics.median(us[E])
        print(f'sac Pendulum-v1 B = {args.batch} host loop --host-envs {E:2d}: {_fmt(us[E])} per iteration = {E * 1e6 / med:9.0f} environment steps/s, '
              f'{1e6 / med:7.0f} train()/s', flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='act,group,loop')
    p.add_argument('--rows', default='1,4,16,64,256', help='E of the act table')
    p.add_argument('--group-rows', default='1,4,16')
    p.add_argument('--host-envs', default='1,4,16')
    p.add_argument('--members', type=int, default=4)
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--warmup', type=int, default=50)
    p.add_argument('--calls', type=int, default=300)
    p.add_argument('--windows', type=int, default=5)
    args = p.parse_args(argv)
    ints = lambda s: [int(v) for v in s.split(',')]  # noqa: E731
    print(f'# {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per arm, median (sorted windows) of {args.windows} windows of {args.calls} '
          f'calls, arms alternated in one process; every call synchronises its stream', flush=True)
    only = args.only.split(',')
    if 'act' in only:
        act_table(args, ints(args.rows))
    if 'group' in only:
        group_table(args, ints(args.group_rows))
    if 'loop' in only:
        loop_table(args, ints(args.host_envs))


if __name__ == '__main__':
    main()
