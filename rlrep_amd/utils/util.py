"""Host-side helpers under the reference's names (utils/util.py:10-104): `unpack_batch`, `Timer`, `eval_policy`,
`weight_init`, `MLP`, `mlp`, `to_np`.  No gym import (the reference only needed the module's name).  Beyond the reference:
`eval_policy_vec` / `lockstep_rollouts` evaluate over several host environments in lockstep (one `select_actions` per step)."""
import time

import numpy as np
import torch
from torch import nn


def unpack_batch(batch):
    """(state, action, next_state, reward, done) -- NOT the Batch field order (utils/util.py:10-11)."""
    return tuple(getattr(batch, f) for f in ('state', 'action', 'next_state', 'reward', 'done'))


class Timer:
    """Wall-clock bookkeeping for the launcher's `Steps per sec` line (utils/util.py:14-37)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._start_time = self._step_time = time.time()
        self._step = 0

    def set_step(self, step):
        self._step, self._step_time = step, time.time()

    def time_cost(self):
        return time.time() - self._start_time

    def steps_per_sec(self, step):
        now = time.time()
        rate = (step - self._step) / max(now - self._step_time, 1e-12)
        self._step, self._step_time = step, now
        return rate


def eval_policy(policy, eval_env, eval_episodes=10):
    """Mean undiscounted return of the deterministic policy over `eval_episodes` episodes (pre-0.26 gym API)."""
    returns = []
    for _ in range(eval_episodes):
        obs, done, ret = eval_env.reset(), False, 0.0
        while not done:
            obs, reward, done, _ = eval_env.step(policy.select_action(np.asarray(obs)))
            ret += reward
        returns.append(ret)
    avg = float(np.mean(returns))
    bar = '-' * 39
    print(f'{bar}\nEvaluation over {eval_episodes} episodes: {avg:.3f}\n{bar}')
    return avg


class EvalResult(float):
    """What eval_policy_vec returns: the mean return (a float), with the per-episode returns, in episode order, in `.returns`."""

    def __new__(cls, returns):
        self = super().__new__(cls, float(np.mean(returns)))
        self.returns = [float(r) for r in returns]
        return self


def lockstep_rollouts(act, envs, counts):
    """Environment j runs counts[j] whole episodes one after the other (reset, then steps until done), all environments in lockstep: every
    step is ONE `act(obs [N, S], active [N] bool) -> actions [N, A]` call, of which the rows of the environments with an episode in progress
    are used (the other rows of `obs` are stale).  Returns [N] lists of returns.  Each environment is reset and stepped exactly as a
    sequential loop over it alone would, so its own random stream is consumed in the same order."""
    N = len(envs)
    left = [int(c) for c in counts]
    out = [[] for _ in envs]
    obs, ret, active = None, np.zeros(N), np.zeros(N, bool)
    for j, env in enumerate(envs):
        if left[j] > 0:
            o = np.asarray(env.reset(), np.float32).reshape(-1)
            if obs is None:
                obs = np.zeros((N, o.shape[0]), np.float32)
            obs[j], active[j] = o, True
    while active.any():
        actions = act(obs, active)
        for j in np.flatnonzero(active):
            o, reward, done, _ = envs[j].step(actions[j])
            ret[j] += reward
            if done:
                out[j].append(ret[j])
                ret[j], left[j] = 0.0, left[j] - 1
                if left[j] > 0:
                    o = envs[j].reset()
                else:
                    active[j] = False
            obs[j] = np.asarray(o, np.float32).reshape(-1)
    return out


def eval_policy_vec(policy, envs, eval_episodes=10):
    """eval_policy over E = len(envs) environments stepped in lockstep: one `policy.select_actions(obs of the running episodes [n, S])` per
    step instead of one select_action per environment step.  Environment i runs episodes i, i + E, ... in that order, so each environment's
    random stream is consumed as a sequential evaluation over that environment would consume it.  Returns an EvalResult: the mean return as
    a float, the per-episode returns (episode order) in `.returns`."""
    E = len(envs)
    counts = [len(range(i, int(eval_episodes), E)) for i in range(E)]

    def act(obs, active):
        actions = np.zeros((E,) + np.shape(envs[0].action_space.low), np.float32)
        actions[active] = policy.select_actions(obs[active])
        return actions
    per_env = lockstep_rollouts(act, envs, counts)
    returns = [per_env[k % E][k // E] for k in range(int(eval_episodes))]
    res = EvalResult(returns)
    bar = '-' * 39
    print(f'{bar}\nEvaluation over {eval_episodes} episodes: {float(res):.3f}\n{bar}')
    return res


def weight_init(m):
    """Orthogonal weights / zero bias for every nn.Linear (applied with Module.apply)."""
    if isinstance(m, nn.Linear):
        nn.init.orthogonal_(m.weight.data)
        if m.bias is not None:
            m.bias.data.zero_()


def mlp(input_dim, hidden_dim, output_dim, hidden_depth, output_mod=None):
    """nn.Sequential of `hidden_depth` x (Linear, ELU) + Linear; Linear layers sit at indices 0, 2, 4, ..."""
    widths = [input_dim] + [hidden_dim] * hidden_depth
    layers = []
    for fan_in, fan_out in zip(widths, widths[1:]):
        layers.extend((nn.Linear(fan_in, fan_out), nn.ELU(inplace=True)))
    layers.append(nn.Linear(widths[-1], output_dim))
    if output_mod is not None:
        layers.append(output_mod)
    return nn.Sequential(*layers)


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, hidden_depth, output_mod=None):
        super().__init__()
        self.trunk = mlp(input_dim, hidden_dim, output_dim, hidden_depth, output_mod)
        self.apply(weight_init)

    def forward(self, x):
        return self.trunk(x)


def to_np(t):
    if t is None:
        return None
    return np.array([]) if t.nelement() == 0 else t.detach().cpu().numpy()
