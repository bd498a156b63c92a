"""Pendulum-v1 for N environments in lockstep as batched torch ops: the example of a simulator that already lives on the GPU, and what the
tests of SACAgent.act_device / ReplayBuffer.add_device drive.

The dynamics are those of envs/pendulum.py (the public gym specification), stated in fp64 and in the same operation order, so that one step
from the same state gives the same state; observations and rewards leave as fp32, as the replay ring stores them.  Start states come from a
`torch.Generator` on the environment's device: no draw-for-draw equality with the NumPy environment's RandomState is claimed.

    env = TorchPendulum(4096, 'cuda', seed=0)
    obs = env.reset()                                   # [N, 3] float32 on the device
    act = agent.act_device(obs, explore=True)           # [N, 1]
    nxt, rew, done = env.step(act)                      # [N, 3], [N], [N] bool -- nothing touches the host
    buffer.add_device(obs, act, nxt, rew, done)
    obs = env.obs                                       # = nxt, except where an episode ended and a new one began

`done` is main.py's done_bool: an episode that ends at its time limit is not a terminal state, so it is False everywhere.  The environments
start together and end only at the 200-step limit, so their limits coincide: the host counts the steps and no device flag is ever read.

`TorchPendulum(..., capturable=True)` is the form a captured graph can replay (envs/sim_loop.py states the contract; SACAgent.iterate_sim):
`step_(actions)` runs the same fp64 operations in the same order, but keeps every piece of state -- `th`, `thd`, `ep_return`, `last_return`,
`obs`, a per-environment step count `steps` and episode count `episodes_dev` -- at a fixed address (`copy_`), counts the steps on the
device and takes the 200-step restart through `torch.where`, so the start-state draw is made on every step and used where an episode
ended.  The draws come from the same `torch.Generator` (listed in `graph_generators` for the graph to register); no draw-for-draw
equality between the two modes is claimed.  `step` is `step_` there, `reset` and `set_state` write in place, and the host attributes `t` /
`episodes` are not kept.
"""
import math

import torch


class TorchPendulum:
    max_speed, max_torque, dt, g, m, l = 8.0, 2.0, 0.05, 10.0, 1.0, 1.0
    _max_episode_steps = 200
    state_dim, action_dim = 3, 1

    def __init__(self, num_envs, device=None, seed=0, capturable=False):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError('TorchPendulum: num_envs must be >= 1')
        self.device = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))
        N = self.num_envs
        self.th = torch.zeros(N, dtype=torch.float64, device=self.device)
        self.thd = torch.zeros(N, dtype=torch.float64, device=self.device)
        self.t = 0                                      # steps of the running episodes (the same for every environment)
        self.episodes = 0                               # finished episodes per environment
        self.ep_return = torch.zeros(N, dtype=torch.float64, device=self.device)       # of the running episodes
        self.last_return = torch.full((N,), float('nan'), dtype=torch.float64, device=self.device)     # of the last finished ones
        self._done = torch.zeros(N, dtype=torch.bool, device=self.device)
        self.obs = self._obs()
        self.capturable = bool(capturable)
        if self.capturable:
            self.graph_generators = (self._gen,)
            self.steps = torch.zeros(N, dtype=torch.int64, device=self.device)          # steps of the running episode, per environment
            self.episodes_dev = torch.zeros(N, dtype=torch.int64, device=self.device)   # finished episodes, per environment
            self._zero_f, self._zero_i = torch.zeros_like(self.ep_return), torch.zeros_like(self.steps)       # (constants: never written)
            self.step, self.reset, self.set_state = self.step_, self._reset_in_place, self._set_state_in_place

    def _obs(self):
        return torch.stack([torch.cos(self.th), torch.sin(self.th), self.thd], dim=1).to(torch.float32)

    def _start(self):
        u = torch.rand(2, self.num_envs, dtype=torch.float64, device=self.device, generator=self._gen)
        self.th = -math.pi + 2.0 * math.pi * u[0]
        self.thd = -1.0 + 2.0 * u[1]
        self.t = 0
        self.ep_return = torch.zeros_like(self.ep_return)

    def reset(self):
        self._start()
        self.obs = self._obs()
        return self.obs

    def set_state(self, th, thd, t=0):
        """tests: continue from the given angles / angular velocities [N] at step t of the episode"""
        self.th = torch.as_tensor(th, dtype=torch.float64, device=self.device).reshape(self.num_envs).clone()
        self.thd = torch.as_tensor(thd, dtype=torch.float64, device=self.device).reshape(self.num_envs).clone()
        self.t = int(t)
        self.obs = self._obs()

    # ---- capturable=True: every piece of state stays where it is, nothing is decided on the host ------------------------------------------
    def _draw_start(self):
        u = torch.rand(2, self.num_envs, dtype=torch.float64, device=self.device, generator=self._gen)
        return -math.pi + 2.0 * math.pi * u[0], -1.0 + 2.0 * u[1]

    def _reset_in_place(self):
        th, thd = self._draw_start()
        self.th.copy_(th)
        self.thd.copy_(thd)
        self.steps.zero_()
        self.ep_return.zero_()
        self.obs.copy_(self._obs())
        return self.obs

    def _set_state_in_place(self, th, thd, t=0):
        """tests: continue from the given angles / angular velocities [N] at step t of every episode"""
        self.th.copy_(torch.as_tensor(th, dtype=torch.float64, device=self.device).reshape(self.num_envs))
        self.thd.copy_(torch.as_tensor(thd, dtype=torch.float64, device=self.device).reshape(self.num_envs))
        self.steps.fill_(int(t))
        self.obs.copy_(self._obs())

    def step_(self, actions):
        """`step` for a captured graph (capturable=True): the same return values from the same fp64 operations; `obs`, `th`, `thd`,
        `ep_return`, `last_return`, `steps` and `episodes_dev` are written in place, and an environment whose step was the 200th of its
        episode files its return and starts anew through torch.where -- no value is read on the host."""
        if not self.capturable:
            raise RuntimeError('TorchPendulum.step_: build the environment with capturable=True')
        u = actions.reshape(self.num_envs).to(torch.float64).clamp(-self.max_torque, self.max_torque)
        th, thd = self.th, self.thd
        wrapped = torch.remainder(th + math.pi, 2 * math.pi) - math.pi
        cost = wrapped * wrapped + 0.1 * (thd * thd) + 0.001 * (u * u)
        thd = thd + (3 * self.g / (2 * self.l) * torch.sin(th) + 3.0 / (self.m * self.l ** 2) * u) * self.dt
        thd = thd.clamp(-self.max_speed, self.max_speed)
        th = th + thd * self.dt
        ret = self.ep_return - cost
        nxt = torch.stack([torch.cos(th), torch.sin(th), thd], dim=1).to(torch.float32)
        reward = (-cost).to(torch.float32)
        t = self.steps + 1
        end = t >= self._max_episode_steps
        th0, thd0 = self._draw_start()
        # (torch.where(..., out=) on its own operand: one kernel per word of state, no temporaries)
        torch.where(end, ret, self.last_return, out=self.last_return)
        torch.where(end, self._zero_f, ret, out=self.ep_return)
        torch.where(end, th0, th, out=self.th)
        torch.where(end, thd0, thd, out=self.thd)
        torch.where(end, self._zero_i, t, out=self.steps)
        self.episodes_dev.add_(end)
        self.obs.copy_(torch.stack([torch.cos(self.th), torch.sin(self.th), self.thd], dim=1))      # (_obs(): copy_ rounds to fp32 as .to() does)
        return nxt, reward, self._done

    def step(self, actions):
        """actions [N, 1] (or [N]) -> (next observations [N, 3] float32, rewards [N] float32, done_bool [N] bool).  Where the step was the
        200th of its episode the return is filed in last_return and a new episode starts: `obs` then holds its first observation."""
        u = actions.reshape(self.num_envs).to(torch.float64).clamp(-self.max_torque, self.max_torque)
        th, thd = self.th, self.thd
        wrapped = torch.remainder(th + math.pi, 2 * math.pi) - math.pi
        cost = wrapped * wrapped + 0.1 * (thd * thd) + 0.001 * (u * u)
        thd = thd + (3 * self.g / (2 * self.l) * torch.sin(th) + 3.0 / (self.m * self.l ** 2) * u) * self.dt
        thd = thd.clamp(-self.max_speed, self.max_speed)
        th = th + thd * self.dt
        self.th, self.thd = th, thd
        self.t += 1
        self.ep_return = self.ep_return - cost
        nxt = self._obs()
        reward = (-cost).to(torch.float32)
        if self.t >= self._max_episode_steps:
            self.last_return = self.ep_return
            self.episodes += 1
            self._start()
            self.obs = self._obs()
        else:
            self.obs = nxt
        return nxt, reward, self._done
