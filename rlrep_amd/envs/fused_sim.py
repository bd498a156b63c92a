"""Fused simulators on the device (include/rlrep.h rlrep_sim_*; csrc/sim_step.hip; DESIGN.md 6i "Fused simulators"): N environments of
Pendulum-v1 or MountainCarContinuous-v0 whose step is ONE launch, one thread per environment -- the simulator the one-graph loop of
envs/sim_loop.py was built for.

    sim = FusedSim('Pendulum-v1', 4096, 'cuda', seed=0)       # or FusedPendulum(4096), FusedMountainCar(4096)
    sim.reset()
    loop = SimLoop(agent, sim, eps_greedy=0.01, start_timesteps=25 * 4096)
    for _ in range(iterations):
        info = agent.iterate_sim(loop, buffer, batch_size, train=loop.t_global >= loop.start_timesteps)

The dynamics, observation, reward and done_bool rule are the device environments' (csrc/group_env.h EnvPendulum / EnvMountainCar: fp64, in the
operation order of envs/pendulum.py and envs/mountain_car.py).  Every piece of state is a torch tensor at a fixed address, structure of
arrays: `x0`, `x1` (float64: theta, theta_dot resp. p, v), `ep_return`, `last_return` (float64), `t` (int32: the step in the episode, -1 =
ended and frozen), `episodes`, `starts` (int64) and `obs` (float32 [N, S]).  Start state k of environment e is a function of (seed, e, k)
-- a Philox block, csrc/group_env.h RL_STREAM_SIM_START -- so the simulator draws from no torch generator and a graph replays it as it
stands: it keeps to SimLoop's simulator contract with no `graph_generators`.

`step_(actions)` (and `step`, the same method) returns the simulator's own `next_obs` [N, S], `reward` [N] and `done` [N] (float32 0 / 1),
written in place on every call.  `step_append_(actions, buffer, ctl)` is the step that also packs the N transitions into the replay ring from
the loop record's cursor and advances the record: with it SimLoop's iteration in front of train() is two launches.

`auto_restart=False` is the form an evaluation takes: an environment whose episode ended is frozen (t = -1) with its return in
`last_return`, while its neighbours go on -- MountainCar's episodes end at different steps.
"""
import ctypes as C

import numpy as np
import torch

from rlrep_amd._lib import lib, check, SimState
from rlrep_amd.core import _stream

MAX_ENVS = 65536                                            # include/rlrep.h RLREP_SIM_MAX_ENVS
KIND_PENDULUM, KIND_MOUNTAIN_CAR_CONTINUOUS = 0, 2          # include/rlrep.h RLREP_ENV_*
# kind -> (name, S, A, time limit, action range): csrc/group_env.h rl_env_kinds
KINDS = {KIND_PENDULUM: ('Pendulum-v1', 3, 1, 200, (-2.0, 2.0)),
         KIND_MOUNTAIN_CAR_CONTINUOUS: ('MountainCarContinuous-v0', 2, 1, 999, (-1.0, 1.0))}
STATE_NAMES = ('x0', 'x1', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')


def sim_kind(kind_or_env_name):
    """the kind (a key of KINDS) of a kind or an --env name, or None where none is built"""
    if isinstance(kind_or_env_name, str):
        for kind, row in KINDS.items():
            if kind_or_env_name.startswith(row[0].split('-')[0]):
                return kind
        return None
    try:
        kind = int(kind_or_env_name)
    except (TypeError, ValueError):
        return None
    return kind if kind in KINDS else None


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class FusedSim(object):
    """N environments of `kind_or_env_name` (a key of KINDS or its --env name) on `device`; created at start state 0 of every environment
    only after `reset()`.  seed: the Philox key of the start states."""

    def __init__(self, kind_or_env_name, num_envs, device=None, seed=0, auto_restart=True):
        name = type(self).__name__
        kind = sim_kind(kind_or_env_name)
        if kind is None:
            raise ValueError(f'{name}: {kind_or_env_name!r} is not built ({", ".join(f"{k} = {v[0]}" for k, v in KINDS.items())})')
        N = int(num_envs)
        if not 1 <= N <= MAX_ENVS:
            raise ValueError(f'{name}: num_envs {num_envs} outside [1, {MAX_ENVS}]')
        self.kind, self.num_envs, self.seed, self.auto_restart = kind, N, int(seed), bool(auto_restart)
        self.env_name, self.state_dim, self.action_dim, self._max_episode_steps, self.action_range = KINDS[kind]
        self.device = dev = torch.device(device if device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'{name}: the fused simulators live on the GPU (got device {dev})')
        f64 = lambda fill=0.0: torch.full((N,), fill, dtype=torch.float64, device=dev)  # noqa: E731
        self.x0, self.x1, self.ep_return, self.last_return = f64(), f64(), f64(), f64(float('nan'))
        self.t = torch.zeros(N, dtype=torch.int32, device=dev)
        self.episodes = torch.zeros(N, dtype=torch.int64, device=dev)
        self.starts = torch.zeros(N, dtype=torch.int64, device=dev)
        self.obs = torch.zeros(N, self.state_dim, dtype=torch.float32, device=dev)
        self.next_obs = torch.zeros(N, self.state_dim, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(N, dtype=torch.float32, device=dev)
        self._st = SimState(kind=kind, n=N, seed=self.seed & 0xFFFFFFFFFFFFFFFF, auto_restart=int(self.auto_restart),
                            **{k: getattr(self, k).data_ptr() for k in STATE_NAMES})
        assert C.sizeof(SimState) == lib.rlrep_sim_state_bytes()

    # ---- launches (stream-ordered, capturable) ----------------------------------------------------------------------------------------------
    def reset(self):
        """ONE launch (rlrep_sim_start): every environment begins a new episode from its next start state; returns `obs`"""
        check(lib.rlrep_sim_start(C.byref(self._st), _stream()), 'sim_start')
        return self.obs

    def _actions(self, actions, what):
        N, A = self.num_envs, self.action_dim
        if (not torch.is_tensor(actions) or actions.device != self.obs.device or actions.dtype != torch.float32 or actions.numel() < N * A
                or tuple(actions.shape) not in ((N, A), (N,)) or (actions.dim() == 2 and actions.stride(1) != 1)):
            raise ValueError(f'{type(self).__name__}.{what}: actions must be a float32 tensor [{N}, {A}] on {self.obs.device} with unit inner stride')
        ld = actions.stride(0) if N > 1 else A
        if ld < A:
            raise ValueError(f'{type(self).__name__}.{what}: the actions\' row stride {ld} is below their width {A}')
        return ld

    def step_(self, actions):
        """ONE launch (rlrep_sim_step): actions [N, A] float32, raw (the kinds clip them) -> (next_obs [N, S], reward [N], done [N] float32),
        the simulator's own tensors, written in place; `obs` then holds what the next step acts on"""
        ld = self._actions(actions, 'step_')
        check(lib.rlrep_sim_step(C.byref(self._st), _ptr(actions), ld, _ptr(self.next_obs), _ptr(self.reward), _ptr(self.done), _stream()), 'sim_step')
        return self.next_obs, self.reward, self.done

    step = step_

    def step_append_(self, actions, buffer, ctl):
        """ONE launch (rlrep_sim_step_append_ctl): the step, the N transitions [obs before the step, action, s', r, done] into `buffer`'s ring
        from the cursor in the loop record `ctl` (int64[8] on the device, envs/sim_loop.py), the fill level into the buffer's size word, the
        record advanced as SimLoop.append advances it.  next_obs / reward / done are NOT written."""
        ld = self._actions(actions, 'step_append_')
        if (buffer.state_dim, buffer.action_dim) != (self.state_dim, self.action_dim):
            raise ValueError(f'{type(self).__name__}.step_append_: needs a ReplayBuffer of {self.state_dim} observations and {self.action_dim} actions')
        check(lib.rlrep_sim_step_append_ctl(C.byref(self._st), _ptr(actions), ld, _ptr(buffer.ring), buffer.max_size, buffer.row, _ptr(buffer._size_dev),
                                            _ptr(ctl), _stream()), 'sim_step_append_ctl')

    # ---- tests ----------------------------------------------------------------------------------------------------------------------------
    def set_state(self, x0, x1, t=0):
        """tests: continue from the given state words [N] at step t (a number or [N]) of the episode; in place.  The observation is the
        host environment's (NumPy cos / sin, rounded to float32)."""
        N = self.num_envs
        x0, x1 = (np.array(np.broadcast_to(np.asarray(v, np.float64), (N,))) for v in (x0, x1))
        obs = np.stack([np.cos(x0), np.sin(x0), x1] if self.kind == KIND_PENDULUM else [x0, x1], axis=1).astype(np.float32)
        self.x0.copy_(torch.from_numpy(x0))
        self.x1.copy_(torch.from_numpy(x1))
        self.t.copy_(torch.from_numpy(np.array(np.broadcast_to(np.asarray(t, np.int32), (N,)))))
        self.obs.copy_(torch.from_numpy(obs))

    def state(self):
        """dict of host copies of every array (synchronises)"""
        return {k: getattr(self, k).cpu().numpy() for k in STATE_NAMES}


class FusedPendulum(FusedSim):
    """Pendulum-v1: 200-step episodes that never terminate (done is always 0)"""

    def __init__(self, num_envs, device=None, seed=0, auto_restart=True):
        super().__init__(KIND_PENDULUM, num_envs, device, seed, auto_restart)


class FusedMountainCar(FusedSim):
    """MountainCarContinuous-v0: the goal ends an episode with done = 1 (unless it falls on the 999th step); x0 / x1 hold position and
    velocity, fp32-representable"""

    def __init__(self, num_envs, device=None, seed=0, auto_restart=True):
        super().__init__(KIND_MOUNTAIN_CAR_CONTINUOUS, num_envs, device, seed, auto_restart)
