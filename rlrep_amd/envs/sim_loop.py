"""The loop around a simulator that lives on the GPU as torch tensors, as ONE graph replay per iteration:

    sim = TorchPendulum(4096, 'cuda', seed=0, capturable=True)
    sim.reset()
    loop = SimLoop(agent, sim, eps_greedy=0.01, start_timesteps=25 * 4096)
    for _ in range(iterations):
        info = agent.iterate_sim(loop, buffer, batch_size, train=loop.t_global >= loop.start_timesteps)

`SACAgent.iterate_sim` captures, once, the act launch (rlrep_act_device_ctl: the actor for the N observations, the exploration mix), the
simulator's `step_`, the append launch (rlrep_replay_add_cols_ctl) and the agent's train() on one stream, and replays that graph afterwards.
What changes from one iteration to the next -- the select_action call counter, the step count, the iteration, the ring cursor -- lives in a
loop record on the device (int64[LOOP_CTL_WORDS], csrc/kparams.h RL_CTL_*) that the two launches read and advance; nothing of it rides by
value in the graph.

The simulator contract.  `sim.obs` is a float32 [N, S] CUDA tensor that the simulator updates IN PLACE (the graph reads its capture-time
address on every replay).  `sim.step_(actions)` takes the [N, A] float32 actions and returns `(next_obs [N, S] float32, reward [N] float32,
done [N] bool or float32)`; afterwards `sim.obs` holds the observations the next iteration acts on (`next_obs`, except where an episode
ended and a new one began).  `step_` uses stream-ordered torch ops only, never reads a value on the host (no `.item()`, no `if tensor:`, no
host-side step counting that changes the ops) and updates every piece of persistent state in place (`copy_`, `add_`, ...): a rebound
attribute would be read from its capture-time address on every replay.  Generators it draws from are listed in `sim.graph_generators` (a
sequence of `torch.Generator`; optional), so that the graph registers them.  envs/torch_pendulum.py `TorchPendulum(capturable=True)` is
the example.

The optional hook.  A simulator may also have `step_append_(actions, buffer, ctl)`: ONE capture-safe launch that steps the simulator AND does
the append launch's work -- the N transitions [sim.obs as it stood before the step, actions, next_obs, reward, done] into `buffer.ring` rows
ctl[START], ctl[START] + 1, ... (wrapping at buffer.max_size), ctl[SIZE] published to `buffer._size_dev`, ITER += 1, T += N, CALLS += N unless
ctl[WARM] (csrc/kparams.h RL_CTL_*: no thread writes a word that a workgroup of the same launch reads).  A loop around such a simulator acts
DIRECTLY on `sim.obs` -- no copy -- and an iteration in front of train() is two launches; `SimLoop(..., fused_append=False)` keeps the
separate route.  envs/fused_sim.py `FusedSim` is the example (rlrep_sim_step_append_ctl).

To the replay buffer a SimLoop shows the face of a device environment (`num_envs`, `set_cursor`, `state()` with `ring_ptr` / `ring_size`):
`ReplayBuffer.collect_on_device` hands it the cursor, `add_device` refuses while it owns it, `adopt_device_cursor` takes it back.
"""
import ctypes as C

import numpy as np
import torch

from rlrep_amd._lib import lib, check
from rlrep_amd.core import _stream

LOOP_CTL_WORDS = 8                                      # include/rlrep.h RLREP_LOOP_CTL_WORDS
CALLS, T_GLOBAL, ITER, NEXT_PTR, START, SIZE, WARM = range(7)            # csrc/kparams.h RL_CTL_*
ACT_MAX_ROWS = 65536
STATE_DTYPE = np.dtype([('ring_ptr', '<i8'), ('ring_size', '<i8'), ('start', '<i8'), ('t_global', '<i8'), ('calls', '<i8'), ('iter', '<i8')])


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class SimLoop(object):
    """The device-resident loop record of `agent` and torch simulator `sim`, and the two launches that read it.  eps_greedy: the probability
    of a uniform action in place of the policy's; start_timesteps: the warm-up, environment steps (a multiple of N) that take uniform actions
    only.  Both ride by value in the captured graph.  fused_append: take the simulator's `step_append_` hook where it has one (the module
    docstring); False keeps the separate copy / act / step_ / append route."""

    def __init__(self, agent, sim, eps_greedy=0.0, start_timesteps=0, fused_append=True):
        name = type(self).__name__
        if getattr(agent, 'R', None) is not None or not hasattr(agent, '_seed'):
            raise ValueError(f'{name}: needs a single agent (seed groups have act_device / add_device as an API only)')
        obs = getattr(sim, 'obs', None)
        S, A = agent.state_dim, agent.action_dim
        if (not torch.is_tensor(obs) or not obs.is_cuda or obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != S
                or not 1 <= obs.shape[0] <= ACT_MAX_ROWS or not obs.is_contiguous()):
            raise ValueError(f'{name}: sim.obs must be a contiguous CUDA float32 tensor [N, {S}] with N in [1, {ACT_MAX_ROWS}]')
        if not callable(getattr(sim, 'step_', None)):
            raise ValueError(f'{name}: the simulator needs step_(actions) -> (next_obs, reward, done), capture-safe (see the module docstring)')
        self.agent, self.sim = agent, sim
        self.fused_append = bool(fused_append) and callable(getattr(sim, 'step_append_', None))
        self.num_envs = N = int(obs.shape[0])
        self.eps_greedy, self.start_timesteps = float(eps_greedy), int(start_timesteps)
        if not 0.0 <= self.eps_greedy <= 1.0:
            raise ValueError(f'{name}: eps_greedy {eps_greedy} outside [0, 1]')
        if self.start_timesteps < 0 or self.start_timesteps % N:
            raise ValueError(f'{name}: start_timesteps {start_timesteps} is not a multiple of the {N} environments (an iteration is all warm-up or none of it)')
        self.seed = int(agent._seed)                    # the Philox key of the mix: what the agent's select_action draws with
        dev = obs.device
        self.ctl = torch.zeros(LOOP_CTL_WORDS, dtype=torch.int64, device=dev)
        self.obs0 = torch.empty(N, S, dtype=torch.float32, device=dev)           # the observations the iteration acted on (the ring's s column)
        self.actions = torch.empty(N, A, dtype=torch.float32, device=dev)
        self.t_global, self.calls, self.iter = 0, 0, 0          # host mirrors of the record (iterate_sim keeps them in step)
        self._held = None                               # what the last captured step returned (the graph's pool owns the memory)

    # ---- the record -----------------------------------------------------------------------------------------------------------------------
    def _read(self):
        return self.ctl.cpu().numpy()                   # (synchronises)

    def _write(self, words):
        self.ctl.copy_(torch.from_numpy(np.ascontiguousarray(words, dtype=np.int64)))

    def state(self):
        """one record (STATE_DTYPE): ring_ptr is the next free ring row, ring_size the fill level; a host copy: synchronises"""
        w = self._read()
        rec = np.zeros(1, STATE_DTYPE)
        rec['ring_ptr'], rec['ring_size'], rec['start'] = w[NEXT_PTR], w[SIZE], w[START]
        rec['t_global'], rec['calls'], rec['iter'] = w[T_GLOBAL], w[CALLS], w[ITER]
        return rec

    def set_cursor(self, ptr, sizes, capacity=None):
        """the ring's next free row and fill level (ReplayBuffer.collect_on_device)"""
        w = self._read()
        w[NEXT_PTR] = int(ptr) % int(capacity) if capacity else int(ptr)
        w[START] = w[NEXT_PTR]
        w[SIZE] = int(np.asarray(sizes).reshape(-1)[0])
        self._write(w)

    def counters(self):
        """(t_global, calls, iter) as the device holds them (synchronises)"""
        w = self._read()
        return int(w[T_GLOBAL]), int(w[CALLS]), int(w[ITER])

    def set_counters(self, t_global, calls, iteration=None):
        """environment steps taken and the select_action call counter the next iteration continues from (and the iteration, the counter of
        the mix's draws, when given)"""
        w = self._read()
        w[T_GLOBAL], w[CALLS] = int(t_global), int(calls)
        if iteration is not None:
            w[ITER] = int(iteration)
            self.iter = int(iteration)
        self._write(w)
        self.t_global, self.calls = int(t_global), int(calls)

    # ---- launches (stream-ordered, capturable) ----------------------------------------------------------------------------------------------
    def act(self, obs, out, capacity):
        """ONE launch (rlrep_act_device_ctl): out[e] = the exploring action for obs[e] at call counter calls + 1 + e, or the mix's uniform
        action; the cursor moves by N rows in a ring of `capacity` rows"""
        N, S, A = self.num_envs, self.agent.state_dim, self.agent.action_dim
        lo, hi = self.agent.action_range
        check(lib.rlrep_act_device_ctl(self.agent.core.h, _ptr(obs), obs.stride(0) if N > 1 else S, N, self.seed, float(lo), float(hi), _ptr(out),
                                       out.stride(0) if N > 1 else A, _ptr(self.ctl), int(capacity), self.eps_greedy, self.start_timesteps, _stream()),
              'act_device_ctl')

    def append(self, buffer, s, a, s2, r, d):
        """ONE launch (rlrep_replay_add_cols_ctl): the N transitions into ring rows start, start + 1, ... (wrapping), the fill level into the
        buffer's size word, the counters advanced"""
        N, S, A = self.num_envs, buffer.state_dim, buffer.action_dim
        ld = lambda t, w: t.stride(0) if N > 1 else w  # noqa: E731
        check(lib.rlrep_replay_add_cols_ctl(_ptr(buffer.ring), buffer.max_size, buffer.row, S, A, _ptr(s), ld(s, S), _ptr(a), ld(a, A), _ptr(s2), ld(s2, S),
                                            _ptr(r), _ptr(d), N, _ptr(buffer._size_dev), _ptr(self.ctl), _stream()), 'replay_add_cols_ctl')

    def step(self, buffer):
        """One iteration without the train(): copy of the observations, act launch, `sim.step_`, append launch -- stream-ordered on the
        current stream, nothing read on the host (what iterate_sim captures).  With the simulator's `step_append_` hook: the act launch
        directly on `sim.obs`, then the hook -- two launches."""
        N, S = self.num_envs, buffer.state_dim
        if self.fused_append:
            self.act(self.sim.obs, self.actions, buffer.max_size)
            self.sim.step_append_(self.actions, buffer, self.ctl)
            return
        self.obs0.copy_(self.sim.obs)
        self.act(self.obs0, self.actions, buffer.max_size)
        nxt, rew, done = self.sim.step_(self.actions)

        def prep(t, shape, name):
            if not torch.is_tensor(t) or t.device != self.obs0.device or tuple(t.shape) not in (shape, shape + (1,)):
                raise ValueError(f'SimLoop: step_ returned {name} that is not a tensor {list(shape)} on {self.obs0.device}')
            t = t if t.dtype == torch.float32 else t.to(torch.float32)
            return t.reshape(shape).contiguous()
        nxt, rew, done = prep(nxt, (N, S), 'next_obs'), prep(rew, (N,), 'reward'), prep(done, (N,), 'done')
        self.append(buffer, self.obs0, self.actions, nxt, rew, done)
        self._held = (nxt, rew, done)

    def advance(self):
        """the host mirrors after one replay; True if the iteration was a warm-up one"""
        warm = self.t_global < self.start_timesteps
        self.t_global += self.num_envs
        self.iter += 1
        return warm
