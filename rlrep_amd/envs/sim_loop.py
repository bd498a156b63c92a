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

A seed group takes `SimLoopGroup` (below): the same contract with `[R, N, ...]` tensors, one record row per member.
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
        self._lead = lead = self._check_agent(agent)    # the axes in front of [N, S]: () for one agent, (R,) for a seed group
        obs = getattr(sim, 'obs', None)
        S, A = agent.state_dim, agent.action_dim
        if (not torch.is_tensor(obs) or not obs.is_cuda or obs.dtype != torch.float32 or obs.dim() != len(lead) + 2 or obs.shape[-1] != S
                or tuple(obs.shape[:-2]) != lead or not 1 <= obs.shape[-2] <= ACT_MAX_ROWS or not obs.is_contiguous()):
            shape = ', '.join([str(n) for n in lead] + ['N', str(S)])
            raise ValueError(f'{name}: sim.obs must be a contiguous CUDA float32 tensor [{shape}] with N in [1, {ACT_MAX_ROWS}]')
        if not callable(getattr(sim, 'step_', None)):
            raise ValueError(f'{name}: the simulator needs step_(actions) -> (next_obs, reward, done), capture-safe (see the module docstring)')
        self.agent, self.sim = agent, sim
        if not lead:
            self.seed = int(agent._seed)                # the Philox key of the mix: what the agent's select_action draws with
        self.fused_append = bool(fused_append) and callable(getattr(sim, 'step_append_', None))
        self.num_envs = N = int(obs.shape[-2])
        self.eps_greedy, self.start_timesteps = float(eps_greedy), int(start_timesteps)
        if not 0.0 <= self.eps_greedy <= 1.0:
            raise ValueError(f'{name}: eps_greedy {eps_greedy} outside [0, 1]')
        if self.start_timesteps < 0 or self.start_timesteps % N:
            raise ValueError(f'{name}: start_timesteps {start_timesteps} is not a multiple of the {N} environments (an iteration is all warm-up or none of it)')
        dev = obs.device
        self.ctl = torch.zeros(*lead, LOOP_CTL_WORDS, dtype=torch.int64, device=dev)
        self.obs0 = torch.empty(*lead, N, S, dtype=torch.float32, device=dev)    # the observations the iteration acted on (the ring's s column)
        self.actions = torch.empty(*lead, N, A, dtype=torch.float32, device=dev)
        self.t_global, self.calls, self.iter = 0, 0, 0          # host mirrors of the record (iterate_sim keeps them in step)
        self._held = None                               # what the last captured step returned (the graph's pool owns the memory)

    def _check_agent(self, agent):
        """the axes in front of [N, S] for `agent`, or ValueError"""
        if getattr(agent, 'R', None) is not None or not hasattr(agent, '_seed'):
            raise ValueError(f'{type(self).__name__}: needs a single agent (a seed group takes SimLoopGroup; its act_device / add_device are the eager API)')
        return ()

    # ---- the record -----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _shared(w):
        """the words CALLS, T, ITER and WARM of a host copy of the record (a view)"""
        return w

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
        w = self._shared(self._read())
        return int(w[T_GLOBAL]), int(w[CALLS]), int(w[ITER])

    def set_counters(self, t_global, calls, iteration=None):
        """environment steps taken and the select_action call counter the next iteration continues from (and the iteration, the counter of
        the mix's draws, when given)"""
        w = self._read()
        sh = self._shared(w)
        sh[T_GLOBAL], sh[CALLS] = int(t_global), int(calls)
        if iteration is not None:
            sh[ITER] = int(iteration)
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
        N, S, lead = self.num_envs, buffer.state_dim, self._lead
        if self.fused_append:
            self.act(self.sim.obs, self.actions, buffer.max_size)
            self.sim.step_append_(self.actions, buffer, self.ctl)
            return
        self.obs0.copy_(self.sim.obs)
        self.act(self.obs0, self.actions, buffer.max_size)
        nxt, rew, done = self.sim.step_(self.actions)

        def prep(t, shape, name):
            if not torch.is_tensor(t) or t.device != self.obs0.device or tuple(t.shape) not in (shape, shape + (1,)):
                raise ValueError(f'{type(self).__name__}: step_ returned {name} that is not a tensor {list(shape)} on {self.obs0.device}')
            t = t if t.dtype == torch.float32 else t.to(torch.float32)
            return t.reshape(shape).contiguous()
        nxt, rew, done = prep(nxt, lead + (N, S), 'next_obs'), prep(rew, lead + (N,), 'reward'), prep(done, lead + (N,), 'done')
        self.append(buffer, self.obs0, self.actions, nxt, rew, done)
        self._held = (nxt, rew, done)

    def advance(self):
        """the host mirrors after one replay; True if the iteration was a warm-up one"""
        warm = self.t_global < self.start_timesteps
        self.t_global += self.num_envs
        self.iter += 1
        return warm


class SimLoopGroup(SimLoop):
    """SimLoop for a seed group (SACSeedBatch / CTRLSACSeedBatch): `sim.obs` is [R, N, S], `sim.step_(actions [R, N, A])`
    returns next_obs [R, N, S], reward [R, N], done [R, N], and `SeedBatchMixin.iterate_sim(loop, buffers, batch_size)` replays the whole
    iteration of every live member as one graph.  envs/fused_sim.py `FusedSimGroup` is the simulator it was built for.

    The record is int64[R, LOOP_CTL_WORDS] (csrc/kparams.h, "the loop record of a group").  CALLS, T, ITER and WARM are the GROUP's, kept in
    row 0 -- one call counter, one step count per member (an iteration adds N), one iteration count, as the group's `_ctr` is one -- and
    advance while at least one member is live.  NEXT, START and SIZE are member r's cursor into its own ring, in row r.  The two launches
    honour the live table: a retired member's cursor, ring, fill level and simulator planes stand still, so a revived member writes on where
    it stopped.  Member r's exploration mix is keyed by seeds[r]."""

    def _check_agent(self, agent):
        if getattr(agent, 'R', None) is None or not hasattr(agent, 'seeds'):
            raise ValueError(f'{type(self).__name__}: needs a seed group (SACSeedBatch / CTRLSACSeedBatch); a single agent takes SimLoop')
        return (int(agent.R),)

    def __init__(self, group, sim, eps_greedy=0.0, start_timesteps=0, fused_append=True):
        super().__init__(group, sim, eps_greedy, start_timesteps, fused_append)
        self.R = int(group.R)
        self.seeds = [int(s) for s in group.seeds]      # the Philox keys of the members' mixes (the library holds them: rlrep_group_set_seeds)
        self.actions.zero_()                            # (a retired member's plane is never written)
        if callable(getattr(sim, 'bind_group', None)):
            sim.bind_group(group)               # (the simulator's launches read the group's live table)

    @staticmethod
    def _shared(w):
        return w[0]

    def state(self):
        """[R] records (STATE_DTYPE): member r's next free ring row and fill level, and the group's counters in every record; a host copy:
        synchronises"""
        w = self._read()
        rec = np.zeros(self.R, STATE_DTYPE)
        rec['ring_ptr'], rec['ring_size'], rec['start'] = w[:, NEXT_PTR], w[:, SIZE], w[:, START]
        rec['t_global'], rec['calls'], rec['iter'] = w[0, T_GLOBAL], w[0, CALLS], w[0, ITER]
        return rec

    def set_cursor(self, ptr, sizes, capacity=None):
        """every member's next free row (the host rings advance in lockstep) and its own fill level (ReplayBufferGroup.collect_on_device)"""
        sizes = np.asarray(sizes, np.int64).reshape(-1)
        if sizes.size != self.R:
            raise ValueError(f'{type(self).__name__}.set_cursor: {sizes.size} fill levels for {self.R} members')
        w = self._read()
        w[:, NEXT_PTR] = int(ptr) % int(capacity) if capacity else int(ptr)
        w[:, START] = w[:, NEXT_PTR]
        w[:, SIZE] = sizes
        self._write(w)

    def act(self, obs, out, capacity):
        """ONE launch (rlrep_group_act_device_ctl): plane r of `out` [R, N, A] is what SimLoop.act gives the standalone agent with seed
        seeds[r] at the group's counters; every live member's cursor moves by N rows in its ring of `capacity` rows"""
        lo, hi = self.agent.action_range
        check(lib.rlrep_group_act_device_ctl(self.agent.core.h, _ptr(obs), self.num_envs, float(lo), float(hi), _ptr(out), _ptr(self.ctl), int(capacity),
                                             self.eps_greedy, self.start_timesteps, _stream()), 'group_act_device_ctl')

    def append(self, buffers, s, a, s2, r, d):
        """ONE launch (rlrep_group_replay_add_cols_ctl): every live member's N transitions (plane r of the five contiguous arrays) into its
        ring from its own start row, its fill level into its size word, the group's counters advanced once"""
        N, S, A = self.num_envs, buffers.state_dim, buffers.action_dim
        check(lib.rlrep_group_replay_add_cols_ctl(self.agent.core.h, _ptr(buffers.rings), buffers.max_size, buffers.row, S, A, _ptr(s), S, _ptr(a), A, _ptr(s2), S,
                                                  _ptr(r), _ptr(d), N, buffers.ring_stride, _ptr(buffers._size_dev), _ptr(self.ctl), _stream()),
              'group_replay_add_cols_ctl')
