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

A kind of the user's own (csrc/sim_jit.h): `CustomFusedSim(source, num_envs, ...)` takes the C++ text of ONE struct -- NX state
doubles, S observations, A actions, LIMIT, TERMINATES, start / observe / dynamics -- and the library compiles it at run time into the same three
launches; `rlrep_amd/envs/kinds/` holds two examples (`example_kind('pendulum')`, `example_kind('point_mass')`).  It is a drop-in for FusedSim
in SimLoop / iterate_sim; its state words are one array `x` float64 [NX, N].  `SimKind(source)` is the compiled kind alone, so that several
simulators (training and evaluation) share one compile.

`auto_restart=False` is the form an evaluation takes: an environment whose episode ended is frozen (t = -1) with its return in
`last_return`, while its neighbours go on -- MountainCar's episodes end at different steps.
"""
import ctypes as C
import os
import re

import numpy as np
import torch

from rlrep_amd._lib import lib, check, SimState, SimKindDesc, SimKindInfo, SimxState
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


class FusedSimGroup(object):
    """R x N environments of `kind_or_env_name` for seed group `group` (include/rlrep.h rlrep_group_sim_*): FusedSim's surface
    over [R, N] tensors -- `obs` [R, N, S], reset(), step_ / step (actions [R, N, A] -> next_obs [R, N, S], reward [R, N], done [R, N]),
    step_append_(actions, buffers, ctl), set_state, state().  seeds: R Philox keys of the start states, kept in a device tensor; member r's
    plane is FusedSim(kind, N, seed=seeds[r]) word for word.  Every launch is ONE launch over grid (ceil(N / 256), R).  reset() restarts the
    whole group; the steps skip the members the group's live table has retired, whose planes stand still.  The group comes with the
    constructor or with bind_group() before the first launch (SimLoopGroup binds its own).  A kind compiled at run time (SimKind /
    CustomFusedSim) has no group form."""

    def __init__(self, kind_or_env_name, members, num_envs, device=None, seeds=None, auto_restart=True, group=None):
        name = type(self).__name__
        if isinstance(kind_or_env_name, (SimKind, CustomFusedSim)):
            raise ValueError(f'{name}: a kind compiled at run time (SimKind / CustomFusedSim) is built for single agents only; a seed group takes '
                             f'the built-in kinds ({", ".join(v[0] for v in KINDS.values())})')
        kind = sim_kind(kind_or_env_name)
        if kind is None:            # (the text of a kind of the user's own ends here too: only CustomFusedSim takes source text)
            raise ValueError(f'{name}: {str(kind_or_env_name)[:40]!r} is not built for seed groups ({", ".join(f"{k} = {v[0]}" for k, v in KINDS.items())}; '
                             'kinds compiled at run time are built for single agents only)')
        R, N = int(members), int(num_envs)
        if R < 1:
            raise ValueError(f'{name}: members {members} is below 1')
        if not 1 <= N <= MAX_ENVS:
            raise ValueError(f'{name}: num_envs {num_envs} outside [1, {MAX_ENVS}]')
        seeds = list(range(R)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != R:
            raise ValueError(f'{name}: {len(seeds)} seeds for {R} members (one Philox key per member)')
        self.kind, self.members, self.num_envs, self.seeds, self.auto_restart = kind, R, N, seeds, bool(auto_restart)
        self.env_name, self.state_dim, self.action_dim, self._max_episode_steps, self.action_range = KINDS[kind]
        self.device = dev = torch.device(device if device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'{name}: the fused simulators live on the GPU (got device {dev})')
        f64 = lambda fill=0.0: torch.full((R, N), fill, dtype=torch.float64, device=dev)  # noqa: E731
        self.x0, self.x1, self.ep_return, self.last_return = f64(), f64(), f64(), f64(float('nan'))
        self.t = torch.zeros(R, N, dtype=torch.int32, device=dev)
        self.episodes = torch.zeros(R, N, dtype=torch.int64, device=dev)
        self.starts = torch.zeros(R, N, dtype=torch.int64, device=dev)
        self.obs = torch.zeros(R, N, self.state_dim, dtype=torch.float32, device=dev)
        self.next_obs = torch.zeros(R, N, self.state_dim, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(R, N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(R, N, dtype=torch.float32, device=dev)
        # uint64 keys in an int64 tensor, bit for bit
        self.seeds_dev = torch.from_numpy(np.array([s & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64).view(np.int64).copy()).to(dev)
        self._st = SimState(kind=kind, n=N, seed=0, auto_restart=int(self.auto_restart), **{k: getattr(self, k).data_ptr() for k in STATE_NAMES})
        assert C.sizeof(SimState) == lib.rlrep_sim_state_bytes()
        self.group = None
        if group is not None:
            self.bind_group(group)

    def bind_group(self, group):
        """the seed group whose live table the launches read (R members)"""
        name = type(self).__name__
        if getattr(group, 'R', None) is None or not hasattr(group, 'seeds'):
            raise ValueError(f'{name}: needs a seed group (SACSeedBatch / CTRLSACSeedBatch)')
        if int(group.R) != self.members:
            raise ValueError(f'{name}: {self.members} members for a seed group of {group.R}')
        if self.group is not None and self.group is not group:
            raise ValueError(f'{name}: the simulator belongs to another group')
        self.group = group

    def _h(self, what):
        if self.group is None:
            raise RuntimeError(f'{type(self).__name__}.{what}: no seed group yet (the launches read its live table): pass group= or call bind_group()')
        return self.group.core.h

    # ---- launches (stream-ordered, capturable) ----------------------------------------------------------------------------------------------
    def reset(self):
        """ONE launch (rlrep_group_sim_start): every environment of EVERY member, retired ones included, begins a new episode from its next
        start state; returns `obs`"""
        check(lib.rlrep_group_sim_start(self._h('reset'), C.byref(self._st), _ptr(self.seeds_dev), _stream()), 'group_sim_start')
        return self.obs

    def _actions(self, actions, what):
        R, N, A = self.members, self.num_envs, self.action_dim
        if (not torch.is_tensor(actions) or actions.device != self.obs.device or actions.dtype != torch.float32
                or tuple(actions.shape) not in ((R, N, A), (R, N)) or not actions.is_contiguous()):
            raise ValueError(f'{type(self).__name__}.{what}: actions must be a contiguous float32 tensor [{R}, {N}, {A}] on {self.obs.device}')
        return A

    def step_(self, actions):
        """ONE launch (rlrep_group_sim_step): actions [R, N, A] float32, raw -> (next_obs [R, N, S], reward [R, N], done [R, N] float32), the
        simulator's own tensors, written in place; a retired member's planes are neither read nor written"""
        ld = self._actions(actions, 'step_')
        check(lib.rlrep_group_sim_step(self._h('step_'), C.byref(self._st), _ptr(self.seeds_dev), _ptr(actions), ld, _ptr(self.next_obs), _ptr(self.reward),
                                       _ptr(self.done), _stream()), 'group_sim_step')
        return self.next_obs, self.reward, self.done

    step = step_

    def step_append_(self, actions, buffers, ctl):
        """ONE launch (rlrep_group_sim_step_append_ctl): the step of every live member, its N transitions into its ring of `buffers` (a
        ReplayBufferGroup) from its own cursor in the group's loop record `ctl` (int64[R, 8], envs/sim_loop.py SimLoopGroup), its fill level
        into its size word, the group's counters advanced once.  next_obs / reward / done are NOT written."""
        ld = self._actions(actions, 'step_append_')
        if (getattr(buffers, 'members', None) != self.members or (buffers.state_dim, buffers.action_dim) != (self.state_dim, self.action_dim)):
            raise ValueError(f'{type(self).__name__}.step_append_: needs a ReplayBufferGroup of {self.members} members, {self.state_dim} observations '
                             f'and {self.action_dim} actions')
        check(lib.rlrep_group_sim_step_append_ctl(self._h('step_append_'), C.byref(self._st), _ptr(self.seeds_dev), _ptr(actions), ld, _ptr(buffers.rings),
                                                  buffers.max_size, buffers.row, buffers.ring_stride, _ptr(buffers._size_dev), _ptr(ctl), _stream()),
              'group_sim_step_append_ctl')

    # ---- tests ----------------------------------------------------------------------------------------------------------------------------
    def set_state(self, x0, x1, t=0):
        """tests: continue from the given state words (anything that broadcasts to [R, N]) at step t of the episode; in place.  The
        observation is the host environment's (NumPy cos / sin, rounded to float32)."""
        shape = (self.members, self.num_envs)
        x0, x1 = (np.array(np.broadcast_to(np.asarray(v, np.float64), shape)) for v in (x0, x1))
        obs = np.stack([np.cos(x0), np.sin(x0), x1] if self.kind == KIND_PENDULUM else [x0, x1], axis=2).astype(np.float32)
        self.x0.copy_(torch.from_numpy(x0))
        self.x1.copy_(torch.from_numpy(x1))
        self.t.copy_(torch.from_numpy(np.array(np.broadcast_to(np.asarray(t, np.int32), shape))))
        self.obs.copy_(torch.from_numpy(obs))

    def state(self):
        """dict of host copies of every array (synchronises)"""
        return {k: getattr(self, k).cpu().numpy() for k in STATE_NAMES}


# ---- kinds compiled at run time (include/rlrep.h rlrep_sim_kind_*, rlrep_simx_*; csrc/sim_jit.h) ------------------------------------------------
MAX_NX, MAX_S, MAX_A = 8, 16, 8                             # include/rlrep.h RLREP_SIMX_MAX_*
KINDS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'kinds')
XSTATE_NAMES = ('x', 'ep_return', 'last_return', 't', 'episodes', 'starts', 'obs')
KERNELS = ('start', 'step', 'step_append_ctl')
# host observations of the example kinds, for set_state (a kind of the user's own passes `observe=` or `obs=`)
_EXAMPLE_OBSERVE = {'KindPendulum': lambda x: np.stack([np.cos(x[0]), np.sin(x[0]), x[1]], axis=1).astype(np.float32),
                    'KindPointMass': lambda x: np.ascontiguousarray(x.T).astype(np.float32)}


def example_kind(which):
    """the text of an example kind: 'pendulum' (Pendulum-v1, the built-in kind's operations) or 'point_mass' (NX = 4, S = 4, A = 2)"""
    path = os.path.join(KINDS_DIR, f'{which}.h')
    if not os.path.exists(path):
        raise ValueError(f'example_kind: no example {which!r} under {KINDS_DIR}')
    with open(path) as f:
        return f.read()


def kind_constants(source):
    """dict(name, S, A, NX, limit, terminates, action_range) read from a kind's text: the first `struct NAME`, the integer constants NX, S, A,
    LIMIT, the bool TERMINATES and, where given, the floats ACT_LO / ACT_HI (default -1, 1).  A constant the text does not spell as a literal
    is None: give it to SimKind by keyword.  The compile holds every one of them to the struct (static_assert)."""
    text = re.sub(r'//[^\n]*|/\*.*?\*/', '', str(source), flags=re.S)
    m = re.search(r'\bstruct\s+([A-Za-z_]\w*)', text)

    def num(name, pat=r'(\d+)', conv=int):
        m = re.search(r'\b' + name + r'\s*=\s*' + pat, text)
        return conv(m.group(1)) if m else None
    flt = r'([-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)f?'
    lo, hi = num('ACT_LO', flt, float), num('ACT_HI', flt, float)
    return dict(name=m.group(1) if m else None, S=num('S'), A=num('A'), NX=num('NX'), limit=num('LIMIT'),
                terminates=num('TERMINATES', r'(true|false)', lambda v: v == 'true'),
                action_range=(-1.0 if lo is None else lo, 1.0 if hi is None else hi))


class SimKind(object):
    """One simulator kind compiled from `source` (the C++ text of one struct: csrc/sim_jit.h) for the current device: rlrep_sim_kind_compile.
    name, S, A, NX, limit, terminates default to what the text spells (kind_constants); the compile refuses a struct that differs from them.
    A compile failure raises RuntimeError with the compiler's log.  Kinds are independent: any number live at once, destroyed in any order."""

    def __init__(self, source, name=None, S=None, A=None, NX=None, limit=None, terminates=None, action_range=None):
        self._h = None
        self.source = str(source) if source is not None else ''
        self.desc(self.source, name=name, S=S, A=A, NX=NX, limit=limit, terminates=terminates)   # (raises on what the text leaves open)
        d, k = self._desc, kind_constants(self.source)
        self.name, self.state_dim, self.action_dim, self.nx, self.limit, self.terminates = d.name.decode(), d.S, d.A, d.NX, d.limit, bool(d.terminates)
        self.action_range = tuple(float(v) for v in (action_range if action_range is not None else k['action_range']))
        h = C.c_void_p()
        check(lib.rlrep_sim_kind_compile(C.byref(d), C.byref(h)), 'sim_kind_compile')
        self._h = h

    def desc(self, source, **given):
        """the rlrep_sim_kind_desc of `source` (kept alive on self)"""
        k = kind_constants(source)
        val = {key: (given.get(key) if given.get(key) is not None else k[key]) for key in ('name', 'S', 'A', 'NX', 'limit', 'terminates')}
        missing = [key for key, v in val.items() if v is None]
        if missing:
            raise ValueError(f'SimKind: the text does not spell {", ".join(missing)} as a literal; give it by keyword')
        self._keep = (str(val['name']).encode(), str(source).encode())
        self._desc = SimKindDesc(name=self._keep[0], source=self._keep[1], S=int(val['S']), A=int(val['A']), NX=int(val['NX']), limit=int(val['limit']),
                                 terminates=int(bool(val['terminates'])))
        return self._desc

    def compile_text(self):
        """the whole text the library compiled: sim_jit.h, the struct, the static_asserts, the kernels"""
        return assembled_text(self._desc)

    def info(self):
        """dict kernel -> dict(regs, scratch_bytes, lds_bytes), as hipFuncGetAttribute reported them after the load"""
        out = SimKindInfo()
        check(lib.rlrep_sim_kind_info(self._h, C.byref(out)), 'sim_kind_info')
        return {k: dict(regs=int(out.regs[i]), scratch_bytes=int(out.scratch_bytes[i]), lds_bytes=int(out.lds_bytes[i])) for i, k in enumerate(KERNELS)}

    def destroy(self):
        if self._h is not None:
            lib.rlrep_sim_kind_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def assembled_text(desc):
    """rlrep_sim_kind_source: the text the library would compile for a SimKindDesc (no GPU)"""
    n = lib.rlrep_sim_kind_source(C.byref(desc), None, 0)
    if n < 0:
        check(int(n), 'sim_kind_source')
    buf = C.create_string_buffer(int(n) + 1)
    lib.rlrep_sim_kind_source(C.byref(desc), buf, int(n) + 1)
    return buf.value.decode()


class CustomFusedSim(FusedSim):
    """N environments of a kind given as text (or as a compiled SimKind) on `device`: FusedSim's interface -- obs, num_envs, seed, reset(),
    step_ / step, step_append_(actions, buffer, ctl), set_state, state() -- and kernel_info().  The state words are `x` float64 [NX, N].
    name: the struct's name, where the text holds several structs.  observe: a host function x [NX, N] float64 -> obs [N, S] float32 that
    set_state uses (the two example kinds bring theirs)."""

    def __init__(self, source, num_envs, device=None, seed=0, auto_restart=True, name=None, observe=None, **constants):
        who = type(self).__name__
        N = int(num_envs)
        if not 1 <= N <= MAX_ENVS:
            raise ValueError(f'{who}: num_envs {num_envs} outside [1, {MAX_ENVS}]')
        self.device = dev = torch.device(device if device is not None else 'cuda')
        if dev.type != 'cuda':
            raise ValueError(f'{who}: the fused simulators live on the GPU (got device {dev})')
        with torch.cuda.device(dev):
            self.kind = source if isinstance(source, SimKind) else SimKind(source, name=name, **constants)
        k = self.kind
        self.num_envs, self.seed, self.auto_restart = N, int(seed), bool(auto_restart)
        self.env_name, self.state_dim, self.action_dim, self.nx, self._max_episode_steps, self.action_range = (k.name, k.state_dim, k.action_dim, k.nx, k.limit,
                                                                                                               k.action_range)
        self._observe = observe if observe is not None else _EXAMPLE_OBSERVE.get(k.name)
        f64 = lambda fill=0.0: torch.full((N,), fill, dtype=torch.float64, device=dev)  # noqa: E731
        self.x = torch.zeros(k.nx, N, dtype=torch.float64, device=dev)
        self.ep_return, self.last_return = f64(), f64(float('nan'))
        self.t = torch.zeros(N, dtype=torch.int32, device=dev)
        self.episodes = torch.zeros(N, dtype=torch.int64, device=dev)
        self.starts = torch.zeros(N, dtype=torch.int64, device=dev)
        self.obs = torch.zeros(N, self.state_dim, dtype=torch.float32, device=dev)
        self.next_obs = torch.zeros(N, self.state_dim, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(N, dtype=torch.float32, device=dev)
        self.done = torch.zeros(N, dtype=torch.float32, device=dev)
        self._st = SimxState(n=N, seed=self.seed & 0xFFFFFFFFFFFFFFFF, auto_restart=int(self.auto_restart),
                             **{name: getattr(self, name).data_ptr() for name in XSTATE_NAMES})
        assert C.sizeof(SimxState) == lib.rlrep_simx_state_bytes()

    def reset(self):
        """ONE launch (rlrep_simx_start): every environment begins a new episode from its next start state; returns `obs`"""
        check(lib.rlrep_simx_start(self.kind._h, C.byref(self._st), _stream()), 'simx_start')
        return self.obs

    def step_(self, actions):
        """ONE launch (rlrep_simx_step): actions [N, A] float32, raw -> (next_obs [N, S], reward [N], done [N] float32), the simulator's own
        tensors, written in place; `obs` then holds what the next step acts on"""
        ld = self._actions(actions, 'step_')
        check(lib.rlrep_simx_step(self.kind._h, C.byref(self._st), _ptr(actions), ld, _ptr(self.next_obs), _ptr(self.reward), _ptr(self.done), _stream()),
              'simx_step')
        return self.next_obs, self.reward, self.done

    step = step_

    def step_append_(self, actions, buffer, ctl):
        """ONE launch (rlrep_simx_step_append_ctl): the step, the N transitions [obs before the step, actions, s', r, done] into `buffer`'s ring
        from the cursor in the loop record `ctl`, the fill level into the buffer's size word, the record advanced as SimLoop.append advances
        it.  next_obs / reward / done are NOT written."""
        ld = self._actions(actions, 'step_append_')
        if (buffer.state_dim, buffer.action_dim) != (self.state_dim, self.action_dim):
            raise ValueError(f'{type(self).__name__}.step_append_: needs a ReplayBuffer of {self.state_dim} observations and {self.action_dim} actions')
        check(lib.rlrep_simx_step_append_ctl(self.kind._h, C.byref(self._st), _ptr(actions), ld, _ptr(buffer.ring), buffer.max_size, buffer.row,
                                             _ptr(buffer._size_dev), _ptr(ctl), _stream()), 'simx_step_append_ctl')

    def set_state(self, x, t=0, obs=None):
        """tests: continue from the state words x [NX, N] (or [NX], the same for every environment) at step t (a number or [N]) of the episode;
        in place.  The observation is `obs` [N, S] where given, else the host `observe` of the kind."""
        N, NX = self.num_envs, self.nx
        x = np.asarray(x, np.float64)
        x = np.array(np.broadcast_to(x.reshape(NX, -1), (NX, N)))
        if obs is None:
            if self._observe is None:
                raise ValueError(f'{type(self).__name__}.set_state: give obs=, or observe= at construction (the kind is known to the device only)')
            obs = self._observe(x)
        obs = np.ascontiguousarray(np.asarray(obs, np.float32).reshape(N, self.state_dim))
        self.x.copy_(torch.from_numpy(x))
        self.t.copy_(torch.from_numpy(np.array(np.broadcast_to(np.asarray(t, np.int32), (N,)))))
        self.obs.copy_(torch.from_numpy(obs))

    def state(self):
        """dict of host copies of every array (synchronises)"""
        return {k: getattr(self, k).cpu().numpy() for k in XSTATE_NAMES}

    def kernel_info(self):
        """dict kernel -> dict(regs, scratch_bytes, lds_bytes) of the compiled kind: scratch_bytes > 0 means the kind spills"""
        return self.kind.info()
