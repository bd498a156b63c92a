"""Environments on the device (include/rlrep.h rlrep_group_env_*, rlrep_env_*; rlrep_amd/csrc/group_env.hip): Pendulum-v1
(DevicePendulumGroup) and MountainCarContinuous-v0 (DeviceMountainCarGroup, whose goal state ends an episode with done = 1) for a seed group,
DevicePendulum and DeviceMountainCar for a single agent of any algorithm (`SACAgent.iterate` / `SACAgent.evaluate`, the same contracts at R = 1).

One record per member lives on the device; `SeedBatchMixin.iterate(env, buffers, batch_size)` acts, explores, steps the dynamics, writes the
replay-ring row and trains every live member in ONE graph replay, and `SeedBatchMixin.evaluate(env, episodes)` scores every live member in one
launch.  The dynamics are those of rlrep_amd/envs/pendulum.py resp. envs/mountain_car.py (fp64 in one lane, rounded to fp32 where those
files round); the random draws are Philox streams of the member's seed, so two groups with equal seeds collect identical transitions.

`num_envs = E` (1..64, default 1) gives every member / the agent E environments: one `iterate` steps all of them in the same launch, writes E
ring rows per member in environment order and trains once.  Environment 0 is the single environment draw for draw; the others draw from
streams of their own (csrc/group_env.h has the table).
"""
import ctypes as C

import numpy as np
import torch

from rlrep_amd._lib import lib, check
from rlrep_amd.core import _stream

KIND_PENDULUM, KIND_MOUNTAIN_CAR_CONTINUOUS = 0, 2          # include/rlrep.h RLREP_ENV_*
# kind -> (name, S, A, time limit): csrc/group_env.h rl_env_kinds
KINDS = {KIND_PENDULUM: ('Pendulum-v1', 3, 1, 200), KIND_MOUNTAIN_CAR_CONTINUOUS: ('MountainCarContinuous-v0', 2, 1, 999)}
STATE_RECORDS, STATE_COUNTERS, STATE_EVAL_STARTS = 0, 1, 2
RETURNS = 16
MAX_EPISODES = 64
MAX_ENVS = 64
EPISODE_STEPS = 200

# csrc/group_env.h EnvRecord
RECORD_DTYPE = np.dtype([('theta', '<f8'), ('theta_dot', '<f8'), ('episode_return', '<f8'), ('ring_ptr', '<i8'), ('nsteps', '<i8'), ('t', '<i4'),
                         ('ring_size', '<i4'), ('episodes_done', '<i4'), ('force', '<i4'), ('force_action', '<f4'), ('act', '<f4'),
                         ('obs', '<f4', (4,)), ('returns', '<f8', (RETURNS,)), ('pad', '<f8', (6,))])
assert RECORD_DTYPE.itemsize == 256
COUNTERS_DTYPE = np.dtype([('t_global', '<i8'), ('calls', '<u8')])


class _DeviceEnvBase(object):
    """What the device environments of a seed group (DeviceEnvGroup, R records) and of a single agent (DeviceEnv, one record) share: the
    records and counters, the returns drain and the checkpoint form.  A subclass sets PREFIX (its entry points in
    include/rlrep.h), FORM (what its snapshots say they are) and creates the handle `h` for `R` records."""

    PREFIX = None
    FORM = None

    def _setup(self, agent, kind, eps_greedy, start_timesteps, R, num_envs=1):
        name = type(self).__name__
        if kind not in KINDS:
            raise ValueError(f'{name}: kind {kind} is not built ({", ".join(f"{k} = {v[0]}" for k, v in KINDS.items())})')
        self.num_envs = int(num_envs)
        if not 1 <= self.num_envs <= MAX_ENVS:
            raise ValueError(f'{name}: num_envs {num_envs} outside [1, {MAX_ENVS}]')
        if int(start_timesteps) % self.num_envs:
            raise ValueError(f'{name}: start_timesteps {start_timesteps} is not a multiple of num_envs {self.num_envs} (a step launch is '
                             'all warm-up or none of it)')
        self.kind = int(kind)
        self.env_name, self.state_dim, self.action_dim, self.max_episode_steps = KINDS[self.kind]
        self.agent, self.R = agent, int(R)
        self.eps_greedy, self.start_timesteps = float(eps_greedy), int(start_timesteps)
        self.t_global, self.calls = 0, 0        # host mirrors of the device counters (iterate keeps them in step)
        self.h = None
        self._drained = [0] * (self.R * self.num_envs)       # finished episodes returns() has handed out, per record
        self.eval_index = 0                     # evaluations run so far (evaluate): the next one's start states

    def _create(self, *args):
        """the handle: the library's create call for one environment, create_n for several"""
        h = C.c_void_p()
        if self.num_envs == 1:
            self._call('create', *args, C.byref(h))
        else:
            self._call('create_n', *args, self.num_envs, C.byref(h))
        self.h = h

    def _call(self, name, *args):
        check(getattr(lib, self.PREFIX + name)(*args), self.PREFIX[len('rlrep_'):] + name)

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            getattr(lib, self.PREFIX + 'destroy')(h)

    def reset(self):
        """Every member starts a fresh episode; ring cursors, counters and returns are zeroed (one launch)."""
        self._call('reset', self.h, _stream())
        self._drained = [0] * (self.R * self.num_envs)
        self.t_global, self.calls = 0, 0

    # ---- records --------------------------------------------------------------------------------------------------------------------
    def _block(self, what, arr, write):
        self._call('state', self.h, what, C.c_void_p(arr.ctypes.data), arr.nbytes, 1 if write else 0, _stream())
        return arr

    def state(self):
        """[R] records (RECORD_DTYPE), [R, num_envs] with several environments; a host copy: synchronises the stream"""
        return self._block(STATE_RECORDS, np.zeros(self._records_shape(), RECORD_DTYPE), False)

    def _records_shape(self):
        return (self.R,) if self.num_envs == 1 else (self.R, self.num_envs)

    def set_state(self, records):
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        if rec.shape != self._records_shape():
            raise ValueError(f'{type(self).__name__}.set_state: needs {" x ".join(str(n) for n in self._records_shape())} records')
        self._block(STATE_RECORDS, rec, True)
        self._drained = [int(n) for n in rec['episodes_done'].reshape(-1)]

    def counters(self):
        """(t_global, calls): steps since reset, and the select_action call counter the next exploring step continues from"""
        c = self._block(STATE_COUNTERS, np.zeros(1, COUNTERS_DTYPE), False)
        return int(c['t_global'][0]), int(c['calls'][0])

    def set_counters(self, t_global, calls):
        c = np.zeros(1, COUNTERS_DTYPE)
        c['t_global'], c['calls'] = int(t_global), int(calls)
        self._block(STATE_COUNTERS, c, True)
        self.t_global, self.calls = int(t_global), int(calls)

    def advance(self):
        """the host mirrors after one replay of the step launch (num_envs steps per member); True if it was a warm-up one"""
        warm = self.t_global < self.start_timesteps
        self.t_global += self.num_envs
        return warm

    def set_cursor(self, ptr, sizes, capacity=None):
        """every member's next free ring row (the rings are filled in lockstep) and fill level, e.g. from a ReplayBufferGroup filled on the
        host.  Environment e's own cursor is (ptr + e) mod capacity: with several environments the ring's `capacity` is needed."""
        if self.num_envs > 1 and (capacity is None or int(capacity) < self.num_envs):
            raise ValueError(f'{type(self).__name__}.set_cursor: {self.num_envs} environments need the ring\'s capacity (at least {self.num_envs} rows)')
        rec = self.state().reshape(self.R, self.num_envs)
        cur = int(ptr) + np.arange(self.num_envs, dtype=np.int64)
        rec['ring_ptr'] = (cur % int(capacity) if capacity else cur)[None, :]
        rec['ring_size'] = np.asarray(sizes, np.int32).reshape(-1, 1)
        self._block(STATE_RECORDS, rec.reshape(self._records_shape()), True)

    def eval_starts(self, episodes):
        """[R, episodes, 2] (theta, theta_dot) resp. (p, v): the start states of the last evaluation (rows of retired members are stale)"""
        return self._block(STATE_EVAL_STARTS, np.zeros((self.R, int(episodes), 2), np.float64), False)

    def returns(self):
        """R lists: the returns of the episodes each member has finished since the last call (at most the last 16 per member are kept on the
        device).  Synchronises the stream: call it where the loop looks at results anyway."""
        rec = self.state().reshape(self.R, self.num_envs)
        out = []
        for r in range(self.R):
            got = []
            for e in range(self.num_envs):                  # (environment by environment)
                i = r * self.num_envs + e
                done, seen = int(rec['episodes_done'][r, e]), self._drained[i]
                first = max(seen, done - RETURNS)
                got += [float(rec['returns'][r, e][k % RETURNS]) for k in range(first, done)]
                self._drained[i] = done
            out.append(got)
        return out

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        t, calls = self.counters()
        return {'kind': self.kind, 'form': self.FORM, 'records': torch.from_numpy(self.state().view(np.uint8).copy()), 't_global': t, 'calls': calls,
                'eval_index': int(self.eval_index), 'num_envs': self.num_envs}

    def load_snapshot(self, snap):
        if snap.get('form', 'group') != self.FORM:              # (snapshots written before single agents had device environments: a group's)
            raise RuntimeError(f'checkpoint does not match this device environment (it holds the environment of a {snap.get("form", "group")}, '
                               f'this one is the environment of a {self.FORM})')
        if (snap.get('kind') != self.kind or int(snap.get('num_envs', 1)) != self.num_envs          # (a snapshot from before num_envs: one environment)
                or snap['records'].numel() != self.R * self.num_envs * RECORD_DTYPE.itemsize):
            raise RuntimeError('checkpoint does not match this device environment (kind / members / num_envs differ)')
        self.set_state(snap['records'].numpy().view(RECORD_DTYPE).reshape(self._records_shape()))
        self.set_counters(snap['t_global'], snap['calls'])
        self.eval_index = int(snap.get('eval_index', 0))


class DeviceEnvGroup(_DeviceEnvBase):
    """The device environments of kind `kind` (a key of KINDS) of seed group `agent` (a SACSeedBatch / CTRLSACSeedBatch with the kind's
    dimensions).  Created reset."""

    PREFIX, FORM = 'rlrep_group_env_', 'group'

    def __init__(self, agent, kind, eps_greedy=0.0, start_timesteps=0, num_envs=1):
        """eps_greedy: the probability of a uniform action in place of the policy's; start_timesteps: the warm-up, steps per member (counted
        since reset) that take uniform actions only, a multiple of num_envs.  Both ride by value in a captured iterate() graph.
        num_envs: environments per member, all stepped by one launch."""
        name = type(self).__name__
        if getattr(agent, 'R', None) is None or not hasattr(agent, 'seeds'):
            raise ValueError(f'{name}: needs a seed group (SACSeedBatch / CTRLSACSeedBatch)')
        self._setup(agent, kind, eps_greedy, start_timesteps, agent.R, num_envs)
        self._create(agent.core.h, self.kind)
        self.reset()

    # ---- launches -------------------------------------------------------------------------------------------------------------------
    def step(self, buffers, eps_greedy, start_timesteps):
        """One step of every environment of every live member into `buffers` (a ReplayBufferGroup): ONE launch on the current stream,
        capturable."""
        lo, hi = self.agent.action_range
        self._call('step', self.agent.core.h, self.h, C.c_void_p(buffers.rings.data_ptr()), buffers.ring_stride, buffers.max_size,
                   C.c_void_p(buffers.size_dev().data_ptr()), lo, hi, float(eps_greedy), int(start_timesteps), _stream())

    def evaluate(self, episodes, eval_index, out):
        """`episodes` mean-action episodes of every live member -> out [R, episodes] float64 (device): ONE launch"""
        self._call('evaluate', self.agent.core.h, self.h, int(episodes), int(eval_index), C.c_void_p(out.data_ptr()), _stream())


class DeviceEnv(_DeviceEnvBase):
    """The device environment of kind `kind` of ONE agent (any of the five algorithms, with the kind's dimensions): the surface of
    DeviceEnvGroup with R = 1 -- state() is one record, returns() one list, eval_starts() [1, episodes, 2].  `SACAgent.iterate(env, buffer,
    batch_size)` steps it and trains in one graph replay, `SACAgent.evaluate(env, episodes)` scores in one launch.  Its Philox key is the
    agent's seed, as select_action's is.  Created reset."""

    PREFIX, FORM = 'rlrep_env_', 'single'

    def __init__(self, agent, kind, eps_greedy=0.0, start_timesteps=0, num_envs=1):
        name = type(self).__name__
        if getattr(agent, 'R', None) is not None or not hasattr(agent, '_seed'):
            raise ValueError(f'{name}: needs a single agent (a seed group takes DeviceEnvGroup)')
        self._setup(agent, kind, eps_greedy, start_timesteps, 1, num_envs)
        self.seed = int(agent._seed)            # the Philox key of every draw: what the agent's select_action draws with
        self._create(agent.core.h, self.kind, self.seed)
        self.reset()

    def step(self, buffer, eps_greedy, start_timesteps):
        """One step of every environment into `buffer` (a ReplayBuffer): ONE launch on the current stream, capturable."""
        lo, hi = self.agent.action_range
        self._call('step', self.agent.core.h, self.h, C.c_void_p(buffer.ring.data_ptr()), buffer.max_size, C.c_void_p(buffer._size_dev.data_ptr()),
                   lo, hi, float(eps_greedy), int(start_timesteps), _stream())

    def evaluate(self, episodes, eval_index, out):
        """`episodes` mean-action episodes -> out [1, episodes] float64 (device): ONE launch"""
        self._call('evaluate', self.agent.core.h, self.h, int(episodes), int(eval_index), C.c_void_p(out.data_ptr()), _stream())


class DevicePendulumGroup(DeviceEnvGroup):
    """Pendulum-v1: 200-step episodes that never terminate (done_bool is always 0)"""

    max_episode_steps = EPISODE_STEPS

    def __init__(self, agent, eps_greedy=0.0, start_timesteps=0, num_envs=1):
        super().__init__(agent, KIND_PENDULUM, eps_greedy, start_timesteps, num_envs)


class DeviceMountainCarGroup(DeviceEnvGroup):
    """MountainCarContinuous-v0: the goal ends an episode with done_bool = 1 (unless it falls on the 999th step: the time limit does not
    count, as in main.py's host loop); the record's theta / theta_dot hold position and velocity, fp32-representable."""

    max_episode_steps = 999

    def __init__(self, agent, eps_greedy=0.0, start_timesteps=0, num_envs=1):
        super().__init__(agent, KIND_MOUNTAIN_CAR_CONTINUOUS, eps_greedy, start_timesteps, num_envs)


class DevicePendulum(DeviceEnv):
    """Pendulum-v1 for a single agent"""

    def __init__(self, agent, eps_greedy=0.0, start_timesteps=0, num_envs=1):
        super().__init__(agent, KIND_PENDULUM, eps_greedy, start_timesteps, num_envs)


class DeviceMountainCar(DeviceEnv):
    """MountainCarContinuous-v0 for a single agent"""

    def __init__(self, agent, eps_greedy=0.0, start_timesteps=0, num_envs=1):
        super().__init__(agent, KIND_MOUNTAIN_CAR_CONTINUOUS, eps_greedy, start_timesteps, num_envs)


def device_class(env_name):
    """the device environment class of --env `env_name`, or None where none is built"""
    if str(env_name).startswith('Pendulum'):
        return DevicePendulumGroup
    if str(env_name).startswith('MountainCarContinuous'):
        return DeviceMountainCarGroup
    return None


def single_device_class(env_name):
    """the device environment class of --env `env_name` for a single agent (--device-loop), or None where none is built"""
    group = device_class(env_name)
    return {DevicePendulumGroup: DevicePendulum, DeviceMountainCarGroup: DeviceMountainCar}.get(group)
