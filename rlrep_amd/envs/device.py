"""Environments of a seed group on the device (include/rlrep.h rlrep_group_env_*; rlrep_amd/csrc/group_env.hip): Pendulum-v1
(DevicePendulumGroup) and MountainCarContinuous-v0 (DeviceMountainCarGroup, whose goal state ends an episode with done = 1).

One record per member lives on the device; `SeedBatchMixin.iterate(env, buffers, batch_size)` acts, explores, steps the dynamics, writes the
replay-ring row and trains every live member in ONE graph replay, and `SeedBatchMixin.evaluate(env, episodes)` scores every live member in one
launch.  The dynamics are those of rlrep_amd/envs/pendulum.py resp. envs/mountain_car.py (fp64 in one lane, rounded to fp32 where those
files round); the random draws are Philox streams of the member's seed, so two groups with equal seeds collect identical transitions.
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
EPISODE_STEPS = 200

# csrc/group_env.h EnvRecord
RECORD_DTYPE = np.dtype([('theta', '<f8'), ('theta_dot', '<f8'), ('episode_return', '<f8'), ('ring_ptr', '<i8'), ('nsteps', '<i8'), ('t', '<i4'),
                         ('ring_size', '<i4'), ('episodes_done', '<i4'), ('force', '<i4'), ('force_action', '<f4'), ('act', '<f4'),
                         ('obs', '<f4', (4,)), ('returns', '<f8', (RETURNS,)), ('pad', '<f8', (6,))])
assert RECORD_DTYPE.itemsize == 256
COUNTERS_DTYPE = np.dtype([('t_global', '<i8'), ('calls', '<u8')])


class DeviceEnvGroup(object):
    """The device environments of kind `kind` (a key of KINDS) of seed group `agent` (a SACSeedBatch / CTRLSACSeedBatch with the kind's
    dimensions).  Created reset."""

    def __init__(self, agent, kind, eps_greedy=0.0, start_timesteps=0):
        """eps_greedy: the probability of a uniform action in place of the policy's; start_timesteps: the warm-up, steps (counted since
        reset) that take uniform actions only.  Both ride by value in a captured iterate() graph."""
        name = type(self).__name__
        if getattr(agent, 'R', None) is None or not hasattr(agent, 'seeds'):
            raise ValueError(f'{name}: needs a seed group (SACSeedBatch / CTRLSACSeedBatch)')
        if kind not in KINDS:
            raise ValueError(f'{name}: kind {kind} is not built ({", ".join(f"{k} = {v[0]}" for k, v in KINDS.items())})')
        self.kind = int(kind)
        self.env_name, self.state_dim, self.action_dim, self.max_episode_steps = KINDS[self.kind]
        self.agent, self.R = agent, agent.R
        self.eps_greedy, self.start_timesteps = float(eps_greedy), int(start_timesteps)
        self.t_global, self.calls = 0, 0        # host mirrors of the device counters (SeedBatchMixin.iterate keeps them in step)
        h = C.c_void_p()
        check(lib.rlrep_group_env_create(agent.core.h, self.kind, C.byref(h)), 'group_env_create')
        self.h = h
        self._drained = [0] * self.R            # finished episodes returns() has handed out, per member
        self.eval_index = 0                     # evaluations run so far (SeedBatchMixin.evaluate): the next one's start states
        self.reset()

    def __del__(self):
        h, self.h = getattr(self, 'h', None), None
        if h:
            lib.rlrep_group_env_destroy(h)

    def reset(self):
        """Every member starts a fresh episode; ring cursors, counters and returns are zeroed (one launch)."""
        check(lib.rlrep_group_env_reset(self.h, _stream()), 'group_env_reset')
        self._drained = [0] * self.R
        self.t_global, self.calls = 0, 0

    # ---- records --------------------------------------------------------------------------------------------------------------------
    def _block(self, what, arr, write):
        check(lib.rlrep_group_env_state(self.h, what, C.c_void_p(arr.ctypes.data), arr.nbytes, 1 if write else 0, _stream()), 'group_env_state')
        return arr

    def state(self):
        """[R] records (RECORD_DTYPE), a host copy: synchronises the stream"""
        return self._block(STATE_RECORDS, np.zeros(self.R, RECORD_DTYPE), False)

    def set_state(self, records):
        rec = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        if rec.shape != (self.R,):
            raise ValueError(f'{type(self).__name__}.set_state: needs {self.R} records')
        self._block(STATE_RECORDS, rec, True)
        self._drained = [int(n) for n in rec['episodes_done']]

    def counters(self):
        """(t_global, calls): steps since reset, and the select_action call counter the next exploring step continues from"""
        c = self._block(STATE_COUNTERS, np.zeros(1, COUNTERS_DTYPE), False)
        return int(c['t_global'][0]), int(c['calls'][0])

    def set_counters(self, t_global, calls):
        c = np.zeros(1, COUNTERS_DTYPE)
        c['t_global'], c['calls'] = int(t_global), int(calls)
        self._block(STATE_COUNTERS, c, True)
        self.t_global, self.calls = int(t_global), int(calls)

    def set_cursor(self, ptr, sizes):
        """every member's ring cursor (the rings are filled in lockstep) and fill level, e.g. from a ReplayBufferGroup filled on the host"""
        rec = self.state()
        rec['ring_ptr'], rec['ring_size'] = int(ptr), np.asarray(sizes, np.int32)
        self._block(STATE_RECORDS, rec, True)

    def eval_starts(self, episodes):
        """[R, episodes, 2] (theta, theta_dot) resp. (p, v): the start states of the last evaluation (rows of retired members are stale)"""
        return self._block(STATE_EVAL_STARTS, np.zeros((self.R, int(episodes), 2), np.float64), False)

    def returns(self):
        """R lists: the returns of the episodes each member has finished since the last call (at most the last 16 per member are kept on the
        device).  Synchronises the stream: call it where the loop looks at results anyway."""
        rec = self.state()
        out = []
        for r in range(self.R):
            done, seen = int(rec['episodes_done'][r]), self._drained[r]
            first = max(seen, done - RETURNS)
            out.append([float(rec['returns'][r][k % RETURNS]) for k in range(first, done)])
            self._drained[r] = done
        return out

    # ---- launches -------------------------------------------------------------------------------------------------------------------
    def step(self, buffers, eps_greedy, start_timesteps):
        """One step of every live member into `buffers` (a ReplayBufferGroup): ONE launch on the current stream, capturable."""
        lo, hi = self.agent.action_range
        check(lib.rlrep_group_env_step(self.agent.core.h, self.h, C.c_void_p(buffers.rings.data_ptr()), buffers.ring_stride, buffers.max_size,
                                       C.c_void_p(buffers.size_dev().data_ptr()), lo, hi, float(eps_greedy), int(start_timesteps), _stream()),
              'group_env_step')

    def evaluate(self, episodes, eval_index, out):
        """`episodes` mean-action episodes of every live member -> out [R, episodes] float64 (device): ONE launch"""
        check(lib.rlrep_group_env_evaluate(self.agent.core.h, self.h, int(episodes), int(eval_index), C.c_void_p(out.data_ptr()), _stream()),
              'group_env_evaluate')

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        t, calls = self.counters()
        return {'kind': self.kind, 'records': torch.from_numpy(self.state().view(np.uint8).copy()), 't_global': t, 'calls': calls,
                'eval_index': int(self.eval_index)}

    def load_snapshot(self, snap):
        if snap.get('kind') != self.kind or snap['records'].numel() != self.R * RECORD_DTYPE.itemsize:
            raise RuntimeError('checkpoint does not match this device environment (kind / members differ)')
        self.set_state(snap['records'].numpy().view(RECORD_DTYPE))
        self.set_counters(snap['t_global'], snap['calls'])
        self.eval_index = int(snap.get('eval_index', 0))


class DevicePendulumGroup(DeviceEnvGroup):
    """Pendulum-v1: 200-step episodes that never terminate (done_bool is always 0)"""

    max_episode_steps = EPISODE_STEPS

    def __init__(self, agent, eps_greedy=0.0, start_timesteps=0):
        super().__init__(agent, KIND_PENDULUM, eps_greedy, start_timesteps)


class DeviceMountainCarGroup(DeviceEnvGroup):
    """MountainCarContinuous-v0: the goal ends an episode with done_bool = 1 (unless it falls on the 999th step: the time limit does not
    count, as in main.py's host loop); the record's theta / theta_dot hold position and velocity, fp32-representable."""

    max_episode_steps = 999

    def __init__(self, agent, eps_greedy=0.0, start_timesteps=0):
        super().__init__(agent, KIND_MOUNTAIN_CAR_CONTINUOUS, eps_greedy, start_timesteps)


def device_class(env_name):
    """the device environment class of --env `env_name`, or None where none is built"""
    if str(env_name).startswith('Pendulum'):
        return DevicePendulumGroup
    if str(env_name).startswith('MountainCarContinuous'):
        return DeviceMountainCarGroup
    return None
