"""Replay rings of a seed group (rlrep_amd/agent/sac/seed_batch.py): one device ring `[R, max_size, row]`, member r's ring at a constant stride.

Every member sees its own transitions; in the environment loop the members step in lockstep, so `add` takes one transition per member and
`flush` moves the staged rows of ALL members into their rings with one launch (rlrep_group_replay_add_sized), which also writes every
member's fill level into `size_dev()[r]` -- the word member r's train prologue bounds its indices by.  Rows are laid out as in ReplayBuffer:
[state | action | next_state | reward | done].
"""
import numpy as np
import torch

from rlrep_amd.utils.streams import raw_stream as _raw_stream


class ReplayBufferGroup(object):
    def __init__(self, members, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096):
        self.members = int(members)
        if self.members < 1:
            raise ValueError('ReplayBufferGroup: members must be >= 1')
        self.max_size = int(max_size)
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        self.row = 2 * self.state_dim + self.action_dim + 2
        self.device = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self.rings = torch.zeros(self.members, self.max_size, self.row, dtype=torch.float32, device=self.device)
        self.ring_stride = self.max_size * self.row                 # floats between two members' rings
        pin = self.device.type == 'cuda'
        self._stage = torch.zeros(self.members, min(int(stage_rows), self.max_size), self.row, dtype=torch.float32, pin_memory=pin)
        self._stage_np = self._stage.numpy()
        self._staged = 0               # rows per member waiting in the staging buffer
        self._stage_start = 0          # ring position of the first staged row (the same for every member: lockstep)
        self._copy_done = None
        self.ptr = 0
        self.sizes = [0] * self.members
        self._size_dev = torch.zeros(self.members, dtype=torch.int32, device=self.device)
        self._size_pushed = None
        self.before_device_write_hooks = []
        self._device_env = None        # the device environment that owns the cursor (collect_on_device); None: the host does

    # ---- what the agent reads ----------------------------------------------------------------
    @property
    def ring(self):
        """member 0's ring: the address the group's programs are built against (member r's is ring_stride floats further)"""
        return self.rings[0]

    @property
    def size(self):
        return self.sizes[0]

    def size_dev(self):
        """int32[R] device words: member r's fill level"""
        if self._size_pushed != self.sizes:
            self._before_device_write()
            self._size_dev.copy_(torch.tensor(self.sizes, dtype=torch.int32))
            self._size_pushed = list(self.sizes)
        return self._size_dev

    def _before_device_write(self):
        for h in self.before_device_write_hooks:
            h()

    # ---- filling ------------------------------------------------------------------------------
    def add(self, state, action, next_state, reward, done):
        """One transition per member: state / next_state [R, S], action [R, A], reward / done [R]."""
        if self._device_env is not None:
            raise RuntimeError('ReplayBufferGroup.add: a device environment has been advancing these rings (SeedBatchMixin.iterate), so the host '
                               'cursor is stale: call adopt_device_cursor() first')
        if self._staged == self._stage.shape[1]:
            self.flush()
        if self._copy_done is not None:
            self._copy_done.synchronize()
            self._copy_done = None
        if self._staged == 0:
            self._stage_start = self.ptr
        S, A, R = self.state_dim, self.action_dim, self.members
        r = self._stage_np[:, self._staged]
        r[:, :S] = np.asarray(state, np.float32).reshape(R, S)
        r[:, S:S + A] = np.asarray(action, np.float32).reshape(R, A)
        r[:, S + A:2 * S + A] = np.asarray(next_state, np.float32).reshape(R, S)
        r[:, 2 * S + A] = np.asarray(reward, np.float32).reshape(R)
        r[:, 2 * S + A + 1] = np.asarray(done, np.float32).reshape(R)
        self._staged += 1
        self.ptr = (self.ptr + 1) % self.max_size
        self.sizes = [min(s + 1, self.max_size) for s in self.sizes]

    def add_batch(self, states, actions, next_states, rewards, dones):
        """E transitions per member in one call: states / next_states [R, E, S], actions [R, E, A], rewards / dones [R, E].  Equal in every
        observable to E add() calls in row order (rings after flush(), ptr, sizes), also where the batch wraps the rings or is larger than the
        staging buffer."""
        if self._device_env is not None:
            raise RuntimeError('ReplayBufferGroup.add_batch: a device environment has been advancing these rings (SeedBatchMixin.iterate), so the host '
                               'cursor is stale: call adopt_device_cursor() first')
        S, A, R = self.state_dim, self.action_dim, self.members
        E = int(np.shape(rewards)[1])
        rows = np.empty((R, E, self.row), np.float32)
        rows[:, :, :S] = np.asarray(states).reshape(R, E, S)
        rows[:, :, S:S + A] = np.asarray(actions).reshape(R, E, A)
        rows[:, :, S + A:2 * S + A] = np.asarray(next_states).reshape(R, E, S)
        rows[:, :, 2 * S + A] = np.asarray(rewards).reshape(R, E)
        rows[:, :, 2 * S + A + 1] = np.asarray(dones).reshape(R, E)
        cap, k = self._stage.shape[1], 0
        while k < E:
            if self._staged == cap:
                self.flush()
            if self._copy_done is not None:
                self._copy_done.synchronize()
                self._copy_done = None
            if self._staged == 0:
                self._stage_start = self.ptr
            n = min(E - k, cap - self._staged)
            self._stage_np[:, self._staged:self._staged + n] = rows[:, k:k + n]
            self._staged += n
            self.ptr = (self.ptr + n) % self.max_size
            self.sizes = [min(s + n, self.max_size) for s in self.sizes]
            k += n

    def add_device(self, states, actions, next_states, rewards, dones):
        """N device-resident transitions per member: states / next_states [R, N, S], actions [R, N, A], rewards / dones [R, N], tensors on the
        rings' device.  ONE launch (rlrep_group_replay_add_cols) packs member r's plane into its ring from row ptr on (wrapping) and writes
        every member's fill level; staged host rows are flushed first.  Like flush(), it does not look at retired members."""
        if self._device_env is not None:
            raise RuntimeError('ReplayBufferGroup.add_device: a device environment has been advancing these rings (SeedBatchMixin.iterate), so the host '
                               'cursor is stale: call adopt_device_cursor() first')
        S, A, R = self.state_dim, self.action_dim, self.members
        if rewards.dim() < 2 or rewards.shape[0] != R:
            raise ValueError(f'ReplayBufferGroup.add_device: rewards {tuple(rewards.shape)} is not [{R}, N]')
        N = int(rewards.shape[1])
        if not 1 <= N <= self.max_size:
            raise ValueError(f'ReplayBufferGroup.add_device: {N} transitions for rings of {self.max_size} rows (N must lie in [1, max_size])')

        def prep(t, shape, name):
            if not torch.is_tensor(t) or t.device != self.rings.device:
                raise ValueError(f'ReplayBufferGroup.add_device: {name} must be a tensor on {self.rings.device}')
            return t.to(torch.float32).reshape(shape).contiguous()
        s, a, s2 = prep(states, (R, N, S), 'states'), prep(actions, (R, N, A), 'actions'), prep(next_states, (R, N, S), 'next_states')
        r, d = prep(rewards, (R, N), 'rewards'), prep(dones, (R, N), 'dones')
        self.flush()
        if len(set(self.sizes)) != 1:
            raise RuntimeError('ReplayBufferGroup.add_device after load() gave the members different fill levels: the lockstep ring takes N rows per member')
        start = self.ptr
        self.ptr = (self.ptr + N) % self.max_size
        self.sizes = [min(v + N, self.max_size) for v in self.sizes]
        self._before_device_write()
        if self.device.type == 'cuda':
            import ctypes as C
            from rlrep_amd._lib import lib, check
            check(lib.rlrep_group_replay_add_cols(C.c_void_p(self.rings.data_ptr()), self.max_size, self.row, start, S, A, C.c_void_p(s.data_ptr()), S,
                                                  C.c_void_p(a.data_ptr()), A, C.c_void_p(s2.data_ptr()), S, C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), N,
                                                  R, self.ring_stride, C.c_void_p(self._size_dev.data_ptr()), self.sizes[0], C.c_void_p(_raw_stream())),
                  'group_replay_add_cols')
            self._size_pushed = list(self.sizes)
            self._copy_done = torch.cuda.Event()
            self._copy_done.record()
        else:
            idx = (start + torch.arange(N)) % self.max_size
            self.rings[:, idx] = torch.cat([s, a, s2, r.reshape(R, N, 1), d.reshape(R, N, 1)], dim=2)

    def flush(self):
        n = self._staged
        if n == 0:
            return
        a = self._stage_start
        self._before_device_write()
        if self.device.type == 'cuda':
            import ctypes as C
            from rlrep_amd._lib import lib, check
            if len(set(self.sizes)) != 1:
                raise RuntimeError('ReplayBufferGroup.add after load() gave the members different fill levels: the lockstep ring takes one row per member')
            # member r's staged rows are block r of the pinned staging buffer [R, stage_rows, row]
            check(lib.rlrep_group_replay_add_sized(C.c_void_p(self.rings.data_ptr()), self.ring_stride, self.members, self.max_size, self.row, a,
                                                   C.c_void_p(self._stage.data_ptr()), self._stage.shape[1] * self.row, n, C.c_void_p(self._size_dev.data_ptr()), self.sizes[0],
                                                   C.c_void_p(_raw_stream())), 'group_replay_add_sized')
            self._size_pushed = list(self.sizes)
            self._copy_done = torch.cuda.Event()
            self._copy_done.record()
        else:
            first = min(n, self.max_size - a)
            self.rings[:, a:a + first].copy_(self._stage[:, :first])
            if first < n:
                self.rings[:, :n - first].copy_(self._stage[:, first:n])
        self._staged = 0

    # ---- device collection (rlrep_amd/envs/device.py) -----------------------------------------------------------------------------
    def collect_on_device(self, env):
        """Hand the cursor to device environment `env`: staged rows are flushed, the environment's records take (ptr, sizes), and from here on
        the step launches advance the rings and the fill levels in size_dev().  add() refuses until adopt_device_cursor()."""
        if self._device_env is env:
            return
        if self._device_env is not None:
            raise RuntimeError('ReplayBufferGroup.collect_on_device: another device environment owns the cursor (adopt_device_cursor() first)')
        self.flush()
        self.size_dev()
        if getattr(env, 'num_envs', 1) > 1:          # (environment e's cursor is (ptr + e) mod max_size)
            env.set_cursor(self.ptr, self.sizes, self.max_size)
        else:
            env.set_cursor(self.ptr, self.sizes)
        self._device_env = env

    def adopt_device_cursor(self):
        """Take the cursor back from the device environment: ptr and sizes become what its records hold (synchronises), and add() continues
        behind the last row the device wrote.  The host ring advances in lockstep, so members whose cursors differ (some were retired
        while the device collected) are refused."""
        env = self._device_env
        if env is None:
            return
        rec = env.state().reshape(self.members, -1)[:, 0]           # (environment 0's cursor is the member's next free row)
        ptrs = sorted(set(int(p) for p in rec['ring_ptr']))
        if len(ptrs) != 1:
            raise RuntimeError(f'ReplayBufferGroup.adopt_device_cursor: the members\' ring cursors differ ({ptrs}): the host ring takes one row per '
                               'member in lockstep')
        self.ptr = ptrs[0] % self.max_size
        self.sizes = [int(n) for n in rec['ring_size']]
        self._size_pushed = list(self.sizes)          # (the step launches have published them)
        self._device_env = None

    def load(self, r, state, action, next_state, reward, done):
        """Bulk-fill member r's ring (tests / synthetic benchmarks), as ReplayBuffer.load does for one ring."""
        n = int(len(state))
        rows = np.concatenate([np.asarray(state, np.float32).reshape(n, -1), np.asarray(action, np.float32).reshape(n, -1),
                               np.asarray(next_state, np.float32).reshape(n, -1), np.asarray(reward, np.float32).reshape(n, 1),
                               np.asarray(done, np.float32).reshape(n, 1)], axis=1)
        self.flush()
        self._before_device_write()
        self.rings[int(r), :n].copy_(torch.from_numpy(rows))
        self.sizes[int(r)] = n
        self.ptr, self._staged = n % self.max_size, 0
