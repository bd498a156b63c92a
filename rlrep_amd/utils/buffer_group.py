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
    def __init__(self, members, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, n_step=1, n_stride=1, critic_n_step=1):
        """n_step > 1: SACSeedBatch.train() learns from n-step rows, every member with its own discount (gather_nstep); n_stride is
        the number of interleaved environments per member that write the rings (ReplayBuffer).  critic_n_step (ReplayBuffer's keyword for the
        representation agents) is refused above 1: seed groups have no n-step critic targets."""
        from rlrep_amd.utils.buffer import _check_nstep, _check_critic_nstep
        self.members = int(members)
        if self.members < 1:
            raise ValueError('ReplayBufferGroup: members must be >= 1')
        self.n_step, self.n_stride = _check_nstep(type(self).__name__, n_step, n_stride, None)
        self.critic_n_step = _check_critic_nstep(type(self).__name__, critic_n_step, self.n_step, None,
                                                 'n-step critic targets are built for one agent, not for a seed group')
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

    def nstep_key(self):
        """what a captured train() bakes in besides the rings when it gathers n-step rows"""
        return ('nstep', self.n_step, self.n_stride)

    def gather_nstep(self, r, ind, gamma):
        """Member r's n-step batch of base rows `ind` for discount `gamma`: ReplayBuffer.gather_nstep on its ring and fill level."""
        from rlrep_amd.utils.buffer import nstep_batch
        r = int(r)
        self.flush()
        size_dev = self.size_dev()[r:r + 1] if self.device.type == 'cuda' else None
        return nstep_batch(self, self.rings[r], size_dev, self.sizes[r], ind, gamma)

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
        if self.n_step > 1 and int(getattr(env, 'num_envs', 1)) != self.n_stride:
            raise ValueError(f'{type(self).__name__}.collect_on_device: n_step {self.n_step} with n_stride {self.n_stride}, but the device environment '
                             f'interleaves num_envs = {int(getattr(env, "num_envs", 1))} trajectories per ring: build the buffers with n_stride = num_envs')
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


# ---- prioritized replay for sac seed groups: DESIGN.md 6g, csrc/per_group.hip ----------------------------------------------------------
def _per_member(x, R, name):
    """a per-member hyper-parameter: a scalar broadcasts, a sequence must have one entry per member"""
    a = np.asarray(x, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, R)
    if a.size != R:
        raise ValueError(f'PrioritizedReplayBufferGroup: {name} has {a.size} entries for {R} members (a scalar, or one value per member)')
    return a.astype(np.float32)


class PrioritizedReplayBufferGroup(ReplayBufferGroup):
    """ReplayBufferGroup whose members each carry priorities in a sum tree of their own: `trees` float32[R, 2P] (P = the smallest power of
    two >= max_size; member r's tree laid out as PrioritizedReplayBuffer's), the scalars float32[R, 4] = {max_p, alpha, beta, eps} per member.
    A row written by add() / add_batch() (at flush()), add_device() or load() gets ITS member's running maximum priority; SACSeedBatch.train()
    samples every live member in proportion to its leaves, weights its critic loss and writes (|TD| + eps)^alpha back -- one launch per step
    for all members, inside the captured train().  Member r is bit for bit what SACAgent(seed=s_r) does with a PrioritizedReplayBuffer(alpha_r,
    beta_r, eps_r) fed the same rows.  `alpha`, `beta`, `eps`: a scalar or one value per member (a sweep over the exponents).  For
    SACSeedBatch.train(); everything else refuses the class by name.  On device='cpu' the same arithmetic runs in NumPy float32."""
    prioritized_group = True          # (NOT `prioritized`: that is the single ring's class, which seed groups and other agents refuse)

    def __init__(self, members, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, alpha=0.6, beta=0.4, eps=1e-6,
                 n_step=1, n_stride=1, critic_n_step=1):
        super().__init__(members, state_dim, action_dim, max_size=max_size, device=device, stage_rows=stage_rows, n_step=n_step, n_stride=n_stride,
                         critic_n_step=critic_n_step)
        R = self.members
        self.P = 1 << max(0, self.max_size - 1).bit_length()
        self.trees = torch.zeros(R, 2 * self.P, dtype=torch.float32, device=self.device)
        self._hyper = np.stack([_per_member(alpha, R, 'alpha'), _per_member(beta, R, 'beta'), _per_member(eps, R, 'eps')], axis=1)     # [R, 3] float32
        scal = np.concatenate([np.ones((R, 1), np.float32), self._hyper], axis=1)
        self._scal = torch.from_numpy(scal).to(self.device)           # [R, 4]: max_p, alpha, beta, eps
        self._draw_bufs = {}
        self.device_epoch = 0

    # ---- hyper-parameters and views --------------------------------------------------------------
    @property
    def alpha(self):
        return [float(v) for v in self._hyper[:, 0]]

    @property
    def eps(self):
        return [float(v) for v in self._hyper[:, 2]]

    @property
    def beta(self):
        return [float(v) for v in self._hyper[:, 1]]

    @beta.setter
    def beta(self, x):
        b = _per_member(x, self.members, 'beta')
        self._hyper[:, 1] = b
        self._before_device_write()
        if len(set(b.tolist())) == 1:
            self._scal[:, 2].fill_(float(b[0]))          # (a fill launch on the caller's stream: no synchronisation)
        else:
            self._scal[:, 2].copy_(torch.from_numpy(b))
        self.device_epoch += 1

    def max_priority(self, r):
        return float(self._scal[int(r), 0].cpu())

    def priorities(self, r):
        """float32[sizes[r]]: the leaves of the rows member r's ring holds (flushes staged rows; synchronises)"""
        self.flush()
        return self.trees[int(r), self.P:self.P + self.sizes[int(r)]].cpu().numpy()

    def tree(self, r):
        """member r's whole tree, float32[2P] (a view)"""
        return self.trees[int(r)]

    def per_key(self):
        """what a captured train() bakes in besides the rings: the trees and the scalar block"""
        return ('per_group', self.trees.data_ptr(), self._scal.data_ptr())

    # ---- writers: every written row gets its member's running maximum priority ---------------------
    def _lib(self):
        import ctypes as C
        from rlrep_amd._lib import lib, check
        return C, lib, check

    def _per_add(self, start, n):
        if n <= 0:
            return
        if self.device.type == 'cuda':
            C, lib, check = self._lib()
            with torch.cuda.device(self.device):
                check(lib.rlrep_group_per_add(C.c_void_p(self.trees.data_ptr()), self.P, C.c_void_p(self._scal.data_ptr()), self.members, self.max_size,
                                              int(start), int(n), C.c_void_p(_raw_stream())), 'group_per_add')
        else:
            from rlrep_amd.utils.buffer import _per_set
            rows = (int(start) + np.arange(int(n))) % self.max_size
            for r in range(self.members):
                _per_set(self.trees[r].numpy(), self.P, rows, self._scal.numpy()[r, 0])
        self.device_epoch += 1

    def _rebuild(self, r):
        if self.device.type == 'cuda':
            C, lib, check = self._lib()
            with torch.cuda.device(self.device):
                check(lib.rlrep_per_rebuild(C.c_void_p(self.trees[r].data_ptr()), self.P, C.c_void_p(_raw_stream())), 'per_rebuild')
        else:
            t = self.trees[r].numpy()
            w = self.P >> 1
            while w >= 1:
                nd = np.arange(w, 2 * w)
                t[nd] = t[2 * nd] + t[2 * nd + 1]
                w >>= 1

    def flush(self):
        a, n = self._stage_start, self._staged
        super().flush()
        self._per_add(a, n)

    def add_device(self, states, actions, next_states, rewards, dones):
        self.flush()                                 # (staged host rows first, with their leaves: the order of transitions is the call order)
        start = self.ptr
        super().add_device(states, actions, next_states, rewards, dones)
        self._per_add(start, int(rewards.shape[1]))

    def load(self, r, state, action, next_state, reward, done):
        """Member r only: its tree is zeroed first (rows the ring no longer holds lose their leaves; max_p stays), rows 0 .. n-1 get its max_p."""
        super().load(r, state, action, next_state, reward, done)
        r, n = int(r), self.sizes[int(r)]
        self.trees[r].zero_()
        if n > 0 and self.device.type == 'cuda':           # (the single ring's add on member r's slices: it takes no agent)
            C, lib, check = self._lib()
            with torch.cuda.device(self.device):
                check(lib.rlrep_per_add(C.c_void_p(self.trees[r].data_ptr()), self.P, C.c_void_p(self._scal[r].data_ptr()), self.max_size, 0, n,
                                        C.c_void_p(_raw_stream())), 'per_add')
        elif n > 0:
            from rlrep_amd.utils.buffer import _per_set
            _per_set(self.trees[r].numpy(), self.P, np.arange(n), self._scal.numpy()[r, 0])
        self.device_epoch += 1

    def collect_on_device(self, env):
        raise RuntimeError('PrioritizedReplayBufferGroup.collect_on_device: a device environment writes ring rows inside its step launch, which '
                           'knows nothing of the priority trees (iterate() takes a plain ReplayBufferGroup)')

    def set_priorities(self, r, leaves, max_priority=None):
        """Overwrite the leaves of member r's rows 0 .. len(leaves) - 1 (every other leaf of its tree becomes 0) and rebuild the tree;
        max_priority, if given, replaces the member's running maximum."""
        r = int(r)
        leaves = np.asarray(leaves, np.float32).reshape(-1)
        n = len(leaves)
        self.flush()
        if n > self.sizes[r]:
            raise ValueError(f'PrioritizedReplayBufferGroup.set_priorities: {n} leaves for a ring that holds {self.sizes[r]} rows')
        self._before_device_write()
        self.trees[r].zero_()
        if max_priority is not None:
            self._scal[r, 0:1].copy_(torch.from_numpy(np.asarray([max_priority], np.float32)))
        self.trees[r, self.P:self.P + n].copy_(torch.from_numpy(leaves))
        self._rebuild(r)
        self.device_epoch += 1

    # ---- the sampler and the priority update (SACSeedBatch calls these inside train()) -------------
    def draw_buffers(self, B):
        """(idx int32[R, B], w float32[R, B]) on the rings' device, one pair per batch size for the life of the buffer group"""
        bufs = self._draw_bufs.get(int(B))
        if bufs is None:
            bufs = self._draw_bufs[int(B)] = (torch.zeros(self.members, int(B), dtype=torch.int32, device=self.device),
                                              torch.ones(self.members, int(B), dtype=torch.float32, device=self.device))
        return bufs

    def draw(self, B, offset, core=None, use_counter=False, given=None, gather=False, seeds=None, live=None):
        """B stratified draws per live member in proportion to its priorities, and their importance weights -> (idx, w) = draw_buffers(B).
        Member r's draws are Philox stream elements 0 .. B-1 of (its seed, offset [+ its device train() counter]); `given` (int32[R, B]): take
        these indices, compute only the weights.  On the device ONE launch for all members (`core`: the sac seed group's HipCore; its seeds);
        `gather`: a second launch copies the drawn rows into every live member's minibatch slot.  On the CPU `seeds` are the members' seeds and
        `live` the members to draw for (default: all)."""
        B = int(B)
        idx, w = self.draw_buffers(B)
        if min(self.sizes) == 0:
            raise RuntimeError('PrioritizedReplayBufferGroup.draw: a member\'s buffer is empty')
        if given is not None:
            g = np.asarray(given.cpu() if torch.is_tensor(given) else given).reshape(self.members, -1)
            if g.shape[1] != B or g.min() < 0 or any(g[r].max() >= self.sizes[r] for r in range(self.members)):
                raise ValueError(f'PrioritizedReplayBufferGroup.draw: given indices must be [{self.members}, {B}] rows inside each member\'s ring')
            idx.copy_(torch.from_numpy(g.astype(np.int32)))
        if self.device.type == 'cuda':
            C, lib, check = self._lib()
            if core is None:
                raise ValueError('PrioritizedReplayBufferGroup.draw: the device sampler runs for a sac seed group (core=group.core)')
            check(lib.rlrep_group_per_sample(core.h, C.c_void_p(self.trees.data_ptr()), self.P, C.c_void_p(self._scal.data_ptr()), C.c_void_p(idx.data_ptr()),
                                             C.c_void_p(w.data_ptr()), B, 0 if given is None else 1, int(offset), 1 if use_counter else 0,
                                             C.c_void_p(self.rings.data_ptr() if gather else None), 4 * self.ring_stride, self.max_size,
                                             C.c_void_p(_raw_stream())), 'group_per_sample')
            return idx, w
        from rlrep_amd.utils.buffer import _per_draw
        from rlrep_amd.utils.philox_host import raw_stream as words
        for r in (range(self.members) if live is None else live):
            t = self.trees[r].numpy()
            if given is None:
                idx[r].copy_(torch.from_numpy(_per_draw(t, self.P, B, words(B, int(seeds[r]), int(offset)))))
            p = t[self.P + idx[r].numpy().astype(np.int64)]
            pmin, beta = p.min(), np.float32(self._hyper[r, 1])
            with np.errstate(divide='ignore', invalid='ignore'):
                wv = np.power((pmin / p).astype(np.float32), beta, dtype=np.float32)
            w[r].copy_(torch.from_numpy(np.where((p == pmin) | (beta == 0), np.float32(1.0), wv).astype(np.float32)))
        return idx, w

    def update(self, B, td=None, core=None, live=None):
        """Every live member: leaf idx[r, j] <- (td[r, j] + eps_r)^alpha_r for the last draw of B (1 when alpha_r == 0; the maximum where an
        index repeats), its max_priority follows, the ancestors are recomputed.  On the device ONE launch; td=None: the |TD| errors the
        group's last weighted critic step left, else float32[R, B]."""
        B = int(B)
        idx, _ = self.draw_buffers(B)
        if self.device.type == 'cuda':
            C, lib, check = self._lib()
            if core is None:
                raise ValueError('PrioritizedReplayBufferGroup.update: the device update runs for a sac seed group (core=group.core)')
            if td is not None and (tuple(td.shape) != (self.members, B) or td.dtype != torch.float32 or not td.is_contiguous() or td.device != self.trees.device):
                raise ValueError(f'PrioritizedReplayBufferGroup.update: td must be a contiguous float32 tensor [{self.members}, {B}] on {self.trees.device}')
            check(lib.rlrep_group_per_update(core.h, C.c_void_p(self.trees.data_ptr()), self.P, C.c_void_p(self._scal.data_ptr()), C.c_void_p(idx.data_ptr()),
                                             C.c_void_p(None if td is None else td.data_ptr()), B, C.c_void_p(_raw_stream())), 'group_per_update')
            return
        from rlrep_amd.utils.buffer import _per_set, PER_MIN_PRIORITY
        td = np.asarray(td, np.float32).reshape(self.members, B)
        s = self._scal.numpy()
        for r in (range(self.members) if live is None else live):
            t = self.trees[r].numpy()
            alpha = np.float32(self._hyper[r, 0])
            new = np.ones(B, np.float32) if alpha == 0 else np.power(td[r] + np.float32(self._hyper[r, 2]), alpha, dtype=np.float32)
            new = np.where(new > PER_MIN_PRIORITY, new, PER_MIN_PRIORITY).astype(np.float32)
            rows = idx[r].numpy().astype(np.int64)
            t[self.P + rows] = 0
            np.maximum.at(t, self.P + rows, new)
            s[r, 0] = max(s[r, 0], new.max())
            _per_set(t, self.P, rows, t[self.P + rows])
