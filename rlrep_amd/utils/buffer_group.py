"""Replay rings of a seed group (rlrep_amd/agent/sac/seed_batch.py): one device ring `[R, max_size, row]`, member r's ring at a constant stride.

Every member sees its own transitions; in the environment loop the members step in lockstep, so `add` takes one transition per member and
`flush` moves the staged rows of ALL members into their rings with one launch (rlrep_group_replay_add_sized), which also writes every
member's fill level into `size_dev()[r]` -- the word member r's train prologue bounds its indices by.  Rows are laid out as in ReplayBuffer:
[state | action | next_state | reward | done].
"""
import numpy as np
import torch

from rlrep_amd.utils._ring import Ring, lib_call
from rlrep_amd.utils.buffer import _check_critic_nstep, _check_nstep, _per_draw, _per_rebuild_host, _per_set, _per_update_host, _per_weights, nstep_batch


class ReplayBufferGroup(Ring):
    _NAME, _ADVANCING, _INTERLEAVES = 'ReplayBufferGroup', 'these rings (SeedBatchMixin.iterate)', ('per ring', 'the buffers')

    def __init__(self, members, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, n_step=1, n_stride=1, critic_n_step=1):
        """n_step > 1: SACSeedBatch.train() learns from n-step rows, every member with its own discount (gather_nstep); n_stride is
        the number of interleaved environments per member that write the rings (ReplayBuffer).  critic_n_step (ReplayBuffer's keyword for the
        representation agents) is refused above 1: seed groups have no n-step critic targets."""
        self.members = int(members)
        if self.members < 1:
            raise ValueError('ReplayBufferGroup: members must be >= 1')
        n_step, n_stride = _check_nstep(type(self).__name__, n_step, n_stride, None)
        critic_n_step = _check_critic_nstep(type(self).__name__, critic_n_step, n_step, None,
                                            'n-step critic targets are built for one agent, not for a seed group')
        super().__init__((self.members,), state_dim, action_dim, max_size, device, stage_rows, n_step, n_stride, critic_n_step)
        self.rings = self._new_ring((self.members,))
        self.ring_stride = self.max_size * self.row                 # floats between two members' rings
        self.sizes = [0] * self.members
        self._size_dev = torch.zeros(self.members, dtype=torch.int32, device=self.device)
        self._size_pushed = None

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

    def _advance(self, n):
        self.sizes = [min(s + n, self.max_size) for s in self.sizes]

    def _fill_levels(self):
        return self.sizes

    def gather_nstep(self, r, ind, gamma):
        """Member r's n-step batch of base rows `ind` for discount `gamma`: ReplayBuffer.gather_nstep on its ring and fill level."""
        r = int(r)
        self.flush()
        size_dev = self.size_dev()[r:r + 1] if self.device.type == 'cuda' else None
        return nstep_batch(self, self.rings[r], size_dev, self.sizes[r], ind, gamma)

    # ---- filling ------------------------------------------------------------------------------
    def add(self, state, action, next_state, reward, done):
        """One transition per member: state / next_state [R, S], action [R, A], reward / done [R]."""
        if self._device_env is not None:
            raise self._stale('add')
        self._stage_ready()
        self._pack_rows((self.members,), state, action, next_state, reward, done, out=self._stage_np[:, self._staged])
        self._staged += 1
        self.ptr = (self.ptr + 1) % self.max_size
        self._advance(1)

    def add_batch(self, states, actions, next_states, rewards, dones):
        """E transitions per member in one call: states / next_states [R, E, S], actions [R, E, A], rewards / dones [R, E].  Equal in every
        observable to E add() calls in row order (rings after flush(), ptr, sizes), also where the batch wraps the rings or is larger than the
        staging buffer."""
        if self._device_env is not None:
            raise self._stale('add_batch')
        E = int(np.shape(rewards)[1])
        self._stage_rows(self._pack_rows((self.members, E), states, actions, next_states, rewards, dones))

    def add_device(self, states, actions, next_states, rewards, dones):
        """N device-resident transitions per member: states / next_states [R, N, S], actions [R, N, A], rewards / dones [R, N], tensors on the
        rings' device.  ONE launch (rlrep_group_replay_add_cols) packs member r's plane into its ring from row ptr on (wrapping) and writes
        every member's fill level; staged host rows are flushed first.  Like flush(), it does not look at retired members."""
        if self._device_env is not None:
            raise self._stale('add_device')
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
        self._advance(N)
        self._before_device_write()
        if self.device.type == 'cuda':
            lib_call(self.device, 'group_replay_add_cols', self.rings.data_ptr(), self.max_size, self.row, start, S, A, s.data_ptr(), S, a.data_ptr(), A,
                     s2.data_ptr(), S, r.data_ptr(), d.data_ptr(), N, R, self.ring_stride, self._size_dev.data_ptr(), self.sizes[0], then=self._wrote)
        else:
            self._write_wrapped(self.rings, start, torch.from_numpy(self._pack_rows((R, N), s, a, s2, r, d)))

    def _wrote(self):
        """after a launch that wrote ring rows and the fill levels: the levels are published, and add() waits for this event before it
        reuses the stage (a fresh event per launch; ReplayBuffer reuses one)"""
        self._size_pushed = list(self.sizes)
        self._copy_done = torch.cuda.Event()
        self._copy_done.record()

    def flush(self):
        n = self._staged
        if n == 0:
            return
        self._before_device_write()
        if self.device.type == 'cuda':
            if len(set(self.sizes)) != 1:
                raise RuntimeError('ReplayBufferGroup.add after load() gave the members different fill levels: the lockstep ring takes one row per member')
            # member r's staged rows are block r of the pinned staging buffer [R, stage_rows, row]
            lib_call(self.device, 'group_replay_add_sized', self.rings.data_ptr(), self.ring_stride, self.members, self.max_size, self.row,
                     self._stage_start, self._stage.data_ptr(), self._stage_cap * self.row, n, self._size_dev.data_ptr(), self.sizes[0], then=self._wrote)
        else:
            self._write_wrapped(self.rings, self._stage_start, self._stage[:, :n])
        self._staged = 0

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
        rows = self._pack_rows((n,), state, action, next_state, reward, done)
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
    def _per_add(self, start, n):
        if n <= 0:
            return
        if self.device.type == 'cuda':
            lib_call(self.device, 'group_per_add', self.trees.data_ptr(), self.P, self._scal.data_ptr(), self.members, self.max_size, int(start), int(n))
        else:
            rows = (int(start) + np.arange(int(n))) % self.max_size
            for r in range(self.members):
                _per_set(self.trees[r].numpy(), self.P, rows, self._scal.numpy()[r, 0])
        self.device_epoch += 1

    def _rebuild(self, r):
        if self.device.type == 'cuda':
            lib_call(self.device, 'per_rebuild', self.trees[r].data_ptr(), self.P)
        else:
            _per_rebuild_host(self.trees[r].numpy(), self.P)

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
            lib_call(self.device, 'per_add', self.trees[r].data_ptr(), self.P, self._scal[r].data_ptr(), self.max_size, 0, n)
        elif n > 0:
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
        idx, w = self.draw_buffers(B)[:2]          # (a subclass may keep more arrays beside them)
        if min(self.sizes) == 0:
            raise RuntimeError('PrioritizedReplayBufferGroup.draw: a member\'s buffer is empty')
        if given is not None:
            g = np.asarray(given.cpu() if torch.is_tensor(given) else given).reshape(self.members, -1)
            if g.shape[1] != B or g.min() < 0 or any(g[r].max() >= self.sizes[r] for r in range(self.members)):
                raise ValueError(f'PrioritizedReplayBufferGroup.draw: given indices must be [{self.members}, {B}] rows inside each member\'s ring')
            idx.copy_(torch.from_numpy(g.astype(np.int32)))
        if self.device.type == 'cuda':
            if core is None:
                raise ValueError('PrioritizedReplayBufferGroup.draw: the device sampler runs for a sac seed group (core=group.core)')
            lib_call(self.device, 'group_per_sample', core.h, self.trees.data_ptr(), self.P, self._scal.data_ptr(), idx.data_ptr(), w.data_ptr(), B,
                     0 if given is None else 1, int(offset), 1 if use_counter else 0, self.rings.data_ptr() if gather else None, 4 * self.ring_stride,
                     self.max_size)
            return idx, w
        from rlrep_amd.utils.philox_host import raw_stream as words
        for r in (range(self.members) if live is None else live):
            t = self.trees[r].numpy()
            if given is None:
                idx[r].copy_(torch.from_numpy(_per_draw(t, self.P, B, words(B, int(seeds[r]), int(offset)))))
            w[r].copy_(torch.from_numpy(_per_weights(t, self.P, idx[r].numpy(), self._hyper[r, 1])))
        return idx, w

    def update(self, B, td=None, core=None, live=None):
        """Every live member: leaf idx[r, j] <- (td[r, j] + eps_r)^alpha_r for the last draw of B (1 when alpha_r == 0; the maximum where an
        index repeats), its max_priority follows, the ancestors are recomputed.  On the device ONE launch; td=None: the |TD| errors the
        group's last weighted critic step left, else float32[R, B]."""
        B = int(B)
        idx = self.draw_buffers(B)[0]
        if self.device.type == 'cuda':
            if core is None:
                raise ValueError('PrioritizedReplayBufferGroup.update: the device update runs for a sac seed group (core=group.core)')
            if td is not None and (tuple(td.shape) != (self.members, B) or td.dtype != torch.float32 or not td.is_contiguous() or td.device != self.trees.device):
                raise ValueError(f'PrioritizedReplayBufferGroup.update: td must be a contiguous float32 tensor [{self.members}, {B}] on {self.trees.device}')
            lib_call(self.device, 'group_per_update', core.h, self.trees.data_ptr(), self.P, self._scal.data_ptr(), idx.data_ptr(),
                     None if td is None else td.data_ptr(), B)
            return
        td = np.asarray(td, np.float32).reshape(self.members, B)
        for r in (range(self.members) if live is None else live):
            _per_update_host(self.trees[r].numpy(), self.P, self._scal.numpy()[r], idx[r].numpy(), td[r], self._hyper[r, 0], self._hyper[r, 2])


# ---- prioritized replay of the critic's minibatch for ctrlsac seed groups: DESIGN.md 6g.1, csrc/per_group.hip ----------------------
class CriticPrioritizedReplayBufferGroup(PrioritizedReplayBufferGroup):
    """PrioritizedReplayBufferGroup for CTRLSACSeedBatch, with CriticPrioritizedReplayBuffer's sampling contract -- hence another name.  A
    ctrlsac member runs its critic and actor steps on the slot-0 minibatch of its LAST feature step; that minibatch alone is drawn from the
    member's tree, the member's critic loss takes its importance weights and the |TD| errors come back as priorities in the same captured
    train().  Every other feature minibatch and all the noise stay the draws a plain ReplayBufferGroup gives at the same seeds and step.
    Member r is bit for bit what CTRLSACAgent(seed=s_r, pipeline=False) does with a CriticPrioritizedReplayBuffer(alpha_r, beta_r, eps_r) fed
    the same rows.  The trees, the scalars and the writers are the parent's; the draw buffers gain td float32[R, B], which the weighted
    critic head writes and update() reads.  For CTRLSACSeedBatch.train() / prepare(); everything else refuses the class by name."""
    prioritized_group = False         # (NOT the parent's contract: what takes a PrioritizedReplayBufferGroup must not mistake this class for one)
    critic_prioritized_group = True

    def __init__(self, members, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, alpha=0.6, beta=0.4, eps=1e-6,
                 n_step=1, n_stride=1, critic_n_step=1):
        if not isinstance(n_step, bool) and int(n_step) == n_step and int(n_step) > 1:
            raise ValueError(f'CriticPrioritizedReplayBufferGroup: n_step {int(n_step)} > 1 is not supported (n_step is the whole minibatch of a sac '
                             'seed group, which takes a PrioritizedReplayBufferGroup)')
        super().__init__(members, state_dim, action_dim, max_size=max_size, device=device, stage_rows=stage_rows, alpha=alpha, beta=beta, eps=eps,
                         n_step=n_step, n_stride=n_stride, critic_n_step=critic_n_step)

    def per_key(self):
        """what a captured train() bakes in besides the rings: the trees and the scalar block, under this class's own tag"""
        return ('critic_per_group', self.trees.data_ptr(), self._scal.data_ptr())

    def collect_on_device(self, env):
        raise RuntimeError('CriticPrioritizedReplayBufferGroup.collect_on_device: a device environment writes ring rows inside its step launch, '
                           'which knows nothing of the priority trees (iterate() takes a plain ReplayBufferGroup)')

    def draw_buffers(self, B):
        """(idx int32[R, B], w float32[R, B], td float32[R, B]) on the rings' device, one triple per batch size for the life of the buffer group"""
        bufs = self._draw_bufs.get(int(B))
        if bufs is None:
            bufs = self._draw_bufs[int(B)] = super().draw_buffers(B) + (torch.zeros(self.members, int(B), dtype=torch.float32, device=self.device),)
        return bufs

    def draw(self, B, offset, core=None, use_counter=False, given=None, gather=False, seeds=None, live=None):
        """The parent's host draw (device='cpu'); on the device the sampler of this class is draw_fill (the parent's two launches are a sac
        seed group's)."""
        if self.device.type == 'cuda':
            raise RuntimeError('CriticPrioritizedReplayBufferGroup.draw: the device sampler of this class is draw_fill (one launch with the gather)')
        idx, w, _ = self.draw_buffers(B)
        super().draw(B, offset, given=given, seeds=seeds, live=live)
        return idx, w

    def draw_fill(self, core, B, offset, use_counter=False, given=None):
        """The critic's minibatch of every live member of a ctrlsac seed group (`core`: the group's HipCore): B stratified draws per member and
        their importance weights as draw() computes them, and the drawn ring rows gathered into the member's minibatch slot 0 -- ONE launch
        on the current stream (rlrep_group_per_sample_fill).  `given` (int32[R, B]): take these indices, compute only the weights, gather.
        -> (idx, w)."""
        B = int(B)
        if min(self.sizes) == 0:
            raise RuntimeError('CriticPrioritizedReplayBufferGroup.draw_fill: a member\'s buffer is empty')
        if self.device.type != 'cuda' or core is None:
            raise ValueError('CriticPrioritizedReplayBufferGroup.draw_fill: the fused launch runs for a ctrlsac seed group on the device '
                             '(core=group.core); on device=\'cpu\' use draw()')
        idx, w, _ = self.draw_buffers(B)
        if given is not None:
            g = np.asarray(given.cpu() if torch.is_tensor(given) else given).reshape(self.members, -1)
            if g.shape[1] != B or g.min() < 0 or any(g[r].max() >= self.sizes[r] for r in range(self.members)):
                raise ValueError(f'CriticPrioritizedReplayBufferGroup.draw_fill: given indices must be [{self.members}, {B}] rows inside each '
                                 'member\'s ring')
            idx.copy_(torch.from_numpy(g.astype(np.int32)))
        lib_call(self.device, 'group_per_sample_fill', core.h, self.rings.data_ptr(), 4 * self.ring_stride, self.max_size, self.trees.data_ptr(), self.P,
                 self._scal.data_ptr(), idx.data_ptr(), w.data_ptr(), B, 0 if given is None else 1, int(offset), 1 if use_counter else 0)
        return idx, w

    def update(self, B, td=None, core=None, live=None):
        """The parent's update() from this buffer group's own td array (td=None: what the last weighted critic step wrote there).  On the
        device ONE launch for all live members (rlrep_group_per_update_td; `core`: the ctrlsac seed group's HipCore)."""
        B = int(B)
        idx, _, own = self.draw_buffers(B)
        td = own if td is None else td
        if self.device.type == 'cuda':
            if core is None:
                raise ValueError('CriticPrioritizedReplayBufferGroup.update: the device update runs for a ctrlsac seed group (core=group.core)')
            if tuple(td.shape) != (self.members, B) or td.dtype != torch.float32 or not td.is_contiguous() or td.device != self.trees.device:
                raise ValueError(f'CriticPrioritizedReplayBufferGroup.update: td must be a contiguous float32 tensor [{self.members}, {B}] on '
                                 f'{self.trees.device}')
            lib_call(self.device, 'group_per_update_td', core.h, self.trees.data_ptr(), self.P, self._scal.data_ptr(), idx.data_ptr(), td.data_ptr(), B)
            return
        super().update(B, td.numpy() if torch.is_tensor(td) else td, live=live)
