"""Device-resident replay ring behind the reference's `ReplayBuffer` API (utils/buffer.py:13-48).

The reference keeps five float64 NumPy rings on the host and, on every `sample`, fancy-indexes them,
casts to float32 and issues five host->device copies.  Here the transitions live on the MI355X as ONE
fp32 array-of-structs ring, row = [state | action | next_state | reward | done] (2S+A+2 floats), so that
a minibatch is gathered by a single kernel (`rlrep_replay_sample`) and the concatenated network inputs
[s,a,s'] / [s,a] are prefixes of a row.  `add` stages rows in pinned host memory and flushes them with
one asynchronous copy per `sample`/`flush`.
"""
import collections
import numpy as np
import torch
from rlrep_amd.utils._ring import Ring, lib_call
from rlrep_amd.utils.streams import current_stream as _current_stream

Batch = collections.namedtuple('Batch', ['state', 'action', 'reward', 'next_state', 'done'])


NSTEP_MAX = 16       # include/rlrep.h RLREP_NSTEP_MAX


def _check_nstep(cls, n_step, n_stride, shard):
    if isinstance(n_step, bool) or isinstance(n_stride, bool) or int(n_step) != n_step or int(n_stride) != n_stride:
        raise ValueError(f'{cls}: n_step {n_step!r} and n_stride {n_stride!r} must be integers')
    n_step, n_stride = int(n_step), int(n_stride)
    if not 1 <= n_step <= NSTEP_MAX:
        raise ValueError(f'{cls}: n_step {n_step} outside [1, {NSTEP_MAX}]')
    if n_stride < 1:
        raise ValueError(f'{cls}: n_stride {n_stride} must be >= 1 (the number of interleaved environments that write the ring)')
    if n_step > 1 and shard is not None:
        raise ValueError(f'{cls}: shard= is not supported with n_step {n_step} > 1 (a shard keeps one transition in `world`: its rows are no trajectory)')
    return n_step, n_stride


def _check_critic_nstep(cls, critic_n_step, n_step, shard, refuse=None):
    """critic_n_step: the chain length of the critic targets of the representation agents.  `refuse`: why this class takes
    none (prioritized and group buffers)."""
    if isinstance(critic_n_step, bool) or int(critic_n_step) != critic_n_step:
        raise ValueError(f'{cls}: critic_n_step {critic_n_step!r} must be an integer')
    critic_n_step = int(critic_n_step)
    if not 1 <= critic_n_step <= NSTEP_MAX:
        raise ValueError(f'{cls}: critic_n_step {critic_n_step} outside [1, {NSTEP_MAX}]')
    if critic_n_step > 1 and n_step > 1:
        raise ValueError(f'{cls}: n_step {n_step} and critic_n_step {critic_n_step} together (n_step is the whole minibatch of a sac agent, '
                         'critic_n_step the critic targets of vlsac / ctrlsac / spedersac / diffsrsac: a buffer trains one kind of agent)')
    if critic_n_step > 1 and refuse is not None:
        raise ValueError(f'{cls}: critic_n_step {critic_n_step} > 1 is not supported ({refuse}): use a plain ReplayBuffer')
    if critic_n_step > 1 and shard is not None:
        raise ValueError(f'{cls}: shard= is not supported with critic_n_step {critic_n_step} > 1 (a shard keeps one transition in `world`: its '
                         'rows are no trajectory)')
    return critic_n_step


NStepTargets = collections.namedtuple('NStepTargets', ['next_state', 'reward', 'done'])


def nstep_rows(ring, ind, size, n_step, n_stride, gamma, S, A):
    """The n-step rows of base rows `ind` in NumPy float32, operation for operation what csrc/nstep.hip computes: ring float32
    [max_size, 2S + A + 2], size = the fill level -> (rows float32 [B, 2S + A] = [s, a, s' of the chain's last row], R [B], D [B])."""
    ring = np.ascontiguousarray(ring, np.float32)
    bits = ring.view(np.uint32)
    cap, SA, gamma = ring.shape[0], S + A, np.float32(gamma)
    ind = np.asarray(ind, np.int64).reshape(-1)
    rows = np.empty((len(ind), SA + S), np.float32)
    Rs, Ds = np.empty(len(ind), np.float32), np.empty(len(ind), np.float32)
    one = np.float32(1.0)
    for b, i0 in enumerate(ind):
        last, g, R = int(i0), one, ring[i0, SA + S]
        for _ in range(1, int(n_step)):
            j = (last + int(n_stride)) % cap
            if not (ring[last, SA + S + 1] == 0 and j < size and np.array_equal(bits[j, :S], bits[last, SA:SA + S])):
                break
            g = np.float32(g * gamma)
            R = np.float32(R + np.float32(g * ring[j, SA + S]))
            last = j
        rows[b, :SA] = ring[i0, :SA]
        rows[b, SA:] = ring[last, SA:SA + S]
        Rs[b] = R
        Ds[b] = np.float32(one - np.float32(g * np.float32(one - ring[last, SA + S + 1])))
    return rows, Rs, Ds


def _nstep_index(buf, ind):
    """base rows `ind` as the int32 device array the n-step launches read, and its length"""
    idx = torch.as_tensor(ind).to(buf.device, torch.int32).reshape(-1).contiguous()
    return idx, int(idx.numel())


def _nstep_launch(buf, entry, n, ring, idx, size_dev, gamma, *outs):
    """ONE launch of a chain-following gather (`entry`: replay_gather_nstep or replay_gather_nstep_targets) for chain length n into `outs`"""
    lib_call(buf.device, entry, ring.data_ptr(), idx.data_ptr(), int(idx.numel()), buf.state_dim, buf.action_dim, buf.max_size, size_dev.data_ptr(),
             n, buf.n_stride, float(gamma), *(t.data_ptr() for t in outs))


def _nstep_host(buf, ring, size, ind, gamma, n):
    """device='cpu': nstep_rows() for chain length n as tensors (rows [B, 2S + A], R [B, 1], D [B, 1])"""
    rows, R, D = nstep_rows(ring.numpy(), np.asarray(torch.as_tensor(ind)), size, n, buf.n_stride, gamma, buf.state_dim, buf.action_dim)
    return torch.from_numpy(rows), torch.from_numpy(R).reshape(-1, 1), torch.from_numpy(D).reshape(-1, 1)


def nstep_batch(buf, ring, size_dev, size, ind, gamma):
    """The n-step Batch of base rows `ind` of `ring` ([max_size, row], buf's or one member's of a buffer group) for discount `gamma`: on the
    device ONE launch (rlrep_replay_gather_nstep) against the fill level word `size_dev`; on the CPU nstep_rows() against `size`.  The six
    arrays the launch wrote stay in buf._nstep_last (XE, XF, XF2, XFpi, R, D: what a minibatch slot holds)."""
    S, A = buf.state_dim, buf.action_dim
    if buf.device.type == 'cuda':
        idx, B = _nstep_index(buf, ind)
        xe = torch.empty(B, 2 * S + A, dtype=torch.float32, device=buf.device)
        xf, xf2, xfpi = (torch.zeros(B, S + A, dtype=torch.float32, device=buf.device) for _ in range(3))
        r, d = (torch.empty(B, 1, dtype=torch.float32, device=buf.device) for _ in range(2))
        _nstep_launch(buf, 'replay_gather_nstep', buf.n_step, ring, idx, size_dev, gamma, xe, xf, xf2, xfpi, r, d)
        buf._nstep_last = dict(XE=xe, XF=xf, XF2=xf2, XFpi=xfpi, R=r, D=d)
    else:
        xe, r, d = _nstep_host(buf, ring, size, ind, gamma, buf.n_step)
    return Batch(state=xe[:, :S].contiguous(), action=xe[:, S:S + A].contiguous(), reward=r, next_state=xe[:, S + A:].contiguous(), done=d)


def nstep_targets(buf, ind, gamma):
    """The n-step critic targets of base rows `ind` of buf's ring for discount `gamma` (critic_n_step, n_stride): NStepTargets(next_state [B, S]
    = s' of the chain's last row, reward [B, 1] = sum_k gamma^k r_k, done [B, 1] = 1 - gamma^(m-1) (1 - d_last)).  On the device ONE launch
    (rlrep_replay_gather_nstep_targets, csrc/nstep_targets.hip) against the device fill level; on the CPU nstep_rows().  The three arrays the
    launch wrote stay in buf._nstep_targets_last (XF2 [B, S + A] with columns [0, S) written, Rn, D: what it overwrites of a minibatch slot)."""
    S, A = buf.state_dim, buf.action_dim
    if buf.device.type == 'cuda':
        idx, B = _nstep_index(buf, ind)
        xf2 = torch.zeros(B, S + A, dtype=torch.float32, device=buf.device)
        r, d = (torch.empty(B, 1, dtype=torch.float32, device=buf.device) for _ in range(2))
        _nstep_launch(buf, 'replay_gather_nstep_targets', buf.critic_n_step, buf.ring, idx, buf.size_dev(), gamma, xf2, r, d)
        buf._nstep_targets_last = dict(XF2=xf2, Rn=r, D=d)
        return NStepTargets(next_state=xf2[:, :S].contiguous(), reward=r, done=d)
    rows, r, d = _nstep_host(buf, buf.ring, buf.size, ind, gamma, buf.critic_n_step)
    return NStepTargets(next_state=rows[:, S + A:].contiguous(), reward=r, done=d)


class ReplayBuffer(Ring):
    _NAME, _ADVANCING, _INTERLEAVES = 'ReplayBuffer', 'this ring (SACAgent.iterate)', ('in the ring', 'the buffer')

    def __init__(self, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, shard=None, n_step=1, n_stride=1, critic_n_step=1):
        """shard=(rank, world): this ring is one shard of a replay partitioned by transition index: every rank is
        offered the same stream of transitions and keeps transition i iff i % world == rank, at slot i // world of its own ring (the
        default, shard=None, keeps everything: each data-parallel rank then owns the transitions of its own environment).
        n_step > 1: SACAgent.train() learns from n-step rows (gather_nstep).  n_stride is the number of interleaved
        environments that write the ring -- row i's successor candidate is row (i + n_stride) mod max_size: 1 for add(), E for add_batch()
        of E rows, N for add_device() of N rows, num_envs for a device environment.
        critic_n_step > 1 (1..16; shares n_stride; not together with n_step > 1): VLSACAgent / CTRLSACAgent / SPEDERSACAgent /
        DIFFSRSACAgent.train() computes the critic targets from n-step returns (gather_nstep_targets) while the feature step keeps
        training on the one-step rows of the same minibatch."""
        n_step, n_stride = _check_nstep(type(self).__name__, n_step, n_stride, shard)
        critic_n_step = _check_critic_nstep(type(self).__name__, critic_n_step, n_step, shard, getattr(self, '_CRITIC_NSTEP_REFUSAL', None))
        super().__init__((), state_dim, action_dim, max_size, device, stage_rows, n_step, n_stride, critic_n_step)
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        self._offered = 0
        self.size = 0
        self.ring = self._new_ring(())
        self._copy_event = None
        self._size_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._size_pushed = -1
        self.device_epoch = 0        # bumped whenever this buffer enqueues device work on the caller's stream (a pipelined train() then orders itself after it)

    def _advance(self, n):
        self.size = min(self.size + n, self.max_size)

    def _fill_levels(self):
        return [self.size]

    # ---- reference API ------------------------------------------------------------------------
    def add(self, state, action, next_state, reward, done):
        if self._device_env is not None:
            raise self._stale('add')
        if self.shard is not None:
            i = self._offered
            self._offered += 1
            if i % self.shard[1] != self.shard[0]:
                return
        self._stage_ready()
        S, A = self.state_dim, self.action_dim
        r = self._stage_np[self._staged]             # (in place in the pinned stage, no temporary row: this is main.py's loop)
        r[:S] = state
        r[S:S + A] = action
        r[S + A:2 * S + A] = next_state
        r[2 * S + A] = reward
        r[2 * S + A + 1] = done
        self._staged += 1
        self.ptr = (self.ptr + 1) % self.max_size
        self._advance(1)

    def add_batch(self, states, actions, next_states, rewards, dones):
        """E transitions in one call: states / next_states [E, S], actions [E, A], rewards / dones [E].  Equal in every observable to E add()
        calls in row order -- the ring after flush(), ptr, size, device_epoch, the shard rule -- also where the batch wraps the ring or is
        larger than the staging buffer (which is then flushed exactly where the E calls would flush it)."""
        if self._device_env is not None:
            raise self._stale('add_batch')
        E = int(np.shape(rewards)[0])
        rows = self._pack_rows((E,), states, actions, next_states, rewards, dones)
        if self.shard is not None:
            i = self._offered + np.arange(E)
            self._offered += E
            rows = rows[i % self.shard[1] == self.shard[0]]
        self._stage_rows(rows)

    def add_device(self, states, actions, next_states, rewards, dones):
        """N transitions that live on the device: states / next_states [N, S], actions [N, A], rewards / dones [N] (or [N, 1]), float32
        tensors on the ring's device (dones may be bool).  ONE launch on the current stream (rlrep_replay_add_cols) packs them into ring rows
        ptr, ptr + 1, ... (wrapping) and writes the new fill level into size_dev(): nothing goes through the host.  Host rows staged by add()
        are flushed first, so the order of transitions is the call order.  ptr, size, device_epoch and the ring end up as add_batch() +
        flush() on the same rows leave them.  N is known on the host: ptr and size advance here."""
        if self._device_env is not None:
            raise self._stale('add_device')
        if self.shard is not None:
            raise ValueError('ReplayBuffer.add_device: a sharded ring (shard=) keeps one transition in `world`; add_device writes every row it is given')
        S, A = self.state_dim, self.action_dim
        N = int(rewards.shape[0])
        if not 1 <= N <= self.max_size:
            raise ValueError(f'ReplayBuffer.add_device: {N} transitions for a ring of {self.max_size} rows (N must lie in [1, max_size])')

        def prep(t, w, name):
            if not torch.is_tensor(t) or t.device != self.ring.device:
                raise ValueError(f'ReplayBuffer.add_device: {name} must be a tensor on {self.ring.device}')
            if t.dtype != torch.float32:
                t = t.to(torch.float32)
            if w is None:
                t = t.reshape(N)
                return t if t.stride(0) == 1 or N == 1 else t.contiguous()
            if tuple(t.shape) != (N, w):
                raise ValueError(f'ReplayBuffer.add_device: {name} {tuple(t.shape)} is not [{N}, {w}]')
            return t if t.stride(1) == 1 and (N == 1 or t.stride(0) >= w) else t.contiguous()
        s, a, s2 = prep(states, S, 'states'), prep(actions, A, 'actions'), prep(next_states, S, 'next_states')
        r, d = prep(rewards, None, 'rewards'), prep(dones, None, 'dones')
        epoch = self.device_epoch
        self.flush()
        start = self.ptr
        self.ptr = (self.ptr + N) % self.max_size
        self._advance(N)
        self._before_device_write()
        if self.device.type == 'cuda':
            ld = lambda t, w: t.stride(0) if N > 1 else w
            lib_call(self.device, 'replay_add_cols', self.ring.data_ptr(), self.max_size, self.row, start, S, A, s.data_ptr(), ld(s, S), a.data_ptr(),
                     ld(a, A), s2.data_ptr(), ld(s2, S), r.data_ptr(), d.data_ptr(), N, self._size_dev.data_ptr(), self.size, then=self._wrote)
        else:
            self._write_wrapped(self.ring, start, torch.from_numpy(self._pack_rows((N,), s, a, s2, r, d)))
        self.device_epoch = epoch + 1           # (one step for the call, staged host rows included: what add_batch() + flush() on the same rows count)

    def _wrote(self):
        """after a launch that wrote ring rows and the fill level: the level is published, and the event add() waits for before it reuses the
        stage is recorded (ONE event for the life of the ring: a fresh one per flush was host time in front of every train() of main.py's loop)"""
        self._size_pushed = self.size
        if self._copy_event is None:
            self._copy_event = torch.cuda.Event()
        self._copy_done = self._copy_event
        self._copy_done.record(_current_stream())

    def flush(self):
        n = self._staged
        self._order_reads()          # (whoever samples after this call, on this stream, sees a flush another stream may still be performing)
        if n == 0:
            return
        self._before_device_write()
        if self.device.type == 'cuda':
            # the C ABI's entry for this row of the path (include/rlrep.h rlrep_replay_add): ONE launch moves the staged rows, wrap-around
            # included and read in place from the pinned staging buffer, and writes the new fill level for the device-side sampler
            lib_call(self.device, 'replay_add_sized', self.ring.data_ptr(), self.max_size, self.row, self._stage_start, self._stage.data_ptr(), n,
                     self._size_dev.data_ptr(), self.size, then=self._wrote)
        else:
            self._write_wrapped(self.ring, self._stage_start, self._stage[:n])
        self._staged = 0
        self.device_epoch += 1

    def adopt_device_cursor(self):
        """Take the cursor back from the device environment: ptr and size become what its record holds (synchronises), and add() continues
        behind the last row the device wrote."""
        env = self._device_env
        if env is None:
            return
        rec = env.state().reshape(-1)                # (environment 0's cursor is the next free row)
        self.ptr = int(rec['ring_ptr'][0]) % self.max_size
        self.size = int(rec['ring_size'][0])
        self._size_pushed = self.size               # (the step launches have published it)
        self._device_env = None

    def load(self, state, action, next_state, reward, done):
        """Bulk-fill the ring (synthetic benchmarks / tests)."""
        if self.shard is not None:
            raise ValueError('load() fills the whole ring and knows nothing of the shard rule: add() the transitions instead')
        n = int(len(state))
        rows = self._pack_rows((n,), state, action, next_state, reward, done)
        self._before_device_write()
        self.ring[:n].copy_(torch.from_numpy(rows))
        self.size, self.ptr, self._staged = n, n % self.max_size, 0
        self.device_epoch += 1

    def save(self, path):
        self.flush()
        torch.cuda.synchronize() if self.device.type == 'cuda' else None
        np.savez_compressed(path, **self._save_arrays())

    def _save_arrays(self):
        """what save() writes (a subclass adds its own arrays)"""
        return dict(ring=self.ring[:self.size].cpu().numpy(), ptr=self.ptr, size=self.size, offered=self._offered)

    def restore(self, path):
        z = np.load(path)
        n = int(z['size'])
        self._before_device_write()
        self.ring[:n].copy_(torch.from_numpy(z['ring']))
        self.ptr, self.size, self._staged = int(z['ptr']), n, 0
        self._offered = int(z['offered']) if 'offered' in z.files else 0      # (files written before round 3 carry no shard counter)
        self.device_epoch += 1

    def size_dev(self):
        """int32[1] device scalar holding `size` (read by the graph-replayed index generator)."""
        if self._size_pushed != self.size:
            self._before_device_write()
            self._size_dev.fill_(self.size)
            self._size_pushed = self.size
            self.device_epoch += 1
        return self._size_dev

    def sample(self, batch_size):
        self.flush()
        ind = torch.from_numpy(np.random.randint(0, self.size, size=batch_size)).to(self.device)
        return self.gather(ind)

    def _order_reads(self):
        """A reader on the caller's stream: the last flush may have been issued on ANOTHER stream (a pipelined train() writes the staged rows on its
        feature stream, sac_agent.py) -- wait for it there."""
        if self._copy_done is not None and self.device.type == 'cuda':
            _current_stream().wait_event(self._copy_done)

    def gather(self, ind):
        S, A = self.state_dim, self.action_dim
        self._order_reads()
        rows = self.ring[ind.long()]
        return Batch(state=rows[:, :S].contiguous(), action=rows[:, S:S + A].contiguous(),
                     reward=rows[:, 2 * S + A:2 * S + A + 1].contiguous(),
                     next_state=rows[:, S + A:2 * S + A].contiguous(),
                     done=rows[:, 2 * S + A + 1:2 * S + A + 2].contiguous())

    def nstep_key(self):
        """what a captured train() bakes in besides the ring when it gathers n-step rows"""
        return ('nstep', self.n_step, self.n_stride)

    def gather_nstep(self, ind, gamma):
        """The n-step batch of base rows `ind` for discount `gamma`: state / action of row ind[b], next_state of the last row of
        its chain, reward R = sum_k gamma^k r_k over the chain and done D = 1 - gamma^(m-1) (1 - d_last), so that r + (1 - done) gamma V(s') is
        the m-step target.  On the device ONE launch (csrc/nstep.hip) against the device fill level; on device='cpu' the same arithmetic in
        NumPy float32.  n_step == 1 returns gather(ind)'s rows."""
        self.flush()
        self._order_reads()
        size_dev = self.size_dev() if self.device.type == 'cuda' else None
        return nstep_batch(self, self.ring, size_dev, self.size, ind, gamma)

    def cnstep_key(self):
        """what a captured train() bakes in besides the ring when it gathers n-step critic targets"""
        return ('cnstep', self.critic_n_step, self.n_stride)

    def gather_nstep_targets(self, ind, gamma):
        """The n-step critic targets of base rows `ind` for discount `gamma` (critic_n_step): NStepTargets(next_state, reward,
        done) -- what replaces the next_state / reward / done of gather(ind) in the critic and actor steps of a representation agent, whose
        feature step keeps gather(ind).  On the device ONE launch (csrc/nstep_targets.hip); on device='cpu' the same arithmetic in NumPy
        float32.  critic_n_step == 1 returns gather(ind)'s three arrays."""
        self.flush()
        self._order_reads()
        return nstep_targets(self, ind, gamma)

    # public array attributes of the reference, materialised on demand (read-only copies)
    def _col(self, a, b):
        self.flush()
        self._order_reads()
        return self.ring[:, a:b].cpu().numpy().astype(np.float64)

    @property
    def state(self):
        return self._col(0, self.state_dim)

    @property
    def action(self):
        return self._col(self.state_dim, self.state_dim + self.action_dim)

    @property
    def next_state(self):
        return self._col(self.state_dim + self.action_dim, 2 * self.state_dim + self.action_dim)

    @property
    def reward(self):
        return self._col(2 * self.state_dim + self.action_dim, 2 * self.state_dim + self.action_dim + 1)

    @property
    def done(self):
        return self._col(2 * self.state_dim + self.action_dim + 1, 2 * self.state_dim + self.action_dim + 2)


# ---- prioritized replay (Schaul et al. 2016) for sac: DESIGN.md 6f, csrc/per.hip ---------------------------------------------------------
def _f32(x):
    return np.float32(x)


PER_MIN_PRIORITY = np.float32(1.17549435e-38)        # the smallest normal float32: the floor of an updated leaf (csrc/per_tree.h)


def _per_set(tree, P, rows, value):
    """host form of per_add / restore: leaves of `rows` <- value, every ancestor one fp32 add of its children"""
    rows = np.asarray(rows, np.int64)
    if rows.size == 0:
        return
    tree[P + rows] = value
    nodes = np.unique((P + rows) >> 1)
    while nodes.size and nodes[0] >= 1:
        tree[nodes] = tree[2 * nodes] + tree[2 * nodes + 1]          # (float32 arrays: one rounded add)
        nodes = np.unique(nodes >> 1)


def _per_draw(tree, P, B, words):
    """host form of per_sample's descent: B stratified draws from uint32 Philox words"""
    total = tree[1]
    seg = _f32(total / _f32(B))
    u = ((words >> np.uint32(8)).astype(np.float32) + _f32(0.5)) * _f32(1.0 / 16777216.0)
    m = (np.arange(B, dtype=np.float32) + u) * seg
    n = np.ones(B, np.int64)
    while n[0] < P:
        l, r = tree[2 * n], tree[2 * n + 1]
        left = (r == 0) | (m < l)
        m = np.where(left, m, m - l).astype(np.float32)
        n = np.where(left, 2 * n, 2 * n + 1)
    return (n - P).astype(np.int32)


def _per_weights(tree, P, idx, beta):
    """host form of per_sample's weights: (pmin / p)^beta over the leaves of rows `idx`, 1 at the minimum and wherever beta == 0"""
    p = tree[P + idx.astype(np.int64)]
    pmin, beta = p.min(), _f32(beta)
    with np.errstate(divide='ignore', invalid='ignore'):
        wv = np.power((pmin / p).astype(np.float32), beta, dtype=np.float32)
    return np.where((p == pmin) | (beta == 0), _f32(1.0), wv).astype(np.float32)


def _per_update_host(tree, P, scal_row, idx, td, alpha, eps):
    """host form of per_update: leaf idx[j] <- (td[j] + eps)^alpha (1 when alpha == 0; the maximum where an index repeats), scal_row[0] = max_p
    follows, the ancestors are recomputed"""
    alpha = _f32(alpha)
    new = np.ones(len(idx), np.float32) if alpha == 0 else np.power(td + _f32(eps), alpha, dtype=np.float32)
    new = np.where(new > PER_MIN_PRIORITY, new, PER_MIN_PRIORITY).astype(np.float32)     # (not positive, or NaN: the floor, as per_update_kernel)
    rows = idx.astype(np.int64)
    tree[P + rows] = 0
    np.maximum.at(tree, P + rows, new)
    scal_row[0] = max(scal_row[0], new.max())
    _per_set(tree, P, rows, tree[P + rows])


def _per_rebuild_host(tree, P):
    """host form of per_rebuild: every internal node from its children, level by level from the leaves up"""
    w = P >> 1
    while w >= 1:
        nd = np.arange(w, 2 * w)
        tree[nd] = tree[2 * nd] + tree[2 * nd + 1]
        w >>= 1


class PrioritizedReplayBuffer(ReplayBuffer):
    """ReplayBuffer whose rows carry priorities in a device-resident sum tree (float32[2P], P = the smallest power of two >= max_size, row
    i's leaf at tree[P + i], an internal node ONE fp32 add of its children).  A row written by add() / add_batch() (at flush()), add_device()
    or load() gets the running maximum priority; SACAgent.train() samples in proportion to the leaves (stratified, one launch), weights the
    critic loss by (N P(j))^-beta normalised by the batch maximum, and writes (|TD| + eps)^alpha back -- all inside the captured train(), no
    host round trip.  `beta` may be assigned at any time (one device word, written on the caller's stream).  For SACAgent on one GPU; every
    other agent refuses the class by name.  On device='cpu' the same arithmetic runs in NumPy float32 (draw() / update())."""
    prioritized = True
    _CRITIC_NSTEP_REFUSAL = 'prioritized replay is built for sac, which has n_step'

    def __init__(self, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, shard=None, alpha=0.6, beta=0.4, eps=1e-6,
                 n_step=1, n_stride=1, critic_n_step=1):
        if shard is not None:
            raise ValueError('PrioritizedReplayBuffer: shard= is not supported (a shard sees one transition in `world`; priorities are per ring)')
        super().__init__(state_dim, action_dim, max_size=max_size, device=device, stage_rows=stage_rows, n_step=n_step, n_stride=n_stride,
                         critic_n_step=critic_n_step)
        self.P = 1 << max(0, self.max_size - 1).bit_length()
        self.tree = torch.zeros(2 * self.P, dtype=torch.float32, device=self.device)
        self._scal = torch.tensor([1.0, alpha, beta, eps], dtype=torch.float32, device=self.device)      # max_p, alpha, beta, eps
        self._hyper = (float(_f32(alpha)), float(_f32(beta)), float(_f32(eps)))
        self._draw_bufs = {}

    # ---- hyper-parameters and views --------------------------------------------------------------
    alpha = property(lambda self: self._hyper[0])
    eps = property(lambda self: self._hyper[2])

    @property
    def beta(self):
        return self._hyper[1]

    @beta.setter
    def beta(self, x):
        self._hyper = (self._hyper[0], float(_f32(x)), self._hyper[2])
        self._before_device_write()
        self._scal[2:3].fill_(float(x))              # (a fill launch on the caller's stream: no synchronisation)
        self.device_epoch += 1

    @property
    def max_priority(self):
        return float(self._scal[0].cpu())

    def priorities(self):
        """float32[size]: the leaves of the rows the ring holds (flushes staged rows; synchronises)"""
        self.flush()
        self._order_reads()
        return self.tree[self.P:self.P + self.size].cpu().numpy()

    def per_key(self):
        """what a captured train() bakes in besides the ring: the tree and the scalar block"""
        return ('per', self.tree.data_ptr(), self._scal.data_ptr())

    # ---- writers: every written row gets the running maximum priority ----------------------------
    def _per_add(self, start, n):
        if n <= 0:
            return
        if self.device.type == 'cuda':
            lib_call(self.device, 'per_add', self.tree.data_ptr(), self.P, self._scal.data_ptr(), self.max_size, int(start), int(n))
        else:
            _per_set(self.tree.numpy(), self.P, (int(start) + np.arange(int(n))) % self.max_size, self._scal.numpy()[0])

    def flush(self):
        a, n = self._stage_start, self._staged
        super().flush()
        self._per_add(a, n)

    def add_device(self, states, actions, next_states, rewards, dones):
        epoch = self.device_epoch
        self.flush()                                 # (staged host rows first, with their leaves: the order of transitions is the call order)
        start = self.ptr
        super().add_device(states, actions, next_states, rewards, dones)
        self._per_add(start, int(rewards.shape[0]))
        self.device_epoch = epoch + 1

    def load(self, state, action, next_state, reward, done):
        super().load(state, action, next_state, reward, done)
        self.tree.zero_()                            # load() resets the ring to its first n rows: rows it no longer holds lose their leaves (max_p stays)
        self._per_add(0, self.size)

    def collect_on_device(self, env):
        raise RuntimeError('PrioritizedReplayBuffer.collect_on_device: a device environment writes ring rows inside its step launch, which knows '
                           'nothing of the priority tree (iterate() / --device-loop take a plain ReplayBuffer)')

    def _save_arrays(self):
        return dict(super()._save_arrays(), per_leaves=self.tree[self.P:self.P + self.size].cpu().numpy(), per_max_p=self._scal[:1].cpu().numpy())

    def restore(self, path):
        super().restore(path)
        z = np.load(path)
        n = self.size
        self.tree.zero_()
        if 'per_leaves' not in z.files:              # a plain ReplayBuffer's file: every row is new
            self._scal[0:1].fill_(1.0)
            self._per_add(0, n)
            return
        self.set_priorities(z['per_leaves'], float(np.asarray(z['per_max_p']).reshape(-1)[0]))

    def set_priorities(self, leaves, max_priority=None):
        """Overwrite the leaves of rows 0 .. len(leaves) - 1 (every other leaf becomes 0) and rebuild the tree; max_priority, if given,
        replaces the running maximum.  What restore() does with a saved tree; also for tests and for priorities computed elsewhere."""
        leaves = np.asarray(leaves, np.float32).reshape(-1)
        n = len(leaves)
        if n > self.size:
            raise ValueError(f'PrioritizedReplayBuffer.set_priorities: {n} leaves for a ring that holds {self.size} rows')
        self.flush()
        self._before_device_write()
        self.tree.zero_()
        if max_priority is not None:
            self._scal[0:1].copy_(torch.from_numpy(np.asarray([max_priority], np.float32)))
        self.tree[self.P:self.P + n].copy_(torch.from_numpy(leaves))
        self.device_epoch += 1
        if self.device.type == 'cuda':
            lib_call(self.device, 'per_rebuild', self.tree.data_ptr(), self.P)
        else:
            _per_rebuild_host(self.tree.numpy(), self.P)

    # ---- the sampler and the priority update (SACAgent calls these inside train()) ---------------
    def draw_buffers(self, B):
        """(idx int32[B], w float32[B]) on the ring's device, one pair per batch size for the life of the buffer (captured graphs bake them in)"""
        bufs = self._draw_bufs.get(int(B))
        if bufs is None:
            bufs = self._draw_bufs[int(B)] = (torch.zeros(int(B), dtype=torch.int32, device=self.device),
                                              torch.ones(int(B), dtype=torch.float32, device=self.device))
        return bufs

    def draw(self, B, seed, offset, core=None, counter_dev=None, given=None):
        """B stratified draws in proportion to the priorities, and their importance weights -> (idx, w) = draw_buffers(B).  The draws are
        Philox stream elements 0 .. B-1 of (seed, offset [+ the device counter]); `given` (int32[B]): take these indices, compute only the
        weights.  On the device ONE launch on the current stream (`core`: the sac agent's HipCore).  An empty buffer is refused here."""
        B = int(B)
        if self.size == 0:
            raise RuntimeError('PrioritizedReplayBuffer.draw: the buffer is empty')
        idx, w = self.draw_buffers(B)[:2]
        if given is not None:
            g = np.asarray(given.cpu() if torch.is_tensor(given) else given).reshape(-1)
            if len(g) != B or g.min() < 0 or g.max() >= self.size:
                raise ValueError(f'PrioritizedReplayBuffer.draw: given indices must be {B} rows in [0, {self.size})')
            idx.copy_(torch.from_numpy(g.astype(np.int32)))
        if self.device.type == 'cuda':
            if core is None:
                raise ValueError('PrioritizedReplayBuffer.draw: the device sampler runs for a sac agent (core=agent.core)')
            self._order_reads()
            lib_call(self.device, 'per_sample', core.h, self.tree.data_ptr(), self.P, self._scal.data_ptr(), idx.data_ptr(), w.data_ptr(), B,
                     0 if given is None else 1, int(seed), int(offset), counter_dev)
            return idx, w
        from rlrep_amd.utils.philox_host import raw_stream as words
        t = self.tree.numpy()
        if given is None:
            idx.copy_(torch.from_numpy(_per_draw(t, self.P, B, words(B, int(seed), int(offset)))))
        w.copy_(torch.from_numpy(_per_weights(t, self.P, idx.numpy(), self._hyper[1])))
        return idx, w

    def update(self, B, td=None, core=None):
        """leaf idx[j] <- (td[j] + eps)^alpha for the last draw of B (1 when alpha == 0; the maximum where an index repeats), max_priority
        follows, the ancestors are recomputed.  On the device ONE launch; td=None: the |TD| errors the agent's last weighted critic step left."""
        B = int(B)
        idx = self.draw_buffers(B)[0]
        if self.device.type == 'cuda':
            if core is None:
                raise ValueError('PrioritizedReplayBuffer.update: the device update runs for a sac agent (core=agent.core)')
            lib_call(self.device, 'per_update', core.h, self.tree.data_ptr(), self.P, self._scal.data_ptr(), idx.data_ptr(),
                     None if td is None else td.data_ptr(), B)
            return
        _per_update_host(self.tree.numpy(), self.P, self._scal.numpy(), idx.numpy(), np.asarray(td, np.float32).reshape(B), self._hyper[0],
                         self._hyper[2])


# ---- prioritized replay of the critic's minibatch for vlsac / ctrlsac / spedersac / diffsrsac: DESIGN.md 6f.1, csrc/per.hip ----------
class CriticPrioritizedReplayBuffer(PrioritizedReplayBuffer):
    """PrioritizedReplayBuffer for the representation agents (VLSACAgent, CTRLSACAgent, SPEDERSACAgent, DIFFSRSACAgent), with another sampling
    contract -- hence another name, as critic_n_step stands to n_step.  These agents run their critic and actor steps on the slot-0 minibatch
    of their LAST feature step; that minibatch alone is drawn from the tree (the parent's sampler, unchanged), the critic loss takes its
    importance weights and the |TD| errors come back as priorities in the same train().  Every other minibatch of the call -- the earlier
    feature steps, spedersac's second slot -- stays the uniform draw a plain ReplayBuffer gives at the same seed and step, and the feature
    losses take no weights: the last feature step sees the prioritized rows unweighted (DESIGN.md 6f.1 says what that costs).  The tree, the
    scalars, the writers, save / restore and the CPU fallback are the parent's; the draw buffers gain td float32[B], which the weighted
    critic head writes and update() reads.  One agent, one GPU, the one-graph or eager train(); SACAgent takes the parent class."""
    prioritized = False               # (NOT the parent's contract: what refuses a PrioritizedReplayBuffer must not mistake this class for one)
    critic_prioritized = True
    _CRITIC_NSTEP_REFUSAL = 'n-step critic targets together with prioritized critic replay are not built'

    def __init__(self, state_dim, action_dim, max_size=int(1e6), device=None, stage_rows=4096, shard=None, alpha=0.6, beta=0.4, eps=1e-6,
                 n_step=1, n_stride=1, critic_n_step=1):
        if shard is not None:
            raise ValueError('CriticPrioritizedReplayBuffer: shard= is not supported (a shard sees one transition in `world`; priorities are per ring)')
        if not isinstance(n_step, bool) and int(n_step) == n_step and int(n_step) > 1:
            raise ValueError(f'CriticPrioritizedReplayBuffer: n_step {int(n_step)} > 1 is not supported (n_step is the whole minibatch of a sac agent, '
                             'which takes a PrioritizedReplayBuffer)')
        super().__init__(state_dim, action_dim, max_size=max_size, device=device, stage_rows=stage_rows, alpha=alpha, beta=beta, eps=eps,
                         n_step=n_step, n_stride=n_stride, critic_n_step=critic_n_step)

    def per_key(self):
        """what a captured train() bakes in besides the ring: the tree and the scalar block, under this class's own tag"""
        return ('critic_per', self.tree.data_ptr(), self._scal.data_ptr())

    def collect_on_device(self, env):
        raise RuntimeError('CriticPrioritizedReplayBuffer.collect_on_device: a device environment writes ring rows inside its step launch, which '
                           'knows nothing of the priority tree (iterate() / --device-loop take a plain ReplayBuffer)')

    def draw_buffers(self, B):
        """(idx int32[B], w float32[B], td float32[B]) on the ring's device, one triple per batch size for the life of the buffer"""
        bufs = self._draw_bufs.get(int(B))
        if bufs is None:
            bufs = self._draw_bufs[int(B)] = super().draw_buffers(B) + (torch.zeros(int(B), dtype=torch.float32, device=self.device),)
        return bufs

    def draw_fill(self, core, B, seed, offset, counter_dev=None, given=None):
        """The critic's minibatch of a representation agent (`core`: its HipCore): B stratified draws and their importance weights as draw()
        computes them, and the drawn ring rows gathered into the agent's minibatch slot 0 -- ONE launch on the current stream
        (rlrep_per_sample_fill).  `given` (int32[B]): take these indices, compute only the weights, gather.  -> (idx, w)."""
        B = int(B)
        if self.size == 0:
            raise RuntimeError('CriticPrioritizedReplayBuffer.draw_fill: the buffer is empty')
        idx, w, _ = self.draw_buffers(B)
        if given is not None:
            g = np.asarray(given.cpu() if torch.is_tensor(given) else given).reshape(-1)
            if len(g) != B or g.min() < 0 or g.max() >= self.size:
                raise ValueError(f'CriticPrioritizedReplayBuffer.draw_fill: given indices must be {B} rows in [0, {self.size})')
            idx.copy_(torch.from_numpy(g.astype(np.int32)))
        self._order_reads()
        lib_call(self.device, 'per_sample_fill', core.h, self.ring.data_ptr(), self.max_size, self.tree.data_ptr(), self.P, self._scal.data_ptr(),
                 idx.data_ptr(), w.data_ptr(), B, 0 if given is None else 1, int(seed), int(offset), counter_dev)
        return idx, w

    def update(self, B, td=None, core=None):
        """The parent's update() from this buffer's own td array (td=None: what the last weighted critic step wrote there).  On the device ONE
        launch that needs no agent (rlrep_per_update_td)."""
        B = int(B)
        idx, _, own = self.draw_buffers(B)
        if self.device.type == 'cuda':
            lib_call(self.device, 'per_update_td', self.tree.data_ptr(), self.P, self._scal.data_ptr(), idx.data_ptr(), (own if td is None else td).data_ptr(), B)
            return
        super().update(B, own if td is None else td)
