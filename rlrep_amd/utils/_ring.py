"""What ReplayBuffer and ReplayBufferGroup (and their prioritized subclasses) share: the pinned staging buffer in front of the device ring(s),
the cursor a device environment may borrow, and the one way both modules call the HIP library.  A group's member axis is a LEADING axis of
the ring and of the stage, so everything here indexes rows as `[..., a:b, :]` and never asks which of the two it serves."""
import numpy as np
import torch

from rlrep_amd.utils.streams import raw_stream as _raw_stream, current_device_index as _current_device_index


def lib_call(device, name, *args, then=None):
    """rlrep_<name>(*args, the current stream) on `device`, checked; `then()` (a ring's bookkeeping after a write) runs in the same device
    context.  Pointers are passed as tensor.data_ptr() or None (_lib.py declares the argument types).  The torch.cuda.device context manager
    is taken only where the current device is not the ring's: it was 15 us of host time in front of every train() of main.py's loop.  The
    library is imported here, not by the module, so the CPU paths work where it has not been built."""
    if device.index is not None and device.index != _current_device_index():
        with torch.cuda.device(device):
            return lib_call(device, name, *args, then=then)
    from rlrep_amd._lib import lib, check
    check(getattr(lib, 'rlrep_' + name)(*args, _raw_stream()), name)
    if then is not None:
        then()


class Ring(object):
    """The staging side of a replay ring.  A subclass names its class and its nouns for the refusals (_NAME, _ADVANCING, _INTERLEAVES), holds
    the ring(s) and the fill level(s), and supplies flush(), size_dev(), _advance(n) (the fill level(s) after n more rows) and _fill_levels()
    (what a device environment's cursor takes)."""

    def __init__(self, lead, state_dim, action_dim, max_size, device, stage_rows, n_step, n_stride, critic_n_step):
        """lead: the axes in front of a ring's rows -- () for one ring, (R,) for a group.  n_step, n_stride, critic_n_step: checked values."""
        self.n_step, self.n_stride, self.critic_n_step = n_step, n_stride, critic_n_step
        self.max_size = int(max_size)
        self.state_dim, self.action_dim = int(state_dim), int(action_dim)
        self.row = 2 * self.state_dim + self.action_dim + 2
        self.device = torch.device(device if device is not None else ('cuda' if torch.cuda.is_available() else 'cpu'))
        self._stage_cap = min(int(stage_rows), self.max_size)
        self._stage = torch.zeros(*lead, self._stage_cap, self.row, dtype=torch.float32, pin_memory=self.device.type == 'cuda')
        self._stage_np = self._stage.numpy()
        self._staged = 0            # rows (per member) waiting in the staging buffer
        self._stage_start = 0       # ring position of the first staged row (the same for every member: lockstep)
        self._copy_done = None
        self.ptr = 0
        # hooks called before the ring / size scalar is overwritten on the caller's stream (a pipelined train() may still be sampling from
        # them on its own stream: each agent that trains from this buffer appends one that makes the caller's stream wait)
        self.before_device_write_hooks = []
        self._device_env = None      # the device environment that owns the cursor (collect_on_device); None: the host does

    def _new_ring(self, lead):
        return torch.zeros(*lead, self.max_size, self.row, dtype=torch.float32, device=self.device)

    def _before_device_write(self):
        for h in self.before_device_write_hooks:
            h()

    def nstep_key(self):
        """what a captured train() bakes in besides the ring(s) when it gathers n-step rows"""
        return ('nstep', self.n_step, self.n_stride)

    def _stale(self, method):
        """the refusal of add / add_batch / add_device while a device environment owns the cursor"""
        return RuntimeError(f'{self._NAME}.{method}: a device environment has been advancing {self._ADVANCING}, so the host cursor is stale: '
                            'call adopt_device_cursor() first')

    # ---- staging --------------------------------------------------------------------------------------------------------------------
    def _pack_rows(self, lead, states, actions, next_states, rewards, dones, out=None):
        """[s | a | s' | r | d] as float32 [*lead, row], in `out` if given"""
        S, A, lead = self.state_dim, self.action_dim, tuple(lead)
        rows = np.empty(lead + (self.row,), np.float32) if out is None else out
        rows[..., :S] = np.asarray(states).reshape(lead + (S,))
        rows[..., S:S + A] = np.asarray(actions).reshape(lead + (A,))
        rows[..., S + A:2 * S + A] = np.asarray(next_states).reshape(lead + (S,))
        rows[..., 2 * S + A] = np.asarray(rewards).reshape(lead)
        rows[..., 2 * S + A + 1] = np.asarray(dones).reshape(lead)
        return rows

    def _stage_ready(self):
        """before a row is staged: a full stage is flushed, the copy that still reads the stage is awaited, an empty stage starts at ptr"""
        if self._staged == self._stage_cap:
            self.flush()
        if self._copy_done is not None:
            self._copy_done.synchronize()
            self._copy_done = None
        if self._staged == 0:
            self._stage_start = self.ptr

    def _stage_rows(self, rows):
        """rows float32 [..., E, row] behind the staged ones, flushed exactly where E add() calls would flush"""
        k, E = 0, rows.shape[-2]
        while k < E:
            self._stage_ready()
            n = min(E - k, self._stage_cap - self._staged)
            self._stage_np[..., self._staged:self._staged + n, :] = rows[..., k:k + n, :]
            self._staged += n
            self.ptr = (self.ptr + n) % self.max_size
            self._advance(n)
            k += n

    def _write_wrapped(self, rings, start, rows):
        """device='cpu': rows [..., n, row] into rows start, start + 1, ... of rings [..., max_size, row], wrapping (n <= max_size)"""
        n = rows.shape[-2]
        first = min(n, self.max_size - start)
        rings[..., start:start + first, :].copy_(rows[..., :first, :])
        if first < n:
            rings[..., :n - first, :].copy_(rows[..., first:, :])

    # ---- device collection (rlrep_amd/envs/device.py) ---------------------------------------------------------------------------------
    def collect_on_device(self, env):
        """Hand the cursor to device environment `env`: staged rows are flushed, the environment's record(s) take (ptr, fill level(s)), and
        from here on the step launches advance the ring(s) and the fill level(s) in size_dev().  add() refuses until adopt_device_cursor()."""
        if self._device_env is env:
            return
        if self._device_env is not None:
            raise RuntimeError(f'{self._NAME}.collect_on_device: another device environment owns the cursor (adopt_device_cursor() first)')
        if getattr(self, 'shard', None) is not None:
            raise ValueError(f'{self._NAME}.collect_on_device: a sharded ring (shard=) keeps one transition in `world`; a device environment '
                             'writes every row it steps')
        num_envs = int(getattr(env, 'num_envs', 1))
        for key in ('n_step', 'critic_n_step'):
            if getattr(self, key) > 1 and num_envs != self.n_stride:
                raise ValueError(f'{type(self).__name__}.collect_on_device: {key} {getattr(self, key)} with n_stride {self.n_stride}, but the device '
                                 f'environment interleaves num_envs = {num_envs} trajectories {self._INTERLEAVES[0]}: build {self._INTERLEAVES[1]} '
                                 'with n_stride = num_envs')
        self.flush()
        self.size_dev()
        if num_envs > 1:                             # (environment e's cursor is (ptr + e) mod max_size)
            env.set_cursor(self.ptr, self._fill_levels(), self.max_size)
        else:
            env.set_cursor(self.ptr, self._fill_levels())
        self._device_env = env
