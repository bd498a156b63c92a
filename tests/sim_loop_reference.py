"""The NumPy float32 restatement of the exploration mix of the captured simulator loop (csrc/actor_tile.hip
actor_tile_kernel_ctl), built on rlrep_amd/utils/philox_host.py.  A plain module, imported like nstep_reference.py.

Row e of iteration `it` draws Philox4x32-10 blocks keyed by the agent's seed with counter {it lo, it hi, e, STREAM_SIM + q}.  Its pick is
word 0 of block q = 0; u_j is word (1 + j) mod 4 of block (1 + j) // 4; a word w becomes ((w >> 8) + 0.5) / 2^24 in float32.  The row takes
min(max(fl(lo + fl(fl(hi - lo) u_j)), lo), hi) in every component j if the iteration is a warm-up one or pick < eps_greedy; otherwise it
keeps the policy's action.  Every fl() is one float32 rounding."""
import numpy as np

from rlrep_amd.utils import philox_host

f32 = np.float32
STREAM_SIM = 0xE2000000


def block(seed, it, e, q):
    """uint32[4]: the Philox block (it, e, q) of the mix.  philox_host.raw_stream counts blocks in counter words 0-1 and carries `offset` in
    words 2-3: block `it` of the stream at offset ((STREAM_SIM + q) << 32) | e."""
    off = ((STREAM_SIM + int(q)) << 32) | int(e)
    return philox_host.raw_stream(4 * (int(it) + 1), seed, off)[4 * int(it):]


def u01(w):
    """env_u01f: the top 24 bits of a word, in (0, 1)"""
    return f32((f32(int(w) >> 8) + f32(0.5)) * f32(1.0 / 16777216.0))


def pick(seed, it, e):
    return u01(block(seed, it, e, 0)[0])


def from_word(w, lo, hi):
    """the uniform action component of Philox word w in [lo, hi]: three float32 operations, then the clamp (u01 rounds to 1.0 for the 128
    largest words, and lo + fl(hi - lo) may lie above hi)"""
    lo, hi = f32(lo), f32(hi)
    a = f32(lo + f32(f32(hi - lo) * u01(w)))
    return min(max(a, lo), hi)


def uniform_action(seed, it, e, A, lo, hi):
    """float32[A]: the uniform action of row e in iteration `it`"""
    return np.array([from_word(block(seed, it, e, (1 + j) // 4)[(1 + j) % 4], lo, hi) for j in range(A)], f32)


def mix(actions, seed, it, warm, eps_greedy, lo, hi):
    """(actions after the mix [N, A] float32, taken [N] bool) for the policy's actions [N, A] of iteration `it`"""
    actions = np.array(actions, f32, copy=True)
    N, A = actions.shape
    taken = np.zeros(N, bool)
    for e in range(N):
        if warm or pick(seed, it, e) < f32(eps_greedy):
            actions[e] = uniform_action(seed, it, e, A, lo, hi)
            taken[e] = True
    return actions, taken
