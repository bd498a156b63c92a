"""Host form of the device's Philox4x32-10 word stream (csrc/philox.h; Salmon et al., SC'11), for the code paths that mirror a device draw
on the CPU (PrioritizedReplayBuffer on device='cpu')."""
import numpy as np

_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def raw_stream(n, seed, offset):
    """uint32[n]: element e is word e & 3 of block e >> 2, counter (block lo, block hi, offset lo, offset hi), key (seed lo, seed hi) --
    the layout of philox_fill_body / per_sample_kernel"""
    nq = (int(n) + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    off = int(offset) & 0xFFFFFFFFFFFFFFFF
    c = [q & _MASK, q >> np.uint64(32), np.full(nq, off & _MASK, np.uint64), np.full(nq, off >> 32, np.uint64)]
    k0, k1 = int(seed) & _MASK, (int(seed) >> 32) & _MASK
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]             # 32 x 32 -> 64 bit products fit a uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c, axis=-1).astype(np.uint32).reshape(-1)[:int(n)]
