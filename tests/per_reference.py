"""NumPy float32 restatement of prioritized replay as DESIGN.md 6f fixes it (TEST INFRASTRUCTURE; a plain module like fixture_io.py):
the sum tree, add, the stratified sampler, the importance weights and the priority update.  Every operation whose order the design spells
out is ONE rounded float32 operation here, so the device kernels (csrc/per.hip) and the buffer's CPU fallback must agree with this file bit
for bit wherever no pow() is involved.  The draws are oracle.philox.raw_stream words."""
import numpy as np
from oracle.philox import raw_stream

f32 = np.float32
PER_STREAM = 3 << 40          # Philox offset of the sampler's stream (1 << 40: indices, 2 << 40: noise)
PER_MIN_PRIORITY = f32(1.17549435e-38)      # the smallest normal float32: the floor of an updated leaf


def tree_size(max_size):
    """P: the smallest power of two >= max_size"""
    P = 1
    while P < max_size:
        P *= 2
    return P


class RefTree(object):
    def __init__(self, max_size, alpha=0.6, beta=0.4, eps=1e-6):
        self.max_size, self.P = int(max_size), tree_size(int(max_size))
        self.tree = np.zeros(2 * self.P, f32)
        self.max_p, self.alpha, self.beta, self.eps = f32(1.0), f32(alpha), f32(beta), f32(eps)

    # ---- the tree ------------------------------------------------------------------------------
    def _fix(self, leaf):
        n = (self.P + int(leaf)) >> 1
        while n >= 1:
            self.tree[n] = f32(self.tree[2 * n] + self.tree[2 * n + 1])
            n >>= 1

    def rebuild(self):
        for n in range(self.P - 1, 0, -1):
            self.tree[n] = f32(self.tree[2 * n] + self.tree[2 * n + 1])

    def set_leaves(self, rows, values):
        rows = np.asarray(rows, np.int64).reshape(-1)
        self.tree[self.P + rows] = np.broadcast_to(np.asarray(values, f32), rows.shape)
        self.rebuild()

    def clear(self):
        """load() resets the ring: every leaf 0 (max_p stays)"""
        self.tree[:] = 0

    def add(self, start, n):
        """rows [start, start + n) mod max_size <- max_p, ancestors recomputed"""
        rows = (int(start) + np.arange(int(n), dtype=np.int64)) % self.max_size
        self.tree[self.P + rows] = self.max_p
        for r in np.unique(rows):
            self._fix(r)

    def invariant_ok(self):
        n = np.arange(1, self.P)
        return bool(np.array_equal(self.tree[n], (self.tree[2 * n] + self.tree[2 * n + 1]).astype(f32)))

    # ---- sample --------------------------------------------------------------------------------
    def sample(self, B, seed, offset):
        """idx int32[B]: draw j descends with m = fl(fl(j + u_j) seg), left while r == 0 or m < l, else m = fl(m - l) and right"""
        words = raw_stream(B, seed, offset)
        total = self.tree[1]
        seg = f32(total / f32(B))
        idx = np.empty(B, np.int32)
        for j in range(B):
            u = f32(f32(f32(words[j] >> np.uint32(8)) + f32(0.5)) * f32(2.0 ** -24))
            m = f32(f32(f32(j) + u) * seg)
            n = 1
            while n < self.P:
                l, r = self.tree[2 * n], self.tree[2 * n + 1]
                if r == 0 or m < l:
                    n = 2 * n
                else:
                    m = f32(m - l)
                    n = 2 * n + 1
            idx[j] = n - self.P
        return idx

    def weights(self, idx):
        """(w float64[B], exact bool[B]): w = (pmin / p)^beta in float64 from the float32 quotient; exact: where the device must return 1.0f"""
        p = self.tree[self.P + np.asarray(idx, np.int64)]
        pmin = p.min()
        exact = (p == pmin) | (self.beta == 0)
        q = (pmin / p).astype(f32)
        w = np.where(exact, 1.0, np.power(q.astype(np.float64), float(self.beta)))
        return w, exact

    # ---- update --------------------------------------------------------------------------------
    def new_priorities(self, td):
        """float64[B]: (fl(td + eps))^alpha, 1 when alpha == 0"""
        td = np.asarray(td, f32)
        if self.alpha == 0:
            return np.ones(td.shape, np.float64)
        return np.power((td + self.eps).astype(f32).astype(np.float64), float(self.alpha))

    def update(self, idx, new):
        """leaves at idx <- the MAXIMUM of `new` (float32) over the duplicates of each index; max_p follows; ancestors recomputed"""
        idx, new = np.asarray(idx, np.int64), np.asarray(new, f32)
        new = np.where(new > PER_MIN_PRIORITY, new, PER_MIN_PRIORITY).astype(f32)        # (not positive, or NaN: the floor -- a touched leaf stays positive)
        self.tree[self.P + idx] = 0
        np.maximum.at(self.tree, self.P + idx, new)
        self.max_p = f32(max(self.max_p, new.max()))
        for r in np.unique(idx):
            self._fix(r)
