"""The NumPy float32 restatement of n-step replay (csrc/nstep.hip), and the synthetic rings the n-step tests share.  A plain
module, imported like per_reference.py.

For a sampled base row i0 of a ring of max_size rows [s | a | s' | r | d] with fill level `size`, discount gamma, chain length n and successor
distance stride:  g = 1, R = r[i0], last = i0;  for k = 1 .. n - 1 with j = (last + stride) mod max_size the chain continues iff
d[last] == 0, j < size and the S words of s[j] equal the S words of s'[last] bit for bit; then g = fl(g gamma), R = fl(R + fl(g r[j])),
last = j.  Output: (s, a) of i0, s' of last, reward R, done fl(1 - fl(g fl(1 - d[last]))).  Every fl() is one float32 rounding."""
import numpy as np

f32 = np.float32


def chain(ring, i0, size, n, stride, gamma, S, A):
    """(last, m, g, R, D) of base row i0: the chain's last row, its length m, g = gamma^(m-1), the reward and the done word"""
    cap, SA = ring.shape[0], S + A
    bits = ring.view(np.uint32)
    gamma, one = f32(gamma), f32(1.0)
    last, m, g, R = int(i0), 1, one, ring[i0, SA + S]
    for _ in range(1, int(n)):
        j = (last + int(stride)) % cap
        if ring[last, SA + S + 1] != 0:
            break
        if j >= size:
            break
        if not np.array_equal(bits[j, :S], bits[last, SA:SA + S]):
            break
        g = f32(g * gamma)
        R = f32(R + f32(g * ring[j, SA + S]))
        last, m = j, m + 1
    D = f32(one - f32(g * f32(one - ring[last, SA + S + 1])))
    return last, m, g, R, D


def nstep_slot(ring, idx, size, n, stride, gamma, S, A):
    """What the gather leaves in a minibatch slot for base rows idx: dict(XE [B, 2S+A] = [s, a, s'], XF [B, S+A] = [s, a], XF2 [B, S+A] with
    columns [0, S) = s' (the rest 0: the gather does not write them), XFpi [B, S+A] with columns [0, S) = s, R [B], D [B]) and m [B], the
    chain lengths."""
    ring = np.ascontiguousarray(ring, f32)
    idx = np.asarray(idx, np.int64).reshape(-1)
    B, SA = len(idx), S + A
    out = dict(XE=np.zeros((B, SA + S), f32), XF=np.zeros((B, SA), f32), XF2=np.zeros((B, SA), f32), XFpi=np.zeros((B, SA), f32),
               R=np.zeros(B, f32), D=np.zeros(B, f32), m=np.zeros(B, np.int64))
    for b, i0 in enumerate(idx):
        last, m, _, R, D = chain(ring, i0, size, n, stride, gamma, S, A)
        out['XE'][b, :SA] = ring[i0, :SA]
        out['XE'][b, SA:] = ring[last, SA:SA + S]
        out['XF'][b] = ring[i0, :SA]
        out['XF2'][b, :S] = ring[last, SA:SA + S]
        out['XFpi'][b, :S] = ring[i0, :S]
        out['R'][b], out['D'][b], out['m'][b] = R, D, m
    return out


def nstep_batch(ring, idx, size, n, stride, gamma, S, A):
    """the n-step rows as the five arrays of a Batch: state, action, reward [B, 1], next_state, done [B, 1]"""
    o = nstep_slot(ring, idx, size, n, stride, gamma, S, A)
    SA = S + A
    return dict(state=o['XE'][:, :S].copy(), action=o['XE'][:, S:SA].copy(), reward=o['R'].reshape(-1, 1), next_state=o['XE'][:, SA:].copy(),
                done=o['D'].reshape(-1, 1))


def trajectories(S, A, steps, envs, seed, p_done=0.06, p_limit=0.06):
    """`steps` transitions of `envs` interleaved synthetic environments in the order a vector loop writes them (step t belongs to environment
    t mod envs): (s, a, s2, r, d).  An environment's next row starts where its last one ended (s = the previous s', bit for bit) unless that
    row was terminal (d = 1, probability p_done) or the episode hit a time limit (probability p_limit: a fresh start state and d = 0, as
    Pendulum's 200 steps leave it)."""
    rng = np.random.default_rng(seed)
    s = np.empty((steps, S), f32); a = rng.uniform(-1, 1, size=(steps, A)).astype(f32); s2 = rng.normal(size=(steps, S)).astype(f32)
    r = rng.normal(size=steps).astype(f32); d = (rng.random(steps) < p_done).astype(f32)
    limit = rng.random(steps) < p_limit
    cur = rng.normal(size=(envs, S)).astype(f32)
    for t in range(steps):
        e = t % envs
        s[t] = cur[e]
        cur[e] = rng.normal(size=S).astype(f32) if (d[t] != 0 or limit[t]) else s2[t]
    return s, a, s2, r, d


def ring_of(rows, max_size):
    """the ring, ptr and size after the rows were added in order to an empty ring of max_size rows (the newest max_size survive)"""
    s, a, s2, r, d = rows
    n = len(r)
    full = np.concatenate([s, a, s2, r.reshape(n, 1), d.reshape(n, 1)], axis=1).astype(f32)
    ring = np.zeros((max_size, full.shape[1]), f32)
    for t in range(n):
        ring[t % max_size] = full[t]
    return ring, n % max_size, min(n, max_size)
