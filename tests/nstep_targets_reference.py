"""The NumPy float32 restatement of the n-step critic-target gather (csrc/nstep_targets.hip), the cases its tests share, and the
composition of the oracle's public steps that the representation agents are held to.  A plain module, imported like nstep_reference.py.

The walk is nstep_reference.chain().  Of it the gather writes XF2[b, 0:S] = s' of the chain's last row, Rn[b] = R and D[b] = 1 - g (1 - d_last);
an index outside the ring writes zeros.  What the feature step reads (XE, XF, R) is the one-step gather's."""
import numpy as np
import torch

from nstep_reference import chain, trajectories, ring_of

f32 = np.float32
CUTS = ('done', 'limit', 'fill', 'head')


def step_of_rows(total, cap):
    """the step number (order of writing) of the row every ring position holds after `total` rows were added; -1: never written"""
    pos = np.arange(cap)
    last = total - 1 - ((total - 1 - pos) % cap)
    return np.where(pos < total, last, -1)


def nstep_targets(ring, idx, size, n, stride, gamma, S, A, total=None):
    """dict(S2 [B, S], Rn [B], D [B], m [B] chain lengths, cut [B]: why a chain shorter than n ended -- 'done' (terminal row), 'fill' (the
    successor lies at or above the fill level), 'head' (the successor holds an OLDER row: the chain ran into the write head of a full ring
    whose head has wrapped), 'limit' (any other state mismatch: a time limit), '' (full length, or the index lies outside the ring)).
    total: rows ever added (for 'head'; default: size)."""
    ring = np.ascontiguousarray(ring, f32)
    cap, SA = ring.shape[0], S + A
    idx = np.asarray(idx, np.int64).reshape(-1)
    B = len(idx)
    steps = step_of_rows(size if total is None else total, cap)
    out = dict(S2=np.zeros((B, S), f32), Rn=np.zeros(B, f32), D=np.zeros(B, f32), m=np.zeros(B, np.int64), cut=[''] * B)
    for b, i0 in enumerate(idx):
        if not 0 <= i0 < cap:
            continue
        last, m, _, R, D = chain(ring, i0, size, n, stride, gamma, S, A)
        out['S2'][b], out['Rn'][b], out['D'][b], out['m'][b] = ring[last, SA:SA + S], R, D, m
        if m < n:
            j = (last + stride) % cap
            out['cut'][b] = ('done' if ring[last, SA + S + 1] != 0 else 'fill' if j >= size else 'head' if steps[j] < steps[last] else 'limit')
    return out


# ---- the kernel test's cases (tests/test_nstep_critic.py; their conditions are checked on the CPU in tests/test_nstep_critic_cpu.py) ---------
CAP, BATCH, FILL = 96, 37, (50, 96 + 29)          # ring rows; samples (one of them outside the ring); rows added: partly filled / full, head wrapped
SHAPES = ((3, 1), (70, 2))                        # (S, A): Pendulum's, and more than 64 compare words
STRIDES, NS, GAMMA = (1, 2, 5), (1, 3, 5, 16), 0.97
CASE_SEED = 19                                    # the smallest seed whose draws meet kernel_case_ok() in every case and at both fill levels


def kernel_case(S, A, stride, total, seed=CASE_SEED):
    """(ring, size, idx int64[BATCH]) of one case: rows of `stride` interleaved trajectories, `total` of them added to a ring of CAP rows;
    the base rows are drawn without replacement, and entry 5 is an index outside the ring"""
    rows = trajectories(S, A, total, stride, 1000 * seed + 10 * S + stride, p_done=0.06, p_limit=0.06)
    ring, _, size = ring_of(rows, CAP)
    idx = np.random.default_rng(seed).permutation(size)[:BATCH].astype(np.int64)
    idx[5] = CAP + 3
    return ring, size, idx


def kernel_case_ok(S, A, stride, n, total, seed=CASE_SEED):
    """the conditions on ONE (shape, stride, n > 1, fill level) case: at least a quarter of the samples have chains of two rows or more, and a
    chain is cut by a terminal row ('done'), by a time limit ('limit') and by the end of what the ring holds -- the fill level ('fill') in
    the partly filled ring, the wrapped write head ('head') in the full one (a full ring has no fill level to run into, a ring that never
    wrapped no write head)"""
    ring, size, idx = kernel_case(S, A, stride, total, seed)
    w = nstep_targets(ring, idx, size, n, stride, GAMMA, S, A, total)
    need = {'done', 'limit', 'fill' if total <= CAP else 'head'}
    return 4 * int((w['m'] >= 2).sum()) >= BATCH and need <= set(w['cut'])


# ---- the oracle composition ---------------------------------------------------------------------------------------------------------------
def critic_batch(batch, targets):
    """the Batch the critic and actor steps see: state / action of the one-step batch, next_state / reward / done of the n-step targets"""
    return type(batch)(state=batch.state, action=batch.action, reward=torch.as_tensor(targets['Rn']).reshape(-1, 1),
                       next_state=torch.as_tensor(targets['S2']), done=torch.as_tensor(targets['D']).reshape(-1, 1))


def oracle_train(o, batches, noise, targets=None):
    """oracle.train(batches, noise) recomposed from the oracle's public steps, so that the feature steps run on the one-step batches and
    critic_step / update_actor_and_alpha on critic_batch(the minibatch they reuse, targets).  targets=None (or n = 1 targets): oracle.train."""
    o.steps += 1
    n, alg = o.extra + 1, o.alg
    info = {}
    for i in range(n):
        if alg == 'vlsac':
            info = o.feature_step(batches[i], noise[i]); o.update_feature_target()
        elif alg == 'ctrlsac':
            info = o.feature_step(batches[i]); o.update_feature_target()
        elif alg == 'spedersac':
            info = o.feature_step(batches[2 * i], batches[2 * i + 1]); o.update_feature_target()
        else:
            info = o.critic_feeder_feature_step(batches[i], noise[2 * i], noise[2 * i + 1])
    if alg == 'ctrlsac':
        o.sync_frozen()
    b = batches[2 * (n - 1)] if alg == 'spedersac' else batches[n - 1]
    if targets is not None:
        b = critic_batch(b, targets)
    k = {'vlsac': n, 'diffsrsac': 2 * n}.get(alg, 0)
    info.update(o.critic_step(b, noise[k]))
    info.update(o.update_actor_and_alpha(b, noise[k + 1]))
    o.update_target()
    return info


def injected_draws(rs, alg, o, S, A, B, F, rows):
    """(idx list, eps list) of one train_injected call in the draw order of the agent (tests/test_hip_parity.py)"""
    nf = o.extra + 1
    idx = [rs.randint(0, rows, size=B) for _ in range(o.n_batches())]
    eps = []
    if alg == 'vlsac':
        eps = [rs.standard_normal((B, F)).astype(f32) for _ in range(nf)]
    if alg == 'diffsrsac':
        for _ in range(nf):
            eps += [rs.randint(0, 1000, size=B), (0.449 * rs.standard_normal((B, S))).astype(f32)]
    eps += [rs.standard_normal((B, A)).astype(f32) for _ in range(2)]
    return idx, eps
