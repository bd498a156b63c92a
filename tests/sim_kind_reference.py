"""Shared by tests/test_sim_kind_jit.py and tests/test_sim_kind_jit_cpu.py: the example kinds' texts and descriptions, the
point mass's forced cases and a random rollout of its NumPy twin (rlrep_amd/envs/point_mass.py).  A plain module, imported like
fused_sim_reference.py.  Reads nothing outside the repository."""
import numpy as np

from rlrep_amd.envs import point_mass as pm

F32 = lambda v: float(np.float32(v))  # noqa: E731


def source(which):
    from rlrep_amd.envs.fused_sim import example_kind
    return example_kind(which)


def desc(text, **over):
    """(SimKindDesc, keep-alive) of a kind's text, fields overridden by keyword (name / source as str)"""
    from rlrep_amd._lib import SimKindDesc
    from rlrep_amd.envs.fused_sim import kind_constants
    k = dict(kind_constants(text), source=text)
    k.update(over)
    keep = (None if k['name'] is None else k['name'].encode(), None if k['source'] is None else k['source'].encode())
    return SimKindDesc(name=keep[0], source=keep[1], S=k['S'], A=k['A'], NX=k['NX'], limit=k['limit'], terminates=int(bool(k['terminates']))), keep


def point_mass_cases(n, seed=0):
    """n random (x[4], a[2], t) of the one-step comparison: positions over the whole box and on the walls, speeds up to the clamp, forces beyond
    the clip, states around the goal radius, steps up to the limit's"""
    g = np.random.RandomState(seed)
    x = np.stack([g.uniform(-2, 2, n), g.uniform(-2, 2, n), g.uniform(-1, 1, n), g.uniform(-1, 1, n)])
    a = g.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
    t = g.randint(0, pm.LIMIT, n).astype(np.int32)
    k = n // 6
    x[:2, :k] = g.uniform(-0.15, 0.15, (2, k))              # around the goal
    x[2:, :k] = g.uniform(-0.3, 0.3, (2, k))
    x[0, k:2 * k] = np.where(g.rand(k) < 0.5, -2.0, 2.0)    # on a wall, some pushing into it
    x[2, k:2 * k] = g.uniform(-1, 1, k)
    x[2:, 2 * k:3 * k] = np.where(g.rand(2, k) < 0.5, -1.0, 1.0)       # at the speed clamp
    t[3 * k:4 * k] = pm.LIMIT - 1                           # the limit's step
    t[:k // 2] = pm.LIMIT - 1                               # ... and around the goal on it
    return x, a, t


# (x, a, t, done, ended): the goal before the limit; the goal on the limit's step; the limit without the goal; neither; the goal, force clipped
FORCED = [((0.05, 0.0, 0.0, 0.0), (0.0, 0.0), 10, 1.0, True),
          ((0.05, 0.0, 0.0, 0.0), (0.0, 0.0), pm.LIMIT - 1, 0.0, True),
          ((1.0, 1.0, 0.0, 0.0), (0.5, -0.5), pm.LIMIT - 1, 0.0, True),
          ((1.0, 1.0, 0.0, 0.0), (0.5, -0.5), 10, 0.0, False),
          ((0.0, 0.06, 0.0, 0.1), (0.0, -3.0), 0, 1.0, True)]


def rollout(n=2048, steps=150, seed=1):
    """a random rollout of the twin with the simulator's episode rules: n environments, start states at random steps of their episodes, a noisy
    proportional-derivative policy towards the origin in half of them and a constant outward push in the rest -> counts of
    (goal before the limit, goal on the limit's step, limit without goal, wall)"""
    g = np.random.RandomState(seed)
    x = np.stack([g.uniform(-1, 1, n), g.uniform(-1, 1, n), np.zeros(n), np.zeros(n)])
    t = g.randint(0, pm.LIMIT, n)
    seek = np.arange(n) % 2 == 0
    push = g.uniform(-1, 1, (n, 2)).astype(np.float32)
    counts = dict(goal=0, goal_on_limit=0, limit=0, wall=0)
    for _ in range(steps):
        pd = (-(g.uniform(0.02, 1.5, (n, 1))) * x[:2].T - 1.5 * x[2:].T + 0.1 * g.randn(n, 2)).astype(np.float32)
        a = np.where(seek[:, None], pd, push)
        out = pm.step_sim(x, t, a)
        on_limit = t + 1 >= pm.LIMIT
        counts['goal'] += int((out['goal'] & ~on_limit).sum())
        counts['goal_on_limit'] += int((out['goal'] & on_limit).sum())
        counts['limit'] += int((~out['goal'] & on_limit).sum())
        counts['wall'] += int(out['wall'].sum())
        assert np.array_equal(out['done'] > 0, out['goal'] & ~on_limit) and np.array_equal(out['ended'], out['goal'] | on_limit)
        x, t = out['x'], out['t']
        e = out['ended']
        x[:, e] = np.stack([g.uniform(-1, 1, e.sum()), g.uniform(-1, 1, e.sum()), np.zeros(e.sum()), np.zeros(e.sum())])
    return counts
