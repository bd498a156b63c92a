"""Population-based training (Jaderberg et al. 2017: truncation selection + perturbation) on the host: who copies whom, and how a copied
member's hyper-parameters move -- and successive halving (Jamieson & Talwalkar 2016): who is retired.  Every function is deterministic in its
arguments (and a `np.random.RandomState` where it draws); none touches the GPU (the device side is SeedBatchMixin.clone_members /
set_member_hyper / retire_members, rlrep_amd/agent/seed_batch.py).
"""
import math

import numpy as np


def _rank_key(scores):
    """sort key, best first: higher is better, NaN below everything, ties to the lower member index"""
    return lambda r: (math.isnan(scores[r]), -scores[r] if not math.isnan(scores[r]) else 0.0, r)


def plan_halving(scores, live, keep, min_live=1):
    """The members to retire, ascending: of the n live members (`live`: one boolean per member) the best max(1, ceil(keep * n)) stay, ranked
    as plan_exploit ranks (higher is better, NaN below everything, ties to the lower index); 0 < keep < 1.  Retired members' scores are not
    looked at and they are never returned; [] when one member is live.  min_live: never fewer than this many members stay (the launcher's
    --halving-min)."""
    scores = [float(s) for s in scores]
    live = [bool(v) for v in live]
    if len(live) != len(scores):
        raise ValueError(f'plan_halving: {len(scores)} scores for {len(live)} members')
    keep = float(keep)
    if not (math.isfinite(keep) and 0.0 < keep < 1.0):
        raise ValueError(f'plan_halving: keep {keep} outside (0, 1)')
    alive = [r for r in range(len(live)) if live[r]]
    if not alive:
        raise ValueError('plan_halving: no live member')
    if int(min_live) < 1:
        raise ValueError(f'plan_halving: min_live {min_live} is below 1')
    stay = max(1, int(min_live), int(math.ceil(keep * len(alive))))
    order = sorted(alive, key=_rank_key(scores))      # best first
    return sorted(order[stay:])


def plan_exploit(scores, fraction, rng):
    """[(src, dst), ...]: members are ranked by score (higher is better, NaN below everything, ties by member index: the lower index ranks
    higher); the bottom k = max(1, floor(fraction * R)) members each take a source `rng` draws from the top k.  R >= 2 and 2 k <= R, so no
    member is both a source and a destination.  Destinations come worst first."""
    scores = [float(s) for s in scores]
    R = len(scores)
    if R < 2:
        raise ValueError(f'plan_exploit: needs at least 2 members (got {R})')
    fraction = float(fraction)
    if not (math.isfinite(fraction) and 0.0 < fraction <= 0.5):
        raise ValueError(f'plan_exploit: fraction {fraction} outside (0, 0.5]')
    k = max(1, int(math.floor(fraction * R)))
    if 2 * k > R:
        raise ValueError(f'plan_exploit: fraction {fraction} of {R} members makes the top and the bottom {k} overlap')
    order = sorted(range(R), key=_rank_key(scores))      # best first
    top, bottom = order[:k], order[R - k:][::-1]
    return [(top[int(rng.randint(k))], dst) for dst in bottom]


def perturb(hyper, keys, factors, rng):
    """A copy of `hyper` with every key of `keys` multiplied by a factor `rng` draws from `factors` (explore step).  tau / feature_tau stay in
    [0, 1]; target_update_period is rounded and stays >= 1; discount moves as 1 - (1 - discount) * f (its distance from 1 is what scales) and
    stays below 1; booleans are refused (nothing to multiply)."""
    factors = [float(f) for f in factors]
    if not factors or not all(math.isfinite(f) and f > 0 for f in factors):
        raise ValueError(f'perturb: factors {factors} must be finite and positive')
    out = dict(hyper)
    for key in keys:
        if key not in hyper:
            raise ValueError(f'perturb: {key!r} is not one of the hyper-parameters ({", ".join(hyper)})')
        v = hyper[key]
        if isinstance(v, (bool, np.bool_)):
            raise ValueError(f'perturb: {key} is a boolean and cannot be perturbed')
        f = factors[int(rng.randint(len(factors)))]
        if key in ('tau', 'feature_tau'):
            out[key] = min(1.0, max(0.0, float(v) * f))
        elif key == 'target_update_period':
            out[key] = max(1, int(round(float(v) * f)))
        elif key == 'discount':
            out[key] = min(1.0 - (1.0 - float(v)) * f, float(np.nextafter(1.0, 0.0)))
        else:
            out[key] = float(v) * f
    return out
