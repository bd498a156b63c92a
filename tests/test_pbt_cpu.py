"""Population-based training on seed groups, host side: rlrep_amd/agent/pbt.py plans and perturbs deterministically and within its bounds,
rlrep_group_clone_members exists and refuses what is not a group, and main.py checks --pbt-* before the GPU (after every older check).
No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from seed_group_util import run_launcher


# ---- plan_exploit -----------------------------------------------------------------------------------------------------------------------
FRACTIONS = (0.01, 0.1, 0.125, 0.2, 0.25, 1.0 / 3.0, 0.4, 0.5)


def _scores(R, rng, nans=0):
    s = rng.randint(0, 5, size=R).astype(np.float64) * 10.0          # ties on purpose
    for r in rng.permutation(R)[:nans]:
        s[r] = float('nan')
    return list(s)


@pytest.mark.parametrize('R', range(2, 17))
def test_plan_exploit_pairs_are_disjoint_ranked_and_deterministic(R):
    from rlrep_amd.agent.pbt import plan_exploit
    for fraction in FRACTIONS:
        k = max(1, int(math.floor(fraction * R)))
        for trial in range(8):
            gen = np.random.RandomState(1000 * R + trial)
            nans = int(gen.randint(0, R + 1)) if trial % 2 else 0
            scores = _scores(R, gen, nans)
            if 2 * k > R:
                with pytest.raises(ValueError):
                    plan_exploit(scores, fraction, np.random.RandomState(0))
                continue
            plan = plan_exploit(scores, fraction, np.random.RandomState(7))
            assert plan == plan_exploit(scores, fraction, np.random.RandomState(7))          # same RandomState seed -> same plan
            srcs, dsts = [s for s, _ in plan], [d for _, d in plan]
            assert len(plan) == k and len(set(dsts)) == k
            assert not set(srcs) & set(dsts)
            assert all(0 <= m < R for m in srcs + dsts)
            key = [(-math.inf if math.isnan(v) else v) for v in scores]          # NaN ranks below everything
            assert max(key[d] for d in dsts) <= min(key[s] for s in srcs)
            # NaN members are destinations first: a scored member is replaced only when every NaN member is
            nan_members = {r for r in range(R) if math.isnan(scores[r])}
            if len(nan_members) >= k:
                assert set(dsts) <= nan_members
            else:
                assert nan_members <= set(dsts)
            assert not any(math.isnan(scores[s]) for s in srcs) or len(nan_members) > R - k


def test_plan_exploit_ties_break_by_member_index_and_sources_vary():
    from rlrep_amd.agent.pbt import plan_exploit
    plan = plan_exploit([1.0] * 8, 0.25, np.random.RandomState(0))
    assert [d for _, d in plan] == [7, 6] and all(s in (0, 1) for s, _ in plan)
    seen = {plan_exploit([1.0] * 8, 0.25, np.random.RandomState(s))[0][0] for s in range(32)}
    assert seen == {0, 1}                                                        # the source is drawn, not always the best
    assert plan_exploit([0.0, 5.0, float('nan'), 3.0], 0.25, np.random.RandomState(0)) == [(1, 2)]


def test_plan_exploit_refuses_one_member_and_overlapping_fractions():
    from rlrep_amd.agent.pbt import plan_exploit
    with pytest.raises(ValueError, match='at least 2 members'):
        plan_exploit([1.0], 0.25, np.random.RandomState(0))
    for bad in (0.6, 0.0, -0.1, float('nan')):
        with pytest.raises(ValueError, match='fraction'):
            plan_exploit([1.0, 2.0, 3.0, 4.0], bad, np.random.RandomState(0))


# ---- perturb ----------------------------------------------------------------------------------------------------------------------------
def test_perturb_keeps_its_bounds_over_1000_draws_and_is_deterministic():
    from rlrep_amd.agent.pbt import perturb
    keys = ('lr', 'tau', 'feature_tau', 'target_update_period', 'discount')
    factors = (0.8, 1.2)
    for start in (dict(lr=3e-4, tau=0.005, feature_tau=0.9, target_update_period=2, discount=0.99, alpha=0.1, auto_entropy_tuning=True),
                  dict(lr=1e-4, tau=1.0, feature_tau=0.0, target_update_period=1, discount=0.999999, alpha=0.2, auto_entropy_tuning=False)):
        rng, rng2 = np.random.RandomState(5), np.random.RandomState(5)
        h = h2 = dict(start)
        for draw in range(1000):
            new = perturb(h, keys, factors, rng)
            assert new == perturb(h2, keys, factors, rng2)
            assert set(new) == set(h) and new['alpha'] == h['alpha'] and new['auto_entropy_tuning'] is h['auto_entropy_tuning']
            assert any(math.isclose(new['lr'], h['lr'] * f, rel_tol=1e-12) for f in factors) and new['lr'] > 0
            for k in ('tau', 'feature_tau'):
                assert 0.0 <= new[k] <= 1.0
                assert any(new[k] == min(1.0, max(0.0, h[k] * f)) for f in factors)
            assert isinstance(new['target_update_period'], int) and new['target_update_period'] >= 1
            assert any(new['target_update_period'] == max(1, int(round(h['target_update_period'] * f))) for f in factors)
            assert new['discount'] < 1.0
            assert any(new['discount'] == min(1.0 - (1.0 - h['discount']) * f, float(np.nextafter(1.0, 0.0))) for f in factors)
            assert h == h2                                                       # the argument is not modified
            h = h2 = new
    with pytest.raises(ValueError, match='boolean'):
        perturb(dict(lr=1e-4, auto_entropy_tuning=True), ['auto_entropy_tuning'], factors, np.random.RandomState(0))
    with pytest.raises(ValueError, match='factors'):
        perturb(dict(lr=1e-4), ['lr'], (0.8, 0.0), np.random.RandomState(0))
    with pytest.raises(ValueError, match='not one of'):
        perturb(dict(lr=1e-4), ['tau'], factors, np.random.RandomState(0))


def test_pbt_module_needs_no_gpu_library():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = 'import sys; import rlrep_amd.agent.pbt; assert "torch" not in sys.modules and "rlrep_amd._lib" not in sys.modules'
    subprocess.run([sys.executable, '-c', code], check=True, cwd=root)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_clone_entry_point_refuses_what_is_not_a_group():
    from rlrep_amd import _lib
    lib = _lib.lib
    src, dst = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    assert lib.rlrep_group_clone_members(None, src, dst, 1, None) == -1
    assert 'not a seed group' in lib.rlrep_last_error().decode()
    assert 'rlrep_group_clone_members' in set(_lib.declared_symbols())
    assert 'rlrep_group_clone_members' in _lib.SIGNATURES


# ---- SeedBatchMixin checks that run before the GPU ------------------------------------------------------------------------------------------
def test_group_classes_have_the_pbt_surface():
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    import inspect
    for cls in (SACSeedBatch, CTRLSACSeedBatch):
        assert callable(cls.clone_members) and callable(cls.set_member_hyper)
        assert inspect.signature(cls.load).parameters['adopt_hyper'].default is False


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------
GROUP = ['--alg', 'sac', '--seeds', '0,1,2,3', '--eval_freq', '100']


@pytest.mark.parametrize('argv, words', [
    (['--alg', 'sac', '--pbt-interval', '100', '--eval_freq', '100'], 'needs a seed group'),
    (['--alg', 'sac', '--pbt-fraction', '0.25'], 'needs a seed group'),
    (['--alg', 'sac', '--seeds', '0', '--pbt-interval', '100', '--eval_freq', '100'], 'at least 2 members'),
    (GROUP + ['--pbt-interval', '150'], 'positive multiple of --eval_freq'),
    (GROUP + ['--pbt-interval', '-100'], 'positive multiple of --eval_freq'),
    (GROUP + ['--pbt-fraction', '0.25'], 'positive multiple of --eval_freq'),          # options without an interval
    (GROUP + ['--pbt-interval', '200', '--pbt-fraction', '0.6'], 'outside (0, 0.5]'),
    (GROUP + ['--pbt-interval', '200', '--pbt-fraction', '0'], 'outside (0, 0.5]'),
    (GROUP + ['--pbt-interval', '200', '--pbt-keys', 'lr,feature_tau'], 'feature_tau is not a sweepable hyper-parameter of --alg sac'),
    (GROUP + ['--pbt-interval', '200', '--pbt-keys', 'hidden_dim'], 'hidden_dim is not a sweepable hyper-parameter'),
    (GROUP + ['--pbt-interval', '200', '--pbt-keys', 'alpha'], 'alpha cannot be perturbed'),
    (GROUP + ['--pbt-interval', '200', '--pbt-keys', 'lr,auto_entropy_tuning'], 'auto_entropy_tuning cannot be perturbed'),
    (GROUP + ['--pbt-interval', '200', '--pbt-factors', '0.8,0'], 'finite positive factors'),
    (GROUP + ['--pbt-interval', '200', '--pbt-factors', '0.8,inf'], 'finite positive factors'),
    (GROUP + ['--pbt-interval', '200', '--pbt-factors', 'big'], 'finite positive factors'),
    (['--alg', 'ctrlsac', '--seeds', '0,1', '--eval_freq', '100', '--pbt-interval', '100', '--pbt-keys', 'feature_tau,beta'], 'beta is not a sweepable'),
])
def test_pbt_arguments_are_checked_before_the_gpu(argv, words):
    with pytest.raises(SystemExit) as e:
        run_launcher(argv + ['--env', 'Pendulum-v1'])
    assert words in str(e.value), str(e.value)


def test_existing_launcher_checks_still_come_first():
    with pytest.raises(SystemExit, match='distinct'):
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '1,1', '--pbt-interval', '5'])
    with pytest.raises(SystemExit, match='sac only'):
        run_launcher(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--pbt-interval', '5'])
    with pytest.raises(SystemExit, match="unknown key 'beta'"):
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--sweep', 'beta=0.9', '--pbt-interval', '5'])


def test_parse_pbt_defaults_and_off():
    from rlrep_amd import main
    import argparse

    def ns(**kw):
        base = dict(pbt_interval=None, pbt_fraction=None, pbt_keys=None, pbt_factors=None, pbt_seed=None, eval_freq=5000)
        base.update(kw)
        return argparse.Namespace(**base)
    assert main.parse_pbt(ns(), 'sac', 4) is None
    assert main.parse_pbt(ns(pbt_interval=0), 'sac', 1) is None
    assert main.parse_pbt(ns(pbt_interval=10000), 'sac', 4) == dict(interval=10000, fraction=0.25, keys=['lr'], factors=[0.8, 1.2], seed=0)
    got = main.parse_pbt(ns(pbt_interval=5000, pbt_keys='lr, feature_tau', pbt_factors='0.5,2', pbt_seed=3, pbt_fraction=0.5), 'ctrlsac', 2)
    assert got == dict(interval=5000, fraction=0.5, keys=['lr', 'feature_tau'], factors=[0.5, 2.0], seed=3)
