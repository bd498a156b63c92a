"""Successive halving on seed groups, host side: rlrep_amd/agent/pbt.py plan_halving ranks as plan_exploit does and never returns a retired
member, rlrep_group_set_live / rlrep_group_get_live exist and refuse what is not a group, both group classes have the retire / revive surface,
and main.py checks --halving-* before the GPU (after every older check).  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from seed_group_util import run_launcher


# ---- plan_halving -----------------------------------------------------------------------------------------------------------------------
def test_plan_halving_ranks_higher_better_nan_first_out_ties_to_the_lower_index():
    from rlrep_amd.agent.pbt import plan_halving
    nan = float('nan')
    assert plan_halving([1.0, 4.0, 3.0, 2.0], [True] * 4, 0.5) == [0, 3]
    assert plan_halving([1.0, nan, 3.0, 2.0], [True] * 4, 0.75) == [1]                  # NaN ranks below everything
    assert plan_halving([nan, nan, -1e30, nan], [True] * 4, 0.25) == [0, 1, 3]
    assert plan_halving([5.0] * 6, [True] * 6, 0.5) == [3, 4, 5]                        # ties: the lower index ranks higher
    assert plan_halving([nan] * 4, [True] * 4, 0.5) == [2, 3]
    assert plan_halving([1.0, 2.0, 3.0], [True] * 3, 0.5) == [0]                        # ceil(0.5 * 3) = 2 stay
    assert plan_halving([3.0, 2.0, 1.0, 0.0, -1.0], [True] * 5, 0.01) == [1, 2, 3, 4]   # never below one live member
    assert plan_halving([3.0, 2.0, 1.0, 0.0, -1.0], [True] * 5, 0.99) == []             # ceil(0.99 * 5) = 5 stay


def test_plan_halving_ignores_retired_members_and_stops_at_one():
    from rlrep_amd.agent.pbt import plan_halving
    # members 1 and 4 are retired: their (excellent / NaN) scores are not looked at and they are never returned
    assert plan_halving([1.0, 100.0, 3.0, 2.0, float('nan'), 0.5], [True, False, True, True, False, True], 0.5) == [0, 5]
    assert plan_halving([1.0, 100.0, 3.0], [False, False, True], 0.5) == []
    assert plan_halving([float('nan')], [True], 0.5) == []
    assert plan_halving([1.0, 2.0, 3.0, 4.0], [1, 1, 1, 1], 0.25, min_live=3) == [0]
    live, scores, seen = [True] * 16, list(np.random.RandomState(3).permutation(16).astype(float)), []
    while sum(live) > 1:                                                                # 16 -> 8 -> 4 -> 2 -> 1
        out = plan_halving(scores, live, 0.5)
        assert out == sorted(out) and all(live[r] for r in out) and not set(out) & set(seen)
        assert max(scores[r] for r in out) < min(scores[r] for r in range(16) if live[r] and r not in out)
        for r in out:
            live[r] = False
        seen += out
        assert sum(live) in (8, 4, 2, 1)
    assert [r for r in range(16) if live[r]] == [int(np.argmax(scores))]
    assert plan_halving(scores, live, 0.5) == []


@pytest.mark.parametrize('R', range(1, 17))
def test_plan_halving_counts_and_is_deterministic(R):
    from rlrep_amd.agent.pbt import plan_halving
    for keep in (0.01, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.99):
        for trial in range(6):
            gen = np.random.RandomState(100 * R + trial)
            scores = list(gen.randint(0, 4, size=R).astype(np.float64))
            for r in gen.permutation(R)[:int(gen.randint(0, R + 1)) if trial % 2 else 0]:
                scores[r] = float('nan')
            live = [bool(v) for v in gen.randint(0, 2, size=R)]
            if not any(live):
                live[int(gen.randint(R))] = True
            n = sum(live)
            out = plan_halving(scores, live, keep)
            assert out == plan_halving(list(scores), list(live), keep)
            assert len(out) == n - max(1, int(math.ceil(keep * n))) and all(live[r] for r in out)
            key = [(-math.inf if math.isnan(v) else v) for v in scores]
            stay = [r for r in range(R) if live[r] and r not in out]
            if out:
                assert max(key[r] for r in out) <= min(key[r] for r in stay)


def test_plan_halving_refuses_bad_arguments():
    from rlrep_amd.agent.pbt import plan_halving
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='keep'):
            plan_halving([1.0, 2.0], [True, True], bad)
    with pytest.raises(ValueError, match='2 scores for 3 members'):
        plan_halving([1.0, 2.0], [True, True, True], 0.5)
    with pytest.raises(ValueError, match='no live member'):
        plan_halving([1.0, 2.0], [False, False], 0.5)
    with pytest.raises(ValueError, match='min_live'):
        plan_halving([1.0, 2.0], [True, True], 0.5, min_live=0)


def test_pbt_module_still_needs_no_gpu_library():
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; from rlrep_amd.agent.pbt import plan_halving; assert plan_halving([1.0, 2.0], [True, True], 0.5) == [0]; '
            'assert "torch" not in sys.modules and "rlrep_amd._lib" not in sys.modules')
    subprocess.run([sys.executable, '-c', code], check=True, cwd=root)


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_live_entry_points_refuse_what_is_not_a_group():
    from rlrep_amd import _lib
    lib = _lib.lib
    mask = (C.c_int32 * 2)(1, 0)
    assert lib.rlrep_group_set_live(None, mask, None) == -1
    assert 'not a seed group' in lib.rlrep_last_error().decode() and 'group_set_live' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_get_live(None, mask) == -1
    assert 'not a seed group' in lib.rlrep_last_error().decode() and 'group_get_live' in lib.rlrep_last_error().decode()
    assert list(mask) == [1, 0]
    for name in ('rlrep_group_set_live', 'rlrep_group_get_live'):
        assert name in set(_lib.declared_symbols()) and name in _lib.SIGNATURES
    assert lib.rlrep_abi_version() == 4


# ---- SeedBatchMixin ---------------------------------------------------------------------------------------------------------------------
def test_group_classes_have_the_halving_surface():
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    for cls in (SACSeedBatch, CTRLSACSeedBatch):
        assert callable(cls.retire_members) and callable(cls.revive_members)
        assert isinstance(cls.live, property) and cls.live.fset is None              # read-only


# ---- launcher ---------------------------------------------------------------------------------------------------------------------------
GROUP = ['--alg', 'sac', '--seeds', '0,1,2,3', '--eval_freq', '100']


@pytest.mark.parametrize('argv, words', [
    (['--alg', 'sac', '--halving-interval', '100', '--eval_freq', '100'], 'successive halving needs a seed group'),
    (['--alg', 'sac', '--halving-keep', '0.5'], 'successive halving needs a seed group'),
    (['--alg', 'sac', '--seeds', '0', '--halving-interval', '100', '--eval_freq', '100'], 'at least 2 members'),
    (GROUP + ['--halving-interval', '150'], 'positive multiple of --eval_freq'),
    (GROUP + ['--halving-interval', '-100'], 'positive multiple of --eval_freq'),
    (GROUP + ['--halving-keep', '0.5'], 'positive multiple of --eval_freq'),            # options without an interval
    (GROUP + ['--halving-min', '2'], 'positive multiple of --eval_freq'),
    (GROUP + ['--halving-interval', '200', '--halving-keep', '1'], 'outside (0, 1)'),
    (GROUP + ['--halving-interval', '200', '--halving-keep', '0'], 'outside (0, 1)'),
    (GROUP + ['--halving-interval', '200', '--halving-keep', '1.5'], 'outside (0, 1)'),
    (GROUP + ['--halving-interval', '200', '--halving-keep', 'nan'], 'outside (0, 1)'),
    (GROUP + ['--halving-interval', '200', '--halving-min', '0'], 'below 1'),
    (GROUP + ['--halving-interval', '200', '--halving-min', '-3'], 'below 1'),
    (GROUP + ['--halving-interval', '200', '--pbt-interval', '200'], 'population-based training over a shrinking population is a later change'),
    (['--alg', 'ctrlsac', '--seeds', '0,1', '--eval_freq', '100', '--halving-interval', '250'], 'positive multiple of --eval_freq'),
])
def test_halving_arguments_are_checked_before_the_gpu(argv, words):
    with pytest.raises(SystemExit) as e:
        run_launcher(argv + ['--env', 'Pendulum-v1'])
    assert words in str(e.value), str(e.value)


def test_existing_launcher_checks_still_come_first():
    with pytest.raises(SystemExit, match='distinct'):
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '1,1', '--halving-interval', '5'])
    with pytest.raises(SystemExit, match='sac and ctrlsac only'):
        run_launcher(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--halving-interval', '5'])
    with pytest.raises(SystemExit, match="unknown key 'beta'"):
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--sweep', 'beta=0.9', '--halving-interval', '5'])
    # ... and the --pbt-* checks, which are older than the --halving-* ones
    with pytest.raises(SystemExit, match='needs a seed group') as e:
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--pbt-interval', '100', '--halving-interval', '100', '--eval_freq', '100'])
    assert '--pbt-*' in str(e.value)
    with pytest.raises(SystemExit, match=r'outside \(0, 0.5\]'):
        run_launcher(GROUP + ['--env', 'Pendulum-v1', '--pbt-interval', '200', '--pbt-fraction', '0.9', '--halving-interval', '150'])


def test_parse_halving_defaults_and_off():
    from rlrep_amd import main
    import argparse

    def ns(**kw):
        base = dict(halving_interval=None, halving_keep=None, halving_min=None, eval_freq=5000)
        base.update(kw)
        return argparse.Namespace(**base)
    assert main.parse_halving(ns(), 4, None) is None
    assert main.parse_halving(ns(halving_interval=0), 1, None) is None
    assert main.parse_halving(ns(halving_interval=10000), 4, None) == dict(interval=10000, keep=0.5, min=1)
    assert main.parse_halving(ns(halving_interval=5000, halving_keep=0.25, halving_min=2), 8, None) == dict(interval=5000, keep=0.25, min=2)
