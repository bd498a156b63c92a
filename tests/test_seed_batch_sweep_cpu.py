"""Hyper-parameter sweeps in seed groups on the host: the C ABI entry points exist and refuse what is not a group, SeedBatchMixin checks
member_hyper before anything touches the GPU, and main.py checks --sweep before the GPU.  No GPU."""
import ctypes as C

import pytest

from seed_group_util import run_launcher


def test_member_hyper_entry_points_refuse_what_is_not_a_group():
    from rlrep_amd import _lib
    lib = _lib.lib
    h = _lib.Hyper()
    assert lib.rlrep_group_set_member_hyper(None, 0, C.byref(h), None) == -1
    assert 'not a seed group' in lib.rlrep_last_error().decode()
    assert lib.rlrep_group_get_member_hyper(None, 0, C.byref(h)) == -1
    assert 'not a seed group' in lib.rlrep_last_error().decode()
    assert {'rlrep_group_set_member_hyper', 'rlrep_group_get_member_hyper'} <= set(_lib.declared_symbols())


def _sac():
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    return SACSeedBatch


def _ctrlsac():
    from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
    return CTRLSACSeedBatch


@pytest.mark.parametrize('cls', [_sac, _ctrlsac])
@pytest.mark.parametrize('seeds, member_hyper, words', [
    ((0, 1), [dict(lr=1e-4)], 'has 1 entries for 2 seeds'),
    ((0, 1), [dict(lr=1e-4), dict(learning_rate=1e-4)], "unknown key 'learning_rate'"),
    ((0, 1), [dict(lr=1e-4), dict(hidden_dim=512)], "'hidden_dim'] is structural"),
    ((0, 1), [dict(), dict(max_batch=128)], "'max_batch'] is structural"),
    ((0, 0), [dict(lr=1e-4), dict(lr=1e-4)], 'duplicate (seed, hyper) pair'),
    ((0, 0), [dict(), dict(tau=None)], 'tau=None is not valid'),
    ((5, 5), [dict(tau=0.005), dict()], 'duplicate (seed, hyper) pair'),        # (an override equal to the default is no difference)
    ((0, 1), [dict(lr=0.0), dict()], 'lr=0.0 is not valid'),
    ((0, 1), [dict(lr=float('nan')), dict()], 'lr=nan is not valid'),
    ((0, 1), [dict(tau=1.5), dict()], 'tau=1.5 is not valid'),
    ((0, 1), [dict(target_update_period=0), dict()], 'target_update_period=0 is not valid'),
    ((0, 1), [dict(alpha=-1.0), dict()], 'alpha=-1.0 is not valid'),
    ((0, 1), [dict(), 'lr=1e-4'], 'is not a dict'),
])
def test_member_hyper_is_checked_before_the_gpu(cls, seeds, member_hyper, words):
    with pytest.raises(ValueError) as e:
        cls()(seeds, 3, 1, None, member_hyper=member_hyper)
    assert words in str(e.value), str(e.value)


def test_member_hyper_keys_per_algorithm():
    with pytest.raises(ValueError, match="'extra_feature_steps'] is structural"):
        _ctrlsac()((0, 1), 3, 1, None, member_hyper=[dict(), dict(extra_feature_steps=2)])
    with pytest.raises(ValueError, match="'use_feature_target'] is structural"):
        _ctrlsac()((0, 1), 3, 1, None, member_hyper=[dict(), dict(use_feature_target=False)])
    with pytest.raises(ValueError, match="unknown key 'feature_tau'"):
        _sac()((0, 1), 3, 1, None, member_hyper=[dict(), dict(feature_tau=0.01)])
    with pytest.raises(ValueError, match='feature_tau=2.0 is not valid'):
        _ctrlsac()((0, 1), 3, 1, None, member_hyper=[dict(), dict(feature_tau=2.0)])
    # without member_hyper, repeated seeds keep their message
    with pytest.raises(ValueError, match='seeds must be distinct'):
        _sac()((0, 0), 3, 1, None)


def test_member_hypers_resolve_against_the_agents_defaults():
    sac, ctrl = _sac(), _ctrlsac()
    hs = sac.member_hypers([0, 0], dict(tau=0.01), [dict(lr=1e-4), dict(discount=0.9, auto_entropy_tuning=0)])
    assert hs[0] == dict(lr=1e-4, discount=0.99, tau=0.01, alpha=0.1, target_update_period=2, auto_entropy_tuning=True)
    assert hs[1] == dict(lr=3e-4, discount=0.9, tau=0.01, alpha=0.1, target_update_period=2, auto_entropy_tuning=False)
    hc = ctrl.member_hypers([1], {}, [dict(feature_tau=0.01)])
    assert hc[0]['lr'] == 1e-4 and hc[0]['feature_tau'] == 0.01


@pytest.mark.parametrize('argv, words', [
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'beta=0.9'], "unknown key 'beta'"),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'feature_tau=0.01'], 'feature_tau is not a hyper-parameter of --alg sac'),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'hidden_dim=256,512'], "unknown key 'hidden_dim'"),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'lr=abc'], "lr='abc' is not valid"),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'lr=-1e-4'], 'lr must be a finite positive number'),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'tau=2'], 'tau must be a number in [0, 1]'),
    (['--alg', 'ctrlsac', '--seeds', '0,1', '--sweep', 'target_update_period=0,1'], 'target_update_period must be an integer >= 1'),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'lr'], 'give KEY=V1,V2'),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'lr=1e-4', '--sweep', 'lr=3e-4'], 'lr is swept twice'),
    (['--alg', 'sac', '--seeds', '0,1', '--sweep', 'lr=1e-4,1e-4'], 'repeated value'),
    (['--alg', 'sac', '--seeds', ','.join(str(s) for s in range(40)), '--sweep', 'lr=1e-4,3e-4'], '80 members, more than a group holds (64)'),
])
def test_sweep_arguments_are_checked_before_the_gpu(argv, words):
    with pytest.raises(SystemExit) as e:
        run_launcher(argv + ['--env', 'Pendulum-v1'])
    assert words in str(e.value), str(e.value)


def test_existing_launcher_checks_come_first():
    # the distinct-seeds and algorithm checks keep their messages, and run before any --sweep check
    with pytest.raises(SystemExit, match='distinct'):
        run_launcher(['--alg', 'sac', '--env', 'Pendulum-v1', '--seeds', '1,1', '--sweep', 'nonsense=1'])
    with pytest.raises(SystemExit, match='sac only'):
        run_launcher(['--alg', 'vlsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--sweep', 'lr=1e-4'])
    with pytest.raises(SystemExit, match='sac only'):
        run_launcher(['--alg', 'diffsrsac', '--env', 'Pendulum-v1', '--seeds', '0,1', '--sweep', 'feature_tau=0.1'])


def test_sweep_tags_and_member_order():
    from rlrep_amd import main
    cfgs = main.parse_sweeps(['lr=1e-4,3e-4', 'tau=0.005,0.01'], 'sac', 2)
    assert [t for t, _ in cfgs] == ['lr=0.0001_tau=0.005', 'lr=0.0001_tau=0.01', 'lr=0.0003_tau=0.005', 'lr=0.0003_tau=0.01']
    assert cfgs[3][1] == dict(lr=3e-4, tau=0.01)
    assert main.parse_sweeps(None, 'sac', 4) == [('', {})]
    assert main.parse_sweeps(['auto_entropy_tuning=true,0', 'target_update_period=1,3'], 'ctrlsac', 1)[1][1] == \
        dict(auto_entropy_tuning=True, target_update_period=3)
