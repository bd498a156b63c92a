"""main.py's evaluation tail for one agent (_Evaluations: what run()'s five loops do at an evaluation step) against a stand-in agent, a
stand-in tensorboard writer and a log directory of its own, and the shared "is not a multiple of it" check against the messages
--num-envs, --host-envs and --torch-envs had when each wrote its own.  No GPU."""
import argparse
import json
import os
import sys
import types

import pytest


class _Agent(object):
    def __init__(self):
        self.saved = []

    def save(self, path, env=None):
        self.saved.append((path, env))


class _Replay(object):
    beta = 0.4


class _Writer(object):
    made = []

    def __init__(self, path):
        self.path, self.scalars, self.flushes, self.closed = path, [], 0, False
        _Writer.made.append(self)

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, value, step))

    def flush(self):
        self.flushes += 1

    def close(self):
        self.closed = True


def _evaluations(tmp_path, monkeypatch, tensorboard=True, **flags):
    from rlrep_amd import main
    from rlrep_amd.utils import util
    if tensorboard:
        monkeypatch.setitem(sys.modules, 'tensorboardX', types.SimpleNamespace(SummaryWriter=_Writer))
    else:
        monkeypatch.setitem(sys.modules, 'tensorboardX', None)              # (the import fails, as where it is not installed)
    args = argparse.Namespace(**dict(dict(save_model=False, per=False, per_beta=0.4, max_timesteps=1000.0), **flags))
    ev = main._Evaluations(args, _Agent(), _Replay(), str(tmp_path / 'log' / '0'))
    ev.timer = util.Timer()
    return ev


def _rows(ev):
    with open(os.path.join(ev.log_path, 'metrics.jsonl')) as f:
        return [json.loads(line) for line in f]


def test_the_files_are_opened_in_a_directory_it_creates(tmp_path, monkeypatch):
    ev = _evaluations(tmp_path, monkeypatch)
    assert os.path.isdir(ev.log_path) and os.path.exists(os.path.join(ev.log_path, 'metrics.jsonl'))
    assert ev.evaluations == [] and ev.tb is _Writer.made[-1] and ev.tb.path == ev.log_path
    ev.close()
    assert _evaluations(tmp_path, monkeypatch, tensorboard=False).tb is None


def test_without_an_info_the_score_is_filed_and_no_row_written(tmp_path, monkeypatch, capsys):
    ev = _evaluations(tmp_path, monkeypatch)
    ev.step(300, lambda: -1234.5, None)
    assert ev.evaluations == [-1234.5]
    assert _rows(ev) == [] and ev.tb.scalars == []
    assert 'Step 300. Steps per sec: ' in capsys.readouterr().out
    assert ev.agent.saved == [] and ev.replay.beta == 0.4


def test_a_row_holds_the_step_the_score_the_rate_and_every_info_key(tmp_path, monkeypatch, capsys):
    ev = _evaluations(tmp_path, monkeypatch)
    taken = []

    def score():
        taken.append(ev.timer._step)            # (the rate is taken before the evaluation runs: steps_per_sec excludes it)
        return -200.0
    ev.step(300, lambda: -900.0, None)
    ev.step(600, score, {'critic_loss': 2, 'alpha': 0.25})
    assert taken == [600] and ev.evaluations == [-900.0, -200.0]
    rows = _rows(ev)
    assert len(rows) == 1 and set(rows[0]) == {'step', 'info/evaluation', 'steps_per_sec', 'info/critic_loss', 'info/alpha'}
    assert rows[0]['step'] == 600 and rows[0]['info/evaluation'] == -200.0 and rows[0]['info/alpha'] == 0.25
    assert rows[0]['info/critic_loss'] == 2.0 and isinstance(rows[0]['info/critic_loss'], float)
    assert isinstance(rows[0]['steps_per_sec'], float) and rows[0]['steps_per_sec'] > 0
    # each info/* key, and no other, goes to tensorboard at that step
    assert sorted(ev.tb.scalars) == [('info/alpha', 0.25, 600), ('info/critic_loss', 2.0, 600), ('info/evaluation', -200.0, 600)]
    assert ev.tb.flushes == 1
    assert 'Step 600. Steps per sec: ' in capsys.readouterr().out
    # without tensorboardX the row is the same
    plain = _evaluations(tmp_path / 'plain', monkeypatch, tensorboard=False)
    plain.step(600, lambda: -200.0, {'critic_loss': 2, 'alpha': 0.25})
    assert [{k: v for k, v in r.items() if k != 'steps_per_sec'} for r in _rows(plain)] == \
        [{k: v for k, v in r.items() if k != 'steps_per_sec'} for r in rows]


def test_save_model_writes_agent_pt_with_the_environment_it_was_given(tmp_path, monkeypatch):
    ev = _evaluations(tmp_path, monkeypatch, save_model=True)
    env = object()
    ev.step(300, lambda: 0.0, None)
    ev.step(600, lambda: 0.0, {'alpha': 1.0}, env=env)
    assert ev.agent.saved == [(os.path.join(ev.log_path, 'agent.pt'), None), (os.path.join(ev.log_path, 'agent.pt'), env)]


def test_per_anneals_beta_by_per_anneals_formula(tmp_path, monkeypatch):
    ev = _evaluations(tmp_path, monkeypatch, per=True, per_beta=0.4, max_timesteps=1000.0)
    seen = []

    def score():
        seen.append(ev.replay.beta)             # (annealed before the evaluation, as the loops had it)
        return 0.0
    ev.step(250, score, None)
    assert seen == [0.4 + (1.0 - 0.4) * 0.25] and ev.replay.beta == seen[0]
    ev.step(1000, score, None)
    assert ev.replay.beta == 1.0


def test_close_closes_the_files_and_prints_the_total_time(tmp_path, monkeypatch, capsys):
    ev = _evaluations(tmp_path, monkeypatch)
    ev.close()
    assert ev.jsonl.closed and ev.tb.closed
    assert capsys.readouterr().out.startswith('Total time cost ')


# ---- the shared "is not a multiple of it" check: the messages of the three flags, as each wrote them itself -----------------------------------
NAMESPACE = dict(num_envs=1, host_envs=1, torch_envs=0, device_env=False, device_loop=False, seeds=None, sweep=None, env='Pendulum-v1',
                 start_timesteps=160.0, eval_freq=160, max_timesteps=1e6, pbt_interval=None, pbt_fraction=None, pbt_keys=None, pbt_factors=None,
                 pbt_seed=None, halving_interval=None, halving_keep=None, halving_min=None)
NOT_A_MULTIPLE = [
    ('_check_num_envs', dict(num_envs=4, device_loop=True, start_timesteps=150.0),
     '--num-envs 4: --start_timesteps 150 is not a multiple of it (a step launch takes 4 steps per member at once)'),
    ('_check_num_envs', dict(num_envs=4, device_env=True, eval_freq=150),
     '--num-envs 4: --eval_freq 150 is not a multiple of it (a step launch takes 4 steps per member at once)'),
    ('_check_num_envs', dict(num_envs=4, device_env=True, start_timesteps=160.5),
     '--num-envs 4: --start_timesteps 160.5 is not a multiple of it (a step launch takes 4 steps per member at once)'),
    ('_check_host_envs', dict(host_envs=4, start_timesteps=150.0),
     '--host-envs 4: --start_timesteps 150 is not a multiple of it (an iteration takes 4 environment steps at once)'),
    ('_check_host_envs', dict(host_envs=4, eval_freq=150),
     '--host-envs 4: --eval_freq 150 is not a multiple of it (an iteration takes 4 environment steps at once)'),
    ('_check_torch_envs', dict(torch_envs=8, start_timesteps=150.0),
     '--torch-envs 8: --start_timesteps 150 is not a multiple of it (an iteration takes 8 environment steps at once)'),
    ('_check_torch_envs', dict(torch_envs=8, eval_freq=150),
     '--torch-envs 8: --eval_freq 150 is not a multiple of it (an iteration takes 8 environment steps at once)'),
]


@pytest.mark.parametrize('check,fields,message', NOT_A_MULTIPLE)
def test_not_a_multiple_keeps_each_flags_message(check, fields, message):
    from rlrep_amd import main
    args = argparse.Namespace(**dict(NAMESPACE, **fields))
    with pytest.raises(SystemExit) as e:
        getattr(main, check)(args)
    assert str(e.value) == message
    getattr(main, check)(argparse.Namespace(**dict(NAMESPACE, **{k: v for k, v in fields.items() if k not in ('start_timesteps', 'eval_freq')})))


@pytest.mark.parametrize('check,flag', [('_check_per', '--per'), ('_check_group_per', '--group-per')])
def test_the_exponent_ranges_keep_each_flags_message(check, flag):
    from rlrep_amd import main
    base = dict(NAMESPACE, alg='sac', per=flag == '--per', group_per=flag == '--group-per', seeds='0,1' if flag == '--group-per' else None)
    for alpha, beta in ((-0.1, 0.4), (0.6, 1.5), (0.6, -0.1)):
        with pytest.raises(SystemExit) as e:
            getattr(main, check)(argparse.Namespace(**dict(base, per_alpha=alpha, per_beta=beta)))
        assert str(e.value) == f'{flag}: --per-alpha {alpha} must be >= 0 and --per-beta {beta} in [0, 1]'
    getattr(main, check)(argparse.Namespace(**dict(base, per_alpha=0.6, per_beta=0.4)))
