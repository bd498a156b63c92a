"""Prioritized replay for sac seed groups, the part that needs no GPU: the CPU form of PrioritizedReplayBufferGroup against
tests/per_reference.py, member by member and bit for bit, through every writer; the per-member scalars; the launcher's checks of
--group-per, all of which run before anything touches the GPU."""
import numpy as np
import pytest
import torch

from per_reference import PER_STREAM, RefTree, f32
from seed_group_util import run_launcher
from rlrep_amd.utils.buffer_group import PrioritizedReplayBufferGroup, ReplayBufferGroup

S, A, R = 3, 1, 3
ALPHA, BETA, EPS = [0.6, 0.0, 0.9], [0.4, 1.0, 0.0], [1e-6, 1e-3, 0.0]
SEEDS = [3, 5, 11]


def _rows(n, seed=0):
    """n transitions per member: [R, n, ...]"""
    r = np.random.default_rng(seed)
    return (r.normal(size=(R, n, S)).astype(np.float32), r.uniform(-1, 1, size=(R, n, A)).astype(np.float32), r.normal(size=(R, n, S)).astype(np.float32),
            r.normal(size=(R, n)).astype(np.float32), (r.random((R, n)) < 0.05).astype(np.float32))


def _pow32(td, eps, alpha):
    return np.ones(len(td), f32) if alpha == 0 else np.power((np.asarray(td, f32) + f32(eps)).astype(f32), f32(alpha), dtype=f32)


def _cpu(**kw):
    kw = dict(dict(alpha=ALPHA, beta=BETA, eps=EPS), **kw)
    return PrioritizedReplayBufferGroup(R, S, A, max_size=1000, device='cpu', stage_rows=64, **kw)


def _refs():
    return [RefTree(1000, ALPHA[r], BETA[r], EPS[r]) for r in range(R)]


def test_scalars_per_member_and_broadcast():
    b = _cpu()
    assert isinstance(b, ReplayBufferGroup) and b.prioritized_group and not getattr(b, 'prioritized', False)
    assert b.P == 1024 and tuple(b.trees.shape) == (R, 2048) and b.trees.dtype == torch.float32 and tuple(b._scal.shape) == (R, 4)
    want = np.array([[1.0, ALPHA[r], BETA[r], EPS[r]] for r in range(R)], f32)
    assert np.array_equal(b._scal.numpy(), want)
    assert b.alpha == [float(f32(v)) for v in ALPHA] and b.beta == [float(f32(v)) for v in BETA] and b.eps == [float(f32(v)) for v in EPS]
    assert [b.max_priority(r) for r in range(R)] == [1.0] * R
    c = PrioritizedReplayBufferGroup(R, S, A, max_size=1000, device='cpu')          # the defaults, broadcast
    assert np.array_equal(c._scal.numpy(), np.tile(np.array([1.0, 0.6, 0.4, 1e-6], f32), (R, 1)))
    e0 = b.device_epoch
    b.beta = 0.7                                     # a scalar: every member
    assert b.beta == [float(f32(0.7))] * R and np.all(b._scal.numpy()[:, 2] == f32(0.7)) and b.device_epoch == e0 + 1
    b.beta = [0.1, 0.2, 0.3]                         # ... or one value per member
    assert np.array_equal(b._scal.numpy()[:, 2], np.array([0.1, 0.2, 0.3], f32)) and np.array_equal(b._scal.numpy()[:, 1], np.array(ALPHA, f32))
    with pytest.raises(ValueError, match='alpha'):
        PrioritizedReplayBufferGroup(R, S, A, max_size=10, device='cpu', alpha=[0.1, 0.2])
    assert b.per_key()[1:] == (b.trees.data_ptr(), b._scal.data_ptr())


def test_cpu_form_equals_the_reference_per_member_through_every_writer():
    b, t = _cpu(), _refs()
    s, a, s2, r, d = _rows(1400)

    def same(what):
        for m in range(R):
            assert np.array_equal(b.trees[m].numpy(), t[m].tree), (what, m)
            assert b.max_priority(m) == float(t[m].max_p), (what, m)
            assert np.array_equal(b.priorities(m), t[m].tree[t[m].P:t[m].P + b.sizes[m]]), (what, m)

    for i in range(150):                     # add(): more than the 64 staging rows, so it flushes on its own
        b.add(s[:, i], a[:, i], s2[:, i], r[:, i], d[:, i])
    b.flush()
    for m in range(R):
        t[m].add(0, 150)
    same('add + flush')
    # sample + update: the members' maxima part ways, so the next rows enter at DIFFERENT priorities
    idx, w = b.draw(64, PER_STREAM + 1, seeds=SEEDS)
    td = (np.random.default_rng(3).random((R, 64)) * 5).astype(np.float32)
    for m in range(R):
        assert np.array_equal(idx[m].numpy(), t[m].sample(64, SEEDS[m], PER_STREAM + 1)), m
        wr, exact = t[m].weights(idx[m].numpy())
        assert np.all(w[m].numpy()[exact] == 1.0) and np.allclose(w[m].numpy(), wr, rtol=1e-6)
    b.update(64, td=td)
    for m in range(R):
        t[m].update(idx[m].numpy(), _pow32(td[m], t[m].eps, t[m].alpha))
    same('update')
    assert b.max_priority(0) > 1.0 and b.max_priority(1) == 1.0 and len({b.max_priority(m) for m in range(R)}) == 3
    # add_batch of 900 rows from row 150: across the wrap of the 1000-row rings and many times the staging capacity
    b.add_batch(s[:, 150:1050], a[:, 150:1050], s2[:, 150:1050], r[:, 150:1050], d[:, 150:1050])
    b.flush()
    for m in range(R):
        # the staging buffer flushes 64 rows at a time: every flush is an add of its own (the maximum does not move in between)
        t[m].add(150, 900)
    same('add_batch across the wrap')
    assert b.ptr == 50 and b.sizes == [1000] * R
    # a staged host row, then add_device: flushed first, in call order
    b.add(s[:, 1050], a[:, 1050], s2[:, 1050], r[:, 1050], d[:, 1050])
    b.add_device(*[torch.from_numpy(x[:, 1051:1400].copy()) for x in (s, a, s2, r, d)])
    for m in range(R):
        t[m].add(50, 1)
        t[m].add(51, 349)
    same('add_device')
    assert b.ptr == 400
    # given indices: only the weights
    given = np.stack([(np.arange(50) * (3 + m)) % 1000 for m in range(R)]).astype(np.int32)
    idx2, w2 = b.draw(50, 0, given=given)
    assert np.array_equal(idx2.numpy(), given)
    for m in range(R):
        wr, exact = t[m].weights(given[m])
        assert np.all(w2[m].numpy()[exact] == 1.0) and np.allclose(w2[m].numpy(), wr, rtol=1e-6)
    # load(r, fewer rows): member 1 alone; the rows its ring no longer holds lose their leaves, the other members' trees stay
    before = [b.trees[m].numpy().copy() for m in range(R)]
    b.load(1, s[1, :300], a[1, :300], s2[1, :300], r[1, :300], d[1, :300])
    t[1].clear(); t[1].add(0, 300)
    assert np.array_equal(b.trees[1].numpy(), t[1].tree) and np.all(b.trees[1].numpy()[1024 + 300:] == 0) and b.sizes == [1000, 300, 1000]
    assert np.array_equal(b.trees[0].numpy(), before[0]) and np.array_equal(b.trees[2].numpy(), before[2])
    # set_priorities(r, ...)
    leaves = (1.0 + np.arange(200) % 7).astype(np.float32)
    b.set_priorities(1, leaves, 7.0)
    t[1].clear(); t[1].set_leaves(np.arange(200), leaves); t[1].max_p = f32(7.0)
    same('set_priorities')
    with pytest.raises(ValueError, match='set_priorities'):
        b.set_priorities(1, np.ones(301, np.float32))
    for m in range(R):
        assert t[m].invariant_ok()


def test_draw_and_update_skip_members_that_are_not_live():
    b = _cpu()
    s, a, s2, r, d = _rows(100, 1)
    for m in range(R):
        b.load(m, s[m], a[m], s2[m], r[m], d[m])
    before = b.trees[1].numpy().copy()
    b.draw(16, PER_STREAM, seeds=SEEDS, live=[0, 2])
    b.update(16, td=np.full((R, 16), 3.0, np.float32), live=[0, 2])
    assert np.array_equal(b.trees[1].numpy(), before) and b.max_priority(1) == 1.0 and b.max_priority(0) > 1.0


def test_collect_on_device_raises():
    with pytest.raises(RuntimeError, match='PrioritizedReplayBufferGroup.collect_on_device'):
        _cpu().collect_on_device(object())


# ---- the launcher, before the GPU -------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'sac', '--env', 'Pendulum-v1', '--group-per', '--max_timesteps', '600', '--start_timesteps', '300', '--eval_freq', '300']


def test_group_per_needs_a_seed_group():
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE)
    assert '--group-per' in str(e.value) and '--seeds' in str(e.value) and '--sweep' in str(e.value)


@pytest.mark.parametrize('argv,named', [(['--alg', 'ctrlsac'] + BASE[2:] + ['--seeds', '0,1'], '--alg ctrlsac'),
                                        (BASE + ['--seeds', '0,1', '--device-env'], '--device-env'),
                                        (BASE + ['--seeds', '0,1', '--per'], '--per'),
                                        (BASE + ['--per'], '--per')])
def test_group_per_is_refused_with_what_it_does_not_run_with(argv, named):
    with pytest.raises(SystemExit) as e:
        run_launcher(argv)
    assert '--group-per' in str(e.value) and named in str(e.value)


def test_sweep_of_per_alpha_needs_group_per():
    argv = [x for x in BASE if x != '--group-per'] + ['--seeds', '0,1', '--sweep', 'per_alpha=0.4,0.6']
    with pytest.raises(SystemExit) as e:
        run_launcher(argv)
    assert 'per_alpha' in str(e.value) and '--group-per' in str(e.value)


def test_group_per_reaches_the_environments(monkeypatch):
    from rlrep_amd import main
    main._check_group_per(main.argparse.Namespace(alg='ctrlsac', seeds=None, sweep=None, device_env=True))      # built by hand, without the field

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(main.envs, 'make', stop)                # the first thing run_seeds does behind its checks
    with pytest.raises(Reached):
        main.run(BASE + ['--seeds', '0,1'])
    with pytest.raises(Reached):                                # the PER exponent as a sweep axis, with the rankings it is allowed with
        main.run(BASE + ['--seeds', '0,1', '--sweep', 'per_alpha=0.4,0.6,0.8', '--halving-interval', '300'])
    with pytest.raises(Reached):
        main.run(BASE + ['--sweep', 'per_alpha=0.4,0.6', '--pbt-interval', '300'])


def test_sweep_of_per_alpha_maps_to_the_members_trees():
    from rlrep_amd import main
    cfg = main.parse_sweeps(['per_alpha=0.4,0.8', 'lr=1e-4,3e-4'], 'sac', 2, group_per=True)
    assert [c['per_alpha'] for _, c in cfg] == [0.4, 0.4, 0.8, 0.8] and [c['lr'] for _, c in cfg] == [1e-4, 3e-4, 1e-4, 3e-4]
    for bad in ('per_alpha=-1,0.5', 'per_alpha=0.5,0.5', 'per_alpha=x'):
        with pytest.raises(SystemExit):
            main.parse_sweeps([bad], 'sac', 2, group_per=True)
