"""CPU-only: prioritized replay.  The NumPy restatement tests/per_reference.py against its own invariants, the CPU fallback
of PrioritizedReplayBuffer against the restatement bit for bit, and the launcher's refusals before the GPU."""
import numpy as np
import pytest
import torch

from per_reference import PER_STREAM, RefTree, f32
from rlrep_amd.utils.buffer import PrioritizedReplayBuffer, ReplayBuffer
from seed_group_util import run_launcher

S, A = 3, 1


def _rows(n, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, S)).astype(np.float32), r.normal(size=(n, A)).astype(np.float32), r.normal(size=(n, S)).astype(np.float32),
            r.normal(size=n).astype(np.float32), (r.random(n) < 0.1).astype(np.float32))


def _pow32(td, eps, alpha):
    return np.power(np.asarray(td, f32) + f32(eps), f32(alpha), dtype=f32)


# ---- the restatement itself -------------------------------------------------------------------------------------------------------------
def test_tree_invariant_after_any_mix_of_adds_and_updates():
    t = RefTree(1000)                       # not a power of two: P = 1024
    assert t.P == 1024 and t.tree.shape == (2048,)
    rng = np.random.default_rng(1)
    ptr, size = 0, 0
    for step in range(40):
        n = int(rng.integers(1, 90))
        t.add(ptr, n)                        # crosses the ring's end several times (40 x ~45 rows into 1000)
        ptr, size = (ptr + n) % 1000, min(size + n, 1000)
        assert t.invariant_ok(), step
        assert np.all(t.tree[t.P + size:] == 0)                 # rows never written and the padding hold 0
        if size >= 64:
            idx = t.sample(64, 7, PER_STREAM + step)
            assert idx.min() >= 0 and idx.max() < size
            t.update(idx, _pow32(rng.random(64) * 3, t.eps, t.alpha))
            assert t.invariant_ok(), step
    assert size == 1000 and ptr != 0


def test_sampled_indices_stay_below_size_with_a_heavy_leaf_and_a_zero_right_subtree():
    t = RefTree(1000)
    t.set_leaves(np.arange(400), 1.0)        # size 400 < 512: the root's right subtree and half of the left one's right are all zero
    t.set_leaves([137], 1e6)                 # one leaf with 10^6 times the others' mass
    assert t.tree[3] == 0 and t.invariant_ok()
    for call in range(50):
        for B in (50, 256):
            idx = t.sample(B, 11, PER_STREAM + call)
            assert idx.min() >= 0 and idx.max() < 400, (call, B, idx.max())
    assert np.mean(t.sample(256, 11, PER_STREAM) == 137) > 0.9
    # total mass in one leaf at the very end of the written range, m = total possible by rounding: still that leaf
    t2 = RefTree(8)
    t2.set_leaves([4], 3.0)
    assert set(t2.sample(64, 3, PER_STREAM).tolist()) == {4}


def test_sampling_frequencies_are_proportional_to_the_priorities():
    t = RefTree(8)
    t.set_leaves(np.arange(8), np.arange(1, 9, dtype=np.float32))
    B, calls = 64, 2000
    counts = np.zeros(8)
    for c in range(calls):
        counts += np.bincount(t.sample(B, 2024, PER_STREAM + c), minlength=8)
    n = B * calls
    p = np.arange(1, 9) / 36.0
    sd = np.sqrt(n * p * (1 - p))            # binomial; stratification only lowers the variance
    assert np.all(np.abs(counts - n * p) <= 5 * sd), (counts, n * p, sd)


def test_duplicate_indices_take_the_maximum_and_max_p_follows():
    t = RefTree(16)
    t.add(0, 16)
    idx = np.array([3, 3, 5, 3, 9, 5], np.int32)
    new = np.array([0.5, 4.0, 0.25, 2.0, 0.125, 0.75], f32)
    t.update(idx, new)
    assert t.tree[t.P + 3] == 4.0 and t.tree[t.P + 5] == 0.75 and t.tree[t.P + 9] == 0.125 and t.tree[t.P + 4] == 1.0
    assert t.max_p == 4.0 and t.invariant_ok()
    t.add(15, 3)                             # wraps: rows 15, 0, 1 at the new maximum
    assert t.tree[t.P + 15] == 4.0 and t.tree[t.P + 0] == 4.0 and t.tree[t.P + 1] == 4.0 and t.tree[t.P + 2] == 1.0 and t.invariant_ok()
    t.update(np.array([7], np.int32), np.array([0.5], f32))
    assert t.max_p == 4.0                    # never decreases


def test_an_updated_leaf_stays_positive():
    """td = 0 with eps = 0, or a NaN td: the touched leaf gets the floor (the smallest normal float32), not 0 -- the row stays in the tree"""
    from per_reference import PER_MIN_PRIORITY
    t = RefTree(16, eps=0.0)
    t.add(0, 16)
    with np.errstate(invalid='ignore'):
        t.update(np.array([2, 5, 5], np.int32), np.array([0.0, np.nan, 0.5], f32))
    assert t.tree[t.P + 2] == PER_MIN_PRIORITY and t.tree[t.P + 5] == 0.5 and t.max_p == 1.0 and t.invariant_ok()
    b = PrioritizedReplayBuffer(S, A, max_size=16, device='cpu', eps=0.0)
    b.load(*_rows(16))
    b.draw(3, 0, 0, given=np.array([2, 5, 5], np.int32))
    with np.errstate(invalid='ignore'):
        b.update(3, td=np.array([0.0, np.nan, 0.5 ** (1 / 0.6)], np.float32))
    leaves = b.priorities()
    assert leaves[2] == PER_MIN_PRIORITY and abs(leaves[5] - 0.5) < 1e-6 and np.all(leaves > 0) and np.isfinite(b.tree.numpy()).all()


def test_weights_are_one_at_the_minimum_and_at_beta_zero():
    t = RefTree(8, beta=1.0)
    t.set_leaves(np.arange(8), np.arange(1, 9, dtype=np.float32))
    w, exact = t.weights(np.array([1, 3, 1, 7]))
    assert exact.tolist() == [True, False, True, False] and np.allclose(w, [1.0, 0.5, 1.0, 0.25])
    t.beta = f32(0)
    assert np.all(t.weights(np.array([1, 3, 7]))[1])


# ---- the buffer's CPU fallback against the restatement, bit for bit ---------------------------------------------------------------------
def _cpu(max_size=1000, **kw):
    return PrioritizedReplayBuffer(S, A, max_size=max_size, device='cpu', stage_rows=64, **kw)


def test_buffer_is_a_replay_buffer_with_the_stated_defaults():
    b = _cpu()
    assert isinstance(b, ReplayBuffer) and b.prioritized
    assert (b.alpha, b.beta, b.eps) == (float(f32(0.6)), float(f32(0.4)), float(f32(1e-6))) and b.max_priority == 1.0
    assert b.P == 1024 and b.tree.shape == (2048,) and b.tree.dtype == torch.float32
    e0 = b.device_epoch
    b.beta = 0.7
    assert b.beta == float(f32(0.7)) and b.device_epoch == e0 + 1 and b._scal[2].item() == f32(0.7)
    with pytest.raises(RuntimeError, match='empty'):
        b.draw(8, 1, PER_STREAM)


def test_cpu_fallback_equals_the_reference_through_every_writer():
    b, t = _cpu(), RefTree(1000)
    s, a, s2, r, d = _rows(1400)
    ptr = 0

    def same(what):
        assert np.array_equal(b.tree.numpy(), t.tree), what
        assert b.max_priority == float(t.max_p), what
        assert np.array_equal(b.priorities(), t.tree[t.P:t.P + b.size]), what

    for i in range(150):                     # add(): more than the 64 staging rows, so it flushes on its own
        b.add(s[i], a[i], s2[i], r[i], d[i])
    b.flush()
    t.add(0, 150); ptr = 150
    same('add')
    b.add_batch(s[150:450], a[150:450], s2[150:450], r[150:450], d[150:450])
    b.flush()
    t.add(ptr, 300); ptr += 300
    same('add_batch')
    # sample + update in between: the next rows enter at the new maximum
    idx, w = b.draw(64, 5, PER_STREAM + 1)
    assert np.array_equal(idx.numpy(), t.sample(64, 5, PER_STREAM + 1))
    wr, exact = t.weights(idx.numpy())
    assert np.all(w.numpy()[exact] == 1.0) and np.allclose(w.numpy(), wr, rtol=1e-6)
    td = (np.random.default_rng(3).random(64) * 5).astype(np.float32)
    b.update(64, td=td)
    t.update(idx.numpy(), _pow32(td, t.eps, t.alpha))
    same('update')
    assert b.max_priority > 1.0
    b.add(s[450], a[450], s2[450], r[450], d[450])              # a staged host row, then add_device: flushed first, in call order
    tt = [torch.from_numpy(x) for x in (s[451:1100], a[451:1100], s2[451:1100], r[451:1100], d[451:1100])]
    b.add_device(*tt)                        # 649 rows from row 451: across the wrap of the 1000-row ring
    t.add(ptr, 1); t.add(ptr + 1, 649); ptr = (ptr + 650) % 1000
    same('add_device across the wrap')
    assert b.size == 1000 and b.ptr == ptr == 100
    idx, _ = b.draw(50, 5, PER_STREAM + 2)
    assert np.array_equal(idx.numpy(), t.sample(50, 5, PER_STREAM + 2))
    # given indices: only the weights
    idx2, w2 = b.draw(50, 0, 0, given=np.arange(50, dtype=np.int32) * 3)
    assert np.array_equal(idx2.numpy(), np.arange(50) * 3)
    wr, exact = t.weights(np.arange(50) * 3)
    assert np.all(w2.numpy()[exact] == 1.0) and np.allclose(w2.numpy(), wr, rtol=1e-6)
    # load() of fewer rows than the ring held: the rows it no longer holds lose their leaves
    assert b.size == 1000 and np.all(b.tree.numpy()[b.P + 700:b.P + 1000] > 0)
    b.load(s[:700], a[:700], s2[:700], r[:700], d[:700])
    t.clear(); t.add(0, 700)
    same('load')
    assert b.size == 700 and np.all(b.tree.numpy()[b.P + 700:] == 0) and b.max_priority > 1.0         # (max_p stays)
    for call in range(5):
        idx, _ = b.draw(256, 5, PER_STREAM + 10 + call)
        assert idx.numpy().min() >= 0 and idx.numpy().max() < 700


def test_save_restore_brings_back_leaves_and_max_p(tmp_path):
    b, t = _cpu(), RefTree(1000)
    s, a, s2, r, d = _rows(700)
    b.load(s, a, s2, r, d)
    t.add(0, 700)
    for k in range(3):
        idx, _ = b.draw(64, 9, PER_STREAM + k)
        td = (np.random.default_rng(k).random(64) * 4).astype(np.float32)
        b.update(64, td=td)
        t.update(idx.numpy(), _pow32(td, t.eps, t.alpha))
    path = str(tmp_path / 'ring.npz')
    b.save(path)
    c = _cpu()
    c.restore(path)
    assert np.array_equal(c.tree.numpy(), t.tree) and c.max_priority == float(t.max_p) and (c.ptr, c.size) == (b.ptr, b.size)
    assert torch.equal(c.ring, b.ring)
    assert np.array_equal(c.draw(64, 9, PER_STREAM + 7)[0].numpy(), b.draw(64, 9, PER_STREAM + 7)[0].numpy())
    # a plain ReplayBuffer's file: every row is new
    plain = ReplayBuffer(S, A, max_size=1000, device='cpu')
    plain.load(s[:300], a[:300], s2[:300], r[:300], d[:300])
    p2 = str(tmp_path / 'plain.npz')
    plain.save(p2)
    c.restore(p2)
    t2 = RefTree(1000)
    t2.add(0, 300)
    assert np.array_equal(c.tree.numpy(), t2.tree) and c.max_priority == 1.0


def test_collect_on_device_and_shard_raise():
    with pytest.raises(ValueError, match='shard'):
        PrioritizedReplayBuffer(S, A, max_size=100, device='cpu', shard=(0, 2))
    with pytest.raises(RuntimeError, match='PrioritizedReplayBuffer.collect_on_device'):
        _cpu().collect_on_device(object())


# ---- the launcher, before the GPU -------------------------------------------------------------------------------------------------------
BASE = ['--alg', 'sac', '--env', 'Pendulum-v1', '--per', '--max_timesteps', '600', '--start_timesteps', '300', '--eval_freq', '300']


@pytest.mark.parametrize('flags,named', [(['--seeds', '0,1'], '--seeds'), (['--sweep', 'lr=1e-4,3e-4'], '--sweep'), (['--device-env'], '--device-env'),
                                         (['--device-loop'], '--device-loop'), (['--pbt-interval', '300'], '--pbt-interval'),
                                         (['--halving-interval', '300'], '--halving-interval')])
def test_per_is_refused_with_the_flags_it_does_not_run_with(flags, named):
    with pytest.raises(SystemExit) as e:
        run_launcher(BASE + flags)
    assert '--per' in str(e.value) and named in str(e.value)


def test_per_needs_sac():
    with pytest.raises(SystemExit) as e:
        run_launcher(['--alg', 'vlsac'] + BASE[2:])
    assert '--per' in str(e.value) and '--alg sac' in str(e.value) and 'vlsac' in str(e.value)


def test_without_per_the_namespace_reaches_the_existing_paths_unchanged(monkeypatch):
    from rlrep_amd import main
    ns = dict(alg='vlsac', seeds='0,1', sweep=None, device_env=True, device_loop=False, pbt_interval=None, halving_interval=None)
    main._check_per(main.argparse.Namespace(**ns))              # built by hand, without the new fields: nothing to refuse
    main._check_per(main.argparse.Namespace(per=False, **ns))
    main._per_anneal(main.argparse.Namespace(**ns), None, 100)  # ... and nothing to anneal

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(main.envs, 'make', stop)                # the first thing the existing path does
    with pytest.raises(Reached):
        main.run(['--alg', 'sac', '--env', 'Pendulum-v1', '--max_timesteps', '600', '--start_timesteps', '300', '--eval_freq', '300'])
    with pytest.raises(Reached):                                # with --per the checks pass and the same path is taken
        main.run(BASE)


def test_beta_is_annealed_linearly_to_one():
    from rlrep_amd import main
    args = main.argparse.Namespace(per=True, per_beta=0.4, max_timesteps=600.0)
    b = _cpu(beta=0.4)
    main._per_anneal(args, b, 300)
    assert b.beta == float(f32(0.7))
    main._per_anneal(args, b, 600)
    assert b.beta == 1.0 and b._scal[2].item() == 1.0
