"""The per-element optimizer bounds of tests/optimizer_reference.py, checked without a GPU: they hold for correct float32 arithmetic (an
emulation of adam_elem in NumPy float32) over a wide dynamic range, they reject five subtly wrong kernels on realistic data, and the float64
reference itself agrees with oracle/optim.py and torch.optim.Adam."""
import numpy as np
import pytest
import torch

import fixture_io  # noqa: F401  (puts the repository root on sys.path)
import optimizer_reference as R

N = 2_000_000
# the record's hyper-parameters: float32 values, as include/rlrep.h's float fields hold them
LR, B1, B2, ADAM_EPS, TAU = (float(np.float32(x)) for x in (3e-4, 0.9, 0.999, 1e-8, 0.005))
STEPS = (1, 2, 3, 1000, 100000)


def _ratios(p0, g, m0, v0, t0, p1, m1, v1, t1, step):
    cfg = (step, LR, B1, B2, ADAM_EPS, TAU)
    out = {q: r for q, (r, _) in R.check_elements(p0, g, m0, v0, p1, m1, v1, cfg).items()}
    out['t'] = R.check_polyak(p1, t0, t1, TAU)[0]
    return out


@pytest.mark.parametrize('step', STEPS)
@pytest.mark.parametrize('p_zero', [True, False], ids=['p0_zero', 'p0_random'])
def test_bounds_hold_for_correct_float32_arithmetic(step, p_zero):
    p0, g, m0, v0, t0 = R.wide_range(N, 1000 + step % 997 + (7 if p_zero else 0), p_zero)
    sc = R.scalars_f32(LR, B1, B2, ADAM_EPS, TAU, step)
    p1, m1, v1, t1 = R.emulate(p0, g, m0, v0, t0, sc)
    assert all(np.isfinite(x).all() for x in (p1, m1, v1, t1))
    r = _ratios(p0, g, m0, v0, t0, p1, m1, v1, t1, step)
    print(f'step {step} p0 {"zero" if p_zero else "random"}: worst error / bound  m {r["m"]:.3f}  v {r["v"]:.3f}  p {r["p"]:.3f}  t {r["t"]:.3f}')
    for q in R.QUANTITIES:
        assert r[q] < 1.0, (q, r[q])
    # every combination of exact zeros among g, m, v occurred
    zs = {(bool(a), bool(b), bool(c)) for a, b, c in zip((g[:20000] == 0), (m0[:20000] == 0), (v0[:20000] == 0))}
    assert len(zs) == 8


MUTATIONS = ('skip4', 'bias_step', 'sqrt_eps_inside', 'tau_swapped', 'polyak_old_p')


def _mutated(mutation, n=4096, step=3):
    p0, g, m0, v0, t0 = R.realistic(n, 5)
    sc = R.scalars_f32(LR, B1, B2, ADAM_EPS, TAU, step, bias_step=step + 1 if mutation == 'bias_step' else None)
    p1, m1, v1, t1 = R.emulate(p0, g, m0, v0, t0, sc, mutation if mutation in ('sqrt_eps_inside', 'tau_swapped', 'polyak_old_p') else None)
    if mutation == 'skip4':           # one four-element group that the launch never touched
        for new, old in ((p1, p0), (m1, m0), (v1, v0), (t1, t0)):
            new[1028:1032] = old[1028:1032]
    return _ratios(p0, g, m0, v0, t0, p1, m1, v1, t1, step)


def test_unmutated_emulation_is_accepted_on_realistic_data():
    r = _mutated(None)
    print('unmutated: ' + '  '.join(f'{q} {r[q]:.3f}' for q in R.QUANTITIES))
    assert max(r.values()) < 1.0, r


@pytest.mark.parametrize('mutation', MUTATIONS)
def test_bounds_reject_subtly_wrong_kernels(mutation):
    r = _mutated(mutation)
    print(f'{mutation}: ' + '  '.join(f'{q} {r[q]:.3g}' for q in R.QUANTITIES))
    assert max(r.values()) > 1e2, (mutation, r)
    # each defect shows where it lives: the Polyak ones leave Adam's three outputs inside their bounds
    if mutation in ('tau_swapped', 'polyak_old_p'):
        assert max(r[q] for q in 'mvp') < 1.0 and r['t'] > 1e2, r
    if mutation in ('bias_step', 'sqrt_eps_inside'):
        assert r['m'] < 1.0 and r['v'] < 1.0 and r['p'] > 1e2, r


def test_check_group_reports_the_element_and_the_closed_gate():
    """check_group on a synthetic arena: a wrong element is reported at its arena index; with the gate closed a moved target is a failure."""
    n, off = 64, 8
    p0, g, m0, v0, t0 = R.realistic(off + n + 8, 9)
    cfg_row = np.zeros(22, np.float32)
    cfg_row[:1].view(np.int32)[0] = 3
    cfg_row[1:6] = [LR, B1, B2, ADAM_EPS, TAU]
    sc = R.scalars_f32(LR, B1, B2, ADAM_EPS, TAU, 3)
    p1, m1, v1, t1 = R.emulate(p0, g, m0, v0, t0, sc)
    before = dict(params=p0, targets=t0, exp_avg=m0, exp_avg_sq=v0)
    after = dict(params=p1.copy(), targets=t1.copy(), exp_avg=m1, exp_avg_sq=v1)
    pmap = [(off + 16, off + 16, 32)]
    res = R.check_group(before, after, g, cfg_row, (off, n), pmap, True)
    assert max(r for r, _ in res.values()) < 1.0, res
    after['params'][off + 21] = p0[off + 21]
    res = R.check_group(before, after, g, cfg_row, (off, n), pmap, True)
    assert res['p'][0] > 1e2 and res['p'][1] == off + 21, res
    after['params'][off + 21] = p1[off + 21]
    res = R.check_group(before, after, g, cfg_row, (off, n), pmap, False)          # gate closed, but the targets moved
    assert res['t'][0] == np.inf, res
    after['targets'] = t0.copy()
    assert R.check_group(before, after, g, cfg_row, (off, n), pmap, False)['t'][0] == 0.0
    mk = R.mask_of(len(p0), [(off, n)])
    assert R.bit_identical_outside(p0, after['params'], mk) >= 0           # the emulation above stepped the elements outside the slice too
    assert R.bit_identical_outside(p0, np.where(mk, after['params'], p0), mk) == -1


def test_reference_agrees_with_torch_and_the_oracle():
    """expected() is Adam as torch.optim.Adam and oracle/optim.py compute it on float64 tensors with the same betas (1e-13), over three
    consecutive steps; polyak_expected() is oracle/optim.py's polyak."""
    from oracle.optim import Adam, polyak
    rs = np.random.RandomState(3)
    n = 1000
    p = 0.05 * rs.standard_normal(n)
    tp = torch.nn.Parameter(torch.tensor(p.copy(), dtype=torch.float64))
    topt = torch.optim.Adam([tp], lr=LR, betas=(B1, B2), eps=ADAM_EPS)
    oP = {'x.w': torch.tensor(p.copy(), dtype=torch.float64)}
    oopt = Adam(['x.w'], LR, (B1, B2), ADAM_EPS)
    m, v = np.zeros(n), np.zeros(n)
    for step in (1, 2, 3):
        g = 1e-3 * rs.standard_normal(n)
        ex = R.expected(p, g, m, v, None, LR, B1, B2, ADAM_EPS, TAU, step)
        tp.grad = torch.tensor(g.copy(), dtype=torch.float64)
        topt.step()
        oopt.step(oP, {'x.w': torch.tensor(g.copy(), dtype=torch.float64)})
        for name, got in (('torch', tp.detach().numpy()), ('oracle', oP['x.w'].numpy())):
            assert np.max(np.abs(got - ex['p']) / np.maximum(np.abs(ex['p']), 1e-3)) < 1e-13, (name, step)
        st = topt.state[tp]
        assert np.max(np.abs(st['exp_avg'].numpy() - ex['m'])) <= 1e-13 * np.max(np.abs(ex['m']))
        assert np.max(np.abs(st['exp_avg_sq'].numpy() - ex['v'])) <= 1e-13 * np.max(np.abs(ex['v']))
        assert np.max(np.abs(oopt.state['x.w']['m'].numpy() - ex['m'])) <= 1e-13 * np.max(np.abs(ex['m']))
        p, m, v = ex['p'], ex['m'], ex['v']
    t0 = 0.05 * rs.standard_normal(n)
    P = {'x.w': torch.tensor(p), 'x_target.w': torch.tensor(t0.copy())}
    polyak(P, 'x', 'x_target', TAU)
    want = R.polyak_expected(p, t0, TAU)
    assert np.max(np.abs(P['x_target.w'].numpy() - want)) <= 1e-13 * np.max(np.abs(want))


def test_temperature_check_accepts_float64_adam_and_rejects_a_wrong_step():
    a0 = np.array([np.log(0.1), 0.02, 3e-4, 4.0])
    good = R.temperature_expected(a0, 0.31, LR, B1, B2, ADAM_EPS)
    res = R.check_temperature(a0, good, LR, B1, B2, ADAM_EPS)
    assert res['ok'] and abs(res['g'] - 0.31) < 1e-12, res
    bad = good.copy()
    bad[0] = a0[0] - (LR / (1.0 - B1 ** 6.0)) * (good[1] / (np.sqrt(good[2]) / np.sqrt(1.0 - B2 ** 6.0) + ADAM_EPS))     # bias correction of step + 1
    assert not R.check_temperature(a0, bad, LR, B1, B2, ADAM_EPS)['ok']
    f32 = good.copy()
    f32[0] = np.float32(good[0])                                  # a float32 log_alpha (quirk Q1 is float64)
    assert not R.check_temperature(a0, f32, LR, B1, B2, ADAM_EPS)['ok']
    late = good.copy()
    late[3] += 1.0
    assert not R.check_temperature(a0, late, LR, B1, B2, ADAM_EPS)['ok']
