"""Every optimizer launch held to float64 Adam, element by element (tests/optimizer_reference.py has the reference and the derivation of the
per-element rounding bounds; tests/test_optimizer_elements_cpu.py shows that the bounds hold for correct float32 arithmetic and reject subtly
wrong kernels).

A test clones the arenas and the optimizer records, runs ONE entry point (or one train() call), and asserts
  1. the record of every group that steps has step + 1;
  2. every element of such a group's slice satisfies the bounds against the gradient the device left in the gradient arena;
  3. outside those slices params / exp_avg / exp_avg_sq are bit-identical, and so is every target element the step's Polyak map does not name;
  4. Polyak'd targets satisfy t1 = tau p1 + (1 - tau) t0 (p1: what the device wrote) within the bound when the gate is open, and are
     bit-identical when it is closed.
Every test prints its worst error / bound ratio per quantity (measured values: docs/history/optimizer_elements.md)."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from fixture_io import Case      # noqa: F401  (puts tests/golden and the repository root on sys.path)
import synth
import optimizer_reference as R
from test_hip_parity import _Space, make_buffer

pytestmark = pytest.mark.gpu

ALGS = ('sac', 'vlsac', 'ctrlsac', 'spedersac', 'diffsrsac')
CLS = {'sac': ('rlrep_amd.agent.sac.sac_agent', 'SACAgent'), 'vlsac': ('rlrep_amd.agent.vlsac.vlsac_agent', 'VLSACAgent'),
       'ctrlsac': ('rlrep_amd.agent.ctrlsac.ctrlsac_agent', 'CTRLSACAgent'), 'spedersac': ('rlrep_amd.agent.spedersac.spedersac_agent', 'SPEDERSACAgent'),
       'diffsrsac': ('rlrep_amd.agent.diffsrsac.diffsrsac_agent', 'DIFFSRSACAgent')}
FEATURE_TWINS = {'sac': (), 'vlsac': ('f',), 'ctrlsac': ('phi',), 'spedersac': ('phi',), 'diffsrsac': ()}      # what a feature step averages
FEATURE_GROUPS = {'sac': [], 'vlsac': [0], 'ctrlsac': [0], 'spedersac': [0], 'diffsrsac': [0, 3]}
CRITIC_GROUPS = {a: ([] if a == 'diffsrsac' else [1]) for a in ALGS}            # quirk Q11: diffsrsac's critic is never trained
ARENAS = ('params', 'targets', 'exp_avg', 'exp_avg_sq')


def _cls(alg):
    mod, name = CLS[alg]
    return getattr(importlib.import_module(mod), name)


def _agent(c, **extra):
    kw = dict(c.kw)
    if c.meta.get('patch_vae_hidden'):
        kw['vae_hidden_dim'] = c.meta['patch_vae_hidden']
    kw.update(extra)
    kw.setdefault('graph', False)
    agent = _cls(c.alg)(state_dim=c.S, action_dim=c.A, action_space=_Space(c.A, c.meta['bound']), max_batch=c.B, **kw)
    agent.core.load_state(c.init)
    assert agent.target_update_period == 2
    return agent


def _counter(core):
    off = core.steps_dev() - core.workspace.data_ptr()
    return int(core.workspace[off:off + 4].view(torch.int32).item())


def _snap(core):
    torch.cuda.synchronize()
    s = {k: getattr(core, k).cpu().numpy() for k in ARENAS}
    s['grads'] = core.grads.cpu().numpy()
    s['alpha'] = core.alpha_state.cpu().numpy()
    s['cfg'] = core.group_cfg().cpu().numpy()
    s['counter'] = _counter(core)
    return s


def _step_of(s, g):
    return int(s['cfg'][g, :1].view(np.int32)[0])


def _where(core, idx, target=False):
    """Names the element for a failure message: tensor, offset inside it, its size, and the offset modulo 4 inside the arena."""
    for name, (arena, group, off, rows, cols) in core.descs.items():
        if (arena == 1) == target and off <= idx < off + rows * cols:
            return f'{name}[{idx - off} of {rows}x{cols}] group {group} arena index {idx} (mod 4: {idx % 4})'
    return f'alignment padding at arena index {idx} (mod 4: {idx % 4})'


def _verify(core, before, after, stepping, twins, gate, label):
    """stepping: groups whose optimizer ran; twins: {group: Polyak map}; gate: {group: open?} (default open).  -> worst ratios per quantity"""
    L = core.layout
    worst = dict.fromkeys(R.QUANTITIES, 0.0)
    for g in range(4):
        want = _step_of(before, g) + (1 if g in stepping else 0)
        if core.alg == 'diffsrsac' and g == 1:
            continue          # (its critic step has no optimizer; what its loss kernel does to the record is not part of this contract)
        assert _step_of(after, g) == want, (label, 'step counter of group', g, _step_of(after, g), want)
    for g in stepping:
        res = R.check_group(before, after, after['grads'], after['cfg'][g], (L.group_offset[g], L.group_floats[g]), twins.get(g, []), gate.get(g, True))
        for q, (r, i) in res.items():
            worst[q] = max(worst[q], r)
            assert r < 1.0, (label, f'group {g}', q, f'error / bound = {r:.3g}', _where(core, i, target=(q == 't')))
    for g, tm in twins.items():
        if g in stepping:
            continue
        for po, to, n in tm:      # a Polyak without an optimizer step (the stand-alone polyak launch; diffsrsac's critic)
            t0, t1 = before['targets'][to:to + n], after['targets'][to:to + n]
            if gate.get(g, True):
                r, i = R.check_polyak(after['params'][po:po + n], t0, t1, R.record(after['cfg'][g])[5])
                worst['t'] = max(worst['t'], r)
                assert r < 1.0, (label, 't', f'error / bound = {r:.3g}', _where(core, to + i, target=True))
            else:
                assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)), (label, 'closed gate, target moved', _where(core, to, target=True))
    mk = R.mask_of(L.param_floats, [(L.group_offset[g], L.group_floats[g]) for g in stepping])
    for k in ('params', 'exp_avg', 'exp_avg_sq'):
        i = R.bit_identical_outside(before[k], after[k], mk)
        assert i < 0, (label, k, 'changed outside the stepping groups', _where(core, i))
    tmk = R.mask_of(L.target_floats, [(to, n) for tm in twins.values() for _, to, n in tm])
    i = R.bit_identical_outside(before['targets'], after['targets'], tmk)
    assert i < 0, (label, 'a target outside the Polyak map changed', _where(core, i, target=True))
    print(f'{label}: worst error / bound  ' + '  '.join(f'{q} {worst[q]:.3f}' for q in R.QUANTITIES))
    return worst


def _unchanged(before, after, label, keys=ARENAS + ('alpha',)):
    for k in keys:
        a, b = before[k], after[k]
        assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64)), (label, k)


def _check_alpha(before, after, label, learn=True):
    if not learn:
        assert np.array_equal(before['alpha'].view(np.uint64), after['alpha'].view(np.uint64)), (label, 'temperature record moved with auto_entropy_tuning=False')
        return
    _, lr, b1, b2, eps, _ = R.record(after['cfg'][2])
    res = R.check_temperature(before['alpha'][:4], after['alpha'][:4], lr, b1, b2, eps)
    print(f'{label}: temperature g {res["g"]:.6g}  rel err v {res["v"]:.2e}  log_alpha {res["log_alpha"]:.2e}')
    assert res['ok'], (label, res, before['alpha'], after['alpha'])


def _draws(c, rs):
    dev = 'cuda'
    out = dict(crit=torch.as_tensor(rs.standard_normal((c.B, c.A)).astype(np.float32), device=dev),
               act=torch.as_tensor(rs.standard_normal((c.B, c.A)).astype(np.float32), device=dev))
    F = c.kw.get('feature_dim', 0)
    if c.alg == 'vlsac':
        out['feat'] = (torch.as_tensor(rs.standard_normal((c.B, F)).astype(np.float32), device=dev), None)
    elif c.alg == 'diffsrsac':
        out['feat'] = (torch.as_tensor((0.449 * rs.standard_normal((c.B, c.S))).astype(np.float32), device=dev),
                       torch.as_tensor(rs.randint(0, 1000, size=c.B).astype(np.int32), device=dev))
    else:
        out['feat'] = (None, None)
    return out


def _setup(alg, **extra):
    """A tiny agent after ONE warm-up train() on the fixture's injected draws: both moments non-zero, both minibatch slots filled, train counter 1."""
    c = Case(alg + '_tiny')
    agent = _agent(c, **extra)
    buf = make_buffer(c)
    agent.train_injected(buf, c.B, c.trains[0]['idx'], c.trains[0]['eps'])
    torch.cuda.synchronize()
    assert _counter(agent.core) == 1
    return c, agent, buf


# ---- (a) step consistency, eager entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ALGS)
def test_eager_entry_points_step_exactly_their_groups(alg):
    c, agent, buf = _setup(alg)
    core = agent.core
    d = _draws(c, np.random.RandomState(17))
    ctw = {1: R.twin_map(core.descs, ('critic',))}
    assert ctw[1], 'no critic / critic_target twins in the layout'
    period = agent.target_update_period

    # feature step: Adam on the feature group(s), Polyak of the feature target in the same launch (update_feature_target is fused: ungated)
    if FEATURE_GROUPS[alg]:
        ftw = R.twin_map(core.descs, FEATURE_TWINS[alg])
        assert bool(ftw) == bool(FEATURE_TWINS[alg])
        b = _snap(core)
        core.feature_step(*d['feat'])
        a = _snap(core)
        _verify(core, b, a, FEATURE_GROUPS[alg], {0: ftw} if ftw else {}, {}, f'{alg} feature step')
        _unchanged(b, a, f'{alg} feature step', ('alpha',))

    # critic step outside a begin_train .. update_target bracket: Adam only (diffsrsac: nothing at all, quirk Q11)
    b = _snap(core)
    core.critic_step(d['crit'])
    a = _snap(core)
    _verify(core, b, a, CRITIC_GROUPS[alg], {}, {}, f'{alg} critic step, no bracket')
    _unchanged(b, a, f'{alg} critic step', ('alpha',))
    if alg == 'diffsrsac':
        _unchanged(b, a, 'diffsrsac critic step moves nothing')

    # the stand-alone Polyak launch, train counter 1: gate closed
    assert b['counter'] % period == 1
    core.update_target()
    a2 = _snap(core)
    _verify(core, a, a2, [], ctw, {1: False}, f'{alg} update_target alone, counter {a2["counter"]} (closed)')

    # bracket at counter 2: the gate is open (the critic group's launch carries the Polyak where the agent has the folded form)
    for expect_open in (True, False):
        b = _snap(core)
        core.begin_train()
        core.critic_step(d['crit'])
        core.update_target()
        a = _snap(core)
        assert a['counter'] == b['counter'] + 1 and (a['counter'] % period == 0) == expect_open
        _verify(core, b, a, CRITIC_GROUPS[alg], ctw, {1: expect_open}, f'{alg} critic step in a bracket, counter {a["counter"]} ({"open" if expect_open else "closed"})')
        if expect_open:
            # ... and the stand-alone launch at the same (even) counter: open
            core.update_target()
            a2 = _snap(core)
            _verify(core, a, a2, [], ctw, {1: True}, f'{alg} update_target alone, counter {a2["counter"]} (open)')

    # actor step: Adam on the actor group, float64 Adam on the temperature
    b = _snap(core)
    core.actor_step(d['act'])
    a = _snap(core)
    _verify(core, b, a, [2], {}, {}, f'{alg} actor step')
    _check_alpha(b, a, f'{alg} actor step')

    if alg == 'ctrlsac':
        b = _snap(core)
        core.sync_frozen()
        a = _snap(core)
        _unchanged(b, a, 'sync_frozen', ('params', 'exp_avg', 'exp_avg_sq', 'alpha'))
        fz = []
        for name, (arena, _g, off, rows, cols) in core.descs.items():
            if name.startswith('phi.'):
                for dst in ('frozen_phi', 'frozen_phi_target'):
                    t = core.descs[dst + name[3:]]
                    assert t[0] == 1
                    fz.append((t[2], rows * cols))
                    assert np.array_equal(a['targets'][t[2]:t[2] + rows * cols].view(np.uint32), a['params'][off:off + rows * cols].view(np.uint32)), (dst, name)
        assert R.bit_identical_outside(b['targets'], a['targets'], R.mask_of(core.layout.target_floats, fz)) < 0


def test_fixed_temperature_is_left_alone():
    c, agent, buf = _setup('sac', auto_entropy_tuning=False)
    core = agent.core
    d = _draws(c, np.random.RandomState(18))
    b = _snap(core)
    core.actor_step(d['act'])
    a = _snap(core)
    _verify(core, b, a, [2], {}, {}, 'sac actor step, fixed temperature')
    _check_alpha(b, a, 'sac actor step, fixed temperature', learn=False)


# ---- (b) the forms only some configurations take ------------------------------------------------------------------------------------------------
def test_vlsac_chained_feature_step():
    """The first of two chained feature steps (rlrep_feature_chain_next): encoder.l1 / f.l1 take their optimizer (and f.l1 its Polyak into
    f_target.l1) in the weight-gradient epilogues (FLAG_ADAM), the rest of the group in adam_l1_kernel, which skips those two ranges."""
    c, agent, buf = _setup('vlsac')
    core = agent.core
    rs = np.random.RandomState(19)
    F = c.kw['feature_dim']
    eps = [torch.as_tensor(rs.standard_normal((c.B, F)).astype(np.float32), device='cuda') for _ in range(2)]
    idx_next = torch.as_tensor(rs.randint(0, buf.size, size=c.B).astype(np.int32), device='cuda')
    ftw = {0: R.twin_map(core.descs, ('f',))}
    b = _snap(core)
    assert core.prefetch_batch(buf.ring, idx_next, c.B, 0), 'the next minibatch must ride in the optimizer launch'
    assert core.feature_chain_next() == 1, 'vlsac_tiny must have the chained form'
    core.feature_step(eps[0])
    a = _snap(core)
    _verify(core, b, a, [0], ftw, {}, 'vlsac chained feature step (epilogue Adam + adam_l1)')
    # the second step, as the header requires: it starts behind the first layers that rode in the launch above
    core.feature_step(eps[1])
    a2 = _snap(core)
    _verify(core, a, a2, [0], ftw, {}, 'vlsac feature step after a chained one')


def _synth_agent(alg, S, A, B, kw):
    from oracle.shapes import param_shapes
    from rlrep_amd.utils.buffer import ReplayBuffer
    from test_large_dims import _retie
    init = synth.init_like(param_shapes(alg, S, A, **kw), seed=99)
    _retie(alg, init)
    init['log_alpha'] = np.log(np.float64(0.1))
    if alg == 'vlsac':
        init['critic.noise'] = np.random.RandomState(5).standard_normal(init['critic.noise'].shape).astype(np.float32)
        init['critic_target.noise'] = init['critic.noise'].copy()
    space = _Space(A, 1.0)
    agent = _cls(alg)(state_dim=S, action_dim=A, action_space=space, max_batch=B, graph=False, **kw)
    agent.core.load_state(init)
    data = synth.replay(S, A, 4096, seed=3)
    buf = ReplayBuffer(S, A, max_size=4096)
    buf.load(data['state'], data['action'], data['next_state'], data['reward'], data['done'])
    buf.flush()
    assert agent.target_update_period == 2
    return agent, buf


@pytest.mark.parametrize('S,A,B,F,H', [(7, 3, 37, 96, 96), (17, 6, 260, 256, 256)])
def test_vlsac_critic_step_sums_split_k_partials_in_the_optimizer_launch(S, A, B, F, H, monkeypatch):
    """The bf16x3 weight gradient of the noise critic leaves split-K partials; the critic group's optimizer launch sums them in split order
    (AdamTask::Slab, aligned form), files the sum in the gradient arena and steps on it.  Two bracketed critic steps (train counter 1: gate
    closed, 2: open), the second one checked; RLREP_DISABLE=fold_ncdw (a finishing launch sums the partials) must give the same bits."""
    from rlrep_amd import _lib
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    outs, launches = [], []
    for form in ('', 'fold_ncdw'):
        if form:
            monkeypatch.setenv('RLREP_DISABLE', form)
        else:
            monkeypatch.delenv('RLREP_DISABLE', raising=False)
        agent, buf = _synth_agent('vlsac', S, A, B, dict(hidden_dim=H, feature_dim=F, extra_feature_steps=1))
        core = agent.core
        rs = np.random.RandomState(11)
        ctw = {1: R.twin_map(core.descs, ('critic',))}
        for k in range(2):
            idx = torch.as_tensor(rs.randint(0, 4096, size=B), device='cuda')
            eps = torch.as_tensor(rs.standard_normal((B, A)).astype(np.float32), device='cuda')
            agent._set_batch(buf.gather(idx))
            b = _snap(core)
            n0 = _lib.lib.rlrep_launch_counter()
            core.begin_train()
            core.critic_step(eps)
            core.update_target()
            n = _lib.lib.rlrep_launch_counter() - n0
            a = _snap(core)
            assert a['counter'] == k + 1
            if k == 1:
                _verify(core, b, a, [1], ctw, {1: True}, f'vlsac critic step {(S, A, B, F, H)} RLREP_DISABLE={form!r}')
        outs.append(a)
        launches.append(n)
        del agent, core
    assert launches[0] < launches[1], ('the folded form must save the finishing launch', launches)
    _unchanged(outs[1], outs[0], 'fold_ncdw on / off', ARENAS)


ANT = dict(phi_and_mu_lr=1e-5, phi_hidden_dim=512, phi_hidden_depth=1, mu_hidden_dim=512, mu_hidden_depth=0, critic_and_actor_lr=3e-4,
           critic_and_actor_hidden_dim=256, feature_dim=512, hidden_dim=256, extra_feature_steps=0)


def _plan(la, lb, R_, Cn, K, lda, ldb, ldc):
    from rlrep_amd import _lib
    out = [C.c_int32() for _ in range(5)]
    assert _lib.lib.rlrep_gemm_plan(la, lb, R_, Cn, K, lda, ldb, ldc, *[C.byref(o) for o in out]) == 0
    return dict(zip(('engine', 'tile', 'splits', 'kchunk', 'scalar'), (o.value for o in out)))


def test_spedersac_feature_step_sums_padded_slab_rows(monkeypatch):
    """The `cols % 4 != 0` branch of the slab sums: phi.trunk.0's [512, S + A] and mu.trunk.0's [512, S] gradients with S + A = 119 and S = 111,
    slab rows padded to 120 / 112 floats.

    Dimensions: the planner (rlrep_gemm_plan, asked on the CPU) sends a weight gradient to the split-K engine only from 2 R Cn K >= 2e8 flops,
    whatever the shape, so nothing much smaller than the Ant network splits; a scan over S, A, hidden widths 64 .. 512 and batches 64 .. 1024
    found splits for both gradients only at S = 111, hidden 512, and there from B = 880 on (K = 2 B = 1760: six splits of 320, the last one
    ragged; at B = 878 the [512, 111] gradient stays on the 16-row engine).  So: tests/test_large_dims.py's Ant network at B = 880."""
    S, A, B, Hd = 111, 8, 880, 512
    monkeypatch.delenv('RLREP_ENABLE', raising=False)
    monkeypatch.delenv('RLREP_DISABLE', raising=False)
    for cols, ldb in ((S + A, S + A), (S, 2 * S + A)):
        assert cols % 4 != 0
        assert _plan(1, 1, Hd, cols, 2 * B, Hd, ldb, cols)['splits'] > 1
    assert _plan(1, 1, Hd, S, 2 * (B - 2), Hd, 2 * S + A, S)['splits'] == 1
    from rlrep_amd import _lib
    outs, launches = [], []
    for form in ('', 'fold_dwfin'):
        if form:
            monkeypatch.setenv('RLREP_DISABLE', form)
        agent, buf = _synth_agent('spedersac', S, A, B, ANT)
        core = agent.core
        rs = np.random.RandomState(12)
        ftw = {0: R.twin_map(core.descs, ('phi',))}
        for k in range(2):
            b1 = buf.gather(torch.as_tensor(rs.randint(0, 4096, size=B), device='cuda'))
            b2 = buf.gather(torch.as_tensor(rs.randint(0, 4096, size=B), device='cuda'))
            agent._set_batch(b1, 0)
            z = torch.zeros(B, 1, device='cuda')
            core.set_batch(1, b2.state, b2.action, z, b2.next_state, z)
            b = _snap(core)
            n0 = _lib.lib.rlrep_launch_counter()
            core.feature_step(None)
            n = _lib.lib.rlrep_launch_counter() - n0
            a = _snap(core)
            if k == 1:
                _verify(core, b, a, [0], ftw, {}, f'spedersac feature step S={S} A={A} B={B} RLREP_DISABLE={form!r}')
        outs.append(a)
        launches.append(n)
        del agent, core
    assert launches[0] == launches[1] - 1, ('no finishing launch in the folded form', launches)
    _unchanged(outs[1], outs[0], 'fold_dwfin on / off', ARENAS)


@pytest.mark.parametrize('alg', ALGS)
def test_benchmarked_mode_steps_every_group_once_per_train(alg):
    """train() as bench.py runs it: graph replay, device draws, the two pipelined chains where the agent has them (vlsac: the snapshot folded
    into the feature group's launch, the riders), extra_feature_steps = 0 so that every group steps once per call.  One call captures the
    graphs; the next two are checked, with a flush() before every read."""
    c = Case(alg + '_tiny')
    extra = dict(graph=True, seed=1234)
    if alg != 'sac':
        extra['extra_feature_steps'] = 0
    pipelined = alg in ('vlsac', 'ctrlsac', 'spedersac')
    if pipelined:
        extra['pipeline'] = True
    agent = _agent(c, **extra)
    core = agent.core
    buf = make_buffer(c)
    agent.train(buf, c.B)
    agent.flush()
    stepping = FEATURE_GROUPS[alg] + CRITIC_GROUPS[alg] + [2]
    twins = {1: R.twin_map(core.descs, ('critic',))}
    if FEATURE_TWINS[alg]:
        twins[0] = R.twin_map(core.descs, FEATURE_TWINS[alg])
    frozen = []
    if alg == 'ctrlsac':         # train() ends its feature steps with frozen_phi, frozen_phi_target <- phi (quirk Q8)
        for name, (arena, _g, off, rows, cols) in core.descs.items():
            if name.startswith('phi.'):
                for dst in ('frozen_phi', 'frozen_phi_target'):
                    frozen.append((off, core.descs[dst + name[3:]][2], rows * cols))
    moved = []
    for call in range(2):
        b = _snap(core)
        agent.train(buf, c.B)
        agent.flush()
        a = _snap(core)
        if pipelined:
            assert agent._pipe is not None, f'{alg} must take the pipelined path'
        assert a['counter'] == b['counter'] + 1
        is_open = a['counter'] % agent.target_update_period == 0
        moved.append(is_open)
        bb, aa = b, a
        if frozen:               # checked here, then taken out of the comparison of untouched targets
            aa = dict(a)
            aa['targets'] = a['targets'].copy()
            for po, to, n in frozen:
                assert np.array_equal(a['targets'][to:to + n].view(np.uint32), a['params'][po:po + n].view(np.uint32)), 'frozen copy != phi'
                aa['targets'][to:to + n] = b['targets'][to:to + n]
        _verify(core, bb, aa, stepping, twins, {1: is_open}, f'{alg} train() call {call}, counter {a["counter"]} (critic target {"moves" if is_open else "rests"})')
        _check_alpha(b, a, f'{alg} train() call {call}')
    assert sorted(moved) == [False, True]


# ---- (c) planted values through the split entry points ---------------------------------------------------------------------------------------
def _plant(core, g, twins, vals):
    """Overwrite group g's slices of params / grads / moments (and the twins' targets) with planted values.  The alignment padding between
    tensors stays zero, as it always is: the critic group's Polyak runs over the whole slice, padding included, and must find 0 -> 0 there."""
    L = core.layout
    off, n = L.group_offset[g], L.group_floats[g]
    used = R.mask_of(L.param_floats, [(o, r * c) for (arena, grp, o, r, c) in core.descs.values() if arena == 0 and grp == g])[off:off + n]
    assert used.any() and not used.all(), 'the slice is expected to hold tensors and some padding'
    p, gr, m, v, t = (torch.as_tensor(np.where(used, x[:n], np.float32(0))).cuda() for x in vals)
    core.params[off:off + n] = p
    core.grads[off:off + n] = gr
    core.exp_avg[off:off + n] = m
    core.exp_avg_sq[off:off + n] = v
    for po, to, cnt in twins:
        core.targets[to:to + cnt] = t[po - off:po - off + cnt]


@pytest.mark.parametrize('p_zero', [True, False], ids=['p0_zero', 'p0_random'])
@pytest.mark.parametrize('which', ['sac_critic', 'sac_actor', 'sac_h40_critic', 'ctrlsac_feature'])
def test_planted_values_through_backward_then_apply(which, p_zero):
    """The CPU test's wide-range values (|g|, |m| in [1e-12, 1e4], v in {0} u [1e-20, 1e6], exact zeros separately and together; p0 = 0 everywhere
    in one run, so that the update itself is the output) planted between *_backward -- whose loss kernel bumps the record from the step - 1
    written before it and derives the scalars -- and *_apply; steps 1, 2, 1000, 100000.  These groups have no slabs and no skip ranges.
    sac_h40: hidden_dim 40, a critic group of several optimizer blocks with a partly filled last one (the tiny groups fit one block)."""
    alg, _, grp = which.rpartition('_')
    g = {'critic': 1, 'actor': 2, 'feature': 0}[grp]
    if alg == 'sac_h40':
        from oracle.shapes import param_shapes
        c = Case('sac_tiny')
        c.kw = dict(c.kw, hidden_dim=40)
        c.init = synth.init_like(param_shapes('sac', c.S, c.A, **c.kw), seed=99)
        for k in list(c.init):
            if k.startswith('critic.'):
                c.init['critic_target' + k[6:]] = c.init[k].copy()
        c.init['log_alpha'] = np.log(np.float64(0.1))
    else:
        c = Case(alg + '_tiny')
    agent = _agent(c)
    core = agent.core
    buf = make_buffer(c)
    buf.flush()
    rs = np.random.RandomState(21)
    eps = torch.as_tensor(rs.standard_normal((c.B, c.A)).astype(np.float32), device='cuda')
    agent._set_batch(buf.gather(torch.as_tensor(rs.randint(0, buf.size, size=c.B), device='cuda')))
    n = core.layout.group_floats[g]
    if alg == 'sac_h40':
        assert n > 2048 and n % 1024 != 0
    twins = R.twin_map(core.descs, {'critic': ('critic',), 'actor': (), 'feature': ('phi',)}[grp])
    alpha0 = core.alpha_state.clone()
    worst = dict.fromkeys(R.QUANTITIES, 0.0)
    gates = set()
    for step in (1, 2, 1000, 100000):
        core.load_state(c.init)                     # the backward below runs on sane parameters whatever the last planting left
        core.alpha_state.copy_(alpha0)
        core.group_cfg().view(torch.int32)[g, 0] = step - 1
        vals = R.wide_range(n, 4000 + step % 991, p_zero)
        if grp == 'critic':          # inside a bracket: the critic group's launch carries the (gated) Polyak
            core.begin_train()
            core.critic_backward(eps)
        elif grp == 'actor':
            core.actor_backward(eps)
        else:
            core.feature_backward(None)
        _plant(core, g, twins, vals)
        b = _snap(core)
        assert _step_of(b, g) == step, 'the loss kernel of the backward bumps the record'
        b['cfg'][g, :1].view(np.int32)[0] = step - 1          # _verify counts the step from the record before the backward
        if grp == 'critic':
            core.critic_apply()
        elif grp == 'actor':
            core.actor_apply()
        else:
            core.feature_apply()
        if grp == 'critic':
            core.update_target()
        a = _snap(core)
        is_open = a['counter'] % agent.target_update_period == 0 if grp == 'critic' else True
        gates.add(is_open)
        w = _verify(core, b, a, [g], {g: twins} if twins else {}, {g: is_open}, f'{which} planted, step {step}, p0 {"zero" if p_zero else "random"}')
        for q in w:
            worst[q] = max(worst[q], w[q])
        assert R.record(a['cfg'][g])[0] == step
    assert gates == ({True, False} if grp == 'critic' else {True})          # the critic target's gate was met open and closed
    print(f'{which} planted p0 {"zero" if p_zero else "random"}: worst over steps  ' + '  '.join(f'{q} {worst[q]:.3f}' for q in R.QUANTITIES))
