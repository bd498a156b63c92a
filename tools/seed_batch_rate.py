"""Aggregate train() rate of a seed batch against R standalone agents replayed back to back on one stream.

    python tools/seed_batch_rate.py --workload sac_pendulum_b64 --members 1,2,4,8,16
    python tools/seed_batch_rate.py --workload ctrlsac_halfcheetah_f2048_b256 --members 1,2,4,8

sac workloads: SACSeedBatch against SACAgent; ctrlsac workloads: CTRLSACSeedBatch against CTRLSACAgent(pipeline=False), the one-graph
train() a ctrlsac group runs (the pipelined two-chain form is not built for groups).

--sweep: the group is a hyper-parameter sweep (member r: seed r // 4, lr / tau / discount (ctrlsac: feature_tau) of configuration r % 4,
SeedBatchMixin member_hyper), measured against a seed-only group of the same R and against R standalone agents built with each member's seed
and hyper-parameters.

--clone: population-based training's exploit step at R = 8, 2 pairs (--workload is ignored: sac HalfCheetah, ctrlsac F = 256 and F = 2048).
Time per SeedBatchMixin.clone_members call (one launch), the bytes it moves and GB/s, against the same effect done on the device without it:
per pair five `copy_` between the members' arena views, then the device records with the destination's hyper words saved and restored
(what SeedBatchMixin.load() does from the host).  Device events around 100 calls after 10 warm-up calls, the two forms alternated, median of
--windows windows.  The clone must not be the slower one at any shape (exit status 1 otherwise).

--retire 0,4,6,7: successive halving at R = 8.  For every K the group with its last K members retired (SeedBatchMixin.retire_members: grid y
stays 8, the retired members' workgroups return at once) against a FRESH group built with only the R' = 8 - K live members, in the same process:
arms alternated, --repeats repeats (at least 3) per arm of --calls calls after --warmup calls, microseconds per train() as median and min .. max.
Retiring must make a train() faster than with all members live for every K > 0 (exit status 1 otherwise); the ratio to the fresh group is what
the empty workgroups cost.

Per R: the group's aggregate rate (R x calls/s), its graph's launch count per call, and the standalone agents' aggregate rate.  Protocol:
--warmup calls (default 300), then the median of --windows windows (default 5) of --calls calls (default 500), timed by host wall clock
around a device synchronisation."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _rate(step, R, warmup, calls, windows):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    rates = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            step()
        torch.cuda.synchronize()
        rates.append(R * calls / (time.perf_counter() - t0))
    return statistics.median(rates)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--workload', default='sac_halfcheetah_b256', choices=['sac_pendulum_b64', 'sac_halfcheetah_b256', 'ctrlsac_halfcheetah_f256_b256',
                                                                          'ctrlsac_halfcheetah_f2048_b256'])
    p.add_argument('--members', default='1,2,4,8,16')
    p.add_argument('--warmup', type=int, default=300)
    p.add_argument('--calls', type=int, default=500)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--group-only', action='store_true', help='skip the standalone agents (a profiler run of the group alone)')
    p.add_argument('--sweep', action='store_true', help='a hyper-parameter sweep group against a seed-only group and R standalone agents')
    p.add_argument('--clone', action='store_true', help='time clone_members against per-arena copy_ calls (R = 8, 2 pairs, three shapes)')
    p.add_argument('--retire', default=None, help='comma-separated numbers of retired members (R = 8): the group against fresh groups of the live members only')
    p.add_argument('--repeats', type=int, default=3, help='--retire: repeats per arm (at least 3)')
    a = p.parse_args(argv)
    if a.retire is not None:
        return retire_main(a)
    if a.clone:
        return clone_main(a)
    if a.sweep:
        return sweep_main(a)
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    alg, S, A, B, kw = bench.WORKLOADS[a.workload]
    alone_kw = {}
    if alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent as Agent
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch as Group
        alone_kw = dict(pipeline=False)
    else:
        from rlrep_amd.agent.sac.sac_agent import SACAgent as Agent
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch as Group
    print(f'# {a.workload}: S={S} A={A} B={B} {kw}; {Group.__name__} against {Agent.__name__}({alone_kw}); {torch.cuda.get_device_name(0)}; '
          f'warmup {a.warmup}, median of {a.windows} x {a.calls} calls')
    print(f'{"R":>3} {"group train()/s":>16} {"launches/call":>14} {"R standalone train()/s":>23} {"ratio":>6}')
    for R in [int(x) for x in a.members.split(',')]:
        seeds = list(range(R))
        rings = ReplayBufferGroup(R, S, A, max_size=bench.REPLAY_N)
        alone_bufs = []
        for r in range(R):
            buf, data = bench.synth_buffer(S, A, r)
            rings.load(r, data['state'], data['action'], data['next_state'], data['reward'], data['done'])
            alone_bufs.append(buf)
        grp = Group(seeds, S, A, bench.Space(A), max_batch=B, **kw)
        g_rate = _rate(lambda: grp.train(rings, B), R, a.warmup, a.calls, a.windows)
        launches = grp._graph_launches
        if a.group_only:
            print(f'{R:>3} {g_rate:>16.0f} {launches:>14d}', flush=True)
            continue
        agents = []
        for s in seeds:
            torch.manual_seed(s)
            agents.append(Agent(S, A, bench.Space(A), max_batch=B, seed=s, **alone_kw, **kw))

        def alone_step():
            for ag, buf in zip(agents, alone_bufs):
                ag.train(buf, B)
        s_rate = _rate(alone_step, R, a.warmup, a.calls, a.windows)
        print(f'{R:>3} {g_rate:>16.0f} {launches:>14d} {s_rate:>23.0f} {g_rate / s_rate:>6.2f}', flush=True)
        del grp, agents, rings, alone_bufs
        torch.cuda.empty_cache()


def _sweep_members(alg, R):
    """R (seed, member_hyper) pairs: four configurations x seeds (seed r // 4 ... every configuration once per seed), all distinct"""
    cfgs = [dict(lr=1e-4, tau=0.005), dict(lr=3e-4, tau=0.01, discount=0.98), dict(lr=2e-4, tau=0.02, target_update_period=1),
            dict(lr=5e-5, discount=0.95, target_update_period=3)]
    if alg == 'ctrlsac':
        for q, c in enumerate(cfgs):
            c['feature_tau'] = 0.005 * (q + 1)
    return [(r // len(cfgs), dict(cfgs[r % len(cfgs)])) for r in range(R)]


def sweep_main(a):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    alg, S, A, B, kw = bench.WORKLOADS[a.workload]
    alone_kw = {}
    if alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent as Agent
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch as Group
        alone_kw = dict(pipeline=False)
    else:
        from rlrep_amd.agent.sac.sac_agent import SACAgent as Agent
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch as Group
    print(f'# {a.workload}: S={S} A={A} B={B} {kw}; sweep {Group.__name__} against a seed-only group and {Agent.__name__}({alone_kw}); '
          f'{torch.cuda.get_device_name(0)}; warmup {a.warmup}, median of {a.windows} x {a.calls} calls')
    print(f'{"R":>3} {"sweep train()/s":>16} {"seeds train()/s":>16} {"sweep/seeds":>12} {"launches/call":>14} {"R standalone train()/s":>23} {"sweep/alone":>12}')
    for R in [int(x) for x in a.members.split(',')]:
        members = _sweep_members(alg, R)
        rings = ReplayBufferGroup(R, S, A, max_size=bench.REPLAY_N)
        alone_bufs = []
        for r in range(R):
            buf, data = bench.synth_buffer(S, A, r)
            rings.load(r, data['state'], data['action'], data['next_state'], data['reward'], data['done'])
            alone_bufs.append(buf)
        sweep = Group([s for s, _ in members], S, A, bench.Space(A), max_batch=B, member_hyper=[h for _, h in members], **kw)
        w_rate = _rate(lambda: sweep.train(rings, B), R, a.warmup, a.calls, a.windows)
        launches = sweep._graph_launches
        del sweep
        seeds = Group(list(range(R)), S, A, bench.Space(A), max_batch=B, **kw)
        s_rate = _rate(lambda: seeds.train(rings, B), R, a.warmup, a.calls, a.windows)
        assert seeds._graph_launches == launches
        del seeds
        if a.group_only:
            print(f'{R:>3} {w_rate:>16.0f} {s_rate:>16.0f} {w_rate / s_rate:>12.3f} {launches:>14d}', flush=True)
            continue
        agents = []
        for s, h in members:
            torch.manual_seed(s)
            agents.append(Agent(S, A, bench.Space(A), max_batch=B, seed=s, **alone_kw, **kw, **h))

        def alone_step():
            for ag, buf in zip(agents, alone_bufs):
                ag.train(buf, B)
        a_rate = _rate(alone_step, R, a.warmup, a.calls, a.windows)
        print(f'{R:>3} {w_rate:>16.0f} {s_rate:>16.0f} {w_rate / s_rate:>12.3f} {launches:>14d} {a_rate:>23.0f} {w_rate / a_rate:>12.2f}', flush=True)
        del agents, rings, alone_bufs
        torch.cuda.empty_cache()


def _us_per_call(step, warmup, calls):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def retire_main(a):
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup
    R = 8
    ks = [int(x) for x in a.retire.split(',')]
    if not ks or any(not 0 <= k < R for k in ks) or a.repeats < 3:
        print(f'--retire: give numbers in [0, {R}) and --repeats >= 3')
        return 2
    alg, S, A, B, kw = bench.WORKLOADS[a.workload]
    if alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch as Group
    else:
        from rlrep_amd.agent.sac.seed_batch import SACSeedBatch as Group

    def rings_of(n):
        rings = ReplayBufferGroup(n, S, A, max_size=bench.REPLAY_N)
        for r in range(n):
            _, data = bench.synth_buffer(S, A, r)
            rings.load(r, data['state'], data['action'], data['next_state'], data['reward'], data['done'])
        return rings
    print(f'# {a.workload}: S={S} A={A} B={B} {kw}; {Group.__name__} R = {R} with K members retired against a fresh group of the R - K live members; '
          f'{torch.cuda.get_device_name(0)}; us per train(), median (min .. max) of {a.repeats} repeats x {a.calls} calls after {a.warmup} warm-up calls, '
          'arms alternated')
    big, big_rings = Group(list(range(R)), S, A, bench.Space(A), max_batch=B, **kw), rings_of(R)
    fresh = {k: (Group(list(range(R - k)), S, A, bench.Space(A), max_batch=B, **kw), rings_of(R - k)) for k in sorted(set(ks))}
    t_big, t_fresh = {k: [] for k in ks}, {k: [] for k in ks}
    for _ in range(a.repeats):
        for k in ks:
            want = [r < R - k for r in range(R)]
            live = big.live
            back, out = [r for r in range(R) if want[r] and not live[r]], [r for r in range(R) if live[r] and not want[r]]
            if back:
                big.revive_members(back)
            if out:
                big.retire_members(out)
            t_big[k].append(_us_per_call(lambda: big.train(big_rings, B), a.warmup, a.calls))
            g, rg = fresh[k]
            t_fresh[k].append(_us_per_call(lambda: g.train(rg, B), a.warmup, a.calls))
    assert big._graph_launches == fresh[ks[0]][0]._graph_launches
    print(f'{"K":>2} {"live":>4} {"retired group us":>30} {"fresh R - K group us":>30} {"retired/fresh":>14} {"retired/all live":>17}')
    med = {k: statistics.median(t_big[k]) for k in ks}
    all_live = med.get(0)
    slower = []
    for k in ks:
        fm = statistics.median(t_fresh[k])
        b = f'{med[k]:.1f} ({min(t_big[k]):.1f} .. {max(t_big[k]):.1f})'
        f = f'{fm:.1f} ({min(t_fresh[k]):.1f} .. {max(t_fresh[k]):.1f})'
        rel = f'{med[k] / all_live:.3f}' if all_live else ''
        print(f'{k:>2} {R - k:>4} {b:>30} {f:>30} {med[k] / fm:>14.3f} {rel:>17}', flush=True)
        if all_live and k > 0 and not med[k] < all_live:
            slower.append(k)
    if slower:
        print(f'# FAILED: with {slower} members retired a train() is not faster than with all {R} live')
        return 1
    return 0


HBM_MEASURED_TBS = 6.29          # measured HBM rate of a float4 copy on the MI355X


def _event_ms(step, warmup, calls):
    for _ in range(warmup):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def clone_main(a):
    R, pairs, warmup, calls = 8, [(0, 4), (1, 5)], 10, 100
    print(f'# clone_members against per-arena copy_ calls; R = {R}, pairs {pairs}; {torch.cuda.get_device_name(0)}; device events around {calls} calls '
          f'after {warmup} warm-up calls, forms alternated, median of {a.windows} windows')
    print(f'{"workload":<32} {"MB moved/call":>14} {"clone us":>9} {"clone GB/s":>11} {"copy_ us":>9} {"copy_ GB/s":>11} {"copy_/clone":>12} {"of 6.29 TB/s":>13}')
    slower = []
    for wl in ('sac_halfcheetah_b256', 'ctrlsac_halfcheetah_f256_b256', 'ctrlsac_halfcheetah_f2048_b256'):
        alg, S, A, B, kw = bench.WORKLOADS[wl]
        if alg == 'ctrlsac':
            from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch as Group
        else:
            from rlrep_amd.agent.sac.seed_batch import SACSeedBatch as Group
        members = _sweep_members(alg, R)
        grp = Group([s for s, _ in members], S, A, bench.Space(A), max_batch=B, member_hyper=[h for _, h in members], **kw)
        m = grp._members
        arenas = ('params', 'targets', 'exp_avg', 'exp_avg_sq', 'alpha_state')
        # read + write bytes of one call: the four arenas, alpha_state and the device records but for 4 x 5 hyper words, per pair
        one = sum(getattr(m[0], k).numel() * getattr(m[0], k).element_size() for k in arenas) + m[0].device_state().numel() - 4 * 5 * 4
        moved = 2 * one * len(pairs)

        def by_copies():
            for s, d in pairs:
                for k in arenas:
                    getattr(m[d], k).copy_(getattr(m[s], k))
                hyper = m[d].group_cfg()[:, 1:6].clone()
                m[d].device_state().copy_(m[s].device_state())
                m[d].group_cfg()[:, 1:6].copy_(hyper)

        def by_clone():
            grp.clone_members(pairs)
        t_clone, t_copy = [], []
        for _ in range(a.windows):
            t_clone.append(_event_ms(by_clone, warmup, calls))
            t_copy.append(_event_ms(by_copies, warmup, calls))
        c, p_ = statistics.median(t_clone), statistics.median(t_copy)
        share = f'{moved / (c * 1e-3) / (HBM_MEASURED_TBS * 1e12):>12.1%}' if wl.endswith('f2048_b256') else f'{"":>12}'
        print(f'{wl:<32} {moved / 1e6:>14.3f} {c * 1e3:>9.1f} {moved / (c * 1e-3) / 1e9:>11.1f} {p_ * 1e3:>9.1f} {moved / (p_ * 1e-3) / 1e9:>11.1f} '
              f'{p_ / c:>12.2f} {share}', flush=True)
        if c > p_:
            slower.append(wl)
        del grp, m
        torch.cuda.empty_cache()
    if slower:
        print(f'# FAILED: clone_members is slower than the copy_ calls at {", ".join(slower)}')
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
