"""What n-step critic targets cost: train()/s of the four representation agents with a plain ring and with critic_n_step = 3
and 5, sac's n_step beside them, the target gather alone beside the full n-step gather, and the plain-buffer rate against another checkout.
Writes profiles/nstep_critic.txt (and prints it).

    python tools/nstep_critic_rate.py                            # every table of this tree
    python tools/nstep_critic_rate.py --parent DIR               # ... and the plain-buffer rate of another checkout (built), alternated with this one

parent:   vlsac_halfcheetah_f256_b256 and ctrlsac_halfcheetah_f256_b256 (bench.py's dimensions), the default train() on a plain 65 536-row
          ring, in child processes (one at a time) that import the package of --parent DIR and of this tree in turn: the same graphs with the
          same launch counts, so the two must agree within the spread between the processes.
train:    the agents' bench.py workloads on a ring of 65 536 rows of synthetic trajectories (episodes of 200 steps): a plain ReplayBuffer
          against critic_n_step = 3 and 5 (sac: n_step), one agent per arm, all arms of a workload in ONE process, alternated.
gather:   rlrep_replay_gather_nstep_targets and rlrep_replay_gather_nstep alone at S = 17 and 376 (B = 256; n = 1, 3, 5): a hipGraph of
          --chain launches of the one kernel on one stream, host clock around a replay and a synchronise, per launch.

Every figure: --warmup calls, then the median (and the sorted values) of --windows windows of --calls calls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nstep_rate import _chain, _fmt, _rate, _setup, _Space, _trajectory_rows, _windows  # noqa: E402

# bench.py's workloads of the five agents: (agent, S, A, B, constructor keywords)
WORKLOADS = {
    'vlsac_halfcheetah_f256_b256': ('vlsac', 17, 6, 256, dict(hidden_dim=256, feature_dim=256, extra_feature_steps=3)),
    'ctrlsac_halfcheetah_f256_b256': ('ctrlsac', 17, 6, 256, dict(hidden_dim=256, feature_dim=256, extra_feature_steps=3)),
    'spedersac_ant_f512_b1024': ('spedersac', 111, 8, 1024, dict(
        phi_and_mu_lr=1e-5, phi_hidden_dim=512, phi_hidden_depth=1, mu_hidden_dim=512, mu_hidden_depth=0,
        critic_and_actor_lr=3e-4, critic_and_actor_hidden_dim=256, feature_dim=512, hidden_dim=256, extra_feature_steps=5)),
    'diffsrsac_halfcheetah_b256': ('diffsrsac', 17, 6, 256, dict(hidden_dim=256, extra_feature_steps=3)),
    'sac_halfcheetah_b256': ('sac', 17, 6, 256, dict(hidden_dim=256)),
}
PARENT_WORKLOADS = ('vlsac_halfcheetah_f256_b256', 'ctrlsac_halfcheetah_f256_b256')
RING = 65536
NS = (3, 5)


def _agent(np, torch, wl):
    import importlib
    alg, S, A, B, kw = WORKLOADS[wl]
    name = {'sac': 'SACAgent', 'vlsac': 'VLSACAgent', 'ctrlsac': 'CTRLSACAgent', 'spedersac': 'SPEDERSACAgent', 'diffsrsac': 'DIFFSRSACAgent'}[alg]
    torch.manual_seed(0)
    return getattr(importlib.import_module(f'rlrep_amd.agent.{alg}.{alg}_agent'), name)(S, A, _Space(np, A), max_batch=B, seed=0, **kw)


def _launches(agent):
    """kernels of the library in one captured train(): (feature chain, critic / actor chain) of the two-chain form, or the one graph's"""
    return agent._pipe['launches'] if getattr(agent, '_pipe', None) else agent._graph_launches


def plain_rates(args, root):
    """{workload: sorted us per train() of each window} with a plain ring, importing the package under `root` (a child process's job)"""
    np, torch = _setup(root)
    from rlrep_amd.utils.buffer import ReplayBuffer
    out = {}
    for wl in PARENT_WORKLOADS:
        _, S, A, B, _ = WORKLOADS[wl]
        agent, buf = _agent(np, torch, wl), ReplayBuffer(S, A, max_size=RING)
        buf.load(*_trajectory_rows(np, S, A, RING, 1))
        out[wl] = _windows(torch, {'plain': lambda: agent.train(buf, B)}, args.warmup, args.calls, args.windows)['plain']
        agent.flush()
        out[wl + '/launches'] = str(_launches(agent))
    return out


def parent_table(args, say):
    rows = {}
    for rep in range(args.repeats):
        for name, root in (('parent', os.path.abspath(args.parent)), ('this', ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', root, '--warmup', str(args.warmup), '--calls', str(args.calls), '--windows', str(args.windows)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=600)
            rows.setdefault(name, []).append(json.loads(res.stdout.strip().splitlines()[-1]))
    for wl in PARENT_WORKLOADS:
        for name in ('parent', 'this'):
            meds = [_rate(r[wl]) for r in rows[name]]
            say(f'{wl} plain ring {RING} [{name:6s}] launches {rows[name][0][wl + "/launches"]}: {statistics.median(meds):9.0f} train()/s, process medians '
                f'{", ".join(f"{m:.0f}" for m in meds)} (spread {100 * (max(meds) - min(meds)) / statistics.median(meds):.1f} %)')
        a, b = statistics.median([_rate(r[wl]) for r in rows['this']]), statistics.median([_rate(r[wl]) for r in rows['parent']])
        say(f'{wl}: this tree / parent = {a / b:.3f}')


def train_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import ReplayBuffer
    for wl, (alg, S, A, B, _) in WORKLOADS.items():
        key = 'n_step' if alg == 'sac' else 'critic_n_step'
        rows = _trajectory_rows(np, S, A, RING, 1)
        arms, agents = {}, {}
        for n in (1,) + NS:
            agent, buf = _agent(np, torch, wl), ReplayBuffer(S, A, max_size=RING, **{key: n})
            buf.load(*rows)
            agents[n] = agent
            arms[n] = lambda agent=agent, buf=buf: agent.train(buf, B)
        us = _windows(torch, arms, args.warmup, args.calls, args.windows)
        for a in agents.values():
            a.flush()
        p = us[1]
        say(f'{wl} ring {RING} plain (launches {_launches(agents[1])}): {_fmt(p)} per train() = {_rate(p):8.0f} train()/s')
        for n in NS:
            q = us[n]
            say(f'{wl} ring {RING} {key} = {n} (launches {_launches(agents[n])}): {_fmt(q)} per train() = {_rate(q):8.0f} train()/s; '
                f'{_rate(q) / _rate(p):.3f} x plain, +{statistics.median(q) - statistics.median(p):.2f} us per train()')
        del arms, agents


def gather_table(args, say, B=256, A=6):
    import ctypes as C
    np, torch = _setup(ROOT)
    from rlrep_amd._lib import lib, check
    from rlrep_amd.utils.buffer import ReplayBuffer
    K = args.chain
    for S in (17, 376):
        buf = ReplayBuffer(S, A, max_size=RING)
        buf.load(*_trajectory_rows(np, S, A, RING, 2))
        size_dev = buf.size_dev()
        idx = torch.from_numpy(np.random.default_rng(3).integers(0, RING, size=B).astype(np.int32)).cuda()
        xe = torch.empty(B, 2 * S + A, device='cuda')
        xf, xf2, xfpi = (torch.zeros(B, S + A, device='cuda') for _ in range(3))
        r, d = torch.empty(B, device='cuda'), torch.empty(B, device='cuda')
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

        def targets(n):
            check(lib.rlrep_replay_gather_nstep_targets(ptr(buf.ring), ptr(idx), B, S, A, RING, ptr(size_dev), n, 1, 0.99, ptr(xf2), ptr(r), ptr(d), stream()),
                  'replay_gather_nstep_targets')

        def full(n):
            check(lib.rlrep_replay_gather_nstep(ptr(buf.ring), ptr(idx), B, S, A, RING, ptr(size_dev), n, 1, 0.99, ptr(xe), ptr(xf), ptr(xf2), ptr(xfpi), ptr(r),
                                                ptr(d), stream()), 'replay_gather_nstep')
        arms = {}
        for n in (1,) + NS:
            arms[f'targets n = {n}'] = _chain(torch, lambda n=n: targets(n), K)
            arms[f'full    n = {n}'] = _chain(torch, lambda n=n: full(n), K)
        us = _windows(torch, arms, max(1, args.warmup // K), max(1, args.calls // K), args.windows)
        for k, v in us.items():
            say(f'gather S = {S:3d} A = {A} B = {B} ring {RING} {k}: {_fmt([u / K for u in v])} per launch (chain of {K})')


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='train,gather')
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain-buffer train()/s is measured beside this tree\'s')
    p.add_argument('--child', default=None, help=argparse.SUPPRESS)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nstep_critic.txt'))
    p.add_argument('--warmup', type=int, default=200)
    p.add_argument('--calls', type=int, default=1000)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--chain', type=int, default=64)
    args = p.parse_args(argv)
    if args.child:
        print(json.dumps(plain_rates(args, args.child)))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.parent:                      # (children first: this process has not opened the GPU yet)
        say(f'# plain-buffer train()/s, child processes alternated ({args.repeats} each): {args.warmup} warm-up calls, median of {args.windows} windows of {args.calls} calls')
        parent_table(args, say)
    np, torch = _setup(ROOT)
    say(f'# {torch.cuda.get_device_name(0)}; {args.warmup} warm-up calls per arm, median (sorted windows) of {args.windows} windows of {args.calls} calls, '
        'arms alternated in one process')
    only = args.only.split(',')
    if 'train' in only:
        train_table(args, say)
    if 'gather' in only:
        gather_table(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
