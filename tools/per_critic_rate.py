"""What prioritized replay of the critic's minibatch costs: the plain-buffer rate against another checkout, train()/s of the
four representation agents with a plain ring and with a CriticPrioritizedReplayBuffer, and the fused sample-and-gather launch beside the two
launches it replaces.  Writes profiles/per_critic.txt (and prints it).

    python tools/per_critic_rate.py                            # every table of this tree
    python tools/per_critic_rate.py --parent DIR               # ... and the plain-buffer rate of another checkout (built), alternated with this one

parent:   tools/nstep_critic_rate.py's table: vlsac_halfcheetah_f256_b256 and ctrlsac_halfcheetah_f256_b256, the default train() on a plain
          65 536-row ring, in child processes (one at a time) that import the package of --parent DIR and of this tree in turn.  The same
          graphs with the same launch counts: the two must agree within the spread between the processes.
train:    the agents' bench.py workloads on a ring of 65 536 rows, three arms in ONE process, alternated: a plain ReplayBuffer in the default
          two-chain form, a plain ReplayBuffer in the one-graph form (pipeline=False), a CriticPrioritizedReplayBuffer (always the one-graph
          form).  The second against the third is what the feature costs; the first shows what the missing two-chain form costs.
fused:    rlrep_per_sample_fill against rlrep_per_sample followed by rlrep_replay_sample on the same stream, each as a hipGraph of --chain
          repetitions, at (S, A) = (17, 6) and (376, 17), B = 256 and 1024, rings of 65 536 and 10^6 rows; per repetition.

Every figure: --warmup calls, then the median (and the sorted values) of --windows windows of --calls calls.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from nstep_critic_rate import WORKLOADS, _launches, parent_table  # noqa: E402
from nstep_rate import _chain, _fmt, _rate, _setup, _Space, _trajectory_rows, _windows  # noqa: E402

RING = 65536
PER_STREAM = 3 << 40


def _agent(np, torch, wl, **extra):
    import importlib
    alg, S, A, B, kw = WORKLOADS[wl]
    name = {'sac': 'SACAgent', 'vlsac': 'VLSACAgent', 'ctrlsac': 'CTRLSACAgent', 'spedersac': 'SPEDERSACAgent', 'diffsrsac': 'DIFFSRSACAgent'}[alg]
    torch.manual_seed(0)
    return getattr(importlib.import_module(f'rlrep_amd.agent.{alg}.{alg}_agent'), name)(S, A, _Space(np, A), max_batch=B, seed=0, **kw, **extra)


def train_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer, ReplayBuffer
    for wl, (alg, S, A, B, _) in WORKLOADS.items():
        if alg == 'sac':
            continue
        rows = _trajectory_rows(np, S, A, RING, 1)
        arms, agents = {}, {}
        for arm, cls, extra in (('plain, two chains', ReplayBuffer, {}), ('plain, one graph', ReplayBuffer, dict(pipeline=False)),
                                ('prioritized critic', CriticPrioritizedReplayBuffer, dict(pipeline=False))):
            agent, buf = _agent(np, torch, wl, **extra), cls(S, A, max_size=RING)
            buf.load(*rows)
            agents[arm] = agent
            arms[arm] = lambda agent=agent, buf=buf: agent.train(buf, B)
        us = _windows(torch, arms, args.warmup, args.calls, args.windows)
        for a in agents.values():
            a.flush()
        one = us['plain, one graph']
        for arm, v in us.items():
            tail = '' if arm == 'plain, one graph' else (f'; {_rate(v) / _rate(one):.3f} x the plain one-graph form, '
                                                         f'{statistics.median(v) - statistics.median(one):+.2f} us per train()')
            say(f'{wl} ring {RING} {arm} (launches {_launches(agents[arm])}): {_fmt(v)} per train() = '
                f'{_rate(v):8.0f} train()/s{tail}')
        del arms, agents


def fused_table(args, say):
    np, torch = _setup(ROOT)
    from rlrep_amd._lib import lib, check
    from rlrep_amd.agent.sac.sac_agent import SACAgent
    from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
    from rlrep_amd.utils.buffer import CriticPrioritizedReplayBuffer
    K = args.chain
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    for S, A in ((17, 6), (376, 17)):
        for ring in (RING, 10 ** 6):
            buf = CriticPrioritizedReplayBuffer(S, A, max_size=ring)
            buf.ring.normal_()                                   # (rows of noise, written on the device: the launches only copy them)
            buf.size, buf.ptr = ring, 0
            buf.set_priorities((1.0 + 99.0 * np.random.default_rng(5).random(ring)).astype(np.float32), 100.0)
            for B in (256, 1024):
                torch.manual_seed(0)
                v = VLSACAgent(S, A, _Space(np, A), max_batch=B, seed=0, graph=False, hidden_dim=64, feature_dim=64, extra_feature_steps=0)
                sac = SACAgent(S, A, _Space(np, A), max_batch=B, seed=0, graph=False, hidden_dim=64)
                idx, w, _ = buf.draw_buffers(B)
                buf.draw_fill(v.core, B, 1, PER_STREAM)          # (sizes the slot for B outside the captures)
                counter = C.c_void_p(lib.rlrep_steps_dev(v.core.h))

                def fused():
                    check(lib.rlrep_per_sample_fill(v.core.h, ptr(buf.ring), ring, ptr(buf.tree), buf.P, ptr(buf._scal), ptr(idx), ptr(w), B, 0, 1, PER_STREAM,
                                                    counter, stream()), 'per_sample_fill')

                def pair():
                    check(lib.rlrep_per_sample(sac.core.h, ptr(buf.tree), buf.P, ptr(buf._scal), ptr(idx), ptr(w), B, 0, 1, PER_STREAM, counter, stream()), 'per_sample')
                    check(lib.rlrep_replay_sample(v.core.h, 0, ptr(buf.ring), ptr(idx), B, stream()), 'replay_sample')
                arms = {'fused launch': _chain(torch, fused, K), 'sample + gather': _chain(torch, pair, K)}
                us = _windows(torch, arms, max(1, args.warmup // K), max(1, args.calls // K), args.windows)
                f, p = [u / K for u in us['fused launch']], [u / K for u in us['sample + gather']]
                say(f'fused (S, A) = ({S}, {A}) B = {B} ring {ring}: fused launch {_fmt(f)}, sample + gather {_fmt(p)} per repetition (chains of {K}); '
                    f'fused / pair = {statistics.median(f) / statistics.median(p):.3f}')
                del arms, v, sac
            del buf


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--only', default='train,fused')
    p.add_argument('--parent', default=None, help='a built checkout of the parent commit: its plain-buffer train()/s is measured beside this tree\'s')
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'per_critic.txt'))
    p.add_argument('--warmup', type=int, default=200)
    p.add_argument('--calls', type=int, default=1000)
    p.add_argument('--windows', type=int, default=5)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--chain', type=int, default=64)
    args = p.parse_args(argv)
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
    if 'fused' in only:
        fused_table(args, say)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
