"""Launcher with the reference's command-line surface (main.py:22-39) driving the MI355X agents.

    python -m rlrep_amd.main --alg sac --env Pendulum-v1 --max_timesteps 2000 --start_timesteps 500

Same flags, same per-algorithm constructor overrides (main.py:81-104), same loop structure (random actions for
`start_timesteps`, then epsilon-greedy 0.01 around `select_action(explore=True)`, one `agent.train()` per
environment step, evaluation every `eval_freq` steps).  Metrics go to `log/<env>/<alg>/<dir>/<seed>/metrics.jsonl`
as {"step": t, "info/<key>": value} lines (and to tensorboardX with the reference's tags if it is installed).

`--seeds 0,1,2,3` (sac and ctrlsac): one SACSeedBatch / CTRLSACSeedBatch trains every seed in the same launches, one environment per seed
stepped in lockstep; each seed has its own np.random.RandomState(seed) for random and epsilon-greedy actions, its own evaluation and its own
log directory.  ctrlsac takes the dimensions build_agent gives it (main.py:90-91).

`--sweep key=v1,v2` (repeatable; with --seeds, or with --seed alone) adds hyper-parameter configurations: the group's members are
product(configurations) x seeds, all trained in the same launches (SeedBatchMixin member_hyper).  A member logs to
`log/<env>/<alg>/<dir>/<tag>/<seed>/metrics.jsonl`, tag = `key=value` joined by `_` (e.g. `lr=0.0001_tau=0.01`).

`--pbt-interval N` (with --seeds / --sweep; N environment steps, a multiple of --eval_freq; 0 = off) turns the group into a population
(population-based training, Jaderberg et al. 2017): at every step t + 1 that is a multiple of N beyond start_timesteps the members are ranked
by their latest evaluation, the bottom `--pbt-fraction` each become a copy of a member drawn from the top fraction (SeedBatchMixin.clone_members,
one launch) and take its hyper-parameters with every `--pbt-keys` entry multiplied by a factor drawn from `--pbt-factors`
(set_member_hyper).  The defaults 0.25 / 0.8,1.2 are the paper's.  Every event is one line of `log/<env>/<alg>/<dir>/pbt.jsonl` (step, src,
dst, scores, old and new values); the members' metrics.jsonl rows are unchanged, and a sweep tag directory keeps naming the member's INITIAL
configuration, whatever PBT has made of it since.

`--halving-interval N` (with --seeds / --sweep; N environment steps, a multiple of --eval_freq; 0 = off) runs successive halving (Jamieson &
Talwalkar 2016) on the group: at every step t + 1 that is a multiple of N beyond start_timesteps the live members are ranked by their latest
evaluation and all but the best `--halving-keep` (default 0.5, rounded up) are retired (SeedBatchMixin.retire_members: their workgroups leave
every launch), never below `--halving-min` live members (default 1).  A retired member's environment is no longer stepped or evaluated and its
metrics.jsonl stops growing; its state stays in the group (and in --save_model checkpoints).  Every halving is one line of
`log/<env>/<alg>/<dir>/halving.jsonl` (step, retired members with their seeds and scores, live count).  Not together with --pbt-interval.

`--device-env` (with --seeds / --sweep and --env Pendulum-v1 or MountainCarContinuous-v0) moves the environments onto the device (rlrep_amd/envs/device.py): acting,
exploring, stepping, the replay-ring row and train() of every live member are one graph replay per step (SeedBatchMixin.iterate) and an
evaluation is one launch (SeedBatchMixin.evaluate); --pbt-interval and --halving-interval rank by those scores.  Exploration and reset draws
come from Philox streams of the members' seeds, so a run differs from the host loop's in its random numbers, not in its algorithm.

`--device-loop` (one agent of any --alg, no --seeds / --sweep, --env Pendulum-v1 or MountainCarContinuous-v0) is the same for a single agent:
`SACAgent.iterate` is one graph replay per step and `SACAgent.evaluate` one launch per evaluation, for sac, vlsac, ctrlsac, spedersac and
diffsrsac alike; --save_model writes the environment's record with the checkpoint.

`--num-envs E` (with --device-env or --device-loop; 1..64, default 1; --start_timesteps and --eval_freq multiples of E) gives every member /
the agent E environments stepped by the same launch: one `iterate` collects E transitions per member and trains once, so the loop counter
advances by E and --max_timesteps stays environment steps per member.  E environments with one update per step is 1/E updates per transition.

`--host-envs E` (1..256, default 1: the loops above, unchanged; --start_timesteps and --eval_freq multiples of E; not with --device-env,
--device-loop, --pbt-interval or --halving-interval) steps E HOST environments per agent / member, seeded seed + i: an iteration is one
`select_actions` launch for all E observations (all R x E with --seeds / --sweep), E `env.step`, one `add_batch` and ONE `train()` -- E
transitions and one update; further updates are the caller's.  Episodes end and reset per environment, and an evaluation steps
min(E, --eval_episodes) environments in lockstep (util.eval_policy_vec).  For environments that live on the host (gym.vector-style
collection on the MuJoCo tasks); --num-envs is the device environments' flag and keeps its meaning.

`--torch-envs N` (1..65536, default 0: the loops above, unchanged; one agent, --env Pendulum-v1; --start_timesteps and --eval_freq multiples
of N) is the loop of a simulator that already lives on the GPU as torch tensors (envs/torch_pendulum.py is the example): an iteration is ONE
`act_device` launch on the device observations, `TorchPendulum.step`, ONE `add_device` launch and ONE `train()` -- no transition crosses the
host.  Warm-up and epsilon-greedy actions are drawn on the device; an evaluation steps min(N, --eval_episodes) environments in lockstep with
`act_device(explore=False)`.

`--sim-graph` (only with --torch-envs N; not with --per) runs that loop as ONE graph replay per iteration (`SACAgent.iterate_sim`,
envs/sim_loop.py): the act launch reads its call counter from a loop record on the device and mixes the exploring uniform actions in itself
(Philox draws of the agent's seed instead of the torch generator's), `TorchPendulum(capturable=True).step_`, the append launch and train()
are captured together.  Evaluations are the eager ones of --torch-envs.

`--fused-sim` (only with --torch-envs N --sim-graph; --env Pendulum-v1 or MountainCarContinuous-v0) makes the simulator of that loop a fused
one (envs/fused_sim.py `FusedSim`, csrc/sim_step.hip): the act launch reads the simulator's observations in place and ONE launch steps the N
environments and appends their transitions, so the graph holds two launches in front of train().  Episodes end and restart per environment
on the device; evaluations step a FusedSim(auto_restart=False) of their own, one act_device and one step launch per step.
With --seeds / --sweep (sac, ctrlsac) all three flags together run the loop for the whole seed group (`SeedBatchMixin.iterate_sim`,
`SimLoopGroup`, `FusedSimGroup`): N environments per member, --start_timesteps counted per member, one graph replay per
iteration for all members, one mean return per member at an evaluation.  Not with --pbt-interval / --halving-interval, --group-per /
--group-critic-per, --device-env, --host-envs, --num-envs or --fused-sim-source.
`--fused-sim-source PATH` (only with all three of --torch-envs N --sim-graph --fused-sim) makes that simulator a kind of your own: PATH holds
the C++ text of one struct (csrc/sim_jit.h; rlrep_amd/envs/kinds/ has two examples), compiled at run time (`CustomFusedSim`, DESIGN.md
6i.2); the agent is built from the kind's S and A, and --env only names the log directory.

`--critic-per` (vlsac, ctrlsac, spedersac, diffsrsac; one agent) trains from a CriticPrioritizedReplayBuffer: the minibatch the critic and actor
steps reuse is drawn from a sum tree on the device, the critic loss is weighted and the |TD| errors come back as priorities (DESIGN.md
6f.1); --per-alpha / --per-beta and the annealing of beta as for --per.  With the plain loop, --host-envs and --torch-envs.

The loops differ in what an iteration is, who draws the exploring action and whether there is an initial evaluation; what they do at an
evaluation step -- anneal beta, take the rate, evaluate, write the row, print, --save_model -- is one copy per side: _Evaluations for one
agent, _GroupEvaluations for a seed group.
"""
import argparse
import functools
import json
import os

import numpy as np
import torch

from rlrep_amd import envs
from rlrep_amd.utils import util, buffer

EPS_GREEDY = 0.01


def build_agent(args, state_dim, action_dim, action_space):
    common = dict(state_dim=state_dim, action_dim=action_dim, action_space=action_space, discount=args.discount,
                  tau=args.tau, hidden_dim=args.hidden_dim, max_batch=args.batch_size)
    if args.alg == 'sac':
        from rlrep_amd.agent.sac.sac_agent import SACAgent
        return SACAgent(**common)
    if args.alg == 'vlsac':
        from rlrep_amd.agent.vlsac.vlsac_agent import VLSACAgent
        return VLSACAgent(**common, extra_feature_steps=args.extra_feature_steps, feature_dim=args.feature_dim)
    if args.alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
        common.update(feature_dim=2048, hidden_dim=1024)                       # hard-coded at main.py:90-91
        return CTRLSACAgent(**common, extra_feature_steps=args.extra_feature_steps)
    if args.alg == 'diffsrsac':
        from rlrep_amd.agent.diffsrsac.diffsrsac_agent import DIFFSRSACAgent
        return DIFFSRSACAgent(**common)
    if args.alg == 'spedersac':
        from rlrep_amd.agent.spedersac.spedersac_agent import SPEDERSACAgent
        return SPEDERSACAgent(**common, extra_feature_steps=5, phi_and_mu_lr=1e-5, phi_hidden_dim=512,
                              phi_hidden_depth=1, mu_hidden_dim=512, mu_hidden_depth=0,
                              critic_and_actor_lr=3e-4, critic_and_actor_hidden_dim=256)   # main.py:95-103
    raise SystemExit(f'--alg {args.alg}: not part of the MI355X hot path (see DESIGN.md, out of scope)')


def run(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--dir', default=0, type=int)
    p.add_argument('--alg', default='diffsrsac')
    p.add_argument('--env', default='HalfCheetah-v4')
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--start_timesteps', default=25e3, type=float)
    p.add_argument('--eval_freq', default=5e3, type=int)
    p.add_argument('--max_timesteps', default=1e6, type=float)
    p.add_argument('--expl_noise', default=0.1)
    p.add_argument('--batch_size', default=256, type=int)
    p.add_argument('--hidden_dim', default=256, type=int)
    p.add_argument('--feature_dim', default=256, type=int)
    p.add_argument('--discount', default=0.99)
    p.add_argument('--tau', default=0.005)
    p.add_argument('--learn_bonus', action='store_true')
    p.add_argument('--save_model', action='store_true')
    p.add_argument('--extra_feature_steps', default=3, type=int)
    p.add_argument('--eval_episodes', default=10, type=int)
    p.add_argument('--log_root', default='log')
    p.add_argument('--seeds', default=None, help='comma-separated seeds trained together (sac and ctrlsac only): rlrep_amd/agent/seed_batch.py')
    p.add_argument('--sweep', action='append', default=None, metavar='KEY=V1,V2',
                   help='hyper-parameter values trained together with the seeds (repeatable; members = product of the sweeps x seeds)')
    p.add_argument('--pbt-interval', default=None, type=int, help='population-based training every N environment steps (a multiple of --eval_freq; 0 = off)')
    p.add_argument('--pbt-fraction', default=None, type=float, help='share of the members replaced at a PBT step, and of those they copy (default 0.25)')
    p.add_argument('--pbt-keys', default=None, help='comma-separated hyper-parameters a copied member perturbs (default lr)')
    p.add_argument('--pbt-factors', default=None, help='comma-separated factors a perturbed value is multiplied by (default 0.8,1.2)')
    p.add_argument('--pbt-seed', default=None, type=int, help='seed of the PBT draws (default 0)')
    p.add_argument('--halving-interval', default=None, type=int, help='successive halving every N environment steps (a multiple of --eval_freq; 0 = off)')
    p.add_argument('--halving-keep', default=None, type=float, help='share of the live members that stay at a halving step, rounded up (default 0.5)')
    p.add_argument('--halving-min', default=None, type=int, help='stop retiring at this many live members (default 1)')
    p.add_argument('--device-env', action='store_true',
                   help='step and score the environments on the device (with --seeds / --sweep and --env Pendulum-v1 or MountainCarContinuous-v0): rlrep_amd/envs/device.py')
    p.add_argument('--device-loop', action='store_true',
                   help='a single agent of any --alg with its environment on the device (--env Pendulum-v1 or MountainCarContinuous-v0): SACAgent.iterate / evaluate')
    p.add_argument('--num-envs', default=1, type=int,
                   help='environments per member / agent on the device, stepped by one launch (with --device-env or --device-loop; 1..64; '
                        '--start_timesteps and --eval_freq multiples of it).  One iterate collects E transitions and trains once: E environments '
                        'with one update per step is 1/E updates per transition')
    p.add_argument('--host-envs', default=1, type=int,
                   help='host environments per agent / member, seeded seed + i (1..256; --start_timesteps and --eval_freq multiples of it; not with '
                        '--device-env, --device-loop, --pbt-interval, --halving-interval).  An iteration is E transitions -- one select_actions launch, '
                        'E env.step, one add_batch -- and one train(); further updates are the caller\'s')
    p.add_argument('--torch-envs', default=0, type=int,
                   help='environments of a torch simulator on the device (one agent, --env Pendulum-v1; 1..65536, 0 = off; --start_timesteps and '
                        '--eval_freq multiples of it; not with --seeds, --sweep, --device-env, --device-loop, --host-envs, --num-envs).  An iteration '
                        'is N transitions -- one act_device launch, one batched step, one add_device launch -- and one train()')
    p.add_argument('--sim-graph', action='store_true',
                   help='with --torch-envs N: act, explore, simulator step, append and train() of an iteration as ONE graph replay '
                        '(SACAgent.iterate_sim; the counters live on the device).  Not with --per')
    p.add_argument('--fused-sim', action='store_true',
                   help='with --torch-envs N --sim-graph: the simulator is a fused one (envs/fused_sim.py FusedSim; --env Pendulum-v1 or '
                        'MountainCarContinuous-v0) whose step and ring append are ONE launch, so an iteration in front of train() is two launches')
    p.add_argument('--per', action='store_true',
                   help='prioritized experience replay (Schaul et al. 2016; --alg sac, one agent): train() samples in proportion to '
                        '(|TD| + eps)^alpha from a sum tree on the device and weights the critic loss; beta is annealed linearly to 1 at '
                        '--max_timesteps, written at every evaluation.  Runs with the plain loop, --host-envs and --torch-envs')
    p.add_argument('--critic-per', action='store_true',
                   help='prioritized replay of the critic minibatch (--alg vlsac, ctrlsac, spedersac or diffsrsac; one agent): the minibatch the critic '
                        'and actor steps reuse is drawn in proportion to (|TD| + eps)^alpha and the critic loss is weighted, while every other '
                        'feature minibatch stays uniform; --per-alpha / --per-beta as for --per, beta annealed to 1 at --max_timesteps.  Runs with '
                        'the plain loop, --host-envs and --torch-envs; not with --seeds / --sweep, --device-loop, --sim-graph or --critic-n-step '
                        '(--alg sac takes --per)')
    p.add_argument('--per-alpha', default=0.6, type=float, help='priority exponent alpha (0 = uniform replay; default 0.6)')
    p.add_argument('--per-beta', default=0.4, type=float, help='initial importance-sampling exponent beta (default 0.4)')
    p.add_argument('--group-per', action='store_true',
                   help='prioritized experience replay for a seed group (--alg sac with --seeds and / or --sweep): every member samples from a sum '
                        'tree of its own, one launch per step for all members; --per-alpha / --per-beta as for --per, beta annealed for all '
                        'members; --sweep per_alpha=0.4,0.6 gives the members different exponents.  Goes with --pbt-interval and '
                        '--halving-interval; not with --device-env or --per')
    p.add_argument('--group-critic-per', action='store_true',
                   help='prioritized replay of the critic minibatch for a seed group (--alg ctrlsac with --seeds and / or --sweep): every member draws '
                        'the minibatch its critic and actor steps reuse from a sum tree of its own and weights its critic loss, one launch per step '
                        'for all members, while every other feature minibatch stays uniform; --per-alpha / --per-beta as for --per, beta annealed '
                        'for all members; --sweep per_alpha=0.4,0.6 gives the members different exponents.  Goes with --pbt-interval, '
                        '--halving-interval and --host-envs; not with --per, --group-per, --critic-per, --device-env or --critic-n-step')
    p.add_argument('--n-step', default=1, type=int,
                   help='n-step returns (--alg sac; 1..16, default 1 = one-step targets): train() gathers, on the device, rows that follow each sampled '
                        'transition up to N steps forward through the replay ring and bootstraps with discount^m.  Goes with --per, --seeds / '
                        '--sweep (discount= included), --group-per, --pbt-interval / --halving-interval, --host-envs, --torch-envs, --device-loop and '
                        '--device-env --num-envs')
    p.add_argument('--n-stride', default=None, type=int,
                   help='the distance between a ring row and its successor (with --n-step): the number of environments whose transitions interleave '
                        'in the ring.  Default: what the chosen loop writes (--host-envs E: E, --torch-envs N: N, --num-envs E: E, else 1)')
    p.add_argument('--critic-n-step', default=1, type=int,
                   help='n-step critic targets (--alg vlsac, ctrlsac, spedersac or diffsrsac; 1..16, default 1 = one-step targets): the critic and '
                        'actor steps of train() bootstrap from rows gathered up to N steps forward through the replay ring, while the feature step '
                        'keeps training on the one-step rows of the same minibatch.  --n-stride as for --n-step.  One agent, one GPU; goes with '
                        '--host-envs, --torch-envs (--sim-graph) and --device-loop --num-envs; not with --seeds / --sweep, --per or --n-step')
    p.add_argument('--fused-sim-source', default=None, metavar='PATH',
                   help='with --torch-envs N --sim-graph --fused-sim: the simulator is a kind of your own, the C++ text of one struct in PATH '
                        '(csrc/sim_jit.h; examples under rlrep_amd/envs/kinds/), compiled at run time (envs/fused_sim.py CustomFusedSim); the '
                        'agent is built from the kind\'s S and A and --env only names the log directory')
    args = p.parse_args(argv)
    _check_fused_sim_source(args)
    _check_nstep(args)
    _check_critic_nstep(args)
    _check_group_critic_per(args)
    _check_group_per(args)
    _check_per(args)
    _check_critic_per(args)
    _check_num_envs(args)
    _check_host_envs(args)
    _check_fused_sim(args)
    _check_torch_envs(args)
    _check_sim_graph(args)
    if args.device_loop:
        _check_device_loop(args)
    if args.seeds is not None or args.sweep:
        return run_seeds(args)
    if _pbt_requested(args):
        raise SystemExit('--pbt-*: population-based training needs a seed group (--seeds and / or --sweep)')
    if _halving_requested(args):
        raise SystemExit('--halving-*: successive halving needs a seed group (--seeds and / or --sweep)')
    if args.device_env:
        raise SystemExit('--device-env: device environments are built for seed groups (give --seeds and / or --sweep)')

    if getattr(args, 'fused_sim_source', None):
        env = eval_env = _KindSpaces(args.fused_kind)
    else:
        env, eval_env = envs.make(args.env), envs.make(args.env)
    env.seed(args.seed)
    eval_env.seed(args.seed)
    max_length = env._max_episode_steps
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)

    state_dim, action_dim = env.observation_space.shape[0], env.action_space.shape[0]
    agent = build_agent(args, state_dim, action_dim, env.action_space)
    if getattr(args, 'per', False):
        replay = buffer.PrioritizedReplayBuffer(state_dim, action_dim, max_size=int(min(args.max_timesteps, 1e6)), alpha=args.per_alpha, beta=args.per_beta,
                                                **_nstep_kw(args))
    elif getattr(args, 'critic_per', False):
        replay = buffer.CriticPrioritizedReplayBuffer(state_dim, action_dim, max_size=int(min(args.max_timesteps, 1e6)), alpha=args.per_alpha,
                                                      beta=args.per_beta, **_nstep_kw(args))
    else:
        replay = buffer.ReplayBuffer(state_dim, action_dim, max_size=int(min(args.max_timesteps, 1e6)), **_nstep_kw(args))
    ev = _Evaluations(args, agent, replay, os.path.join(_log_root(args), str(args.seed)))
    if args.device_loop:
        return _single_device_loop(args, agent, replay, ev)
    if args.host_envs > 1:
        return _host_envs_loop(args, agent, replay, ev)
    if args.torch_envs and args.sim_graph and args.fused_sim:
        return _fused_sim_loop(args, agent, replay, ev)
    if args.torch_envs and args.sim_graph:
        return _sim_graph_loop(args, agent, replay, ev)
    if args.torch_envs:
        return _torch_envs_loop(args, agent, replay, ev)
    evaluate = functools.partial(util.eval_policy, agent, eval_env, args.eval_episodes)
    ev.evaluations.append(evaluate())

    state, done = env.reset(), False
    ep_reward, ep_steps, ep_num, info = 0.0, 0, 0, None
    ev.timer = util.Timer()
    for t in range(int(args.max_timesteps)):
        ep_steps += 1
        if t < args.start_timesteps or np.random.uniform(0, 1) < EPS_GREEDY:
            action = env.action_space.sample()
        else:
            action = agent.select_action(state, explore=True)
        next_state, reward, done, _ = env.step(action)
        replay.add(state, action, next_state, reward, float(done) if ep_steps < max_length else 0)
        state = next_state
        ep_reward += reward
        if t >= args.start_timesteps:
            info = agent.train(replay, batch_size=args.batch_size)
        if done:
            print(f'Total T: {t + 1} Episode Num: {ep_num + 1} Episode T: {ep_steps} Reward: {ep_reward:.3f}')
            state, done = env.reset(), False
            ep_reward, ep_steps, ep_num = 0.0, 0, ep_num + 1
        if (t + 1) % args.eval_freq == 0:
            ev.step(t + 1, evaluate, info)
    ev.close()
    return agent, ev.evaluations


def _nstep_stride(args):
    """the successor distance of the ring the chosen loop writes: --n-stride, or the number of environments the loop interleaves"""
    if getattr(args, 'n_stride', None) is not None:
        return int(args.n_stride)
    for v in (getattr(args, 'host_envs', 1), getattr(args, 'torch_envs', 0), getattr(args, 'num_envs', 1)):
        if int(v or 0) > 1:
            return int(v)
    return 1


def _check_device_stride(args):
    """the stride rule of the device loops, for --n-step and --critic-n-step alike: a device environment writes --num-envs rows per step"""
    E = int(getattr(args, 'num_envs', 1))
    if (getattr(args, 'device_loop', False) or getattr(args, 'device_env', False)) and _nstep_stride(args) != E:
        raise SystemExit(f'--n-stride {_nstep_stride(args)}: a device environment interleaves --num-envs {E} trajectories in the ring; the stride must be {E}')


def _nstep_kw(args):
    """the n-step keywords of the replay buffer classes (nothing without --n-step: the buffers are built as before)"""
    n, cn = int(getattr(args, 'n_step', 1)), int(getattr(args, 'critic_n_step', 1))
    if cn > 1:
        return dict(critic_n_step=cn, n_stride=_nstep_stride(args))
    return dict(n_step=n, n_stride=_nstep_stride(args)) if n > 1 else {}


def _check_critic_nstep(args):
    """--critic-n-step: SystemExit, before anything touches the GPU, on what n-step critic targets do not run with (an argument namespace
    without the attribute -- built by hand -- is a run without it)"""
    cn = int(getattr(args, 'critic_n_step', 1))
    if not 1 <= cn <= 16:
        raise SystemExit(f'--critic-n-step {cn}: n-step critic targets take 1..16 steps')
    if cn == 1:
        return
    if args.alg == 'sac':
        raise SystemExit(f'--critic-n-step {cn}: a sac agent owns its whole minibatch: give --n-step {cn} (--critic-n-step is for --alg vlsac, '
                         'ctrlsac, spedersac and diffsrsac, whose feature step keeps the one-step rows)')
    if args.alg not in ('vlsac', 'ctrlsac', 'spedersac', 'diffsrsac'):
        raise SystemExit(f'--critic-n-step {cn}: built for --alg vlsac, ctrlsac, spedersac and diffsrsac (got --alg {args.alg})')
    if int(getattr(args, 'n_step', 1)) > 1:
        raise SystemExit('--critic-n-step: not together with --n-step (a replay buffer trains one kind of agent)')
    for flag, given in (('--seeds', getattr(args, 'seeds', None) is not None), ('--sweep', bool(getattr(args, 'sweep', None))),
                        ('--per', getattr(args, 'per', False)), ('--group-per', getattr(args, 'group_per', False)),
                        ('--device-env', getattr(args, 'device_env', False))):
        if given:
            raise SystemExit(f'--critic-n-step {cn}: not with {flag} (n-step critic targets are built for one agent and a plain replay buffer)')
    _check_device_stride(args)


def _check_nstep(args):
    """--n-step / --n-stride: SystemExit, before anything touches the GPU, on what n-step returns do not run with (an argument namespace without
    the attributes -- the tests build those by hand -- has none)."""
    n, stride = int(getattr(args, 'n_step', 1)), getattr(args, 'n_stride', None)
    if not 1 <= n <= 16:
        raise SystemExit(f'--n-step {n}: n-step returns take 1..16 steps')
    if stride is not None and int(stride) < 1:
        raise SystemExit(f'--n-stride {stride}: the distance between a ring row and its successor must be >= 1')
    if n == 1:
        if stride is not None and int(getattr(args, 'critic_n_step', 1)) <= 1:      # (--critic-n-step N shares --n-stride)
            raise SystemExit('--n-stride: it is the successor distance of n-step returns: give --n-step N (N > 1) with it')
        return
    if args.alg != 'sac':
        raise SystemExit(f'--n-step {n}: n-step returns are built for --alg sac (got --alg {args.alg}: the feature step of the representation agents '
                         'models one-step dynamics and their critic reuses its minibatch)')
    _check_device_stride(args)


def _check_per(args):
    """--per: SystemExit, before anything touches the GPU, on what prioritized replay does not run with (an argument namespace without the
    field -- built by hand -- is a run without it)"""
    if not getattr(args, 'per', False):
        return
    if args.alg != 'sac':
        raise SystemExit(f'--per: prioritized replay is built for --alg sac (got --alg {args.alg}: the representation agents reuse their last '
                         'feature minibatch for the critic step)')
    for flag, given in (('--seeds', args.seeds is not None), ('--sweep', bool(args.sweep)), ('--device-env', args.device_env),
                        ('--device-loop', args.device_loop), ('--pbt-interval', _pbt_requested(args)),
                        ('--halving-interval', _halving_requested(args))):
        if given:
            raise SystemExit(f'--per: prioritized replay trains ONE agent from a ring the host or add_device fills; it does not go with {flag}')
    _check_per_exponents('--per', args)


def _check_critic_per(args):
    """--critic-per: SystemExit, before anything touches the GPU, on what prioritized replay of the critic minibatch does not run with (a
    namespace without the field is a run without it)"""
    if not getattr(args, 'critic_per', False):
        return
    if args.alg == 'sac':
        raise SystemExit('--critic-per: a sac agent owns its whole minibatch: give --per (--critic-per is for --alg vlsac, ctrlsac, spedersac and '
                         'diffsrsac, whose critic reuses the last feature minibatch)')
    if args.alg not in ('vlsac', 'ctrlsac', 'spedersac', 'diffsrsac'):
        raise SystemExit(f'--critic-per: built for --alg vlsac, ctrlsac, spedersac and diffsrsac (got --alg {args.alg})')
    for flag, given in (('--per', getattr(args, 'per', False)), ('--group-per', getattr(args, 'group_per', False)),
                        ('--seeds', getattr(args, 'seeds', None) is not None), ('--sweep', bool(getattr(args, 'sweep', None))),
                        ('--device-env', getattr(args, 'device_env', False)), ('--device-loop', getattr(args, 'device_loop', False)),
                        ('--sim-graph', getattr(args, 'sim_graph', False)), ('--critic-n-step', int(getattr(args, 'critic_n_step', 1)) > 1),
                        ('--n-step', int(getattr(args, 'n_step', 1)) > 1)):
        if given:
            raise SystemExit(f'--critic-per: prioritized critic replay trains ONE agent from a ring the host or add_device fills, with one-step '
                             f'targets; it does not go with {flag}')
    _check_per_exponents('--critic-per', args)


def _check_group_per(args):
    """--group-per: SystemExit, before anything touches the GPU, on what prioritized replay of a seed group does not run with (a namespace
    without the field is a run without it)"""
    if not getattr(args, 'group_per', False):
        return
    if getattr(args, 'per', False):
        raise SystemExit('--group-per: it is the seed-group form of prioritized replay and does not go with --per (the single-agent form); give one of them')
    if args.alg != 'sac':
        raise SystemExit(f'--group-per: prioritized replay of a seed group is built for --alg sac (got --alg {args.alg}: the representation agents '
                         'reuse their last feature minibatch for the critic step)')
    if args.seeds is None and not args.sweep:
        raise SystemExit('--group-per: prioritized replay of a seed group needs a seed group: give --seeds and / or --sweep (one agent takes --per)')
    for flag, given in (('--device-env', args.device_env), ('--device-loop', getattr(args, 'device_loop', False))):
        if given:
            raise SystemExit(f'--group-per: a device environment writes ring rows inside its step launch, which knows nothing of the priority '
                             f'trees; it does not go with {flag}')
    _check_per_exponents('--group-per', args)


def _check_group_critic_per(args):
    """--group-critic-per: SystemExit, before anything touches the GPU, on what prioritized critic replay of a seed group does not run with (a
    namespace without the field is a run without it)"""
    if not getattr(args, 'group_critic_per', False):
        return
    for flag, given in (('--per', getattr(args, 'per', False)), ('--group-per', getattr(args, 'group_per', False)),
                        ('--critic-per', getattr(args, 'critic_per', False))):
        if given:
            raise SystemExit(f'--group-critic-per: it is the ctrlsac seed-group form of prioritized replay and does not go with {flag}; give one of them')
    if args.alg != 'ctrlsac':
        raise SystemExit(f'--group-critic-per: prioritized critic replay of a seed group is built for --alg ctrlsac (got --alg {args.alg}: a sac seed '
                         'group takes --group-per, the other representation agents have no seed groups)')
    if getattr(args, 'seeds', None) is None and not getattr(args, 'sweep', None):
        raise SystemExit('--group-critic-per: prioritized critic replay of a seed group needs a seed group: give --seeds and / or --sweep (one agent '
                         'takes --critic-per)')
    for flag, given in (('--device-env', getattr(args, 'device_env', False)), ('--device-loop', getattr(args, 'device_loop', False))):
        if given:
            raise SystemExit(f'--group-critic-per: a device environment writes ring rows inside its step launch, which knows nothing of the priority '
                             f'trees; it does not go with {flag}')
    for flag, given in (('--critic-n-step', int(getattr(args, 'critic_n_step', 1)) > 1), ('--n-step', int(getattr(args, 'n_step', 1)) > 1)):
        if given:
            raise SystemExit(f'--group-critic-per: prioritized critic replay of a seed group has one-step targets; it does not go with {flag}')
    _check_per_exponents('--group-critic-per', args)


def _check_per_exponents(flag, args):
    """the ranges of --per-alpha and --per-beta, for `flag` (--per or --group-per)"""
    if not 0.0 <= float(args.per_alpha) or not 0.0 <= float(args.per_beta) <= 1.0:
        raise SystemExit(f'{flag}: --per-alpha {args.per_alpha} must be >= 0 and --per-beta {args.per_beta} in [0, 1]')


def _per_anneal(args, replay, t):
    """--per / --group-per: beta rises linearly from --per-beta to 1.0 at --max_timesteps; written (one device word per member) at the evaluation
    boundaries"""
    if getattr(args, 'per', False) or getattr(args, 'group_per', False) or getattr(args, 'critic_per', False) or getattr(args, 'group_critic_per', False):
        frac = min(1.0, float(t) / float(args.max_timesteps))
        replay.beta = 1.0 if frac >= 1.0 else float(args.per_beta) + (1.0 - float(args.per_beta)) * frac


def _check_num_envs(args):
    """--num-envs: SystemExit, before anything touches the GPU, on what it does not run with"""
    E = int(args.num_envs)
    if E != 1 and not (args.device_env or args.device_loop):
        raise SystemExit('--num-envs: several environments per agent are stepped on the device; give --device-env (seed groups) or --device-loop (one agent)')
    if not 1 <= E <= 64:
        raise SystemExit(f'--num-envs {E}: outside [1, 64]')
    _check_multiple('--num-envs', E, args, f'a step launch takes {E} steps per member at once')


def _check_multiple(flag, n, args, why):
    """--start_timesteps and --eval_freq are multiples of `flag`'s value n, or SystemExit: an iteration of its loop is n steps, all warm-up or
    none of it, and evaluations fall between iterations"""
    for name, value in (('--start_timesteps', args.start_timesteps), ('--eval_freq', args.eval_freq)):
        if value != int(value) or int(value) % n:
            raise SystemExit(f'{flag} {n}: {name} {value:g} is not a multiple of it ({why})')


def _check_host_envs(args):
    """--host-envs: SystemExit, before anything touches the GPU, on what it does not run with"""
    E = int(args.host_envs)
    if not 1 <= E <= 256:
        raise SystemExit(f'--host-envs {E}: outside [1, 256]')
    if E == 1:
        return
    for flag, given in (('--device-env', args.device_env), ('--device-loop', args.device_loop), ('--pbt-interval', _pbt_requested(args)),
                        ('--halving-interval', _halving_requested(args))):
        if given:
            raise SystemExit(f'--host-envs {E}: several host environments per agent do not go with {flag} (device environments take --num-envs; '
                             'ranking a population over vector environments is not built)')
    _check_multiple('--host-envs', E, args, f'an iteration takes {E} environment steps at once')


def _host_envs(name, seed, n):
    """n host environments `name`, environment i seeded seed + i"""
    out = [envs.make(name) for _ in range(n)]
    for i, e in enumerate(out):
        e.seed(seed + i)
    return out


def _host_envs_loop(args, agent, replay, ev):
    """run()'s loop over E = --host-envs host environments (seeded seed + i): an iteration is ONE `select_actions` launch, E `env.step`, one
    `add_batch` (done_bool per environment by run()'s rule) and one `train()`.  During warm-up, and with probability epsilon afterwards, an
    environment's action is its action space's uniform sample, drawn in environment order as run() draws it.  Episodes end and reset per
    environment; an evaluation is util.eval_policy_vec over min(E, --eval_episodes) environments."""
    E = int(args.host_envs)
    envs_ = _host_envs(args.env, args.seed, E)
    eval_envs = _host_envs(args.env, args.seed, min(E, int(args.eval_episodes)))
    max_length = envs_[0]._max_episode_steps
    evaluate = functools.partial(util.eval_policy_vec, agent, eval_envs, args.eval_episodes)
    ev.evaluations.append(evaluate())
    states = np.stack([np.asarray(e.reset(), np.float32) for e in envs_])
    action_dim = envs_[0].action_space.shape[0]
    ep_reward, ep_steps, ep_num, info = np.zeros(E), np.zeros(E, np.int64), 0, None
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), E):             # one iteration is E environment steps
        ep_steps += 1
        warm = t0 < args.start_timesteps
        greedy = None if warm else agent.select_actions(states, explore=True)
        actions = np.zeros((E, action_dim), np.float32)
        for i, e in enumerate(envs_):
            actions[i] = e.action_space.sample() if warm or np.random.uniform(0, 1) < EPS_GREEDY else greedy[i]
        nexts, rewards, dones = np.zeros_like(states), np.zeros(E, np.float32), np.zeros(E, np.float32)
        resets = []
        for i, e in enumerate(envs_):
            nexts[i], reward, done, _ = e.step(actions[i])
            rewards[i] = reward
            dones[i] = float(done) if ep_steps[i] < max_length else 0.0
            ep_reward[i] += reward
            if done:
                resets.append(i)
        replay.add_batch(states, actions, nexts, rewards, dones)
        states = nexts
        for i in resets:
            ep_num += 1
            print(f'Total T: {t0 + E} Episode Num: {ep_num} Env: {i} Episode T: {ep_steps[i]} Reward: {ep_reward[i]:.3f}')
            states[i] = envs_[i].reset()
            ep_reward[i], ep_steps[i] = 0.0, 0
        if not warm:
            info = agent.train(replay, batch_size=args.batch_size)
        t = t0 + E
        if t % args.eval_freq == 0:
            ev.step(t, evaluate, info)
    ev.close()
    return agent, ev.evaluations


def _torch_envs_group(args):
    """--seeds / --sweep with --torch-envs N --sim-graph --fused-sim: the one-graph simulator loop of a seed group (_fused_sim_group_loop)"""
    return bool((getattr(args, 'seeds', None) is not None or getattr(args, 'sweep', None)) and int(getattr(args, 'torch_envs', 0) or 0)
                and getattr(args, 'sim_graph', False) and getattr(args, 'fused_sim', False))


def _check_torch_envs(args):
    """--torch-envs: SystemExit, before anything touches the GPU, on what it does not run with"""
    N = int(args.torch_envs)
    if N == 0:
        return
    if not 1 <= N <= 65536:
        raise SystemExit(f'--torch-envs {N}: outside [1, 65536]')
    # a seed group runs the fused one-graph loop only (--sim-graph --fused-sim: SeedBatchMixin.iterate_sim); the newer attributes are read
    # with getattr, for callers that build the Namespace themselves
    group = _torch_envs_group(args)
    for flag, given in (('--seeds', args.seeds is not None and not group), ('--sweep', bool(args.sweep) and not group), ('--device-env', args.device_env),
                        ('--device-loop', args.device_loop), ('--host-envs', args.host_envs > 1), ('--num-envs', args.num_envs > 1)):
        if given:
            raise SystemExit(f'--torch-envs {N}: the torch simulator loop runs ONE agent and does not go with {flag} (a seed group takes '
                             '--torch-envs N --sim-graph --fused-sim, the fused one-graph loop, and none of the other collection flags)')
    if group:
        for flag, given in (('--pbt-interval', hasattr(args, 'pbt_interval') and _pbt_requested(args)),
                            ('--halving-interval', hasattr(args, 'halving_interval') and _halving_requested(args)),
                            ('--group-per', bool(getattr(args, 'group_per', False))), ('--group-critic-per', bool(getattr(args, 'group_critic_per', False))),
                            ('--fused-sim-source', bool(getattr(args, 'fused_sim_source', None)))):
            if given:
                raise SystemExit(f'--torch-envs {N}: the one-graph simulator loop of a seed group (--seeds / --sweep with --sim-graph --fused-sim) does '
                                 f'not go with {flag}')
    if not args.env.startswith('Pendulum') and not getattr(args, 'fused_sim', False):         # (--fused-sim has checked --env against its own kinds)
        raise SystemExit(f'--torch-envs {N}: the example simulator is Pendulum-v1 (got --env {args.env})')
    _check_multiple('--torch-envs', N, args, f'an iteration takes {N} environment steps at once')
    if N > min(args.max_timesteps, 1e6):
        raise SystemExit(f'--torch-envs {N}: more environments than the replay ring has rows (min(--max_timesteps, 1e6))')


def _torch_eval(agent, env, episodes):
    """mean return of `episodes` mean-action episodes, env.num_envs at a time in lockstep: one act_device launch per step, one copy at the end"""
    returns = []
    while len(returns) < episodes:
        obs = env.reset()
        for _ in range(env._max_episode_steps):
            env.step(agent.act_device(obs, explore=False))
            obs = env.obs
        returns.extend(env.last_return.cpu().tolist())
    return float(np.mean(returns[:episodes]))


def _torch_envs_loop(args, agent, replay, ev):
    """run()'s loop over N = --torch-envs environments of a simulator on the device (envs/torch_pendulum.py): an iteration is ONE `act_device`
    launch, one batched `step`, ONE `add_device` launch and one `train()`; nothing of a transition crosses the host.  During warm-up, and
    with probability epsilon afterwards, an environment's action is uniform in the action range, drawn on the device.  Evaluations follow
    every --eval_freq steps (none before the first step)."""
    from rlrep_amd.envs.torch_pendulum import TorchPendulum
    N, dev = int(args.torch_envs), replay.device
    env = TorchPendulum(N, dev, seed=args.seed)
    eval_env = TorchPendulum(min(N, int(args.eval_episodes)), dev, seed=args.seed + 100)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(args.seed))
    lo, hi = agent.action_range
    A = env.action_dim
    evaluate = functools.partial(_torch_eval, agent, eval_env, int(args.eval_episodes))
    info, episodes = None, 0
    obs = env.reset()
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), N):             # one iteration is N environment steps
        uniform = lo + (hi - lo) * torch.rand(N, A, dtype=torch.float32, device=dev, generator=gen)
        if t0 < args.start_timesteps:
            actions = uniform
        else:
            pick = torch.rand(N, 1, dtype=torch.float32, device=dev, generator=gen) < EPS_GREEDY
            actions = torch.where(pick, uniform, agent.act_device(obs, explore=True))
        nexts, rewards, dones = env.step(actions)
        replay.add_device(obs, actions, nexts, rewards, dones)
        obs = env.obs
        if env.episodes != episodes:
            episodes = env.episodes
            print(f'Total T: {t0 + N} Episode Num: {episodes * N} Mean reward: {float(env.last_return.mean()):.3f}')
        if t0 >= args.start_timesteps:
            info = agent.train(replay, batch_size=args.batch_size)
        t = t0 + N
        if t % args.eval_freq == 0:
            ev.step(t, evaluate, info)
    ev.close()
    return agent, ev.evaluations


def _check_sim_graph(args):
    """--sim-graph: SystemExit, before anything touches the GPU, on what it does not run with"""
    if not getattr(args, 'sim_graph', False):
        return
    if not int(args.torch_envs):
        raise SystemExit('--sim-graph: the one-graph simulator loop is a form of the torch simulator loop; give --torch-envs N with it')
    if getattr(args, 'per', False):
        raise SystemExit('--sim-graph: the captured append of --torch-envs does not write the priority tree and does not go with --per')


def _sim_graph_loop(args, agent, replay, ev):
    """_torch_envs_loop with --sim-graph: an iteration is ONE `iterate_sim` graph replay -- the act launch with the exploration mix, the
    capturable simulator's `step_`, the append launch and train().  The environments run in lockstep, so every 200th iteration ends an
    episode in all of them.  Evaluations are _torch_eval's, on a simulator of their own."""
    from rlrep_amd.envs.sim_loop import SimLoop
    from rlrep_amd.envs.torch_pendulum import TorchPendulum
    N, dev = int(args.torch_envs), replay.device
    env = TorchPendulum(N, dev, seed=args.seed, capturable=True)
    eval_env = TorchPendulum(min(N, int(args.eval_episodes)), dev, seed=args.seed + 100)
    env.reset()
    loop = SimLoop(agent, env, eps_greedy=EPS_GREEDY, start_timesteps=int(args.start_timesteps))
    evaluate = functools.partial(_torch_eval, agent, eval_env, int(args.eval_episodes))
    info = None
    ev.timer = util.Timer()
    for k, t0 in enumerate(range(0, int(args.max_timesteps), N)):           # one iteration is N environment steps
        out = agent.iterate_sim(loop, replay, args.batch_size, train=t0 >= args.start_timesteps)
        info = out if out is not None else info
        if (k + 1) % env._max_episode_steps == 0:
            print(f'Total T: {t0 + N} Episode Num: {(k + 1) // env._max_episode_steps * N} Mean reward: {float(env.last_return.mean()):.3f}')
        t = t0 + N
        if t % args.eval_freq == 0:
            ev.step(t, evaluate, info)
    ev.close()
    return agent, ev.evaluations


FUSED_SIM_ENVS = ('Pendulum-v1', 'MountainCarContinuous-v0')               # envs/fused_sim.py KINDS


def _check_fused_sim(args):
    """--fused-sim: SystemExit, before anything touches the GPU, on what it does not run with"""
    if not getattr(args, 'fused_sim', False):
        return
    if not int(args.torch_envs) or not getattr(args, 'sim_graph', False):
        raise SystemExit('--fused-sim: the fused simulators are simulators of the one-graph simulator loop; give --torch-envs N --sim-graph with it')
    if not getattr(args, 'fused_sim_source', None) and not args.env.startswith(tuple(n.split('-')[0] for n in FUSED_SIM_ENVS)):
        raise SystemExit(f'--fused-sim: only {" and ".join(FUSED_SIM_ENVS)} are built as fused simulators (got --env {args.env})')


def _check_fused_sim_source(args):
    """--fused-sim-source PATH: SystemExit, before anything touches the GPU, unless it comes with --torch-envs N --sim-graph --fused-sim, PATH
    is readable and its text spells the kind's constants; leaves the text and the constants on args (fused_kind_text, fused_kind)"""
    path = getattr(args, 'fused_sim_source', None)
    if not path:
        return
    for flag, given in (('--torch-envs N', int(args.torch_envs) > 0), ('--sim-graph', getattr(args, 'sim_graph', False)),
                        ('--fused-sim', getattr(args, 'fused_sim', False))):
        if not given:
            raise SystemExit(f'--fused-sim-source: a kind of your own is a simulator of the fused one-graph loop; give {flag} with it '
                             '(--torch-envs N --sim-graph --fused-sim)')
    from rlrep_amd.envs.fused_sim import kind_constants
    try:
        with open(path) as f:
            args.fused_kind_text = f.read()
    except OSError as exc:
        raise SystemExit(f'--fused-sim-source: cannot read {path}: {exc}')
    args.fused_kind = k = kind_constants(args.fused_kind_text)
    missing = [key for key in ('name', 'S', 'A', 'NX', 'limit', 'terminates') if k[key] is None]
    if missing:
        raise SystemExit(f'--fused-sim-source: {path} does not spell {", ".join(missing)} as a literal (csrc/sim_jit.h describes a kind\'s struct)')


class _KindSpaces(object):
    """what run() reads of a host environment, for a kind that exists on the device only: the spaces' shapes and the action range"""

    def __init__(self, k):
        lo, hi = k['action_range']
        self.observation_space = type('Space', (), dict(shape=(int(k['S']),)))()
        self.action_space = type('Space', (), dict(shape=(int(k['A']),), low=np.full(int(k['A']), lo, np.float32), high=np.full(int(k['A']), hi, np.float32)))()
        self._max_episode_steps = int(k['limit'])

    def seed(self, seed):
        pass


def _fused_eval(agent, env, episodes):
    """_torch_eval for a FusedSim(auto_restart=False): env.num_envs mean-action episodes at a time, one act_device launch and one step launch
    per step -- an environment whose episode ended is frozen with its return in last_return -- and one copy at the end.  Every round resets
    first, so it draws fresh start states."""
    returns = []
    act = torch.empty(env.num_envs, env.action_dim, dtype=torch.float32, device=env.obs.device)
    while len(returns) < episodes:
        env.reset()
        for _ in range(env._max_episode_steps):
            env.step_(agent.act_device(env.obs, explore=False, out=act))
        returns.extend(env.last_return.cpu().tolist())
    return float(np.mean(returns[:episodes]))


def _fused_sim_loop(args, agent, replay, ev):
    """_sim_graph_loop with --fused-sim: the simulator is a FusedSim of --env, so an `iterate_sim` graph replay holds the act launch, the
    step-and-append launch and train().  Episodes end per environment (MountainCar's at different steps) and are counted on the device:
    their number and the mean of the last returns are printed where an evaluation synchronises anyway, and no iteration reads the host."""
    from rlrep_amd.envs.fused_sim import CustomFusedSim, FusedSim, SimKind
    from rlrep_amd.envs.sim_loop import SimLoop
    N, dev = int(args.torch_envs), replay.device
    if getattr(args, 'fused_sim_source', None):             # a kind of the user's own: ONE run-time compile, shared by the two simulators
        kind = SimKind(args.fused_kind_text)
        env = CustomFusedSim(kind, N, dev, seed=args.seed)
        eval_env = CustomFusedSim(kind, min(N, int(args.eval_episodes)), dev, seed=args.seed + 100, auto_restart=False)
    else:
        env = FusedSim(args.env, N, dev, seed=args.seed)
        eval_env = FusedSim(args.env, min(N, int(args.eval_episodes)), dev, seed=args.seed + 100, auto_restart=False)
    env.reset()
    loop = SimLoop(agent, env, eps_greedy=EPS_GREEDY, start_timesteps=int(args.start_timesteps))

    def evaluate():
        score = _fused_eval(agent, eval_env, int(args.eval_episodes))
        episodes = int(env.episodes.sum())
        if episodes:
            print(f'Total T: {loop.t_global} Episode Num: {episodes} Mean reward: {float(torch.nanmean(env.last_return)):.3f}')
        return score
    info = None
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), N):                         # one iteration is N environment steps
        out = agent.iterate_sim(loop, replay, args.batch_size, train=t0 >= args.start_timesteps)
        info = out if out is not None else info
        t = t0 + N
        if t % args.eval_freq == 0:
            ev.step(t, evaluate, info)
    ev.close()
    return agent, ev.evaluations


def _check_device_loop(args):
    """--device-loop is the single agent's device environment; SystemExit, before anything touches the GPU, on what it does not run with"""
    for flag, given in (('--seeds', args.seeds is not None), ('--sweep', bool(args.sweep)), ('--pbt-*', _pbt_requested(args)),
                        ('--halving-*', _halving_requested(args)), ('--device-env', args.device_env)):
        if given:
            raise SystemExit(f'--device-loop: runs ONE agent with its environment on the device and does not go with {flag}; a seed group takes '
                             '--device-env (with --seeds and / or --sweep)')
    from rlrep_amd.envs.device import single_device_class
    if single_device_class(args.env) is None:
        raise SystemExit(f'--device-loop: only Pendulum-v1 and MountainCarContinuous-v0 are built on the device (got --env {args.env}); run without --device-loop')


def _single_device_loop(args, agent, replay, ev):
    """run()'s loop with the environment on the device (--device-loop), _device_loop's shape for one agent: an initial evaluation, one
    `agent.iterate` per step -- act, explore, step, ring row and train() in one graph replay -- and one `agent.evaluate` launch every
    --eval_freq.  The exploration and reset draws are Philox streams of the agent's seed instead of NumPy generators; the metrics.jsonl rows
    keep their keys, and --save_model writes the environment's record with the checkpoint."""
    from rlrep_amd.envs.device import single_device_class
    E = int(args.num_envs)
    env = single_device_class(args.env)(agent, eps_greedy=EPS_GREEDY, start_timesteps=int(args.start_timesteps), num_envs=E)
    evaluate = functools.partial(agent.evaluate, env, args.eval_episodes)
    ev.evaluations.append(evaluate())
    info = None
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), E):            # one iterate is E environment steps
        out = agent.iterate(env, replay, args.batch_size, train=t0 >= args.start_timesteps)
        info = out if out is not None else info
        t = t0 + E - 1
        if (t + 1) % args.eval_freq == 0:
            ev.step(t + 1, evaluate, info, env=env)
    ev.close()
    return agent, ev.evaluations


def _log_root(args):
    return os.path.join(args.log_root, args.env, args.alg, str(args.dir))


class _MemberPolicy(object):
    """eval_policy's view of one member of a seed batch (deterministic actions: the other members' rows are ignored)"""

    def __init__(self, group, r):
        self.group, self.r = group, r
        self.obs = np.zeros((group.R, group.state_dim), np.float32)

    def select_action(self, state):
        self.obs[self.r] = np.asarray(state, np.float32).reshape(-1)
        return self.group.select_action(self.obs)[self.r]


def _group_class(alg):
    if alg == 'ctrlsac':
        from rlrep_amd.agent.ctrlsac.seed_batch import CTRLSACSeedBatch
        return CTRLSACSeedBatch
    from rlrep_amd.agent.sac.seed_batch import SACSeedBatch
    return SACSeedBatch


def parse_sweeps(sweeps, alg, n_seeds, group_per=False):
    """--sweep arguments -> [(tag, {key: value})] in product order (one ('', {}) without a sweep).  SystemExit on an unknown key, a key --alg
    does not take, a bad or repeated value, or more members than a group holds.  per_alpha (the priority exponent of a member's replay tree)
    is a key under --group-per only; run_seeds hands it to the buffer group, not to the agent."""
    import itertools
    if not sweeps:
        return [('', {})]
    cls = _group_class(alg)
    sac, ctrl = (_group_class(a).SWEEP_KEYS for a in ('sac', 'ctrlsac'))
    i = sac.index('alpha')                  # (the message names what ctrlsac alone takes, feature_tau, beside tau)
    known = sac[:i] + tuple(k for k in ctrl if k not in sac) + sac[i:]
    axes = []
    for arg in sweeps:
        key, eq, vals = str(arg).partition('=')
        key = key.strip()
        if not eq or not vals.strip():
            raise SystemExit(f'--sweep {arg}: give KEY=V1,V2,..., e.g. --sweep lr=1e-4,3e-4')
        if key == 'per_alpha':
            if not group_per:
                raise SystemExit(f'--sweep {arg}: per_alpha is the priority exponent of a seed group\'s replay trees: it needs --group-per (--alg ctrlsac: --group-critic-per)')
            try:
                values = [float(v) for v in vals.split(',')]
                if any(not (0.0 <= v < float('inf')) for v in values):
                    raise ValueError
            except ValueError:
                raise SystemExit(f'--sweep {arg}: per_alpha takes finite numbers >= 0')
            if len(set(values)) != len(values):
                raise SystemExit(f'--sweep {arg}: repeated value')
            if key in [k for k, _ in axes]:
                raise SystemExit(f'--sweep {arg}: {key} is swept twice')
            axes.append((key, values))
            continue
        if key not in known:
            raise SystemExit(f'--sweep {arg}: unknown key {key!r} (sweepable: {", ".join(known)})')
        if key not in cls.SWEEP_KEYS:
            raise SystemExit(f'--sweep {arg}: {key} is not a hyper-parameter of --alg {alg} (it takes {", ".join(cls.SWEEP_KEYS)})')
        if key in [k for k, _ in axes]:
            raise SystemExit(f'--sweep {arg}: {key} is swept twice')
        values = []
        for v in vals.split(','):
            try:
                values.append(cls.normalise_hyper(key, v.strip(), '--sweep'))
            except ValueError as e:
                raise SystemExit(f'--sweep {arg}: {e}')
        if len(set(values)) != len(values):
            raise SystemExit(f'--sweep {arg}: repeated value')
        axes.append((key, values))
    configs = []
    for combo in itertools.product(*[v for _, v in axes]):
        cfg = dict(zip([k for k, _ in axes], combo))
        configs.append(('_'.join(f'{k}={v}' for k, v in cfg.items()), cfg))
    from rlrep_amd._lib import lib
    cap = int(lib.rlrep_group_max_members())
    if len(configs) * n_seeds > cap:
        raise SystemExit(f'--sweep: {len(configs)} configurations x {n_seeds} seeds = {len(configs) * n_seeds} members, more than a group holds ({cap})')
    return configs


def _ranking_interval(flag, what, value, eval_freq, members):
    """--pbt-interval / --halving-interval -> the interval.  SystemExit on fewer than 2 members or an interval that is not a positive multiple
    of --eval_freq."""
    if members < 2:
        raise SystemExit(f'{flag}: {what} needs at least 2 members (the group has {members})')
    interval, freq = int(value or 0), int(eval_freq)
    if interval <= 0 or freq <= 0 or interval % freq:
        raise SystemExit(f'{flag} {value}: give a positive multiple of --eval_freq ({freq}): members are ranked by their latest evaluation')
    return interval


PBT_OPTIONS = ('pbt_interval', 'pbt_fraction', 'pbt_keys', 'pbt_factors', 'pbt_seed')


def _pbt_requested(args):
    # (--pbt-interval 0 alone is "off", spelled out)
    return bool(args.pbt_interval) or any(getattr(args, k) is not None for k in PBT_OPTIONS if k != 'pbt_interval')


def parse_pbt(args, alg, members):
    """--pbt-* -> None (off) or dict(interval, fraction, keys, factors, seed).  SystemExit on fewer than 2 members, an interval that is not a
    positive multiple of --eval_freq, a fraction outside (0, 0.5], a key --alg does not sweep or that cannot be perturbed, bad factors."""
    import math
    if not _pbt_requested(args):
        return None
    interval = _ranking_interval('--pbt-interval', 'population-based training', args.pbt_interval, args.eval_freq, members)
    fraction = 0.25 if args.pbt_fraction is None else float(args.pbt_fraction)
    if not (math.isfinite(fraction) and 0.0 < fraction <= 0.5):
        raise SystemExit(f'--pbt-fraction {args.pbt_fraction}: outside (0, 0.5]')
    cls = _group_class(alg)
    keys = [k.strip() for k in str('lr' if args.pbt_keys is None else args.pbt_keys).split(',') if k.strip()]
    if not keys:
        raise SystemExit(f'--pbt-keys {args.pbt_keys}: give at least one key, e.g. --pbt-keys lr,tau')
    for k in keys:
        if k not in cls.SWEEP_KEYS:
            raise SystemExit(f'--pbt-keys {args.pbt_keys}: {k} is not a sweepable hyper-parameter of --alg {alg} (it takes {", ".join(cls.SWEEP_KEYS)})')
        if k in ('alpha', 'auto_entropy_tuning'):
            raise SystemExit(f'--pbt-keys {args.pbt_keys}: {k} cannot be perturbed (alpha is the initial temperature only, auto_entropy_tuning is a boolean)')
    if len(set(keys)) != len(keys):
        raise SystemExit(f'--pbt-keys {args.pbt_keys}: repeated key')
    try:
        factors = [float(f) for f in str('0.8,1.2' if args.pbt_factors is None else args.pbt_factors).split(',') if f.strip()]
    except ValueError:
        factors = []
    if not factors or not all(math.isfinite(f) and f > 0 for f in factors):
        raise SystemExit(f'--pbt-factors {args.pbt_factors}: give finite positive factors, e.g. --pbt-factors 0.8,1.2')
    return dict(interval=interval, fraction=fraction, keys=keys, factors=factors, seed=int(args.pbt_seed or 0))


def pbt_step(agent, scores, cfg, rng, step, log):
    """One exploit / explore step on a seed group: plan, clone in one launch, retune every destination; one `log` line per destination."""
    from rlrep_amd.agent import pbt
    pairs = pbt.plan_exploit(scores, cfg['fraction'], rng)
    agent.clone_members(pairs)
    for src, dst in pairs:
        old = agent.member_hyper(dst)
        new = pbt.perturb(agent.member_hyper(src), cfg['keys'], cfg['factors'], rng)
        retune = {k: new[k] for k in new if k != 'alpha'}
        agent.set_member_hyper(dst, **retune)
        now = agent.member_hyper(dst)
        log.write(json.dumps({'step': int(step), 'src': int(src), 'dst': int(dst), 'scores': [float(s) for s in scores],
                              'old': {k: old[k] for k in retune}, 'new': {k: now[k] for k in retune}}) + '\n')
    log.flush()
    return pairs


HALVING_OPTIONS = ('halving_interval', 'halving_keep', 'halving_min')


def _halving_requested(args):
    # (--halving-interval 0 alone is "off", spelled out)
    return bool(args.halving_interval) or any(getattr(args, k) is not None for k in HALVING_OPTIONS if k != 'halving_interval')


def parse_halving(args, members, pbt_cfg):
    """--halving-* -> None (off) or dict(interval, keep, min).  SystemExit on fewer than 2 members, an interval that is not a positive multiple
    of --eval_freq, keep outside (0, 1), min below 1, or together with --pbt-interval."""
    import math
    if not _halving_requested(args):
        return None
    interval = _ranking_interval('--halving-interval', 'successive halving', args.halving_interval, args.eval_freq, members)
    keep = 0.5 if args.halving_keep is None else float(args.halving_keep)
    if not (math.isfinite(keep) and 0.0 < keep < 1.0):
        raise SystemExit(f'--halving-keep {args.halving_keep}: outside (0, 1)')
    least = 1 if args.halving_min is None else int(args.halving_min)
    if least < 1:
        raise SystemExit(f'--halving-min {args.halving_min}: below 1 (at least one member of a group stays live)')
    if pbt_cfg is not None:
        raise SystemExit('--halving-interval together with --pbt-interval: population-based training over a shrinking population is a later change; '
                         'run one of the two')
    return dict(interval=interval, keep=keep, min=least)


def halving_step(agent, scores, seeds, cfg, step, log):
    """One halving on a seed group: plan, retire the losers (one launch), one `log` line.  Returns the retired members."""
    from rlrep_amd.agent import pbt
    out = pbt.plan_halving(scores, agent.live, cfg['keep'], cfg['min'])
    if out:
        agent.retire_members(out)
        log.write(json.dumps({'step': int(step), 'retired': [int(r) for r in out], 'seeds': [int(seeds[r]) for r in out],
                              'scores': [float(scores[r]) for r in out], 'live': int(sum(agent.live))}) + '\n')
        log.flush()
    return out


class _Evaluations(object):
    """What run()'s five loops do at an evaluation step, and the files it needs: the metrics.jsonl row (mirrored to tensorboardX if it is
    installed), the print, --save_model.  `evaluations` is the scores so far; a loop with an initial evaluation files it, and every loop
    starts `timer` (util.Timer) where its first iteration begins."""

    def __init__(self, args, agent, replay, log_path):
        self.args, self.agent, self.replay, self.log_path = args, agent, replay, log_path
        os.makedirs(log_path, exist_ok=True)
        self.jsonl = open(os.path.join(log_path, 'metrics.jsonl'), 'a')
        try:
            from tensorboardX import SummaryWriter
            self.tb = SummaryWriter(log_path)
        except ImportError:
            self.tb = None
        self.evaluations, self.timer = [], None

    def step(self, t, score, info, env=None):
        """Step `t` was an evaluation step: score() runs the evaluation (behind the rate, so that steps_per_sec excludes it), info is the
        latest train()'s (None before the first: no row), env the device environment a checkpoint carries."""
        _per_anneal(self.args, self.replay, t)          # (a no-op where the loop cannot run with --per: --sim-graph and --device-loop refuse it)
        sps = self.timer.steps_per_sec(t)
        self.evaluations.append(score())
        if info is not None:
            row = {'step': t, 'info/evaluation': float(self.evaluations[-1]), 'steps_per_sec': sps}
            row.update({f'info/{k}': float(v) for k, v in info.items()})
            self.jsonl.write(json.dumps(row) + '\n')
            self.jsonl.flush()
            if self.tb is not None:
                for k, v in row.items():
                    if k.startswith('info/'):
                        self.tb.add_scalar(k, v, t)
                self.tb.flush()
        print('Step {}. Steps per sec: {:.4g}.'.format(t, sps))
        if self.args.save_model:
            self.agent.save(os.path.join(self.log_path, 'agent.pt'), env=env)

    def close(self):
        self.jsonl.close()
        if self.tb is not None:
            self.tb.close()
        print('Total time cost {:.4g}s.'.format(self.timer.time_cost()))


class _GroupEvaluations(object):
    """What run_seeds' three loops do at an evaluation step, and the files it needs: the members' metrics.jsonl rows, the print, the PBT step,
    the halving step (and with it `live`), --save_model.  `evaluations[r]` is member r's scores so far; the loop files the initial ones and
    starts `timer` (util.Timer) where its first iteration begins."""

    def __init__(self, args, agent, seeds, logs, pbt_cfg, halving_cfg):
        self.args, self.agent, self.seeds, self.logs, self.root = args, agent, seeds, logs, _log_root(args)
        self.pbt_cfg, self.halving_cfg = pbt_cfg, halving_cfg
        self.pbt_rng = self.pbt_log = self.halving_log = None
        if pbt_cfg is not None:
            self.pbt_rng = np.random.RandomState(pbt_cfg['seed'])
            self.pbt_log = open(os.path.join(self.root, 'pbt.jsonl'), 'a')
        if halving_cfg is not None:
            self.halving_log = open(os.path.join(self.root, 'halving.jsonl'), 'a')
        self.evaluations, self.live, self.timer = None, agent.live, None

    def step(self, step, scores, infos, env=None):
        """Step `step` was an evaluation step: scores() runs the evaluation (behind the rate, so that steps_per_sec excludes it) and
        scores()[r] is live member r's (a retired member's entry is not read), infos the latest train()'s, env the device environment a
        checkpoint carries."""
        args, agent, evaluations = self.args, self.agent, self.evaluations
        _per_anneal(args, agent.replay, step)           # (a no-op where the loop cannot run with --group-per: --device-env refuses it)
        sps = self.timer.steps_per_sec(step)
        scores = scores()
        for r in range(agent.R):
            if not self.live[r]:
                continue
            evaluations[r].append(scores[r])
            if infos is not None:
                row = {'step': step, 'info/evaluation': float(evaluations[r][-1]), 'steps_per_sec': sps}
                row.update({f'info/{k}': float(v) for k, v in infos[r].items()})
                self.logs[r].write(json.dumps(row) + '\n')
                self.logs[r].flush()
        print('Step {}. Steps per sec (per seed): {:.4g}.'.format(step, sps))

        def due(cfg):
            return cfg is not None and step % cfg['interval'] == 0 and step > args.start_timesteps

        if due(self.pbt_cfg):
            pbt_step(agent, [e[-1] for e in evaluations], self.pbt_cfg, self.pbt_rng, step, self.pbt_log)
        if due(self.halving_cfg):
            halving_step(agent, [e[-1] for e in evaluations], self.seeds, self.halving_cfg, step, self.halving_log)
            self.live = agent.live
        if args.save_model:
            agent.save(os.path.join(self.root, 'seed_batch.pt'), env=env)

    def close(self):
        for f in self.logs + [f for f in (self.pbt_log, self.halving_log) if f is not None]:
            f.close()
        print('Total time cost {:.4g}s.'.format(self.timer.time_cost()))


def run_seeds(args):
    """The loop of run() for several seeds at once: R environments in lockstep, one SACSeedBatch, one ReplayBufferGroup."""
    seeds = [int(s) for s in str(args.seeds).split(',') if s.strip() != ''] if args.seeds is not None else [int(args.seed)]
    if not seeds or len(set(seeds)) != len(seeds):
        raise SystemExit(f'--seeds {args.seeds}: give distinct integer seeds, e.g. --seeds 0,1,2,3')
    if args.alg not in ('sac', 'ctrlsac'):
        raise SystemExit(f'--seeds: seed batches are built for --alg sac and ctrlsac only (got --alg {args.alg}); run one process per seed instead')
    group_per = bool(getattr(args, 'group_per', False))
    group_cper = bool(getattr(args, 'group_critic_per', False))
    configs = parse_sweeps(args.sweep, args.alg, len(seeds), group_per=group_per or group_cper)
    swept = bool(args.sweep)
    tags = [t for t, _ in configs for _ in seeds]
    # per_alpha belongs to the members' replay trees, not to the agent: taken out of the members' hyper-parameters
    per_alphas = [float(cfg.get('per_alpha', getattr(args, 'per_alpha', 0.6))) for _, cfg in configs for _ in seeds]
    member_hyper = [{k: v for k, v in cfg.items() if k != 'per_alpha'} for _, cfg in configs for _ in seeds] if swept else None
    seeds = [s for _ in configs for s in seeds]              # member = (configuration, seed), configurations outermost
    pbt_cfg = parse_pbt(args, args.alg, len(seeds))
    halving_cfg = parse_halving(args, len(seeds), pbt_cfg)
    if args.device_env and not str(args.env).startswith(('Pendulum', 'MountainCarContinuous')):
        raise SystemExit(f'--device-env: only Pendulum-v1 and MountainCarContinuous-v0 are built on the device (got --env {args.env}); run without --device-env')
    from rlrep_amd.utils.buffer_group import ReplayBufferGroup, PrioritizedReplayBufferGroup, CriticPrioritizedReplayBufferGroup
    R = len(seeds)
    envs_, evals_ = [envs.make(args.env) for _ in seeds], [envs.make(args.env) for _ in seeds]
    for s, e, ev in zip(seeds, envs_, evals_):
        e.seed(s)
        ev.seed(s)
    rngs = [np.random.RandomState(s) for s in seeds]
    max_length = envs_[0]._max_episode_steps
    logs = []
    for tag, s in zip(tags, seeds):
        path = os.path.join(_log_root(args), *([tag] if swept else []), str(s))
        os.makedirs(path, exist_ok=True)
        logs.append(open(os.path.join(path, 'metrics.jsonl'), 'a'))
    space = envs_[0].action_space
    state_dim, action_dim = envs_[0].observation_space.shape[0], space.shape[0]
    lo, hi = np.asarray(space.low, np.float32), np.asarray(space.high, np.float32)
    common = dict(discount=args.discount, tau=args.tau, hidden_dim=args.hidden_dim, max_batch=args.batch_size)
    if args.alg == 'ctrlsac':
        common.update(feature_dim=2048, hidden_dim=1024, extra_feature_steps=args.extra_feature_steps)          # as build_agent (main.py:90-91)
    if (group_per or group_cper) and any('per_alpha' in cfg for _, cfg in configs):
        common['distinct_members'] = False          # (members that differ in per_alpha alone share a seed and the agent's hyper-parameters)
    agent = _group_class(args.alg)(seeds, state_dim, action_dim, space, member_hyper=member_hyper, **common)
    if group_per:
        replay = PrioritizedReplayBufferGroup(R, state_dim, action_dim, max_size=int(min(args.max_timesteps, 1e6)), alpha=per_alphas, beta=args.per_beta,
                                              **_nstep_kw(args))
    elif group_cper:
        replay = CriticPrioritizedReplayBufferGroup(R, state_dim, action_dim, max_size=int(min(args.max_timesteps, 1e6)), alpha=per_alphas,
                                                    beta=args.per_beta)
    else:
        replay = ReplayBufferGroup(R, state_dim, action_dim, max_size=int(min(args.max_timesteps, 1e6)), **_nstep_kw(args))
    agent.replay = replay                           # (what the members train from: for callers of run())
    ev = _GroupEvaluations(args, agent, seeds, logs, pbt_cfg, halving_cfg)
    if args.device_env:
        return _device_loop(args, agent, replay, ev)
    if args.host_envs > 1:
        return _host_envs_group_loop(args, agent, replay, ev, seeds)
    if _torch_envs_group(args):
        return _fused_sim_group_loop(args, agent, replay, ev, seeds)
    policies = [_MemberPolicy(agent, r) for r in range(R)]

    def evaluate():
        return [util.eval_policy(policies[r], evals_[r], args.eval_episodes) if ev.live[r] else None for r in range(R)]

    ev.evaluations = [[s] for s in evaluate()]
    states = np.stack([np.asarray(e.reset(), np.float32) for e in envs_])
    ep_steps = np.zeros(R, np.int64)
    infos = None
    staged = None                           # the rows of the last replay.add: a retired member's ring takes its last row again (nobody samples it)
    ev.timer = util.Timer()
    for t in range(int(args.max_timesteps)):
        ep_steps += 1
        live = ev.live
        greedy = None if t < args.start_timesteps else agent.select_action(states, explore=True)
        actions = np.zeros((R, action_dim), np.float32)
        for r in range(R):
            if not live[r]:
                continue
            if t < args.start_timesteps or rngs[r].uniform(0, 1) < EPS_GREEDY:
                actions[r] = rngs[r].uniform(lo, hi)
            else:
                actions[r] = greedy[r]
        nexts, rewards, dones = np.zeros_like(states), np.zeros(R, np.float32), np.zeros(R, np.float32)
        resets = []
        for r, e in enumerate(envs_):
            if not live[r]:
                continue
            ns, rew, done, _ = e.step(actions[r])
            nexts[r], rewards[r] = ns, rew
            dones[r] = float(done) if ep_steps[r] < max_length else 0.0
            if done:
                resets.append(r)
        for r in range(R):
            if not live[r]:
                states[r], actions[r], nexts[r], rewards[r], dones[r] = (a[r] for a in staged)
        replay.add(states, actions, nexts, rewards, dones)
        staged = (states, actions, nexts, rewards, dones)
        states = nexts.copy()
        for r in resets:
            states[r] = envs_[r].reset()
            ep_steps[r] = 0
        if t >= args.start_timesteps:
            infos = agent.train(replay, batch_size=args.batch_size)
        if (t + 1) % args.eval_freq == 0:
            ev.step(t + 1, evaluate, infos)
    ev.close()
    return agent, ev.evaluations


def _host_envs_group_loop(args, agent, replay, ev, seeds):
    """run_seeds' loop over E = --host-envs host environments per member (member r's environment i seeded seeds[r] + i): an iteration is ONE
    `select_actions` launch for all R x E observations, R x E `env.step`, one `add_batch` and one `train()` of every member.  Member r's
    generator draws its environments' random and epsilon-greedy actions in environment order; an evaluation steps min(E, --eval_episodes)
    environments per member, all members in lockstep, with one `select_actions` per step.  (No member retires here: --pbt-interval and
    --halving-interval are refused with --host-envs.)"""
    R, E, n_eval = agent.R, int(args.host_envs), min(int(args.host_envs), int(args.eval_episodes))
    envs_ = [_host_envs(args.env, s, E) for s in seeds]
    eval_envs = [e for s in seeds for e in _host_envs(args.env, s, n_eval)]
    rngs = [np.random.RandomState(s) for s in seeds]
    space = envs_[0][0].action_space
    max_length = envs_[0][0]._max_episode_steps
    lo, hi = np.asarray(space.low, np.float32), np.asarray(space.high, np.float32)
    obs_eval = np.zeros((R, E, agent.state_dim), np.float32)
    counts = [len(range(i, int(args.eval_episodes), n_eval)) for _ in seeds for i in range(n_eval)]

    def evaluate():
        def act(obs, active):
            obs_eval[:, :n_eval] = obs.reshape(R, n_eval, -1)
            return agent.select_actions(obs_eval)[:, :n_eval].reshape(R * n_eval, -1)
        per_env = util.lockstep_rollouts(act, eval_envs, counts)
        return [float(np.mean([x for env_returns in per_env[r * n_eval:(r + 1) * n_eval] for x in env_returns])) for r in range(R)]

    ev.evaluations = [[s] for s in evaluate()]
    states = np.stack([[np.asarray(e.reset(), np.float32) for e in member] for member in envs_])
    ep_steps = np.zeros((R, E), np.int64)
    infos = None
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), E):             # one iteration is E environment steps of every member
        ep_steps += 1
        warm = t0 < args.start_timesteps
        greedy = None if warm else agent.select_actions(states, explore=True)
        actions = np.zeros((R, E, agent.action_dim), np.float32)
        for r in range(R):
            for i in range(E):
                actions[r, i] = rngs[r].uniform(lo, hi) if warm or rngs[r].uniform(0, 1) < EPS_GREEDY else greedy[r, i]
        nexts, rewards, dones = np.zeros_like(states), np.zeros((R, E), np.float32), np.zeros((R, E), np.float32)
        resets = []
        for r in range(R):
            for i, e in enumerate(envs_[r]):
                nexts[r, i], rewards[r, i], done, _ = e.step(actions[r, i])
                dones[r, i] = float(done) if ep_steps[r, i] < max_length else 0.0
                if done:
                    resets.append((r, i))
        replay.add_batch(states, actions, nexts, rewards, dones)
        states = nexts
        for r, i in resets:
            states[r, i] = envs_[r][i].reset()
            ep_steps[r, i] = 0
        if not warm:
            infos = agent.train(replay, batch_size=args.batch_size)
        t = t0 + E
        if t % args.eval_freq == 0:
            ev.step(t, evaluate, infos)
    ev.close()
    return agent, ev.evaluations


def _fused_sim_group_loop(args, agent, replay, ev, seeds):
    """run_seeds' loop with --torch-envs N --sim-graph --fused-sim: N fused environments per member (envs/fused_sim.py FusedSimGroup, member
    r's start states keyed by its seed), an iteration is ONE `iterate_sim` graph replay of every member -- the act launch with the exploration
    mix, the step-and-append launch, train().  --start_timesteps counts steps per member.  An evaluation steps min(N, --eval_episodes)
    environments per member on a FusedSimGroup(auto_restart=False) with the group's act_device(explore=False) and reports one mean return per
    member from last_return; none is made before the first step, as in the single agent's loop.  (No member retires here: --pbt-interval and
    --halving-interval are refused with --torch-envs.)"""
    from rlrep_amd.envs.fused_sim import FusedSimGroup
    from rlrep_amd.envs.sim_loop import SimLoopGroup
    R, N, dev, episodes = agent.R, int(args.torch_envs), replay.device, int(args.eval_episodes)
    n_eval = min(N, episodes)
    env = FusedSimGroup(args.env, R, N, dev, seeds=seeds, group=agent)
    eval_env = FusedSimGroup(args.env, R, n_eval, dev, seeds=[s + 100 for s in seeds], auto_restart=False, group=agent)
    env.reset()
    loop = SimLoopGroup(agent, env, eps_greedy=EPS_GREEDY, start_timesteps=int(args.start_timesteps))
    act = torch.zeros(R, n_eval, env.action_dim, dtype=torch.float32, device=dev)

    def evaluate():
        returns = [[] for _ in range(R)]
        while len(returns[0]) < episodes:               # every round resets first, so it draws fresh start states
            eval_env.reset()
            for _ in range(eval_env._max_episode_steps):
                eval_env.step_(agent.act_device(eval_env.obs, explore=False, out=act))
            for r, row in enumerate(eval_env.last_return.cpu().tolist()):
                returns[r].extend(row)
        finished = int(env.episodes.sum())
        if finished:
            print(f'Total T: {loop.t_global} Episode Num: {finished} Mean reward: {float(torch.nanmean(env.last_return)):.3f}')
        return [float(np.mean(returns[r][:episodes])) for r in range(R)]

    ev.evaluations = [[] for _ in range(R)]
    infos = None
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), N):             # one iteration is N environment steps of every member
        out = agent.iterate_sim(loop, replay, args.batch_size, train=t0 >= args.start_timesteps)
        infos = out if out is not None else infos
        t = t0 + N
        if t % args.eval_freq == 0:
            ev.step(t, evaluate, infos)
    ev.close()
    return agent, ev.evaluations


def _device_loop(args, agent, replay, ev):
    """run_seeds' loop with the environments on the device (--device-env): one `agent.iterate` per step -- act, explore, step, ring row and
    train() of every live member in one graph replay -- and one `agent.evaluate` launch per evaluation.  The exploration and reset draws are
    Philox streams of the members' seeds instead of NumPy generators, and an evaluation's start states are a function of (seed, evaluation
    index, episode); the metrics.jsonl / pbt.jsonl / halving.jsonl rows keep their keys."""
    from rlrep_amd.envs.device import device_class
    E = int(args.num_envs)
    env = device_class(args.env)(agent, eps_greedy=EPS_GREEDY, start_timesteps=int(args.start_timesteps), num_envs=E)

    def evaluate():
        return [float(s) for s in agent.evaluate(env, args.eval_episodes)]

    ev.evaluations = [[s] for s in evaluate()]
    infos = None
    ev.timer = util.Timer()
    for t0 in range(0, int(args.max_timesteps), E):            # one iterate is E environment steps of every live member
        out = agent.iterate(env, replay, args.batch_size, train=t0 >= args.start_timesteps)
        infos = out if out is not None else infos
        t = t0 + E - 1
        if (t + 1) % args.eval_freq == 0:
            ev.step(t + 1, evaluate, infos, env=env)
    ev.close()
    return agent, ev.evaluations


if __name__ == '__main__':
    run()
