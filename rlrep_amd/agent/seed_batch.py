"""What a seed batch does whatever its algorithm: R independent agents -- one per seed -- trained by the SAME launches.

Nobody reports an RL result from one seed; a single B = 256 agent leaves most of the MI355X idle between its launches.  A seed batch lays R
agents of identical shape out at a constant byte stride in ONE allocation (include/rlrep.h rlrep_group_create): the step programs are built
once, against member 0, and every launch of a train() runs all members (member = grid y, every pointer moved by member * stride).  So R seeds
cost one train() graph of exactly one agent's launch count, not R of them.

SeedBatchMixin goes in front of the standalone agent class (SACSeedBatch(SeedBatchMixin, SACAgent), CTRLSACSeedBatch(SeedBatchMixin,
CTRLSACAgent)): member cores, the train() pools inside the member block, the group train prologue, select_action for every member in one
launch (select_actions: for E observations per member), member export and checkpoints.  Initialisation rule: member r is initialised exactly as `torch.manual_seed(seeds[r]); Agent(...,
seed=seeds[r])` initialises, and draws its sample indices and noise from the Philox stream of seed seeds[r].

Sweeps: `member_hyper=[dict, ...]` (one dict per member) lets members differ in the hyper-parameters no launch's shape depends on (SWEEP_KEYS:
lr, discount, tau, alpha, target_update_period, auto_entropy_tuning; ctrlsac also feature_tau).  The constructor kwargs are the shared
defaults; member r is then `torch.manual_seed(seeds[r]); Agent(..., seed=seeds[r], **defaults, **member_hyper[r])`.  Seeds may repeat as long
as the (seed, hyper) pairs are distinct.  Everything else -- dimensions, extra_feature_steps, use_feature_target, max_batch -- is structural:
shared by every member and refused in a member dict.

Population-based training: `clone_members([(src, dst), ...])` makes member dst a copy of member src on the device, in one launch (exploit),
and `set_member_hyper(r, lr=...)` retunes a live member (explore); both leave the captured train() graph as it is.  A cloned member keeps its
own hyper-parameters, seed, replay ring and metric history.  rlrep_amd/agent/pbt.py plans who copies whom; `lineage` records what happened.

Successive halving: `retire_members([r, ...])` takes members out of every launch (include/rlrep.h rlrep_group_set_live: the workgroups of a
retired member return at once; grid y and the captured graph stay) and `revive_members` puts them back.  A retired member's state is frozen, not
gone: member(r), member_snapshot(r), set_member_hyper(r) and clone_members work on it, so "clone a winner into a retired slot, perturb, revive"
respawns it.  train() returns None in its place, select_action a row of zeros.  pbt.plan_halving plans who goes.
"""
import contextlib
import ctypes as C
import inspect
import math
import os

import numpy as np
import torch

from rlrep_amd._lib import lib, check
from rlrep_amd.core import HipCore, _stream
from rlrep_amd.agent.sac.sac_agent import ArenaModule, SELECT_MAX_ROWS, ACT_MAX_ROWS
from rlrep_amd.utils import switches as _sw


class _MemberCore(HipCore):
    """Member r's view of a group core: the arenas, device records and metric history of its block (no handle of its own)."""

    def __init__(self, group, r):                   # (HipCore.__init__ is not run: nothing is allocated or created)
        self.__dict__.update({k: v for k, v in group.__dict__.items() if not k.startswith('_hist') and k not in ('_mt',)})
        self._group, self._r, self._delta = group, r, r * group.member_stride
        base = group._skew + self._delta

        def carve(i, dtype):
            o = base + self._offs[i]
            return group._block[o:o + self._sizes[i]].view(dtype)
        self.params, self.targets, self.grads = carve(0, torch.float32), carve(1, torch.float32), carve(2, torch.float32)
        self.exp_avg, self.exp_avg_sq = carve(3, torch.float32), carve(4, torch.float32)
        self.workspace, self.alpha_state = carve(5, torch.uint8), carve(6, torch.float64)
        self._metrics_ptr = group._metrics_ptr + self._delta

    def __del__(self):
        pass

    def _ws_off(self, member0_ptr):
        return member0_ptr - self._group.workspace.data_ptr()

    def sync_step_mirror(self):
        off = self._ws_off(lib.rlrep_steps_dev(self.h))
        w = self.workspace[off:off + 32].view(torch.int32)
        w[2] = w[0]

    def group_cfg(self):
        off = self._ws_off(lib.rlrep_group_cfg_dev(self.h))
        return self.workspace[off:off + 4 * 22 * 4].view(torch.float32).view(4, 22)

    def _history_views(self):
        if not hasattr(self, '_hist'):
            ring, seq, cap, tag = self._group._history_views()
            o_r, o_q = self._ws_off(ring.data_ptr()), self._ws_off(seq.data_ptr())
            r = self.workspace[o_r:o_r + ring.numel() * 4].view(torch.float32).view(*ring.shape)
            q = self.workspace[o_q:o_q + 4].view(torch.int32)
            self._hist = (r, q, cap, tag)
        return self._hist


class _Member(object):
    """What `<Alg>SeedBatch.member(r)` returns: the reference's module attributes of member r, views into its block."""

    def __init__(self, core, modules):
        self.core = core
        for m in modules:
            setattr(self, m, ArenaModule(core, m))

    @property
    def log_alpha(self):
        return self.core.alpha_state[0]

    @property
    def alpha(self):
        return self.core.alpha_state[0].exp()


class SeedBatchMixin(object):
    """SeedBatchMixin + Agent: one agent per seed, trained together.  `train(buffers, batch_size)` takes a ReplayBufferGroup
    (rlrep_amd/utils/buffer_group.py) -- member r samples ring r -- and returns a list of R info dicts.  The single-GPU whole-train() graph is
    the only form (no data parallel, no eager steps)."""

    # constructor kwargs a member may override (member_hyper): what the group launches read per member (include/rlrep.h
    # rlrep_group_set_member_hyper) or what only initialisation uses (alpha)
    SWEEP_KEYS = ('lr', 'discount', 'tau', 'alpha', 'target_update_period', 'auto_entropy_tuning')
    PREFETCH_POLICY_EARLY = False         # no group form of rlrep_prefetch_policy_early (the library refuses it)
    SEED_GROUP = True                     # (SACAgent._check_critic_nstep: n-step critic targets are built for one agent)

    @classmethod
    def _agent_class(cls):
        mro = cls.__mro__
        return mro[mro.index(SeedBatchMixin) + 1]

    @classmethod
    def sweep_defaults(cls):
        """{key: the standalone agent's default} for every SWEEP_KEYS entry"""
        sig = inspect.signature(cls._agent_class().__init__)
        return {k: sig.parameters[k].default for k in cls.SWEEP_KEYS}

    @classmethod
    def normalise_hyper(cls, key, value, who=None):
        """value of a sweepable key as the agent stores it; ValueError (naming `who` and the key) when it is not one the library accepts"""
        who = who or cls.__name__
        try:
            if key == 'target_update_period':
                if isinstance(value, float) and not value.is_integer():
                    raise ValueError
                v = int(value)
                ok = v >= 1
            elif key == 'auto_entropy_tuning':
                if isinstance(value, str):
                    if value.lower() not in ('0', '1', 'true', 'false'):
                        raise ValueError
                    value = value.lower() in ('1', 'true')
                v, ok = bool(value), True
            else:
                v = float(value)
                ok = math.isfinite(v) and {'lr': v > 0, 'alpha': v > 0, 'tau': 0 <= v <= 1, 'feature_tau': 0 <= v <= 1}.get(key, True)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            need = {'lr': 'a finite positive number', 'alpha': 'a finite positive number', 'tau': 'a number in [0, 1]',
                    'feature_tau': 'a number in [0, 1]', 'target_update_period': 'an integer >= 1', 'discount': 'a finite number',
                    'auto_entropy_tuning': 'a boolean'}[key]
            raise ValueError(f'{who}: {key}={value!r} is not valid ({key} must be {need})')
        return v

    @classmethod
    def member_hypers(cls, seeds, kwargs, member_hyper, distinct=True):
        """Each member's sweepable hyper-parameters (dicts in SWEEP_KEYS order), checked before anything touches the GPU."""
        name = cls.__name__
        defaults = cls.sweep_defaults()
        base = {k: cls.normalise_hyper(k, kwargs.get(k, defaults[k])) for k in cls.SWEEP_KEYS}
        if member_hyper is None:
            return [dict(base) for _ in seeds]
        member_hyper = list(member_hyper)
        if len(member_hyper) != len(seeds):
            raise ValueError(f'{name}: member_hyper has {len(member_hyper)} entries for {len(seeds)} seeds (one dict per member)')
        structural = set(inspect.signature(cls._agent_class().__init__).parameters) - set(cls.SWEEP_KEYS) - {'self', '_hip'}
        out = []
        for r, mh in enumerate(member_hyper):
            if not isinstance(mh, dict):
                raise ValueError(f'{name}: member_hyper[{r}] is not a dict')
            for k in mh:
                if k in cls.SWEEP_KEYS:
                    continue
                if k in structural or k in ('max_batch', 'seed', 'pipeline', 'graph'):
                    raise ValueError(f'{name}: member_hyper[{r}][{k!r}] is structural (shared by every member of a group): pass it to the constructor')
                raise ValueError(f'{name}: member_hyper[{r}] has unknown key {k!r} (sweepable: {", ".join(cls.SWEEP_KEYS)})')
            h = dict(base)
            h.update({k: cls.normalise_hyper(k, v, f'{name}: member_hyper[{r}]') for k, v in mh.items()})
            out.append(h)
        seen = {}
        for r, (s, h) in enumerate(zip(seeds, out) if distinct else ()):
            key = (s, tuple(h.items()))
            if key in seen:
                raise ValueError(f'{name}: members {seen[key]} and {r} have the same seed {s} and the same hyper-parameters (duplicate (seed, hyper) pair)')
            seen[key] = r
        return out

    def __init__(self, seeds, state_dim, action_dim, action_space, member_hyper=None, **kwargs):
        name = type(self).__name__
        self.seeds = [int(s) for s in seeds]
        if not self.seeds:
            raise ValueError(f'{name}: at least one seed')
        if member_hyper is None and len(set(self.seeds)) != len(self.seeds):
            raise ValueError(f'{name}: seeds must be distinct')
        kwargs = dict(kwargs)
        # distinct_members=False: members may share (seed, hyper-parameters) -- they differ in something the agent does not see, the priority
        # exponents of their replay trees (PrioritizedReplayBufferGroup)
        distinct = bool(kwargs.pop('distinct_members', True))
        self._mhyper = self.member_hypers(self.seeds, kwargs, member_hyper, distinct=distinct)
        self._swept = member_hyper is not None
        self.lineage = []                       # one record per clone / retune (clone_members, set_member_hyper); checkpoints carry it
        self.R = len(self.seeds)
        self._live = [True] * self.R            # retire_members / revive_members; checkpoints carry it
        kwargs = dict(kwargs)
        kwargs.pop('seed', None)
        kwargs['seed'] = self.seeds[0]
        kwargs.update(self._mhyper[0])          # the group is created with member 0's values; the others' go in right after (_make_core)
        super().__init__(state_dim, action_dim, action_space, **kwargs)
        if self.world_size > 1 or self._dp or not self.use_graph:
            raise RuntimeError(f'{name}: a seed group runs the single-GPU whole-train() graph only')
        self.world_size = 1
        seeds_arr = (C.c_uint64 * self.R)(*self.seeds)
        check(lib.rlrep_group_set_seeds(self.core.h, C.cast(seeds_arr, C.c_void_p), self.R, _stream()), 'group_set_seeds')

    # ---- construction -----------------------------------------------------------------------------------------------------------------
    def _make_core(self, dims, hyper):
        ni, ne = self._pool_sizes(self.max_batch)
        # the index and noise pools of a train() sit behind the arenas of every member: the prologue writes member r's at the member stride
        core = HipCore(self.ALG, dims, hyper, members=len(self.seeds), member_extra_bytes=4 * (ni + ne) + 512)
        if self._swept:
            for r in range(len(self.seeds)):
                h = self._hyper_struct(core, self._mhyper[r])
                check(lib.rlrep_group_set_member_hyper(core.h, r, C.byref(h), _stream()), 'group_set_member_hyper')
        return core

    def _hyper_struct(self, core, hp):
        """the library's hyper record of a member with sweepable values `hp`, the group's structural fields unchanged (as _finish_init
        builds a standalone agent's)"""
        h = type(core.hyper).from_buffer_copy(core.hyper)
        for k, v in self._lr_hyper(hp['lr']).items():
            setattr(h, k, float(v))
        h.discount, h.tau = hp['discount'], hp['tau']
        if 'feature_tau' in hp:
            h.feature_tau = hp['feature_tau']
        h.target_update_period, h.learn_alpha = hp['target_update_period'], int(hp['auto_entropy_tuning'])
        return h

    def member_hyper(self, r):
        """member r's sweepable hyper-parameters: `Agent(..., seed=seeds[r], **member_hyper(r))` (with the group's other kwargs) is its
        standalone twin"""
        return dict(self._mhyper[r])

    def _check_member(self, where, r, named=None):
        """ValueError naming `where` unless 0 <= r < R; `named`: what the message says instead of 'member r'"""
        if not 0 <= r < self.R:
            raise ValueError(f'{where}: {named or f"member {r}"} outside [0, {self.R})')

    # ---- population-based training: exploit (clone) and explore (retune) between two train() calls ---------------------------------------
    def clone_members(self, pairs):
        """pairs = [(src, dst), ...]: member dst becomes member src -- parameters, targets, Adam moments and step counts, temperature state,
        train() counter -- in ONE launch on the current stream (include/rlrep.h rlrep_group_clone_members).  dst keeps its hyper-parameters,
        seed, replay ring and metric history (info dicts returned earlier stay valid); the captured train() graph is kept.  No member may be
        both a source and a destination, no destination may repeat."""
        name = type(self).__name__
        try:
            pairs = [(int(s), int(d)) for s, d in pairs]
        except (TypeError, ValueError):
            raise ValueError(f'{name}.clone_members: pairs must be a list of (src, dst) member indices')
        if not 1 <= len(pairs) <= self.R:
            raise ValueError(f'{name}.clone_members: {len(pairs)} pairs outside [1, {self.R}]')
        for s, d in pairs:
            for r in (s, d):
                self._check_member(f'{name}.clone_members', r, f'pair ({s}, {d}) names a member')
            if s == d:
                raise ValueError(f'{name}.clone_members: pair ({s}, {d}) copies member {s} onto itself')
        dsts = [d for _, d in pairs]
        for d in dsts:
            if dsts.count(d) > 1:
                raise ValueError(f'{name}.clone_members: member {d} is a destination twice')
        both = sorted(set(dsts) & {s for s, _ in pairs})
        if both:
            raise ValueError(f'{name}.clone_members: member {both[0]} is both a source and a destination')
        n = len(pairs)
        src, dst = (C.c_int32 * n)(*[s for s, _ in pairs]), (C.c_int32 * n)(*dsts)
        check(lib.rlrep_group_clone_members(self.core.h, src, dst, n, _stream()), 'group_clone_members')
        for s, d in pairs:
            self.lineage.append({'train_calls': int(self.steps), 'kind': 'clone', 'members': [s, d], 'old': None, 'new': None})

    def set_member_hyper(self, r, **kw):
        """Retune live member r: keys from SWEEP_KEYS but `alpha` (the INITIAL temperature: it has no meaning for a member that is already
        training).  The member's device words change (rlrep_group_set_member_hyper); the captured graph reads them at its next replay."""
        name = type(self).__name__
        r = int(r)
        self._check_member(f'{name}.set_member_hyper', r)
        for k in kw:
            if k == 'alpha':
                raise ValueError(f'{name}.set_member_hyper: alpha is the initial temperature only (a live member\'s temperature is its '
                                 'alpha_state, which training owns); it cannot be retuned')
            if k not in self.SWEEP_KEYS:
                raise ValueError(f'{name}.set_member_hyper: unknown key {k!r} (retunable: {", ".join(k for k in self.SWEEP_KEYS if k != "alpha")})')
        new = {k: self.normalise_hyper(k, v, f'{name}.set_member_hyper') for k, v in kw.items()}
        self._apply_member_hyper(r, new)

    # ---- successive halving: members leave and re-enter the launches between two train() calls ------------------------------------------------
    @property
    def live(self):
        """[R] booleans: False for a retired member"""
        return list(self._live)

    def retire_members(self, members):
        """Members `members` leave every launch from the next train() / select_action on: nothing of theirs is read or written until they are
        revived (their step counters stand still, so a revived member draws what it would have drawn next).  At least one member stays live.
        At most ONE launch on the current stream (the live table); the captured train() graph is kept."""
        self._set_live(members, False)

    def revive_members(self, members):
        """Retired members `members` rejoin the launches, with the state they were retired with (or were given since: clone_members,
        set_member_hyper)."""
        self._set_live(members, True)

    def _set_live(self, members, on):
        what = 'revive_members' if on else 'retire_members'
        name = f'{type(self).__name__}.{what}'
        try:
            members = [int(r) for r in members]
        except (TypeError, ValueError):
            raise ValueError(f'{name}: members must be a list of member indices')
        if not members:
            raise ValueError(f'{name}: no member named')
        live = list(self._live)
        for r in members:
            self._check_member(name, r)
            if members.count(r) > 1:
                raise ValueError(f'{name}: member {r} is named twice')
            if live[r] == on:
                raise ValueError(f'{name}: member {r} is ' + ('live already' if on else 'retired already'))
            live[r] = on
        if not any(live):
            raise ValueError(f'{name}: members {members} are the last live members (at least one member of a group stays live)')
        self._upload_live(live)
        self.lineage.append({'event': 'revive' if on else 'retire', 'kind': 'revive' if on else 'retire', 'members': list(members),
                             'step': int(self.steps)})

    def _upload_live(self, live):
        mask = (C.c_int32 * self.R)(*[1 if v else 0 for v in live])
        check(lib.rlrep_group_set_live(self.core.h, mask, _stream()), 'group_set_live')          # (refuses a call inside a train())
        self._live = [bool(v) for v in live]
        if _sw.opt('grp_compact'):              # (measured, not adopted: grid y = the live members, so the graph is captured again)
            self._graph = None

    def _apply_member_hyper(self, r, new):
        old = self.member_hyper(r)
        hp = dict(old)
        hp.update(new)
        check(lib.rlrep_group_set_member_hyper(self.core.h, r, C.byref(self._hyper_struct(self.core, hp)), _stream()), 'group_set_member_hyper')
        self._mhyper[r] = hp
        self._swept = True
        self.lineage.append({'train_calls': int(self.steps), 'kind': 'retune', 'members': [r], 'old': {k: old[k] for k in new}, 'new': dict(new)})

    def _init_parameters(self):
        group = self.core
        self._members = [_MemberCore(group, r) for r in range(self.R)]
        saved = torch.random.get_rng_state()
        try:
            for r, s in enumerate(self.seeds):
                torch.manual_seed(s)
                self.core = self._members[r]
                super()._init_parameters()
                self.core.alpha_state[0] = float(np.log(self._mhyper[r]['alpha']))
        finally:
            self.core = group
            torch.random.set_rng_state(saved)
        self._member_views = [_Member(m, self.MODULES) for m in self._members]

    # ---- pools inside the member block ------------------------------------------------------------------------------------------------
    def _buf(self, key, shape, dtype=torch.float32):
        if key not in ('pool_idx', 'pool_eps'):
            return super()._buf(key, shape, dtype)
        n = int(np.prod(shape))
        ni, _ = self._pool_sizes(self.max_batch)
        c = self.core
        off = c._skew + c.member_extra_offset + (0 if key == 'pool_idx' else ((4 * ni + 255) & ~255))
        return c._block[off:off + 4 * n].view(dtype).view(*shape)

    def _draw_pools(self, buffer, B, g, ipool, epool):
        if not g:
            raise RuntimeError(f'{type(self).__name__}: eager train() forms are not built for seed groups')
        check(lib.rlrep_group_train_prologue(self.core.h, C.c_void_p(buffer.ring.data_ptr()), 4 * buffer.ring_stride, C.c_void_p(buffer.size_dev().data_ptr()),
                                             C.c_void_p(ipool.data_ptr()), ipool.numel(), C.c_void_p(epool.data_ptr()), epool.numel(),
                                             1 << 40, 2 << 40, B, _stream()),
              'group_train_prologue')

    def _sample_into(self, buffer, B, key, slot=0, g=False):
        if key == 'warm':
            # a standalone agent gathers one eager minibatch before its first capture: it sizes the programs for B outside the capture and
            # draws one index set from the host counter.  A group has no eager gather: it sizes its programs and keeps the counter in step
            check(lib.rlrep_group_prepare(self.core.h, int(B)), 'group_prepare')
            self._ctr += 1
            return
        return super()._sample_into(buffer, B, key, slot, g)

    def _gather(self, buffer, slot, idx, B):
        """An n-step buffer group: the chain-following gather of every live member, behind the prologue's own (which it overwrites), on the
        members' index pools; member r's discount is its hyper record's.  A plain group: the prologue's gather (the call is recognised)."""
        n = self._nstep(buffer)
        if n <= 1:
            return super()._gather(buffer, slot, idx, B)
        self._gather_nstep(buffer, idx, B, per_member=False)

    def _gather_nstep(self, buffer, idx, B, per_member):
        check(lib.rlrep_group_replay_gather_nstep(self.core.h, C.c_void_p(buffer.rings.data_ptr()), 4 * buffer.ring_stride, C.c_void_p(idx.data_ptr()),
                                                  1 if per_member else 0, int(B), buffer.max_size, C.c_void_p(buffer.size_dev().data_ptr()),
                                                  self._nstep(buffer), buffer.n_stride, _stream()), 'group_replay_gather_nstep')

    @staticmethod
    def _graph_cache_key(buffer, B):
        key = (buffer.rings.data_ptr(), buffer.size_dev().data_ptr(), int(buffer.max_size), buffer.members, B)
        per = getattr(buffer, 'per_key', None)               # (a prioritized buffer group: its trees and scalar block are baked in as well)
        key = key if per is None else key + per()
        if int(getattr(buffer, 'n_step', 1)) > 1:
            key = key + buffer.nstep_key()
        return key

    # ---- prioritized replay (utils/buffer_group.py PrioritizedReplayBufferGroup) ---------------------------------------------
    @staticmethod
    def _per(buffer):
        return bool(getattr(buffer, 'prioritized_group', False))

    def _check_per(self, buffer, what):
        """A prioritized buffer GROUP trains a sac seed group through train(); everything else refuses it by its class name, before
        anything is launched.  (The single ring's class is refused by _refuse_per / SACAgent._check_per, as before.)"""
        if not self._per(buffer):
            return super()._check_per(buffer, what)
        name, cls = type(self).__name__, type(buffer).__name__
        self._check_nstep(buffer, what)
        if self.ALG != 'sac':
            raise RuntimeError(f'{name}.{what}: {cls} is built for SACSeedBatch only ({self.ALG} reuses its last feature minibatch for the critic '
                               'step; what prioritisation means there is open): use a plain ReplayBufferGroup -- or, to prioritise that '
                               'minibatch alone, a CriticPrioritizedReplayBufferGroup')
        if what == 'iterate':
            raise RuntimeError(f'{name}.iterate: {cls} cannot be written by a device environment (its step launch knows nothing of the priority '
                               'trees): use a plain ReplayBufferGroup')
        if what == 'train_injected':
            raise RuntimeError(f'{name}.train_injected: a seed group has no eager train() form; given indices go through {cls}.draw(given=...)')

    # ---- prioritized replay of the critic's minibatch (utils/buffer_group.py CriticPrioritizedReplayBufferGroup) ---------------
    @staticmethod
    def _cper(buffer):
        """the single ring's class (which _check_critic_per goes on refusing for a seed group) or the buffer group's"""
        return bool(getattr(buffer, 'critic_prioritized', False) or getattr(buffer, 'critic_prioritized_group', False))

    def _check_critic_per(self, buffer, what):
        """A CriticPrioritizedReplayBufferGroup trains a ctrlsac seed group through train() and prepare(); everything else refuses it by its
        class name, before anything is launched.  (The single ring's class is refused as before.)"""
        if not getattr(buffer, 'critic_prioritized_group', False):
            return super()._check_critic_per(buffer, what)
        name, cls = type(self).__name__, type(buffer).__name__
        if self.ALG != 'ctrlsac':
            raise RuntimeError(f'{name}.{what}: {cls} is built for CTRLSACSeedBatch only (a {self.ALG} seed group owns its whole minibatch): use '
                               'PrioritizedReplayBufferGroup')
        if what in ('iterate', 'iterate_sim'):
            raise RuntimeError(f'{name}.{what}: {cls} cannot be written by a device environment or a captured simulator loop (their launches know '
                               'nothing of the priority trees): use a plain ReplayBufferGroup')
        if what == 'train_injected':
            raise RuntimeError(f'{name}.train_injected: a seed group has no eager train() form; given indices go through {cls}.draw_fill(given=...)')
        if what not in ('train', 'prepare'):
            raise RuntimeError(f'{name}.{what}: {cls} trains a ctrlsac seed group through train() and prepare() only')

    def _before_capture(self, buffer, B, train=True):
        """The draw buffers of a CriticPrioritizedReplayBufferGroup are allocated OUTSIDE the capture: allocated inside it, their zero / one
        fills would be nodes of the graph and every replay would reset the rows of a retired member, which must stand still."""
        if train and getattr(buffer, 'critic_prioritized_group', False):
            buffer.draw_buffers(B)
        super()._before_capture(buffer, B, train)

    def _sample_into_critic_per(self, buffer, B, key, g):
        """The minibatch the critic reuses, of every live member from its own tree: ONE launch draws the indices and the importance weights
        into the buffer group's draw buffers and gathers the drawn rows into the members' slot 0 (rlrep_group_per_sample_fill) -- in front of
        the last feature step, where the single agent makes it, followed by the early policy prefetch where a group has one."""
        if not g or self._inject is not None:
            raise RuntimeError(f'{type(self).__name__}: eager train() forms are not built for seed groups')
        idx, _ = buffer.draw_fill(self.core, B, self.PER_STREAM, use_counter=True)
        self._bufs['idx_' + key] = idx
        if self._pool is not None and key == self._early_key:
            self.core.prefetch_policy_early(self._pool['eps_crit'], self._pool['eps_act'])

    def _sample_into_per(self, buffer, B, key, g):
        """The minibatch of every live member from its own tree: one launch draws the indices and the importance weights into the buffer
        group's draw buffers, a second gathers the drawn rows into the members' slots (rlrep_group_per_sample issues both)."""
        if not g or self._inject is not None:
            raise RuntimeError(f'{type(self).__name__}: eager train() forms are not built for seed groups')
        nstep = self._nstep(buffer) > 1          # (the n-step gather replaces the sampler's plain one: the launch count stays)
        idx, _ = buffer.draw(B, self.PER_STREAM, core=self.core, use_counter=True, gather=not nstep)
        self._bufs['idx_' + key] = idx
        if nstep:
            self._gather_nstep(buffer, idx, B, per_member=True)

    # ---- surface ----------------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _history_capture(self):
        with super()._history_capture():
            yield
        # members file their records in rings of their own, and a retired member's ring stands still: one record count per member
        self._mhist_n = [m.history_seq() for m in self._members] if self._hist else [0] * self.R

    def _refuse_per(self, buffers, what):
        if getattr(buffers, 'prioritized', False):
            raise RuntimeError(f'{type(self).__name__}.{what}: {type(buffers).__name__} is built for one SACAgent on one GPU; a seed group samples '
                               'its members\' rings uniformly (ReplayBufferGroup)')

    def train(self, buffers, batch_size):
        """One train() of every live member: ONE graph replay.  Returns R entries (member order): an info dict, fetched when read, or None for
        a retired member."""
        self._refuse_per(buffers, 'train')
        self._check_per(buffers, 'train')
        if getattr(buffers, 'members', None) != self.R:
            raise ValueError(f'{type(self).__name__}.train: needs a ReplayBufferGroup of {self.R} members')
        self.steps += 1
        return self._train_graph(buffers, batch_size)

    update = train

    # ---- device environments (rlrep_amd/envs/device.py): collect, train and score without a host round trip -------------------------------
    def iterate(self, env, buffers, batch_size, train=True):
        """One environment step of every live member on the device -- act, explore, step the dynamics, write the ring row
        (rlrep_group_env_step) -- and, with `train`, one train() of every live member on the rings as they then stand: ONE graph replay, no host
        round trip.  `env` is a DeviceEnvGroup (envs/device.py) of this group, `buffers` a ReplayBufferGroup whose cursor the device owns from here on
        (ReplayBufferGroup.adopt_device_cursor gives it back).  Returns what train() returns, or None without `train`.  The step's exploring
        draw is the one `select_action(states, explore=True)` would make now: both count calls in the same counter."""
        self._refuse_per(buffers, 'iterate')
        self._check_per(buffers, 'iterate')
        name = type(self).__name__
        if getattr(buffers, 'members', None) != self.R:
            raise ValueError(f'{name}.iterate: needs a ReplayBufferGroup of {self.R} members')
        if getattr(env, 'agent', None) is not self:
            raise ValueError(f'{name}.iterate: the device environment belongs to another group')
        return self._iterate(env, buffers, batch_size, train, lambda: env.step(buffers, env.eps_greedy, env.start_timesteps), '_iter')

    # ---- simulators on the device (rlrep_amd/envs/sim_loop.py SimLoopGroup): the whole iteration of every live member as one graph replay ---
    def iterate_sim(self, loop, buffers, batch_size, train=True):
        """One iteration of the loop around a simulator of R x N environments on the device -- act on every live member's N observations and
        mix in its exploring uniform actions (rlrep_group_act_device_ctl), step the simulator, append every live member's N transitions to its
        own ring (rlrep_group_replay_add_cols_ctl; with envs/fused_sim.py FusedSimGroup the step does the append: two launches in all) --
        and, with `train`, one train() of every live member on the rings as they then stand: ONE graph replay, no host round trip.  `loop` is
        a SimLoopGroup of this group, `buffers` a ReplayBufferGroup whose cursor the device owns from here on.  Returns what train() returns,
        or None without `train`.  Member r is bit for bit SACAgent(seed=seeds[r]).iterate_sim on a SimLoop of its own; retire_members /
        revive_members keep the captured graph, and a retired member's ring, cursor and simulator planes stand still.  An n-step buffer
        group (sac) needs n_stride = N.  Not for the prioritized buffer groups (the captured append does not write the priority trees)."""
        name, cls = type(self).__name__, type(buffers).__name__
        self._refuse_per(buffers, 'iterate_sim')
        if self._per(buffers) or getattr(buffers, 'critic_prioritized_group', False):
            raise RuntimeError(f'{name}.iterate_sim: {cls} cannot be written by the captured simulator loop (its append launch does not write the '
                               'priority trees): use a plain ReplayBufferGroup, or the eager act_device / add_device / train() loop')
        self._check_per(buffers, 'iterate_sim')         # (n-step rows: refused for a ctrlsac group, as iterate refuses them)
        if (getattr(buffers, 'members', None) != self.R
                or (getattr(buffers, 'state_dim', None), getattr(buffers, 'action_dim', None)) != (self.state_dim, self.action_dim)):
            raise ValueError(f'{name}.iterate_sim: needs a ReplayBufferGroup of {self.R} members, {self.state_dim} observations and {self.action_dim} actions')
        if getattr(loop, 'agent', None) is not self or getattr(loop, 'R', None) != self.R:
            raise ValueError(f'{name}.iterate_sim: the simulator loop belongs to another group')
        N = int(loop.num_envs)
        if N > buffers.max_size:
            raise ValueError(f'{name}.iterate_sim: {N} environments for rings of {buffers.max_size} rows')
        return self._iterate(loop, buffers, batch_size, train, lambda: loop.step(buffers), '_sim', getattr(loop.sim, 'graph_generators', ()))

    def evaluate(self, env, episodes, eval_index=None):
        """Mean return of `episodes` mean-action episodes per member, [R] float64 (NaN for a retired member): ONE launch
        (rlrep_group_env_evaluate) and one copy back.  The start states are a function of (member seed, eval_index, episode); by default
        eval_index counts the evaluations of `env`, so successive evaluations see fresh starts and every member of a sweep sharing a seed the
        same ones."""
        if getattr(env, 'agent', None) is not self:
            raise ValueError(f'{type(self).__name__}.evaluate: the device environment belongs to another group')
        episodes = int(episodes)
        if eval_index is None:
            eval_index = env.eval_index
            env.eval_index += 1
        out = torch.full((self.R, episodes), float('nan'), dtype=torch.float64, device=self.core.device)
        env.evaluate(episodes, eval_index, out)
        return out.mean(dim=1).cpu().numpy()

    def _history_info(self):
        half = max(1, self.core.history_capacity() // 2)
        out = []
        for r, m in enumerate(self._members):
            if not self._live[r]:
                out.append(None)
                continue
            n = self._mhist_n[r]
            self._mhist_n[r] += 1
            if n % half == half - 1:
                m.history_resolve()
            out.append(m.info(lazy_source=m.history_source(n)))
        return out

    def member(self, r):
        return self._member_views[r]

    def select_action(self, states, explore=False):
        """states [R, S] -> actions [R, A]: ONE launch over pinned buffers; member r acts as the standalone agent with seed seeds[r] does with
        the same call counter (every member's exploration draw is keyed by its own seed and the shared counter).  A retired member's
        observation is not read and its action row is zeros."""
        sel = getattr(self, '_gsel', None)
        if sel is None:
            sel = self._gsel = dict(obs=torch.empty(self.R, self.state_dim, dtype=torch.float32).pin_memory(),
                                    act=torch.empty(self.R, self.action_dim, dtype=torch.float32).pin_memory())
        sel['obs'].numpy()[:] = np.asarray(states, dtype=np.float32).reshape(self.R, self.state_dim)
        for r in range(self.R):
            if not self._live[r]:
                sel['act'].numpy()[r] = 0.0     # (the launch leaves a retired member's row unwritten)
        if explore:
            self._ctr += 1
        lo, hi = self.action_range
        check(lib.rlrep_group_select_action(self.core.h, C.c_void_p(sel['obs'].data_ptr()), 1 if explore else 0, self._ctr << 20, lo, hi,
                                            C.c_void_p(sel['act'].data_ptr()), _stream()), 'group_select_action')
        torch.cuda.current_stream().synchronize()
        return sel['act'].numpy().copy()

    def select_actions(self, states, explore=False):
        """states [R, E, S] -> actions [R, E, A]: ONE launch over pinned buffers (rlrep_group_select_action_n, grid (E, R)).  [r, e] is what the
        standalone agent with seed seeds[r] returns as the e-th of E successive select_action calls: with `explore`, row e draws at call
        counter _ctr + 1 + e and the counter then advances by E; without it the counter stands still.  A retired member's observations are
        not read and its rows are zeros."""
        states = np.asarray(states, dtype=np.float32)
        if states.ndim != 3 or states.shape[0] != self.R or states.shape[2] != self.state_dim or not 1 <= states.shape[1] <= SELECT_MAX_ROWS:
            raise ValueError(f'{type(self).__name__}.select_actions: states {states.shape} is not [{self.R}, E, {self.state_dim}] with E in '
                             f'[1, {SELECT_MAX_ROWS}]')
        E = states.shape[1]
        bufs = self.__dict__.setdefault('_gsel_n', {})
        sel = bufs.get(E)
        if sel is None:
            sel = bufs[E] = (torch.empty(self.R, E, self.state_dim, dtype=torch.float32).pin_memory(),
                             torch.empty(self.R, E, self.action_dim, dtype=torch.float32).pin_memory())
        obs, act = sel
        obs.numpy()[:] = states
        for r in range(self.R):
            if not self._live[r]:
                act.numpy()[r] = 0.0            # (the launch leaves a retired member's rows unwritten)
        lo, hi = self.action_range
        check(lib.rlrep_group_select_action_n(self.core.h, C.c_void_p(obs.data_ptr()), E, 1 if explore else 0, (self._ctr + 1) << 20 if explore else 0,
                                              lo, hi, C.c_void_p(act.data_ptr()), _stream()), 'group_select_action_n')
        if explore:
            self._ctr += E
        torch.cuda.current_stream().synchronize()
        return act.numpy().copy()

    def act_device(self, obs, explore=False, out=None):
        """obs [R, N, S], a contiguous CUDA float32 tensor -> actions [R, N, A] on the device (`out` if given, contiguous), N up to 65 536:
        ONE launch on the current stream (rlrep_group_act_device, grid (ceil(N / 16), R)), no copy and no synchronisation.  Plane r is bit for
        bit what the standalone agent with seed seeds[r] gets from act_device at the same call counter: with `explore`, row e draws at
        _ctr + 1 + e and the counter then advances by N; without it the counter stands still.  A retired member's observations are not read;
        its rows of `out` are left as they were, and a fresh result has zeros there."""
        R, S, A = self.R, self.state_dim, self.action_dim
        if (not torch.is_tensor(obs) or not obs.is_cuda or obs.dtype != torch.float32 or obs.dim() != 3 or obs.shape[0] != R or obs.shape[2] != S
                or not 1 <= obs.shape[1] <= ACT_MAX_ROWS or not obs.is_contiguous()):
            raise ValueError(f'{type(self).__name__}.act_device: obs must be a contiguous CUDA float32 tensor [{R}, N, {S}] with N in [1, {ACT_MAX_ROWS}]')
        N = int(obs.shape[1])
        if out is None:
            out = (torch.empty if all(self._live) else torch.zeros)(R, N, A, dtype=torch.float32, device=obs.device)
        elif (not torch.is_tensor(out) or out.device != obs.device or out.dtype != torch.float32 or tuple(out.shape) != (R, N, A) or not out.is_contiguous()):
            raise ValueError(f'{type(self).__name__}.act_device: out must be a contiguous float32 tensor [{R}, {N}, {A}] on {obs.device}')
        lo, hi = self.action_range
        check(lib.rlrep_group_act_device(self.core.h, C.c_void_p(obs.data_ptr()), N, 1 if explore else 0, (self._ctr + 1) << 20 if explore else 0,
                                         lo, hi, C.c_void_p(out.data_ptr()), _stream()), 'group_act_device')
        if explore:
            self._ctr += N
        return out

    def member_snapshot(self, r):
        """Member r as a checkpoint of the standalone agent class (its load() accepts it): continue one seed alone."""
        torch.cuda.synchronize()
        c = self._members[r]
        return {'format': self.CHECKPOINT_FORMAT, 'device_state_bytes': int(c.device_state().numel()), 'alg': self.ALG, 'params': c.params.cpu(),
                'targets': c.targets.cpu(), 'exp_avg': c.exp_avg.cpu(), 'exp_avg_sq': c.exp_avg_sq.cpu(), 'alpha_state': c.alpha_state.cpu(),
                'device_state': c.device_state().cpu(), 'steps': self.steps, 'noise_ctr': self._ctr, 'seed': self.seeds[r], 'layout': list(c.order),
                'hyper': self.member_hyper(r)}

    def state_snapshot(self, env=None):
        snap = {'format': 'rlrep-seed-batch-1', 'seeds': list(self.seeds), 'members': [self.member_snapshot(r) for r in range(self.R)],
                'lineage': [dict(e) for e in self.lineage], 'live': list(self._live)}
        if env is not None:         # a device environment's records and counters (rlrep_amd/envs/device.py)
            snap['device_env'] = env.snapshot()
        return snap

    def save(self, path, env=None):
        torch.save(self.state_snapshot(env), path)

    def load(self, path_or_snapshot, adopt_hyper=False, env=None):
        """adopt_hyper: members whose hyper-parameters differ from the checkpoint's take the checkpoint's (a population-based run is resumed
        into a group built with the initial values); otherwise such a checkpoint is refused.  env: a device environment takes the
        checkpoint's records, or a fresh reset when the checkpoint carries none."""
        snap = torch.load(path_or_snapshot) if isinstance(path_or_snapshot, (str, bytes, os.PathLike)) else path_or_snapshot
        if snap.get('format') != 'rlrep-seed-batch-1' or list(snap['seeds']) != self.seeds:
            raise RuntimeError('checkpoint does not match this seed batch (format / seeds differ)')
        torch.cuda.synchronize()
        for r, ms in enumerate(snap['members']):
            c = self._members[r]
            if ms['layout'] != list(c.order) or ms['device_state'].numel() != c.device_state().numel():
                raise RuntimeError('checkpoint does not match this seed batch (dimensions differ)')
            if 'hyper' in ms and dict(ms['hyper']) != self.member_hyper(r) and not (adopt_hyper and set(ms['hyper']) == set(self.SWEEP_KEYS)):
                raise RuntimeError(f'checkpoint does not match this seed batch (member {r} hyper-parameters differ: {dict(ms["hyper"])} '
                                   f'against {self.member_hyper(r)})')
        for r, ms in enumerate(snap['members']):
            if 'hyper' in ms and dict(ms['hyper']) != self.member_hyper(r):
                hp = {k: self.normalise_hyper(k, v) for k, v in ms['hyper'].items()}
                self._apply_member_hyper(r, {k: v for k, v in hp.items() if k != 'alpha'})
                self._mhyper[r]['alpha'] = hp['alpha']          # (the initial temperature: a record only, alpha_state comes with the checkpoint)
        self.lineage = [dict(e) for e in snap.get('lineage', [])]
        live = [bool(v) for v in snap.get('live', [True] * self.R)]          # (a checkpoint written before members could retire: all live)
        if len(live) != self.R or not any(live):
            raise RuntimeError('checkpoint does not match this seed batch (live mask)')
        if live != self._live:
            self._upload_live(live)
        for r, ms in enumerate(snap['members']):
            c = self._members[r]
            for k, dst in (('params', c.params), ('targets', c.targets), ('exp_avg', c.exp_avg), ('exp_avg_sq', c.exp_avg_sq),
                           ('alpha_state', c.alpha_state)):
                dst.copy_(ms[k])
            hyper = c.group_cfg()[:, 1:6].clone()
            c.device_state().copy_(ms['device_state'])
            c.group_cfg()[:, 1:6].copy_(hyper)
            c.sync_step_mirror()
        self.steps, self._ctr = snap['members'][0]['steps'], snap['members'][0]['noise_ctr']
        self._graph = None
        torch.cuda.synchronize()
        if env is not None:
            if 'device_env' in snap:
                env.load_snapshot(snap['device_env'])
            else:
                env.reset()
