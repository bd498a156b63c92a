"""Every ValueError / RuntimeError that ReplayBuffer, PrioritizedReplayBuffer, ReplayBufferGroup and PrioritizedReplayBufferGroup raise on
device='cpu', provoked once and compared with the full message as each class wrote it when it carried its own copy of the check (the table
below was taken from that code).  No GPU."""
import numpy as np
import pytest
import torch

S, A, CAP, R = 3, 2, 7, 3


class _Env(object):
    """stand-in device environment: takes the cursor, and reports the records it was built with"""
    def __init__(self, num_envs=1, ptrs=(0,)):
        self.num_envs, self.ptrs = num_envs, ptrs

    def set_cursor(self, *cursor):
        pass

    def state(self):
        rec = np.zeros((len(self.ptrs), self.num_envs), dtype=[('ring_ptr', np.int64), ('ring_size', np.int64)])
        rec['ring_ptr'] = np.asarray(self.ptrs).reshape(-1, 1)
        return rec


def _one(cls='ReplayBuffer', **kw):
    from rlrep_amd.utils import buffer
    return getattr(buffer, cls)(S, A, max_size=CAP, device='cpu', stage_rows=3, **kw)


def _group(cls='ReplayBufferGroup', members=R, **kw):
    from rlrep_amd.utils import buffer_group
    return getattr(buffer_group, cls)(members, S, A, max_size=CAP, device='cpu', stage_rows=3, **kw)


def _host(*lead):
    """(states, actions, next_states, rewards, dones) of zeros with leading shape `lead`, in NumPy"""
    return np.zeros(lead + (S,)), np.zeros(lead + (A,)), np.zeros(lead + (S,)), np.zeros(lead), np.zeros(lead)


def _dev(*lead, **swap):
    """the same as tensors on the CPU; swap=: argument name -> what to pass in its place"""
    t = dict(zip(('states', 'actions', 'next_states', 'rewards', 'dones'), (torch.from_numpy(x).float() for x in _host(*lead))))
    t.update(swap)
    return tuple(t.values())


def _stale(buf):
    buf.collect_on_device(_Env())
    return buf


def _filled(buf, n=2):
    if hasattr(buf, 'members'):
        for _ in range(n):
            buf.add(*_host(buf.members))
    else:
        for _ in range(n):
            buf.add(*_host())
    return buf


STALE_ONE = ('a device environment has been advancing this ring (SACAgent.iterate), so the host cursor is stale: call adopt_device_cursor() '
             'first')
STALE_GROUP = ('a device environment has been advancing these rings (SeedBatchMixin.iterate), so the host cursor is stale: call '
               'adopt_device_cursor() first')
NO_TRAJECTORY = "(a shard keeps one transition in `world`: its rows are no trajectory)"

REFUSALS = [
    # ---- the n-step checks of the constructors (the class name in front) -------------------------------------------------------------------
    ('nstep-integer', lambda: _one(n_step=2.5), ValueError, 'ReplayBuffer: n_step 2.5 and n_stride 1 must be integers'),
    ('nstep-bool', lambda: _group(n_stride=True), ValueError, 'ReplayBufferGroup: n_step 1 and n_stride True must be integers'),
    ('nstep-range', lambda: _one('PrioritizedReplayBuffer', n_step=17), ValueError, 'PrioritizedReplayBuffer: n_step 17 outside [1, 16]'),
    ('nstep-stride', lambda: _group('PrioritizedReplayBufferGroup', n_stride=0), ValueError,
     'PrioritizedReplayBufferGroup: n_stride 0 must be >= 1 (the number of interleaved environments that write the ring)'),
    ('nstep-shard', lambda: _one(n_step=3, shard=(1, 2)), ValueError, f'ReplayBuffer: shard= is not supported with n_step 3 > 1 {NO_TRAJECTORY}'),
    ('cnstep-integer', lambda: _one(critic_n_step=1.5), ValueError, 'ReplayBuffer: critic_n_step 1.5 must be an integer'),
    ('cnstep-range', lambda: _group(critic_n_step=0), ValueError, 'ReplayBufferGroup: critic_n_step 0 outside [1, 16]'),
    ('cnstep-with-nstep', lambda: _one(n_step=2, critic_n_step=3), ValueError,
     'ReplayBuffer: n_step 2 and critic_n_step 3 together (n_step is the whole minibatch of a sac agent, critic_n_step the critic targets of '
     'vlsac / ctrlsac / spedersac / diffsrsac: a buffer trains one kind of agent)'),
    ('cnstep-prioritized', lambda: _one('PrioritizedReplayBuffer', critic_n_step=3), ValueError,
     'PrioritizedReplayBuffer: critic_n_step 3 > 1 is not supported (prioritized replay is built for sac, which has n_step): use a plain '
     'ReplayBuffer'),
    ('cnstep-group', lambda: _group(critic_n_step=3), ValueError,
     'ReplayBufferGroup: critic_n_step 3 > 1 is not supported (n-step critic targets are built for one agent, not for a seed group): use a '
     'plain ReplayBuffer'),
    ('cnstep-prioritized-group', lambda: _group('PrioritizedReplayBufferGroup', critic_n_step=2), ValueError,
     'PrioritizedReplayBufferGroup: critic_n_step 2 > 1 is not supported (n-step critic targets are built for one agent, not for a seed '
     'group): use a plain ReplayBuffer'),
    ('cnstep-shard', lambda: _one(critic_n_step=3, shard=(1, 2)), ValueError,
     f'ReplayBuffer: shard= is not supported with critic_n_step 3 > 1 {NO_TRAJECTORY}'),
    # ---- the other constructor refusals ------------------------------------------------------------------------------------------------
    ('prioritized-shard', lambda: _one('PrioritizedReplayBuffer', shard=(1, 2)), ValueError,
     'PrioritizedReplayBuffer: shard= is not supported (a shard sees one transition in `world`; priorities are per ring)'),
    ('group-members', lambda: _group(members=0), ValueError, 'ReplayBufferGroup: members must be >= 1'),
    ('per-member-length', lambda: _group('PrioritizedReplayBufferGroup', alpha=[0.5, 0.6]), ValueError,
     'PrioritizedReplayBufferGroup: alpha has 2 entries for 3 members (a scalar, or one value per member)'),
    ('per-member-length-beta', lambda: setattr(_group('PrioritizedReplayBufferGroup'), 'beta', [0.1] * 4), ValueError,
     'PrioritizedReplayBufferGroup: beta has 4 entries for 3 members (a scalar, or one value per member)'),
    # ---- the stale cursor: three methods of two classes --------------------------------------------------------------------------------
    ('stale-add', lambda: _stale(_one()).add(*_host()), RuntimeError, f'ReplayBuffer.add: {STALE_ONE}'),
    ('stale-add_batch', lambda: _stale(_one()).add_batch(*_host(2)), RuntimeError, f'ReplayBuffer.add_batch: {STALE_ONE}'),
    ('stale-add_device', lambda: _stale(_one()).add_device(*_dev(2)), RuntimeError, f'ReplayBuffer.add_device: {STALE_ONE}'),
    ('stale-group-add', lambda: _stale(_group()).add(*_host(R)), RuntimeError, f'ReplayBufferGroup.add: {STALE_GROUP}'),
    ('stale-group-add_batch', lambda: _stale(_group()).add_batch(*_host(R, 2)), RuntimeError, f'ReplayBufferGroup.add_batch: {STALE_GROUP}'),
    ('stale-group-add_device', lambda: _stale(_group()).add_device(*_dev(R, 2)), RuntimeError, f'ReplayBufferGroup.add_device: {STALE_GROUP}'),
    # ---- the shard refusals ------------------------------------------------------------------------------------------------------------
    ('shard-add_device', lambda: _one(shard=(1, 2)).add_device(*_dev(2)), ValueError,
     'ReplayBuffer.add_device: a sharded ring (shard=) keeps one transition in `world`; add_device writes every row it is given'),
    ('shard-collect', lambda: _one(shard=(1, 2)).collect_on_device(_Env()), ValueError,
     'ReplayBuffer.collect_on_device: a sharded ring (shard=) keeps one transition in `world`; a device environment writes every row it steps'),
    ('shard-load', lambda: _one(shard=(1, 2)).load(*_host(2)), ValueError,
     'load() fills the whole ring and knows nothing of the shard rule: add() the transitions instead'),
    # ---- add_device: the range of N, the device and the shapes -------------------------------------------------------------------------
    ('add_device-none', lambda: _one().add_device(*_dev(0)), ValueError,
     'ReplayBuffer.add_device: 0 transitions for a ring of 7 rows (N must lie in [1, max_size])'),
    ('add_device-many', lambda: _one().add_device(*_dev(8)), ValueError,
     'ReplayBuffer.add_device: 8 transitions for a ring of 7 rows (N must lie in [1, max_size])'),
    ('add_device-host-array', lambda: _one().add_device(*_dev(2, states=np.zeros((2, S), np.float32))), ValueError,
     'ReplayBuffer.add_device: states must be a tensor on cpu'),
    ('add_device-device', lambda: _one().add_device(*_dev(2, dones=torch.zeros(2, device='meta'))), ValueError,
     'ReplayBuffer.add_device: dones must be a tensor on cpu'),
    ('add_device-shape', lambda: _one().add_device(*_dev(2, actions=torch.zeros(2, A + 1))), ValueError,
     'ReplayBuffer.add_device: actions (2, 3) is not [2, 2]'),
    ('add_device-shape-rows', lambda: _one().add_device(*_dev(2, next_states=torch.zeros(3, S))), ValueError,
     'ReplayBuffer.add_device: next_states (3, 3) is not [2, 3]'),
    ('group-add_device-members', lambda: _group().add_device(*_dev(R, 2, rewards=torch.zeros(2, 2))), ValueError,
     'ReplayBufferGroup.add_device: rewards (2, 2) is not [3, N]'),
    ('group-add_device-flat', lambda: _group().add_device(*_dev(R, 2, rewards=torch.zeros(R))), ValueError,
     'ReplayBufferGroup.add_device: rewards (3,) is not [3, N]'),
    ('group-add_device-none', lambda: _group().add_device(*_dev(R, 0)), ValueError,
     'ReplayBufferGroup.add_device: 0 transitions for rings of 7 rows (N must lie in [1, max_size])'),
    ('group-add_device-many', lambda: _group().add_device(*_dev(R, 8)), ValueError,
     'ReplayBufferGroup.add_device: 8 transitions for rings of 7 rows (N must lie in [1, max_size])'),
    ('group-add_device-host-array', lambda: _group().add_device(*_dev(R, 2, actions=np.zeros((R, 2, A), np.float32))), ValueError,
     'ReplayBufferGroup.add_device: actions must be a tensor on cpu'),
    ('group-add_device-device', lambda: _group().add_device(*_dev(R, 2, next_states=torch.zeros(R, 2, S, device='meta'))), ValueError,
     'ReplayBufferGroup.add_device: next_states must be a tensor on cpu'),
    ('group-add_device-after-load', lambda: (lambda g: (g.load(0, *_host(2)), g.add_device(*_dev(R, 2))))(_group()), RuntimeError,
     'ReplayBufferGroup.add_device after load() gave the members different fill levels: the lockstep ring takes N rows per member'),
    # ---- collect_on_device of the four classes, and the cursor coming back ------------------------------------------------------------
    ('collect-another', lambda: _stale(_one()).collect_on_device(_Env()), RuntimeError,
     'ReplayBuffer.collect_on_device: another device environment owns the cursor (adopt_device_cursor() first)'),
    ('collect-nstep', lambda: _one(n_step=3, n_stride=2).collect_on_device(_Env(num_envs=4)), ValueError,
     'ReplayBuffer.collect_on_device: n_step 3 with n_stride 2, but the device environment interleaves num_envs = 4 trajectories in the ring: '
     'build the buffer with n_stride = num_envs'),
    ('collect-cnstep', lambda: _one(critic_n_step=3, n_stride=2).collect_on_device(_Env()), ValueError,
     'ReplayBuffer.collect_on_device: critic_n_step 3 with n_stride 2, but the device environment interleaves num_envs = 1 trajectories in the '
     'ring: build the buffer with n_stride = num_envs'),
    ('collect-prioritized', lambda: _one('PrioritizedReplayBuffer').collect_on_device(_Env()), RuntimeError,
     'PrioritizedReplayBuffer.collect_on_device: a device environment writes ring rows inside its step launch, which knows nothing of the '
     'priority tree (iterate() / --device-loop take a plain ReplayBuffer)'),
    ('collect-group-another', lambda: _stale(_group()).collect_on_device(_Env()), RuntimeError,
     'ReplayBufferGroup.collect_on_device: another device environment owns the cursor (adopt_device_cursor() first)'),
    ('collect-group-nstep', lambda: _group(n_step=3, n_stride=2).collect_on_device(_Env(num_envs=4)), ValueError,
     'ReplayBufferGroup.collect_on_device: n_step 3 with n_stride 2, but the device environment interleaves num_envs = 4 trajectories per ring: '
     'build the buffers with n_stride = num_envs'),
    ('collect-prioritized-group', lambda: _group('PrioritizedReplayBufferGroup').collect_on_device(_Env()), RuntimeError,
     'PrioritizedReplayBufferGroup.collect_on_device: a device environment writes ring rows inside its step launch, which knows nothing of the '
     'priority trees (iterate() takes a plain ReplayBufferGroup)'),
    ('adopt-group-cursors-differ', lambda: (lambda g: (g.collect_on_device(_Env(ptrs=(4, 2, 4))), g.adopt_device_cursor()))(_group()), RuntimeError,
     "ReplayBufferGroup.adopt_device_cursor: the members' ring cursors differ ([2, 4]): the host ring takes one row per member in lockstep"),
    # ---- prioritized replay: set_priorities, draw ----------------------------------------------------------------------------------------
    ('set_priorities-overflow', lambda: _filled(_one('PrioritizedReplayBuffer')).set_priorities(np.ones(3)), ValueError,
     'PrioritizedReplayBuffer.set_priorities: 3 leaves for a ring that holds 2 rows'),
    ('group-set_priorities-overflow', lambda: _filled(_group('PrioritizedReplayBufferGroup')).set_priorities(1, np.ones(5)), ValueError,
     'PrioritizedReplayBufferGroup.set_priorities: 5 leaves for a ring that holds 2 rows'),
    ('draw-empty', lambda: _one('PrioritizedReplayBuffer').draw(4, 0, 0), RuntimeError, 'PrioritizedReplayBuffer.draw: the buffer is empty'),
    ('group-draw-empty', lambda: (lambda g: (g.load(0, *_host(2)), g.draw(4, 0, seeds=[0] * R)))(_group('PrioritizedReplayBufferGroup')),
     RuntimeError, "PrioritizedReplayBufferGroup.draw: a member's buffer is empty"),
    ('draw-given-length', lambda: _filled(_one('PrioritizedReplayBuffer')).draw(4, 0, 0, given=[0, 1, 0]), ValueError,
     'PrioritizedReplayBuffer.draw: given indices must be 4 rows in [0, 2)'),
    ('draw-given-range', lambda: _filled(_one('PrioritizedReplayBuffer')).draw(4, 0, 0, given=torch.tensor([0, 1, 2, 0])), ValueError,
     'PrioritizedReplayBuffer.draw: given indices must be 4 rows in [0, 2)'),
    ('draw-given-negative', lambda: _filled(_one('PrioritizedReplayBuffer')).draw(2, 0, 0, given=[0, -1]), ValueError,
     'PrioritizedReplayBuffer.draw: given indices must be 2 rows in [0, 2)'),
    ('group-draw-given-length', lambda: _filled(_group('PrioritizedReplayBufferGroup')).draw(4, 0, given=np.zeros((R, 3), np.int32)), ValueError,
     "PrioritizedReplayBufferGroup.draw: given indices must be [3, 4] rows inside each member's ring"),
    ('group-draw-given-range', lambda: _filled(_group('PrioritizedReplayBufferGroup')).draw(2, 0, given=torch.tensor([[0, 1], [0, 2], [1, 1]])),
     ValueError, "PrioritizedReplayBufferGroup.draw: given indices must be [3, 2] rows inside each member's ring"),
]


@pytest.mark.parametrize('provoke,error,message', [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_the_refusal_keeps_its_message(provoke, error, message):
    with pytest.raises(error) as e:
        provoke()
    assert type(e.value) is error and str(e.value) == message


def test_the_refused_calls_are_accepted_once_the_reason_is_gone():
    """the stand-ins above are refused for the reason in the table, not for being stand-ins: the same calls pass where the reason is absent"""
    one, group = _one(n_step=3, n_stride=2), _group(n_step=3, n_stride=2)
    one.add_device(*_dev(2))
    group.add_device(*_dev(R, 2))
    for buf, env in ((one, _Env(num_envs=2)), (group, _Env(num_envs=2, ptrs=(2, 2, 2)))):
        buf.collect_on_device(env)
        buf.collect_on_device(env)              # (the owner again: no refusal)
        buf.adopt_device_cursor()
        assert buf._device_env is None and buf.ptr == (2 if buf is group else 0)
    one.add(*_host())
    group.add_batch(*_host(R, 2))
    per, pgroup = _filled(_one('PrioritizedReplayBuffer')), _filled(_group('PrioritizedReplayBufferGroup'))
    per.set_priorities(np.ones(2))
    pgroup.set_priorities(1, np.ones(2))
    per.draw(4, 0, 0, given=[0, 1, 1, 0])
    pgroup.draw(2, 0, given=np.zeros((R, 2), np.int32))
