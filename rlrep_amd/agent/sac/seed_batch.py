"""SACSeedBatch: R independent SAC agents -- one per seed -- trained by the SAME launches.

Nobody reports an RL result from one seed; a single B = 256 agent leaves most of the MI355X idle between its ~5 us launches.  A seed batch
lays R agents of identical shape out at a constant byte stride in ONE allocation (include/rlrep.h rlrep_group_create): the step programs are
built once, against member 0, and every launch of a train() runs all members (member = grid y, every pointer moved by member * stride).
So R seeds cost one train() graph of exactly one agent's launch count, not R of them.

Initialisation rule: member r is initialised exactly as `torch.manual_seed(seeds[r]); SACAgent(..., seed=seeds[r])` initialises, and draws
its sample indices and noise from the Philox stream of seed seeds[r].  Member r therefore computes, bit for bit, what that standalone agent
computes on the same replay ring (tests/test_seed_batch.py).
"""
from rlrep_amd.agent.sac.sac_agent import SACAgent
from rlrep_amd.agent.seed_batch import SeedBatchMixin, _Member, _MemberCore  # noqa: F401  (this module's names before they were shared)


class SACSeedBatch(SeedBatchMixin, SACAgent):
    """SACSeedBatch(seeds, state_dim, action_dim, action_space, **SACAgent kwargs): one SAC agent per seed, trained together.

    `train(buffers, batch_size)` takes a ReplayBufferGroup (rlrep_amd/utils/buffer_group.py) -- member r samples ring r -- and returns a list of
    R info dicts.  The single-GPU whole-train() graph is the only form (no data parallel, no eager steps).  The group machinery is
    SeedBatchMixin's (rlrep_amd/agent/seed_batch.py)."""
