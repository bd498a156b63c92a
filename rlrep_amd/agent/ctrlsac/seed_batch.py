"""CTRLSACSeedBatch: R independent ctrlsac agents -- one per seed -- trained by the SAME launches.

The ctrlsac form of SACSeedBatch (rlrep_amd/agent/seed_batch.py has what the two share).  Every launch of one train() -- the feature steps
with their InfoNCE loss, the frozen_phi copies (quirk Q8), the critic and actor steps -- runs all R members, so R seeds cost one train()
graph of exactly one CTRLSACAgent(pipeline=False) graph's launch count.

Initialisation rule: member r is initialised exactly as `torch.manual_seed(seeds[r]); CTRLSACAgent(..., seed=seeds[r])` initialises, and
draws its sample indices and noise from the Philox stream of seed seeds[r].  Member r therefore computes, bit for bit, what that standalone
agent computes with pipeline=False on the same replay ring (tests/test_seed_batch_ctrlsac.py).  The pipelined two-chain train() is not
built for groups: a group always runs the one-graph form.
"""
from rlrep_amd.agent.ctrlsac.ctrlsac_agent import CTRLSACAgent
from rlrep_amd.agent.seed_batch import SeedBatchMixin


class CTRLSACSeedBatch(SeedBatchMixin, CTRLSACAgent):
    """CTRLSACSeedBatch(seeds, state_dim, action_dim, action_space, **CTRLSACAgent kwargs): one ctrlsac agent per seed, trained together.

    `train(buffers, batch_size)` takes a ReplayBufferGroup (rlrep_amd/utils/buffer_group.py) -- member r samples ring r -- and returns a list of
    R info dicts.  Only the single-GPU one-graph train() is built: pipeline=True, graph=False and data parallel are refused."""

    SWEEP_KEYS = SeedBatchMixin.SWEEP_KEYS + ('feature_tau',)

    def __init__(self, seeds, state_dim, action_dim, action_space, **kwargs):
        kwargs = dict(kwargs)
        if kwargs.get('pipeline', False):
            raise RuntimeError('CTRLSACSeedBatch: the pipelined two-chain train() is not built for seed groups (pipeline=False only)')
        kwargs['pipeline'] = False
        super().__init__(seeds, state_dim, action_dim, action_space, **kwargs)
