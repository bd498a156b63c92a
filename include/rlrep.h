/*
 * rlrep.h -- C ABI of librlrep_hip.so: the MI355X-native (gfx950) update hot path of rl-rep.
 *
 * The reference (haotiansun14/rl-rep) has NO FFI/operator layer: its boundary for this path is the
 * Python class API of the agents.  Each entry point below therefore names the reference method it
 * replaces (paths relative to the reference repository root):
 *
 *   rlrep_agent_create        <- SACAgent.__init__        agent/sac/sac_agent.py:19-81
 *                                VLSACAgent.__init__      agent/vlsac/vlsac_agent.py:71-123
 *                                CTRLSACAgent.__init__    agent/ctrlsac/ctrlsac_agent.py:127-210
 *                                SPEDERSACAgent.__init__  agent/spedersac/spedersac_agent.py:102-179
 *                                DIFFSRSACAgent.__init__  agent/diffsrsac/diffsrsac_agent.py:95-176
 *   rlrep_feature_step        <- feature_step             vlsac_agent.py:126-162, ctrlsac_agent.py:213-251,
 *                                                         spedersac_agent.py:181-219;
 *                                critic_feeder_feature_step  diffsrsac_agent.py:271-318
 *                                (+ update_feature_target: vlsac :240-242, ctrlsac :253-255, speder :221-223)
 *   rlrep_critic_step         <- critic_step              sac_agent.py:105-135 and per-agent overrides
 *   rlrep_actor_alpha_step    <- update_actor_and_alpha   sac_agent.py:138-166 and per-agent overrides
 *   rlrep_prefetch_policy     <- (no counterpart: reorders the forward half of update_actor_and_alpha, sac_agent.py:141-150,
 *                                into critic_step's launches)
 *   rlrep_update_target       <- update_target            sac_agent.py:99-102
 *   rlrep_train               <- train                    sac_agent.py:169-188, vlsac_agent.py:245-273, ...
 *   rlrep_set_batch           <- Batch / unpack_batch     utils/buffer.py:7-10, utils/util.py:10-11
 *   rlrep_replay_add/_sample  <- ReplayBuffer.add/.sample utils/buffer.py:28-48
 *   rlrep_actor_forward       <- SACAgent.select_action   sac_agent.py:89-96
 *
 * Conventions
 *   - plain C types only; every pointer named *_dev is a DEVICE pointer owned by the caller (e.g. a torch
 *     tensor's data_ptr()); the library never allocates or frees device memory on the hot path
 *     (it uploads small task tables into the caller-provided workspace at create time);
 *   - all tensors are contiguous row-major fp32 unless stated; nn.Linear weights are [out,in];
 *   - every call is ASYNCHRONOUS and stream-ordered on `stream` (a hipStream_t passed as void*);
 *     no call synchronises the device; calls on one agent are not thread-safe;
 *   - return value: 0 on success, negative rlrep_status otherwise; rlrep_last_error() gives text.
 */
#ifndef RLREP_H
#define RLREP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLREP_ABI_VERSION 4      /* 4: exchange scratch + reduced region in the comm block (two-shot, batch-coupled exchanges inside the launches), rlrep_comm_connect_local, time-bounded waits; dims.world_size, layout_info.exchange_floats */

typedef enum {
    RLREP_OK = 0,
    RLREP_ERR_ARG = -1,        /* bad argument / unsupported dimension */
    RLREP_ERR_HIP = -2,        /* a HIP runtime call failed */
    RLREP_ERR_STATE = -3,      /* call order violated (e.g. step before set_batch) */
    RLREP_ERR_NOMEM = -4       /* caller-provided workspace too small */
} rlrep_status;

typedef enum {
    RLREP_ALG_SAC = 0,
    RLREP_ALG_VLSAC = 1,
    RLREP_ALG_CTRLSAC = 2,
    RLREP_ALG_SPEDERSAC = 3,
    RLREP_ALG_DIFFSRSAC = 4
} rlrep_alg;

/* Network dimensions (mirrors the reference constructors' dimension kwargs).
 * vlsac: feature_dim is any positive multiple of 4 (every noise-critic kernel moves 16-byte rows) and num_noise is 20; no upper bound on
 * feature_dim comes from the kernels -- what rlrep_layout can size is accepted -- and the suite runs widths up to 1024 against the oracle. */
typedef struct {
    int32_t alg;               /* rlrep_alg */
    int32_t state_dim;         /* S */
    int32_t action_dim;        /* A */
    int32_t hidden_dim;        /* critic hidden (sac/vlsac/ctrlsac `hidden_dim`, speder `critic_and_actor_hidden_dim`) */
    int32_t actor_hidden_dim;  /* actor trunk hidden (sac/vlsac: hidden_dim; ctrlsac: 256; speder: critic_and_actor_hidden_dim) */
    int32_t feature_dim;       /* F */
    int32_t vae_hidden_dim;    /* vlsac Encoder/Decoder/GaussianFeature hidden (reference default 256) */
    int32_t phi_hidden_dim;    /* ctrlsac hidden_dim / speder phi_hidden_dim / diffsr phi_hidden_dim */
    int32_t phi_hidden_depth;  /* speder, diffsr (ctrlsac: 2 fixed) */
    int32_t mu_hidden_dim;     /* ctrlsac hidden_dim / speder mu_hidden_dim / diffsr nabla_mu_hidden_dim */
    int32_t mu_hidden_depth;   /* speder, diffsr (ctrlsac: 2 fixed) */
    int32_t num_noise;         /* vlsac critic noise rows (20) / diffsr num_noises (1000) */
    int32_t max_batch;         /* largest batch size this agent will be stepped with */
    int32_t rank;              /* data-parallel rank of this replica (0 when world_size == 1) */
    int32_t flags;             /* RLREP_FLAG_* */
    int32_t world_size;        /* data-parallel replicas the WORKSPACE is sized for (0 / 1: one; must equal hyper.world_size when > 1): ctrlsac's score
                                  matrix is [B, world * B], and an attached agent (rlrep_comm_attach) keeps its deferred step programs */
} rlrep_dims;

/* vlsac / ctrlsac / spedersac constructed with use_feature_target=False (vlsac_agent.py:113-114,176-179,214-219,257-258;
 * ctrlsac_agent.py:167-168,185-186,268-273,340-346; spedersac_agent.py:150-151,306-307): no Polyak copy of the feature net; vlsac's critic
 * and actor steps read the LIVE f, ctrlsac's critic step reads frozen_phi.  The target tensors stay in the layout and are never touched. */
#define RLREP_FLAG_NO_FEATURE_TARGET 1

/* Hyper-parameters (mirrors the reference constructors' scalar kwargs). */
typedef struct {
    float lr_feature;          /* feature optimizer(s) */
    float lr_critic;
    float lr_actor;            /* actor and log_alpha optimizers */
    float discount;
    float tau;                 /* critic target Polyak rate */
    float feature_tau;         /* feature target Polyak rate */
    float target_entropy;      /* -action_dim */
    float sigma_scale;         /* diffsr sigma_scale_factor */
    int32_t target_update_period;
    int32_t extra_feature_steps;
    int32_t learn_alpha;       /* auto_entropy_tuning */
    int32_t world_size;        /* data-parallel replicas: local losses are scaled by 1/(B*world_size) */
    float beta1, beta2, adam_eps;
    float critic_reg_lambda;   /* diffsr critic_elu_layer_regularizer_lambda (diffsrsac_agent.py:62-90,215-227): enters q_loss_reg only */
} rlrep_hyper;

/* One named tensor inside an arena (what nn.Parameter views / state_dict() are built from). */
typedef struct {
    char name[72];             /* reference state_dict key, e.g. "encoder.mean_linear.weight" */
    int32_t arena;             /* rlrep_arena */
    int32_t group;             /* optimizer group: 0 feature, 1 critic, 2 actor, 3 feature2 (diffsr nabla-mu), -1 none */
    int64_t offset;            /* in floats from the arena base */
    int32_t rows, cols;        /* bias: rows=n, cols=1 */
} rlrep_tensor_desc;

typedef enum {
    RLREP_ARENA_PARAM = 0,     /* trainable parameters            (fp32) */
    RLREP_ARENA_TARGET = 1,    /* target / frozen copies + vlsac noise + diffsr alphabars (fp32) */
    RLREP_ARENA_COUNT = 2
} rlrep_arena;

/* Sizes the caller must allocate (floats unless stated). grad/exp_avg/exp_avg_sq arenas have the
 * PARAM arena's size and layout (+ RLREP_GRAD_TAIL floats of cross-rank-reducible partial sums at the
 * end of the grad arena). */
typedef struct {
    int64_t param_floats;
    int64_t target_floats;
    int64_t grad_floats;       /* = param_floats + RLREP_GRAD_TAIL */
    int64_t workspace_bytes;   /* activations, batch slots, task tables, metric partials */
    int64_t group_offset[4];   /* start of each optimizer group inside the PARAM arena (floats) */
    int64_t group_floats[4];
    int32_t n_tensors;
    int32_t n_metrics;
    int64_t exchange_floats;   /* exchange scratch (rlrep_comm_create) that moves the agent's batch-coupled feature exchanges into its launches (0: none) */
} rlrep_layout_info;

#define RLREP_GRAD_TAIL 256

/* Device pointers handed over at create time; they must outlive the agent. */
typedef struct {
    float* param_dev;
    float* target_dev;
    float* grad_dev;
    float* exp_avg_dev;
    float* exp_avg_sq_dev;
    void* workspace_dev;
    double* alpha_state_dev;   /* 4 doubles: log_alpha, exp_avg, exp_avg_sq, step   (quirk Q1: float64) */
} rlrep_arenas;

/* A minibatch as five separate device arrays (utils/buffer.py:7-10 field order). */
typedef struct {
    const float* state_dev;       /* [B,S] */
    const float* action_dev;      /* [B,A] */
    const float* reward_dev;      /* [B,1] */
    const float* next_state_dev;  /* [B,S] */
    const float* done_dev;        /* [B,1] */
    int32_t batch;
} rlrep_batch;

typedef struct rlrep_agent rlrep_agent;

/* ---- introspection ------------------------------------------------------------------------ */
int32_t rlrep_abi_version(void);
const char* rlrep_last_error(void);

/* Layout of every tensor of algorithm dims->alg.  `descs` may be NULL to query counts only. */
int32_t rlrep_layout(const rlrep_dims* dims, rlrep_layout_info* info, rlrep_tensor_desc* descs, int32_t cap);

/* Names of the metrics slots written by the step programs (reference dict keys). */
int32_t rlrep_metric_names(int32_t alg, char (*names)[32], int32_t cap);

/* ---- lifetime ----------------------------------------------------------------------------- */
int32_t rlrep_agent_create(const rlrep_dims* dims, const rlrep_hyper* hyper, const rlrep_arenas* arenas,
                           void* stream, rlrep_agent** out);
void rlrep_agent_destroy(rlrep_agent* agent);

/* ---- data: minibatch slots ---------------------------------------------------------------- */
/* slot 0 = the batch used by feature/critic/actor steps; slot 1 = spedersac's second ("random") batch. */
int32_t rlrep_set_batch(rlrep_agent* agent, int32_t slot, const rlrep_batch* batch, void* stream);

/* Device-resident replay ring: rows of [s | a | s' | r | d] (row length 2S+A+2 floats). */
int32_t rlrep_replay_row_floats(const rlrep_dims* dims);
/* ReplayBuffer.add (utils/buffer.py:28-36), batched: `nrows` staged rows (pinned host memory, row_floats floats each) enter the ring at
 * slot `ptr` and wrap around its end (ptr' = (ptr + nrows) % capacity is the caller's to keep, as `self.ptr` is in the reference).
 * Asynchronous on `stream`: at most two copies.  nrows <= capacity. */
int32_t rlrep_replay_add(float* ring_dev, int64_t capacity, int32_t row_floats, int64_t ptr,
                         const float* rows_host, int64_t nrows, void* stream);
/* The same plus the ring's new fill level written to the device scalar the index generator reads (`size_dev`, may be NULL), in ONE launch that
 * reads the staged rows in place: `rows_host` must be pinned (mapped) host memory (RLREP_ERR_ARG otherwise).  What ReplayBuffer.flush() issues in
 * front of every train() of main.py's loop. */
int32_t rlrep_replay_add_sized(float* ring_dev, int64_t capacity, int32_t row_floats, int64_t ptr, const float* rows_host, int64_t nrows,
                               int32_t* size_dev, int32_t new_size, void* stream);
/* gather rows idx_dev[0..batch) of the ring into a batch slot */
int32_t rlrep_replay_sample(rlrep_agent* agent, int32_t slot, const float* ring_dev, const int32_t* idx_dev,
                            int32_t batch, void* stream);
/* Philox4x32-10 fills: uniform indices in [0,hi) and N(0,1) noise (counter-based, replayable). */
int32_t rlrep_fill_indices(int32_t* dst_dev, int64_t n, int32_t hi, uint64_t seed, uint64_t offset, void* stream);
int32_t rlrep_fill_normal(float* dst_dev, int64_t n, float std, uint64_t seed, uint64_t offset, void* stream);
/* The bare Philox4x32-10 bijection the fills are built on, for known-answer tests (Random123 kat_vectors):
 * ctr_key_dev uint32[n][6] = (counter x4, key x2) -> out_dev uint32[n][4].  Not on any hot path. */
int32_t rlrep_philox_raw(const uint32_t* ctr_key_dev, uint32_t* out_dev, int64_t n, void* stream);

/* Graph-replay-safe variants: the Philox offset is `offset + *counter_dev` and the index range is `*hi_dev`,
 * both read on the device at execution time (rlrep_steps_dev() is the agent's train() counter). */
int32_t rlrep_fill_indices_dev(int32_t* dst_dev, int64_t n, const int32_t* hi_dev, uint64_t seed, uint64_t offset,
                               const int32_t* counter_dev, void* stream);
int32_t rlrep_fill_normal_dev(float* dst_dev, int64_t n, float std, uint64_t seed, uint64_t offset,
                              const int32_t* counter_dev, void* stream);
const int32_t* rlrep_steps_dev(rlrep_agent* agent);
/* The four optimizer groups' device records: 22 32-bit words each -- {int32 step; float lr, beta1, beta2, eps, tau; 8 derived floats
 * recomputed on every step; 8 words of running beta^step powers (double) with the (step, betas) they belong to}.  A checkpoint restores `step` only and keeps the constructor's hyper-parameters (rlrep_amd/agent/sac). */
const void* rlrep_group_cfg_dev(rlrep_agent* agent);
#define RLREP_GROUP_CFG_WORDS 22

/* ---- launch-saving forms of the sampling calls (graph-replayed train()) -------------------------
 * rlrep_train_prologue == rlrep_begin_train + rlrep_fill_indices_dev(idx_pool) + rlrep_fill_normal_dev(eps_pool) +
 * rlrep_replay_sample(slot 0, ring, idx_pool[0:batch]) in ONE launch (same generator streams, same results): the
 * gather recomputes its indices from the counter-based generator instead of waiting for the pool.  The following
 * rlrep_replay_sample(agent, 0, ring, idx_pool, batch, ..) is recognised and skipped.
 * rlrep_prefetch_batch arms the gather of the NEXT minibatch (slot 0) to ride in the next optimizer launch
 * (rlrep_*_apply / *_step): by then the current step has finished reading the slot.  The matching
 * rlrep_replay_sample(agent, 0, ring, idx, batch, ..) is then skipped.  Returns 1 if armed, 0 if not (batch size change). */
int32_t rlrep_train_prologue(rlrep_agent* agent, const float* ring_dev, const int32_t* size_dev, int32_t* idx_pool_dev, int64_t n_idx,
                             float* eps_pool_dev, int64_t n_eps, uint64_t seed, uint64_t idx_offset, uint64_t eps_offset,
                             int32_t batch, void* stream);
int32_t rlrep_prefetch_batch(rlrep_agent* agent, const float* ring_dev, const int32_t* idx_dev, int32_t batch);
/* the same for minibatch slot `slot` (1: spedersac's second, "random" minibatch, agent/spedersac/spedersac_agent.py:181-186): both gathers of the
 * next feature step ride in this step's optimizer launch */
int32_t rlrep_prefetch_batch_slot(rlrep_agent* agent, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch);

/* ---- step programs ------------------------------------------------------------------------ */
/* eps pointers: caller-provided standard-normal noise (parity runs inject the oracle's tensors).
 *   vlsac feature: eps[B,F];  diffsr feature: noise_idx int32[B] + eps[B,S] (already scaled by sigma);
 *   critic/actor: eps[B,A].                                                                        */
int32_t rlrep_feature_step(rlrep_agent* agent, const float* eps_dev, const int32_t* noise_idx_dev, void* stream);
int32_t rlrep_critic_step(rlrep_agent* agent, const float* eps_dev, void* stream);
int32_t rlrep_actor_alpha_step(rlrep_agent* agent, const float* eps_dev, void* stream);
/* Optional launch saving for the sequence critic step -> actor step ON THE SAME BATCH (what train() does,
 * sac_agent.py:180-187): the forward half of update_actor_and_alpha (policy on s, features of (s, a_pi)) reads
 * nothing critic_step writes, so the library can run it inside the critic step's launches.  Call
 * rlrep_prefetch_policy(agent, eps_actor) right before rlrep_critic_step / _backward with the noise the actor step
 * will be given; the following rlrep_actor_alpha_step / _backward called with the SAME eps pointer then resumes after
 * its forward half.  Returns 1 if armed, 0 if this agent / shape has no such variant (then nothing changes), < 0 on
 * error.  Any new batch or feature step in between disarms it; results are identical either way. */
int32_t rlrep_prefetch_policy(rlrep_agent* agent, const float* eps_actor_dev);
/* One step earlier, for agents whose critic / actor steps reuse the minibatch of the LAST feature step (vlsac: train()
 * samples once per feature iteration and keeps the last batch, vlsac_agent.py:246-262): armed before that feature step,
 * BOTH policy forwards (on s' with eps_critic for the critic step's TD target, on s with eps_actor for the actor step)
 * ride in its first launches, and the critic step called with the same eps_critic pointer starts with the three
 * f_target forwards side by side.  Returns 1 if armed, 0 if the agent has no such variant. */
int32_t rlrep_prefetch_policy_early(rlrep_agent* agent, const float* eps_critic_dev, const float* eps_actor_dev);
/* Polyak critic -> critic_target iff (steps % target_update_period == 0), steps kept on the device. */
int32_t rlrep_update_target(rlrep_agent* agent, void* stream);
/* steps += 1 (device counter; graph-replay safe).  Also opens a train() bracket that rlrep_update_target closes: inside
 * it the Polyak critic -> critic_target (same tau, same steps % period gate) is performed by the critic step's Adam
 * launch and rlrep_update_target only closes the bracket -- nothing in between reads critic_target (train():
 * sac_agent.py:169-190).  Without a preceding rlrep_begin_train every entry point does exactly what its reference
 * method does. */
int32_t rlrep_begin_train(rlrep_agent* agent, void* stream);

/* Split entry points for data-parallel training: backward part writes the group's gradient arena, apply part runs
 * Adam / Polyak / temperature update; rlrep_*_step == backward immediately followed by apply.  With hyper.world_size > 1 the
 * gradient arena is COMPLETE after the backward part: the caller all-reduces grad_dev[group_offset .. +group_floats (+tail)]
 * between the two -- or has attached a comm (rlrep_comm_attach), in which case the apply part sums the ranks' arenas itself and
 * the caller issues nothing.  EXCEPTION, hyper.world_size == 1 only: gradients that arrive as split-K partials (vlsac critic
 * l1 / l4, spedersac phi / mu weight gradients) are summed BY THE APPLY PART's optimizer launch, which files the sums in grad_dev
 * too; between backward and apply those ranges of grad_dev hold the previous step's values.  A single-rank caller that inspects
 * or clips gradients between the two parts sets RLREP_DISABLE=fold_ncdw,fold_dwfin (the finishing launches come back). */
int32_t rlrep_feature_backward(rlrep_agent* agent, const float* eps_dev, const int32_t* noise_idx_dev, void* stream);
int32_t rlrep_feature_apply(rlrep_agent* agent, void* stream);
int32_t rlrep_critic_backward(rlrep_agent* agent, const float* eps_dev, void* stream);
int32_t rlrep_critic_apply(rlrep_agent* agent, void* stream);
int32_t rlrep_actor_backward(rlrep_agent* agent, const float* eps_dev, void* stream);
int32_t rlrep_actor_apply(rlrep_agent* agent, void* stream);

/* Batch-coupled representation losses under data parallelism (ctrlsac's in-batch negatives, spedersac's second
 * moment) need a collective INSIDE the feature backward.  The feature backward is therefore cut into
 * rlrep_feature_exchange_count()+1 parts; after part k the caller performs exchange k on a library buffer:
 *   kind 1: all-gather  -- every rank contributes `count` floats at ptr + local_off (in place, rank-major)
 *   kind 2: all-reduce SUM of `count` floats at ptr.
 *   kind 3: `count` floats at ptr = the gradient arena at float offset local_off are FINAL (diffsrsac: the nabla-mu head's weight + bias
 *           gradient, 99 % of that group's bytes, taken first): their all-reduce SUM may be issued now, asynchronously, and has to be complete --
 *           like that of the rest of the group, which the caller reduces after the last part -- before rlrep_feature_apply.
 * With world_size == 1 there are no exchanges and rlrep_feature_backward runs everything. */
int32_t rlrep_feature_exchange_count(rlrep_agent* agent);
int32_t rlrep_feature_exchange(rlrep_agent* agent, int32_t k, int32_t* kind, float** ptr_dev, int64_t* count, int64_t* local_off);
int32_t rlrep_feature_backward_part(rlrep_agent* agent, int32_t part, const float* eps_dev, const int32_t* noise_idx_dev, void* stream);

/* ---- deferred critic / actor steps (vlsac) ---------------------------------------------------
 * The feature steps of train(t+1) read nothing that the critic and actor steps of train(t) write, and the critic / actor steps
 * read only f_target, the last minibatch, their policy noise and the step counter from the feature side.  rlrep_defer_snapshot
 * copies exactly those (ONE launch) after the last feature step of train(t); rlrep_deferred_critic_actor then runs critic_step,
 * update_actor_and_alpha and the (period-gated) critic-target Polyak of train(t) against the snapshot, so a caller may issue it
 * on a second stream / graph branch next to train(t+1)'s feature steps.  Same arithmetic and the same sequence of updates
 * per parameter as the sequential entry points (tests/test_hip_parity.py::test_deferred_pipeline_is_equivalent); the caller
 * must order: snapshot(t) into set s after feature steps(t) AND after the deferred pair that last used set s; deferred(t) after
 * snapshot(t) and after deferred(t-1); anything that reads the critic / actor (select_action, checkpoints, metrics of those steps)
 * after deferred(t).  There are rlrep_defer_supported()
 * sets (3), so with set = t % 3 a snapshot only waits for the pair of train(t-3): the DEVICE needs two, the third keeps a HOST that waits for
 * that older pair before launching the next feature chain a full call ahead of the device. */
int32_t rlrep_defer_supported(rlrep_agent* agent);          /* number of snapshot sets (3) or 0 */
int32_t rlrep_defer_snapshot(rlrep_agent* agent, int32_t set, const float* eps_critic_dev, const float* eps_actor_dev, void* stream);
/* Folded form: called BEFORE the last feature step of train(t), rlrep_defer_arm makes that step's optimizer launch (rlrep_feature_apply)
 * write snapshot set `set` as well -- the minibatch slices, noise and step counter by extra blocks, the f_target block by the lanes that
 * produce its new values -- and the rlrep_defer_snapshot that follows with the same arguments launches nothing (one dependent launch
 * less on the chain that bounds vlsac's train(): agent/vlsac/vlsac_agent.py:245-273 has no counterpart, it is a scheduling device).
 * The caller's ordering duties move accordingly: the set must be free when that LAST feature step is issued.  Returns 1 if armed, 0 if
 * the agent / configuration has no folded form (then rlrep_defer_snapshot copies as before). */
int32_t rlrep_defer_arm(rlrep_agent* agent, int32_t set, const float* eps_critic_dev, const float* eps_actor_dev);
int32_t rlrep_deferred_critic_actor(rlrep_agent* agent, int32_t set, void* stream);
/* The same in four parts for data-parallel callers (all-reduce of the critic / actor gradient slices after parts 0 and 2):
 * 0 critic backward, 1 critic apply (+ period-gated critic-target Polyak), 2 actor backward, 3 actor + temperature apply. */
int32_t rlrep_deferred_part(rlrep_agent* agent, int32_t set, int32_t part, void* stream);
/* Host-only: closes a rlrep_begin_train / rlrep_train_prologue bracket without launching anything (the critic-target update of a
 * deferred train() runs inside rlrep_deferred_critic_actor). */
int32_t rlrep_end_train(rlrep_agent* agent);

/* ctrlsac: frozen_phi, frozen_phi_target <- phi (ctrlsac_agent.py:344-346). No-op for other agents. */
int32_t rlrep_sync_frozen(rlrep_agent* agent, void* stream);

/* ---- inference ---------------------------------------------------------------------------- */
/* action[n,A] = tanh(mu + eps*std) (eps_dev != NULL) or tanh(mu) (NULL), clamped to [lo,hi]. */
int32_t rlrep_actor_forward(rlrep_agent* agent, const float* obs_dev, int32_t n, const float* eps_dev,
                            float lo, float hi, float* action_dev, void* stream);

/* SACAgent.select_action for ONE observation (sac_agent.py:89-96; main.py:126 calls it once per environment step) in ONE launch: the three
 * actor layers, the tanh-Gaussian head and -- explore != 0 -- the standard-normal draw rlrep_fill_normal(eps[A], 1, seed, offset) would give,
 * action = clamp(tanh(mu + eps * std), lo, hi) (explore == 0: tanh(mu)).  obs[S] / action[A]: device pointers, or (the *_on_host flags)
 * pinned host buffers, which the kernel then reads / writes in place: no copy on either side, the caller synchronises `stream` and reads. */
int32_t rlrep_select_action(rlrep_agent* agent, const float* obs, int32_t obs_on_host, int32_t explore, uint64_t seed, uint64_t offset,
                            float lo, float hi, float* action, int32_t action_on_host, void* stream);

/* rlrep_select_action for `rows` observations in ONE launch (additive to ABI 4; vector host environments, parallel evaluation episodes): one
 * workgroup per row.  Row e reads obs[e * S ..], writes action[e * A ..] and draws at offset + (e << 20): with offset = c << 20 that is E
 * successive rlrep_select_action calls at call counters c, c + 1, ... in row order, and every row is bit for bit what rlrep_select_action
 * computes for that observation at that offset (same kernel body, same summation order; rows == 1 gives its bytes).  obs [rows, S] /
 * action [rows, A]: device pointers or (the *_on_host flags) pinned host buffers read / written in place.  rows in [1,
 * RLREP_SELECT_MAX_ROWS] (at most one workgroup per CU).  Refused with RLREP_ERR_ARG before anything is launched, the message starting
 * with "select_action_n:": a null argument, rows outside the range, a seed group's handle, a *_on_host buffer that is not pinned. */
#define RLREP_SELECT_MAX_ROWS 256
int32_t rlrep_select_action_n(rlrep_agent* agent, const float* obs, int32_t obs_on_host, int32_t rows, int32_t explore, uint64_t seed,
                              uint64_t offset, float lo, float hi, float* action, int32_t action_on_host, void* stream);

/* The actor for `rows` DEVICE-RESIDENT observations in ONE launch (additive to ABI 4; simulators that live on the GPU): a 256-thread workgroup
 * takes 16 rows through actor.trunk.{0,2,4} with fp32 MFMAs, the activations in LDS, so every weight it fetches serves 16 rows.  Row e reads
 * obs_dev[e * ld_obs ..], writes action_dev[e * ld_act ..] (ld_obs >= S, ld_act >= A: column views of wider tensors work) and draws at
 * offset + (e << 20) as rlrep_select_action_n does.  A row's action depends on its observation, the weights and its draw alone -- not on rows,
 * on its tile or on its place in it (one accumulation order for every row) -- and agrees with rlrep_select_action_n within fp32 summation order.
 * Stream-ordered: no copy, no allocation, no synchronisation; nothing is rebuilt when `rows` changes.  Refused with RLREP_ERR_ARG before
 * anything is launched, the message starting with "act_device:": a null argument, rows outside [1, RLREP_ACT_MAX_ROWS], a row stride below the
 * row width, a seed group's handle, dimensions whose activation tiles exceed the LDS of one workgroup. */
#define RLREP_ACT_MAX_ROWS 65536
int32_t rlrep_act_device(rlrep_agent* agent, const float* obs_dev, int64_t ld_obs, int32_t rows, int32_t explore, uint64_t seed, uint64_t offset,
                         float lo, float hi, float* action_dev, int64_t ld_act, void* stream);
/* n DEVICE-RESIDENT transitions into the replay ring in ONE launch (additive to ABI 4): ring rows start, start + 1, ... (modulo max_size) become
 * [s[i], a[i], s2[i], r[i], d[i]] from s [n, S] / a [n, A] / s2 [n, S] with row strides ld_s / ld_a / ld_s2 and r [n] / d [n]; size_dev (may be
 * NULL) receives new_size as rlrep_replay_add_sized writes it.  Refused by name ("replay_add_cols:") before the launch: a null ring or array,
 * n outside [1, max_size], row_floats != 2 S + A + 2, start outside the ring, a row stride below its width. */
int32_t rlrep_replay_add_cols(float* ring_dev, int64_t max_size, int32_t row_floats, int64_t start, int32_t S, int32_t A, const float* s, int64_t ld_s,
                              const float* a, int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n, int32_t* size_dev,
                              int32_t new_size, void* stream);

/* ---- the simulator loop as one graph replay (additive to ABI 4) --------------------------------------------------------------
 * rlrep_act_device and rlrep_replay_add_cols take the call counter, `start` and `new_size` by value, so a captured graph would repeat one
 * iteration.  The two forms below read them from a loop record instead: ctl_dev, int64[RLREP_LOOP_CTL_WORDS] in caller-owned device memory
 * (word 0 calls: the select_action call counter; 1 t_global: environment steps; 2 iter: loop iterations; 3 next_ptr, 4 start, 5 size: the ring
 * cursor; 6 warm: the iteration in flight is a warm-up one; 7 unused).  The caller writes words 0-3 and 5 before the first iteration; one
 * iteration is the act form, the simulator's step, the append form, in that order on one stream.  In either launch no thread writes a word that
 * a workgroup of the same launch reads: the act form reads calls / t_global / iter and one of its threads sets start = next_ptr, next_ptr =
 * (next_ptr + rows) mod max_size, size = min(size + rows, max_size), warm = (t_global < start_timesteps); the append form reads start / size /
 * warm and one of its threads publishes size to size_dev and sets iter += 1, t_global += n, and calls += n unless warm.  Each is ONE launch,
 * stream-ordered and capturable: no copy, no allocation, no synchronisation.
 *
 * rlrep_act_device_ctl: row e's network output is bit for bit rlrep_act_device(explore = 1, offset = (calls + 1) << 20).  Behind it the
 * exploration mix: row e takes min(max(lo + (hi - lo) * u_j, lo), hi) in every component j (each operation rounded to fp32 on its own) if
 * t_global < start_timesteps, or if its pick is below eps_greedy.  The draws are Philox4x32-10 blocks keyed by `seed` with counter
 * {iter lo, iter hi, e, 0xE2000000 + q}: the pick is word 0 of block q = 0, u_j word (1 + j) mod 4 of block (1 + j) / 4, each word w taken
 * as ((w >> 8) + 0.5) / 2^24.  Refused with RLREP_ERR_ARG before the launch ("act_device_ctl:"): a null argument, rows outside
 * [1, RLREP_ACT_MAX_ROWS] or above max_size, a row stride below the row width, a seed group's handle, eps_greedy outside [0, 1], dimensions
 * whose activation tiles exceed the LDS of one workgroup.
 * rlrep_replay_add_cols_ctl: rlrep_replay_add_cols with start and the fill level from the record.  Refused by name ("replay_add_cols_ctl:")
 * before the launch: a null ring, array or record, n outside [1, max_size], row_floats != 2 S + A + 2, a row stride below its width. */
#define RLREP_LOOP_CTL_WORDS 8
int32_t rlrep_act_device_ctl(rlrep_agent* agent, const float* obs_dev, int64_t ld_obs, int32_t rows, uint64_t seed, float lo, float hi, float* action_dev,
                             int64_t ld_act, int64_t* ctl_dev, int64_t max_size, float eps_greedy, int64_t start_timesteps, void* stream);
int32_t rlrep_replay_add_cols_ctl(float* ring_dev, int64_t max_size, int32_t row_floats, int32_t S, int32_t A, const float* s, int64_t ld_s, const float* a,
                                  int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n, int32_t* size_dev, int64_t* ctl_dev,
                                  void* stream);

/* ---- fused simulators for the simulator loop (additive to ABI 4; DESIGN.md 6i "Fused simulators", csrc/sim_step.hip) -------------------------
 * n environments (1..RLREP_SIM_MAX_ENVS) of one kind (RLREP_ENV_PENDULUM, RLREP_ENV_MOUNTAIN_CAR_CONTINUOUS: the device environments' dynamics,
 * observation, reward and done_bool rule) stepped by ONE launch, one thread per environment.  The state is caller-owned device memory,
 * structure of arrays (rlrep_sim_state): x0, x1 the two fp64 state words; ep_return the fp64 sum of the fp32 rewards of the running episode;
 * last_return the return of the last finished one; t the step in the episode, -1 = ended and frozen; episodes the finished episodes; starts
 * the start states drawn so far; obs [n, S] float32, the current observation, updated in place.  Start state k of environment e is the kind's
 * start of the Philox4x32-10 block with key `seed` and counter {k lo, k hi, e, 0xE3000000}.
 *   rlrep_sim_start            every environment begins a new episode from start state starts[e]: starts[e] += 1, t = 0, ep_return = 0, obs =
 *                              the start's observation; episodes and last_return stay.
 *   rlrep_sim_step             act[e * ld_act] is the RAW action (the kinds clip it themselves).  Writes next_obs[e], reward[e] and done[e]
 *                              (float32 0 / 1: the goal reached before the limit's step), ep_return += reward; where the episode has ended (the
 *                              goal, or the time limit) last_return = ep_return, episodes += 1 and the environment restarts as rlrep_sim_start
 *                              does; otherwise t += 1 and obs = next_obs.  With auto_restart = 0 an environment that ended is frozen instead
 *                              (t = -1, its state, obs and ep_return as the last step left them): its step writes next_obs = obs, reward = 0,
 *                              done = 0 and changes nothing.
 *   rlrep_sim_step_append_ctl  the step, and transition e packed into ring row (start + e) mod max_size as [obs before the step, the action as
 *                              given, next_obs, reward, done], start from the loop record as rlrep_act_device_ctl left it; one thread does
 *                              what rlrep_replay_add_cols_ctl's does (size to size_dev, which may be NULL; iter += 1, t_global += n, calls += n
 *                              unless warm), under the same rule.  With it an iteration in front of train() is two launches.
 * Each is ONE launch, stream-ordered and capturable: no copy, no allocation, no synchronisation, nothing read on the host.  Refused with
 * RLREP_ERR_ARG before any launch, the message starting with the entry point's name ("sim_start:", "sim_step:", "sim_step_append_ctl:"): a
 * null pointer, an unknown kind, n outside [1, RLREP_SIM_MAX_ENVS] or above max_size, ld_act below the kind's A, row_floats != 2 S + A + 2.
 * rlrep_sim_state_bytes: sizeof(rlrep_sim_state), for bindings to check their mirror against. */
#define RLREP_SIM_MAX_ENVS 65536
typedef struct rlrep_sim_state {
    double* x0; double* x1; double* ep_return; double* last_return;
    int32_t* t; int64_t* episodes; int64_t* starts; float* obs;
    int32_t kind, n;
    uint64_t seed;
    int32_t auto_restart, reserved;
} rlrep_sim_state;
int32_t rlrep_sim_state_bytes(void);
int32_t rlrep_sim_start(const rlrep_sim_state* sim, void* stream);
int32_t rlrep_sim_step(const rlrep_sim_state* sim, const float* act, int64_t ld_act, float* next_obs, float* reward, float* done, void* stream);
int32_t rlrep_sim_step_append_ctl(const rlrep_sim_state* sim, const float* act, int64_t ld_act, float* ring_dev, int64_t max_size, int32_t row_floats,
                                  int32_t* size_dev, int64_t* ctl_dev, void* stream);

/* ---- fused simulators of a kind compiled at run time (additive to ABI 4; DESIGN.md 6i.2, csrc/sim_jit.h, csrc/sim_jit.hip) -------------------
 * The caller hands over the C++ text of ONE struct, `name` (csrc/sim_jit.h documents it; rlrep_amd/envs/kinds/ holds two examples): NX state
 * doubles (1..RLREP_SIMX_MAX_NX), S observations (1..RLREP_SIMX_MAX_S), A actions (1..RLREP_SIMX_MAX_A), LIMIT >= 1, TERMINATES, and the
 * functions start, observe and dynamics.  rlrep_sim_kind_compile compiles sim_jit.h + that text + static_asserts that hold the struct's
 * constants to the description + the three kernels for the current device with hiprtc (-O3 -ffp-contract=off: fp64 arithmetic as written) and
 * loads the module; the kernels are launched with hipModuleLaunchKernel.  A compile failure is RLREP_ERR_HIP with the compiler's log, from
 * its first error on and truncated, in rlrep_last_error().  rlrep_sim_kind_source writes the text that would be compiled (NUL-terminated,
 * truncated to cap) and returns its full length, or a negative RLREP_ERR_*; rlrep_sim_kind_code compiles that text for `arch` (e.g. "gfx950")
 * WITHOUT a device into code_out (cap bytes) and sets *size_out -- for checking a kind where no GPU is.  rlrep_sim_kind_info: the
 * description's constants and, per kernel (0 start, 1 step, 2 step_append_ctl), registers, scratch (spill) bytes and static LDS bytes as
 * hipFuncGetAttribute reported them after the load.  Kinds are independent objects: any number live at once, destroyed in any order.  A
 * kind's record BEGINS with its rlrep_sim_kind_info_t, and the refusals of rlrep_simx_* read nothing else of it.
 *
 * rlrep_simx_state is rlrep_sim_state with `x` float64 [NX, n] (word i of environment e at x[i * n + e]) in place of x0 / x1.  Block q of
 * start state k of environment e is the Philox4x32-10 block with key `seed` and counter {k lo, k hi, e, 0xE3000000 + q}; start() receives
 * 4 * ceil(NX / 2) words.  rlrep_simx_start / _step / _step_append_ctl are rlrep_sim_start / _step / _step_append_ctl rule for rule, with
 * act[e * ld_act + j], j < A, and ring row [s | a_0..a_{A-1} | s' | r | done].  Each is ONE launch, stream-ordered and capturable: no copy,
 * no allocation, no synchronisation, nothing read on the host.
 * Refused with RLREP_ERR_ARG before any GPU call, the message starting with the entry point's name ("sim_kind_compile:", "simx_start:",
 * "simx_step:", "simx_step_append_ctl:"): a null description, name or kind; a null or empty source; S, A, NX or limit outside the caps; a
 * null array; n outside [1, RLREP_SIM_MAX_ENVS] or above max_size; ld_act below A; row_floats != 2 S + A + 2. */
#define RLREP_SIMX_MAX_NX 8
#define RLREP_SIMX_MAX_S 16
#define RLREP_SIMX_MAX_A 8
typedef struct rlrep_sim_kind rlrep_sim_kind;
typedef struct rlrep_sim_kind_desc {
    const char* name;                  /* the struct's name in `source` (a C identifier) */
    const char* source;                /* the C++ text of the struct (and whatever helpers it needs) */
    int32_t S, A, NX, limit, terminates, reserved;
} rlrep_sim_kind_desc;
typedef struct rlrep_sim_kind_info_t {
    int32_t S, A, NX, limit, terminates, reserved;
    int32_t regs[3], scratch_bytes[3], lds_bytes[3];
} rlrep_sim_kind_info_t;
typedef struct rlrep_simx_state {
    double* x; double* ep_return; double* last_return;
    int32_t* t; int64_t* episodes; int64_t* starts; float* obs;
    int32_t n, auto_restart;
    uint64_t seed;
} rlrep_simx_state;
int32_t rlrep_simx_state_bytes(void);
int32_t rlrep_sim_kind_compile(const rlrep_sim_kind_desc* desc, rlrep_sim_kind** kind_out);
void rlrep_sim_kind_destroy(rlrep_sim_kind* kind);
int32_t rlrep_sim_kind_info(const rlrep_sim_kind* kind, rlrep_sim_kind_info_t* info_out);
int64_t rlrep_sim_kind_source(const rlrep_sim_kind_desc* desc, char* text_out, int64_t cap);
int32_t rlrep_sim_kind_code(const rlrep_sim_kind_desc* desc, const char* arch, void* code_out, int64_t cap, int64_t* size_out);
int32_t rlrep_simx_start(const rlrep_sim_kind* kind, const rlrep_simx_state* sim, void* stream);
int32_t rlrep_simx_step(const rlrep_sim_kind* kind, const rlrep_simx_state* sim, const float* act, int64_t ld_act, float* next_obs, float* reward,
                        float* done, void* stream);
int32_t rlrep_simx_step_append_ctl(const rlrep_sim_kind* kind, const rlrep_simx_state* sim, const float* act, int64_t ld_act, float* ring_dev,
                                   int64_t max_size, int32_t row_floats, int32_t* size_dev, int64_t* ctl_dev, void* stream);

/* ---- prioritized replay for sac (additive to ABI 4; DESIGN.md 6f, csrc/per.hip) ------------------------------------------------------
 * The priorities live beside the ring in a caller-owned sum tree: tree_dev float32[2 P], P = the smallest power of two >= the ring's rows,
 * node n = tree[2n] + tree[2n + 1] (one fp32 add), row i's leaf = tree[P + i], leaves of unwritten rows 0 (the caller zeroes the tree once).
 * scal_dev float32[4] = {max_p (starts at 1), alpha, beta, eps}.  One launch each, one workgroup each, stream-ordered, no host round trip.
 *   rlrep_per_add      leaves of rows [start, start + n) mod capacity <- max_p as this launch reads it; their ancestors are recomputed.
 *   rlrep_per_rebuild  every internal node from the leaves (after the caller restored them).
 *   rlrep_per_sample   batch stratified draws: total = tree[1], seg = total / batch, draw j descends with m = (j + u_j) seg, u_j from Philox
 *                      stream element j (seed, offset + *counter_dev if given) as ((word >> 8) + 0.5) 2^-24; left while r == 0 or m < l, else
 *                      m -= l and right.  given != 0: idx_dev[batch] is an INPUT.  w_dev[j] = (pmin / p_j)^beta with pmin the smallest sampled
 *                      priority, exactly 1 where p_j == pmin or beta == 0.  The buffer must hold a row (tree[1] > 0): the caller's to check.
 *   rlrep_critic_step_weighted   rlrep_critic_step with the critic loss mean_b w[b] ((q1 - y)^2 + (q2 - y)^2); leaves
 *                      td[b] = 0.5 (|q1 - y| + |q2 - y|) in the agent's workspace (rlrep_per_td_dev).  Same launch count as rlrep_critic_step.
 *   rlrep_per_update   leaf idx[j] <- (td[j] + eps)^alpha (1 when alpha == 0; the MAXIMUM where an index repeats), max_p = max(max_p, those),
 *                      ancestors recomputed; a new priority that is not positive or not a number becomes FLT_MIN.  td_dev NULL: the last weighted critic step's (batch must be its batch).
 * The entry points that take an agent refuse, by name: a seed group's handle, an agent that is not sac, world_size > 1. */
int32_t rlrep_per_add(float* tree_dev, int64_t P, const float* scal_dev, int64_t capacity, int64_t start, int64_t n, void* stream);
int32_t rlrep_per_rebuild(float* tree_dev, int64_t P, void* stream);
int32_t rlrep_per_sample(rlrep_agent* agent, const float* tree_dev, int64_t P, const float* scal_dev, int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given,
                         uint64_t seed, uint64_t offset, const int32_t* counter_dev, void* stream);
int32_t rlrep_per_update(rlrep_agent* agent, float* tree_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch, void* stream);
int32_t rlrep_critic_step_weighted(rlrep_agent* agent, const float* eps_dev, const float* w_dev, void* stream);
const float* rlrep_per_td_dev(rlrep_agent* agent);

/* ---- prioritized replay of the CRITIC's minibatch for vlsac / ctrlsac / spedersac / diffsrsac (additive to ABI 4; DESIGN.md 6f.1, csrc/per.hip)
 * These agents reuse the slot-0 minibatch of their last feature step for the critic and actor steps; that minibatch alone is drawn from the
 * tree (tree, scalars and sampler exactly as above), every other minibatch of a train() stays the uniform draw.
 *   rlrep_per_sample_fill     rlrep_per_sample and rlrep_replay_sample(slot 0) of the drawn rows in ONE launch: idx_dev[batch] and w_dev[batch] as
 *                             rlrep_per_sample writes them, ring rows idx into minibatch slot 0.  Never skipped (it overwrites a gather the
 *                             train prologue or an optimizer launch ran) and a new batch to every prefetch, as rlrep_replay_sample is.
 *                             capacity: the ring's rows (<= P); no row outside it is read whatever a given index says.
 *   rlrep_critic_weights_arm  the NEXT rlrep_critic_step / rlrep_critic_backward runs with the critic loss mean_b w[b] ((q1 - y)^2 + (q2 - y)^2)
 *                             -- whichever program it takes, the one behind rlrep_prefetch_policy_early included; only the head launch differs
 *                             -- and writes td[b] = 0.5 (|q1 - y| + |q2 - y|) into the CALLER's td_dev.  That step disarms; so do two nulls.
 *                             Same launch count as the unweighted step.  Returns 1 armed, 0 disarmed.
 *   rlrep_per_update_td       rlrep_per_update with the caller's td_dev, no agent (as rlrep_per_add has none).
 * The two entry points that take an agent refuse, by name: a seed group's handle, a sac agent ("use rlrep_per_sample /
 * rlrep_critic_step_weighted"), world_size > 1. */
int32_t rlrep_per_sample_fill(rlrep_agent* agent, const float* ring_dev, int64_t capacity, const float* tree_dev, int64_t P, const float* scal_dev,
                              int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given, uint64_t seed, uint64_t offset, const int32_t* counter_dev,
                              void* stream);
int32_t rlrep_critic_weights_arm(rlrep_agent* agent, const float* w_dev, float* td_dev);
int32_t rlrep_per_update_td(float* tree_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch, void* stream);

/* ---- prioritized replay for sac SEED GROUPS (additive to ABI 4; DESIGN.md 6g, csrc/per_group.hip) --------------------------------------------
 * Every member has a tree and a scalar block of its own, owned by the caller: trees_dev float32[members, 2 P] (member m's tree at m * 2 P
 * floats, laid out as above), scal_dev float32[members, 4], the draw buffers idx_dev int32[members, batch] and w_dev float32[members, batch].
 * One launch each (the sample with its gather: two), grid (x, members), stream-ordered and capturable; member m computes bit for bit what the rlrep_per_* entry points compute
 * for a single agent created with seed seeds[m] on m's slices.  Retired members (rlrep_group_set_live) are skipped by all but rlrep_group_per_add.
 *   rlrep_group_per_add      rlrep_per_add for every member, retired ones included (the ring writers write every member's ring): no agent.
 *   rlrep_group_per_sample   rlrep_per_sample for every live member: key = the member's seed (rlrep_group_set_seeds), stream offset
 *                            `offset` + the member's train() counter when use_counter != 0.  ring_dev != NULL (member 0's ring; rings of
 *                            `capacity` rows ring_stride_bytes apart): a second launch GATHERS the drawn rows into the members' minibatch
 *                            slot 0 (a group has no rlrep_replay_sample); batch must then be the prepared batch (rlrep_group_prepare).
 *   rlrep_group_critic_step_weighted   rlrep_critic_step_weighted for every live member, w_dev[members, B]; discount from the member's hyper record.
 *   rlrep_group_per_update   rlrep_per_update for every live member; td_dev NULL: each member's |TD| of the last weighted critic step
 *                            (rlrep_group_per_td_dev: member 0's, member m's lies m member strides further), else float32[members, batch].
 * The entry points that take an agent refuse, by name: a single agent's handle ("not a seed group"), a ctrlsac group, world_size > 1. */
int32_t rlrep_group_per_add(float* trees_dev, int64_t P, const float* scal_dev, int32_t members, int64_t capacity, int64_t start, int64_t n, void* stream);
int32_t rlrep_group_per_sample(rlrep_agent* group, const float* trees_dev, int64_t P, const float* scal_dev, int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given,
                               uint64_t offset, int32_t use_counter, const float* ring_dev, int64_t ring_stride_bytes, int64_t capacity, void* stream);
int32_t rlrep_group_per_update(rlrep_agent* group, float* trees_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch, void* stream);
int32_t rlrep_group_critic_step_weighted(rlrep_agent* group, const float* eps_dev, const float* w_dev, void* stream);
const float* rlrep_group_per_td_dev(rlrep_agent* group);

/* ---- prioritized replay of the CRITIC's minibatch for ctrlsac SEED GROUPS (additive to ABI 4; DESIGN.md 6g.1, csrc/per_group.hip) ----------
 * The group forms of rlrep_per_sample_fill / rlrep_critic_weights_arm / rlrep_per_update_td.  Trees, scalars and draw buffers as for sac seed
 * groups above (trees_dev float32[members, 2 P], scal_dev float32[members, 4], idx_dev int32[members, batch], w_dev float32[members, batch]);
 * td_dev float32[members, batch] is the caller's too.  Member m computes bit for bit what the single-agent entry points compute for a ctrlsac
 * agent created with seed seeds[m] on m's slices; retired members (rlrep_group_set_live) are skipped: nothing of theirs is read or written.
 *   rlrep_group_per_sample_fill     rlrep_per_sample_fill for every live member in ONE launch, grid (1 + G, members): key = the member's seed,
 *                                   stream offset `offset` + the member's train() counter when use_counter != 0; rings_dev is member 0's ring,
 *                                   rings of `capacity` rows (<= P) ring_stride_bytes apart; the drawn rows go into every live member's minibatch
 *                                   slot 0.  No row outside a member's ring is read whatever a given index says.  A new batch to every
 *                                   prefetch, as rlrep_replay_sample is.  batch must be the prepared batch (rlrep_group_prepare).
 *   rlrep_group_critic_weights_arm  the NEXT rlrep_critic_step / rlrep_critic_backward of the group runs with member m's critic loss weighted by
 *                                   w_dev[m] and writes td_dev[m][b] = 0.5 (|q1 - y| + |q2 - y|).  Same launch count as the unweighted step: only
 *                                   the head launch differs.  That step disarms; so do two nulls.  Returns 1 armed, 0 disarmed.
 *   rlrep_group_per_update_td       rlrep_per_update_td for every live member, td_dev[members, batch].
 * All three accept a ctrlsac seed group on one GPU and refuse, by name: a single agent's handle ("not a seed group"), a sac group (which takes
 * rlrep_group_per_sample / rlrep_group_critic_step_weighted / rlrep_group_per_update), world_size > 1, a batch that is not the prepared batch,
 * null arguments, capacity outside [1, P]. */
int32_t rlrep_group_per_sample_fill(rlrep_agent* group, const float* rings_dev, int64_t ring_stride_bytes, int64_t capacity, const float* trees_dev, int64_t P,
                                    const float* scal_dev, int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given, uint64_t offset, int32_t use_counter,
                                    void* stream);
int32_t rlrep_group_critic_weights_arm(rlrep_agent* group, const float* w_dev, float* td_dev);
int32_t rlrep_group_per_update_td(rlrep_agent* group, float* trees_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch,
                                  void* stream);

/* ---- n-step returns for sac (additive to ABI 4; DESIGN.md 6h, csrc/nstep.hip) ---------------------------------------------------------------
 * A replay gather that follows each sampled row's trajectory forward through the ring, ONE launch, stream-ordered and capturable.  For base row
 * i0 = idx_dev[b] of a ring of max_size rows [s | a | s' | r | d] with fill level *size_dev and successor distance `stride` (the number of
 * interleaved environments that wrote the ring):  g = 1, R = r[i0], last = i0;  for k = 1 .. n - 1 with j = (last + stride) mod max_size the
 * chain continues iff d[last] == 0, j < *size_dev and the S words of s[j] equal those of s'[last] bit for bit; then g = g * gamma,
 * R = R + g * r[j], last = j.  The output row is (s, a) of i0, s' of `last`, reward R and done 1 - g (1 - d[last]), every operation one
 * correctly rounded fp32 operation: the critic heads' y = R + (1 - D) gamma tv then is the n-step target, and n = 1 is rlrep_replay_sample.
 *   rlrep_replay_sample_nstep   the gather into minibatch slot 0 of ONE sac agent, gamma = its discount.  Never skipped: it overwrites the
 *                               gather a preceding rlrep_train_prologue ran.  Refuses, by name: a seed group's handle, an agent that is not
 *                               sac, world_size > 1, n outside [1, RLREP_NSTEP_MAX], stride < 1.
 *   rlrep_replay_gather_nstep   the same rows into caller-owned arrays, no agent: xe [batch, 2 S + A] = [s, a, s'], xf [batch, S + A] = [s, a],
 *                               xf2 [batch, S + A] (columns [0, S) = s'; the rest untouched), xfpi [batch, S + A] (columns [0, S) = s), r, d [batch].
 *   rlrep_group_replay_gather_nstep   the gather into slot 0 of every live member of a sac SEED GROUP, one launch on grid (x, members): member m's
 *                               ring (rings_dev + m * ring_stride_bytes), fill level size_dev[m] and discount -- read from its hyper record on the
 *                               device, so rlrep_group_set_member_hyper holds at the next replay.  idx_per_member == 0: idx_dev lies in member 0's
 *                               block (the index pool rlrep_group_train_prologue wrote) and moves by the member stride; otherwise idx_dev is
 *                               int32[members, batch] (the draw buffers of rlrep_group_per_sample, called with a NULL ring).  batch must be the
 *                               prepared batch.  Refuses, by name: a single agent's handle ("not a seed group"), a ctrlsac group, world_size > 1. */
#define RLREP_NSTEP_MAX 16
int32_t rlrep_replay_sample_nstep(rlrep_agent* agent, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch, int64_t max_size,
                                  const int32_t* size_dev, int32_t n, int32_t stride, void* stream);
int32_t rlrep_replay_gather_nstep(const float* ring_dev, const int32_t* idx_dev, int32_t batch, int32_t S, int32_t A, int64_t max_size, const int32_t* size_dev,
                                  int32_t n, int32_t stride, float gamma, float* xe_dev, float* xf_dev, float* xf2_dev, float* xfpi_dev, float* r_dev, float* d_dev,
                                  void* stream);
/* Read-back of a minibatch slot (tests and tools): which = 0 .. 5 -> XE [batch, 2 S + A], XF [batch, S + A], XF2 [batch, S + A], XFpi [batch, S + A],
 * R [batch], D [batch], dense, inside the agent's workspace; valid once the stream has passed the gather.  A group: member 0's (member m's lies
 * m member strides further).  which = 6 -> Rn [batch], the reward array the critic heads of the representation agents read: R itself (the
 * same pointer) unless rlrep_set_critic_nstep gave it storage of its own, which lies OUTSIDE the workspace.  NULL for a bad argument. */
const float* rlrep_slot_dev(rlrep_agent* agent, int32_t slot, int32_t which);
int32_t rlrep_group_replay_gather_nstep(rlrep_agent* group, const float* rings_dev, int64_t ring_stride_bytes, const int32_t* idx_dev, int32_t idx_per_member,
                                        int32_t batch, int64_t max_size, const int32_t* size_dev, int32_t n, int32_t stride, void* stream);

/* ---- n-step CRITIC targets for vlsac / ctrlsac / spedersac / diffsrsac (additive to ABI 4; DESIGN.md 6h, csrc/nstep_targets.hip) -------------
 * The feature step of these agents models one-step dynamics from the same minibatch the critic and actor steps reuse, so the minibatch stays
 * one-step where the feature step reads it (XE, XF, R) and only what the critic and actor steps read of the NEXT state and the return is
 * replaced: XF2[:, 0:S] = s' of the chain's last row, D = 1 - gamma^(m-1) (1 - d_last), and a reward array of the heads' own, Rn = sum_k
 * gamma^k r_k.  The walk, its stopping rules and its arithmetic are those of rlrep_replay_sample_nstep above, bit for bit.
 *   rlrep_set_critic_nstep             on != 0: slot 0 (and every deferred set's snapshot) gets an Rn of its own -- one device allocation of the
 *                                      agent's, the workspace layout stays what rlrep_layout reported -- and the step programs are rebuilt with
 *                                      the critic heads reading it; on == 0: Rn is R again.  NOT stream-ordered: it synchronises the device,
 *                                      call it outside any capture.  Until it is called every program, launch count and array is what it was.
 *                                      Refuses, by name: a seed group's handle, sac (it has rlrep_replay_sample_nstep), world_size > 1.
 *   rlrep_replay_sample_nstep_targets  ONE launch behind the rlrep_replay_sample (or the train prologue, or the optimizer launch that carried
 *                                      the gather) of the slot-0 minibatch the critic reuses, in front of the feature step on it: overwrites
 *                                      XF2[:, 0:S], Rn and D of slot 0, gamma = the agent's discount; leaves XE, XF, XFpi, R and columns
 *                                      [S, S + A) of XF2.  Never skipped.  Refuses what rlrep_set_critic_nstep refuses, slot != 0, n outside
 *                                      [1, RLREP_NSTEP_MAX], stride < 1, and an agent rlrep_set_critic_nstep(agent, 1) was not called on.
 *   rlrep_replay_gather_nstep_targets  the same three arrays into caller-owned memory, no agent: xf2 [batch, S + A] (columns [0, S) written),
 *                                      rn [batch], d [batch].
 * An index outside [0, max_size) writes zeros.  Not built: prioritized replay for these agents, seed groups, data parallel. */
int32_t rlrep_set_critic_nstep(rlrep_agent* agent, int32_t on);
int32_t rlrep_replay_sample_nstep_targets(rlrep_agent* agent, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch, int64_t max_size,
                                          const int32_t* size_dev, int32_t n, int32_t stride, void* stream);
int32_t rlrep_replay_gather_nstep_targets(const float* ring_dev, const int32_t* idx_dev, int32_t batch, int32_t S, int32_t A, int64_t max_size,
                                          const int32_t* size_dev, int32_t n, int32_t stride, float gamma, float* xf2_dev, float* rn_dev, float* d_dev, void* stream);

/* ---- metrics ------------------------------------------------------------------------------ */
/* device float array of n_metrics slots, valid after the stream has passed the producing step */
const float* rlrep_metrics_dev(rlrep_agent* agent);

/* Profiling hook: launch stage `stage` of step program `program` once (0 feature_bwd, 1 feature_apply,
 * 2 critic_bwd, 3 critic_apply, 4 actor_bwd, 5 actor_apply, 6 update_target); its inputs are whatever the
 * previous full step left in the workspace.  rlrep_stage_count/_name enumerate the stages. */
/* ---- data-parallel exchanges inside the launches (csrc/comm.hip, csrc/dp_pull.h) ---------------------------
 * The reference is one process: no counterpart.  The gradient exchange belongs between its `loss.backward()` and `optimizer.step()` pairs
 * (agent/vlsac/vlsac_agent.py:153-154, 183-184, 229-230; ctrlsac_agent.py:243-244; spedersac_agent.py:211-212; diffsrsac_agent.py:311-314), the
 * batch-coupled ones inside the feature losses (spedersac_agent.py:197-205: Phibar and v over the global batch; ctrlsac_agent.py:226-231: in-batch
 * negatives over the global batch).
 * A comm owns ONE block of device memory, [arena_floats | scratch_floats | reduced region (world >= 3) | flag words], exported over hipIpc and
 * mapped by every peer: the caller passes rlrep_comm_arena() as rlrep_arenas.grad_dev, so every rank's gradients lie where every peer can read
 * them.  Lifecycle, identical on every rank: create -> handle -> (exchange the handles, world x rlrep_comm_handle_bytes() in rank order, by any
 * means: torch.distributed.all_gather_object) -> connect -> rlrep_agent_create(..., grad_dev = rlrep_comm_arena()) -> attach.  (Several ranks in
 * ONE process -- the loopback form of tools/exp/dp_loopback.py and tests -- skip handle / connect and call rlrep_comm_connect_local.)
 * After rlrep_comm_attach the optimizer launch of every attached group (rlrep_*_apply, the fused *_step entry points, the deferred chain)
 * waits -- bounded -- for the peers' gradients of that step, sums every rank's gradient of its elements IN RANK ORDER (bit-identical on every
 * rank; one-shot pull, or reduce-scatter + all-gather inside the same launch for slices of at least two_shot_floats when world >= 3) and does
 * not end before every peer has read this rank's: ZERO launches per all-reduce, nothing on the host changes between calls (hipGraph-capturable),
 * and the caller issues NO collective for those groups.  Groups above max_floats stay with the caller's all-reduce between backward and apply.
 * With scratch_floats >= rlrep_layout_info.exchange_floats the batch-coupled exchanges move into the step programs too (spedersac: pushed by the
 * column-sum launches, summed by their consumers, no launch; ctrlsac: one pull launch each) and rlrep_feature_exchange_count() drops to 0.
 * rlrep_comm_allreduce / _allgather are the same exchanges as stand-alone launches (probe / tests).  A wait that runs out (rlrep_comm_set_timeout;
 * default 120 s: a watchdog) sets a bit of the error word; the launch applies NOTHING and drains: rlrep_comm_status reads that word from mapped
 * host memory WITHOUT synchronising. */
typedef struct rlrep_comm rlrep_comm;
int32_t rlrep_comm_create(int32_t rank, int32_t world, int64_t arena_floats, int64_t scratch_floats, rlrep_comm** out);
float* rlrep_comm_arena(rlrep_comm* comm);
float* rlrep_comm_scratch(rlrep_comm* comm);
int32_t rlrep_comm_handle_bytes(void);
int32_t rlrep_comm_handle(rlrep_comm* comm, void* out, int32_t cap);
int32_t rlrep_comm_connect(rlrep_comm* comm, const void* handles);
int32_t rlrep_comm_connect_local(rlrep_comm* comm, rlrep_comm* const* peers);
int32_t rlrep_comm_set_timeout(rlrep_comm* comm, int64_t timeout_us);
int32_t rlrep_comm_attach(rlrep_agent* agent, rlrep_comm* comm, int64_t max_floats, int64_t two_shot_floats, int32_t* attached_mask);
int32_t rlrep_comm_allreduce(rlrep_comm* comm, int64_t block_offset_floats, int64_t n, float* out_dev, int32_t mode, int64_t timeout_us, void* stream);
int32_t rlrep_comm_allgather(rlrep_comm* comm, int64_t block_offset_floats, int64_t n_per_rank, void* stream);
int32_t rlrep_comm_probe_fill(rlrep_comm* comm, int64_t block_offset_floats, int64_t n, int32_t round, void* stream);
float rlrep_comm_probe_value(int32_t rank, int32_t round, int64_t i);
int32_t rlrep_comm_probe_slots(rlrep_comm* comm, int64_t n, int32_t round, float* out_dev, int64_t timeout_us, void* stream);
int32_t rlrep_comm_status(rlrep_comm* comm, uint32_t* late_mask, int32_t clear);
int32_t rlrep_comm_fine_grained(rlrep_comm* comm);
/* debug / measurement only: mark every peer as arrived for the next `ahead` epochs of `channel` in this rank's flags (one stream then plays several ranks
 * in turn; 1 << 30: one attached replica runs alone and pays the protocol, not the waiting -- tools/exp/dp_loopback.py) */
int32_t rlrep_comm_debug_preset(rlrep_comm* comm, int32_t channel, int32_t ahead);
void rlrep_comm_destroy(rlrep_comm* comm);

/* vlsac noise-critic weight images (bf16x3 shadows of critic.l1 / l4 and their targets; no reference counterpart: nn.Linear has no such
 * copies).  Default: every critic step regenerates them with one launch.  Between rlrep_images_managed(agent, 1) and (agent, 0) the step
 * entry points skip that launch (inside a rlrep_begin_train .. rlrep_update_target bracket the critic group's optimizer launch keeps live and
 * target images current) and the caller runs rlrep_refresh_images after anything else wrote critic / critic_target.  images_managed returns
 * 1 if the agent keeps images, 0 if there is nothing to manage. */
int32_t rlrep_images_managed(rlrep_agent* agent, int32_t on);
int32_t rlrep_refresh_images(rlrep_agent* agent, void* stream);

/* Chained feature steps (vlsac, one GPU; no reference counterpart: a launch-saving form of `for _ in range(extra_feature_steps + 1):
 * feature_step(...)`, vlsac_agent.py:250-256).  Called after rlrep_prefetch_batch has armed the NEXT step's minibatch and before this step's
 * rlrep_feature_step: this step's weight-gradient launch then applies the optimizer to the two first layers in its epilogues, and its optimizer
 * launch skips them and carries the next step's first launch (encoder.l1 / f.l1, rows read from the ring through the index pool) as leading
 * tiles; the next rlrep_feature_backward starts at its second launch.  Same arithmetic in the same order per parameter.  1: armed, 0: not
 * available (nothing changes).  The next call on the agent's feature path must be that next step (plain, no rlrep_prefetch_policy_early). */
int32_t rlrep_feature_chain_next(rlrep_agent* agent);

int32_t rlrep_stage_count(rlrep_agent* agent, int32_t program);
const char* rlrep_stage_name(rlrep_agent* agent, int32_t program, int32_t stage);
int32_t rlrep_run_stage(rlrep_agent* agent, int32_t program, int32_t stage, void* stream);
/* What a stage launches (bench.py groups the stages of a train() into kernel families with it, and prices them): the kernel family
 * (RLREP_ENGINE_*), the ALGORITHMIC flops of its products (2 * rows * columns * inner length per product; 0 for non-GEMM stages) and the
 * algorithmic bytes (every operand and result of a product once, 4 bytes per element; optimizer stages: 28 bytes per parameter + 12 per
 * Polyak-averaged target element).  No reference counterpart (the reference has no kernels of its own). */
#define RLREP_ENGINE_OTHER 0        /* elementwise / loss / gather / copy kernels */
#define RLREP_ENGINE_GEMM16 1       /* gemm16_kernel / gemm16_duo_kernel: the 16-row fp32-MFMA tile engine */
#define RLREP_ENGINE_HEADS_VAE 2    /* heads_vae_kernel (vlsac: both Gaussian heads + sample / KL on a 16 x 16 tile) */
#define RLREP_ENGINE_LDS64 3        /* gemm_lds_kernel<64,...> (+ its split-K finishing blocks) */
#define RLREP_ENGINE_LDS128 4       /* gemm_lds_kernel<128,...> on fp32 MFMA */
#define RLREP_ENGINE_X3 5           /* gemm_x3_kernel: the 128-wide tile on the bf16 pipe, exact three-way split */
#define RLREP_ENGINE_NOISE_CRITIC 6 /* nc_fwd / nc_dx / nc_dw kernels (vlsac noise critic, bf16x3) */
#define RLREP_ENGINE_OPTIMIZER 7    /* adam_kernel (Adam + Polyak + metric finalisation + riders) */
#define RLREP_ENGINE_SCORE 8        /* diffsr score kernels (HBM-bound pass over [B, F*S]) */
int32_t rlrep_stage_info(rlrep_agent* agent, int32_t program, int32_t stage, int32_t* engine, double* flops, double* bytes);

/* Unit-test hook: ONE product on the path's GEMM engines with caller buffers (tests/test_gemm_engines.py checks both
 * engines against NumPy on every operand layout, epilogue, ragged edge and split-K plan).
 *   C[R,Cn] = epilogue( sum_k opA(r,k) * opB(c,k) )
 *   la / lb: 0 = row-major operand [rows, K] (ld = row stride), 1 = k-major operand [K, rows]
 *   epi: 0 forward: act(acc + bias)        (act: 0 none, 1 relu, 2 elu, 3 sin (+ pre-activation to out2), 4 tanh)
 *        1 dX:      acc * act'(aux), flags & 1: C += ...
 *        3 dW:      acc, flags & 1: C += ..., flags & 2: out2[r] = sum_k opA(r,k) (bias gradient)
 *   engine: 0 = 16-row tile engine (gemm16), 1 = LDS-tiled engine (gemm_lds), 2 = its 128-wide tile on the bf16 pipe
 *   (bf16x3: three-way operand split, six MFMAs, fp32 accuracy); bt (0 auto, 64, 128; with engine 2 also 256 = the persistent
 *   256 x 128 tile, which has no sin / tanh epilogue) and splits
 *   (0 auto) override the LDS engine's plan; workspace holds its split-K slabs (splits*R*(Cn+1) floats), which a finishing launch adds
 *   in split order -- or, with flags & 4 on the 64-wide bf16x3 tile (engine 2, bt 64), the last split workgroup of every output tile
 *   (a ticket word per tile behind the slabs: + ceil(R/64)*ceil(Cn/64) floats of workspace), bit-identically and without a second launch.
 * Returns 0, or RLREP_ERR_ARG when the engine cannot run the shape (alignment rules in gemm_lds.hip). */
int32_t rlrep_gemm(int32_t engine, int32_t la, int32_t lb, const float* a_dev, int32_t lda, const float* b_dev, int32_t ldb,
                   float* c_dev, int32_t ldc, int32_t rows, int32_t cols, int32_t inner, int32_t epi, int32_t act, int32_t flags,
                   const float* bias_dev, const float* aux_dev, int32_t ldaux, float* out2_dev, int32_t bt, int32_t splits,
                   float* workspace_dev, int64_t workspace_floats, void* stream);

/* Unit-test hook of the 16-row tile engine alone (tests/test_gemm16_engine.py): a TABLE of 1..8 independent products in ONE launch, through
 * the launchers and the tile numbering the step programs use -- which rlrep_gemm (one task, 16-column tiles) cannot reach: 32- / 64-column
 * tiles (nf = 2 / 4), multi-task directories, the front ends that load operands from preloaded scalars (one or two tasks with inner % 256 == 0
 * or inner <= 64; three or four tasks of one shape), the weight-gradient launch's dealing of tiles to the XCDs, and the duo form.
 * Fields as rlrep_gemm's arguments; out2 of a forward task has c's row stride; r1u[rows] / r1v[cols]: dX adds r1u[r] * r1v[c] to the product
 * before the activation derivative (both or neither); scale multiplies the product (1.0: none).
 *   duo_split == 0: every task has layouts la / lb and tiles of 16 * nf columns;
 *   duo_split  > 0: tasks [0, duo_split) are row-major x k-major products (dX form, 16-column tiles), the rest k-major x k-major ones
 *                   (weight-gradient form, 16 * nf2 columns, nf2 = 1 or 4) -- one launch of both forms; la / lb are ignored.
 * Which front end the launch got: the difference of rlrep_front_end_counts around the call.  RLREP_ERR_ARG (before any GPU call) for ntasks
 * outside 1..8, nf not in {1, 2, 4}, a null a / b / c, non-positive extents or an epilogue outside {0, 1, 3}.  The fused-loss, policy and
 * reparameterisation epilogues (the last with its fused short product and mse phase) have a hook of their own, rlrep_heads; the ELU form of the
 * fused short product, its forward form and the optimizer epilogues are reachable only through an agent. */
typedef struct rlrep_gemm16_task {
    const float* a; const float* b; float* c;
    int32_t lda, ldb, ldc, rows, cols, inner;
    int32_t epi, act, flags;              /* as rlrep_gemm: epi 0 / 1 / 3, act 0..4, flags bit 0 accumulate, bit 1 bias gradient */
    const float* bias; const float* aux; int32_t ldaux; float* out2;
    const float* r1u; const float* r1v;   /* dX: optional rank-1 term, may be NULL */
    float scale;                          /* multiplies the product; 1.0 default */
} rlrep_gemm16_task;
int32_t rlrep_gemm16_table(int32_t la, int32_t lb, int32_t nf, const rlrep_gemm16_task* tasks, int32_t ntasks,
                           int32_t duo_split, int32_t nf2, int32_t low_prio, void* stream);

/* Host-only (no GPU call): the GEMM engine the program builder picks for a product of these dimensions and layouts --
 * *engine 0 = 16-row tile engine, 1 = LDS-tiled fp32-MFMA, 2 = LDS-tiled bf16x3 -- with its tile edge (64 / 128; 256 = the persistent
 * 256 x 128 tile of engine 2), split-K plan and which sides fall back to 4-byte accesses (bit 0: A, bit 1: B, bit 2: C). */
int32_t rlrep_gemm_plan(int32_t la, int32_t lb, int32_t rows, int32_t cols, int32_t inner, int32_t lda, int32_t ldb, int32_t ldc,
                        int32_t* engine, int32_t* tile, int32_t* splits, int32_t* kchunk, int32_t* scalar_sides);

/* Unit-test hook of the representation-loss kernels (csrc/replearn.hip; tests/test_replearn_kernels.py): ONE launch of one kernel on caller
 * buffers, with no agent, through the launcher the step programs use and with the block counts the program builder computes.  The records
 * carry the fields of the launch records (csrc/kparams.h) except the group counter (always null: nothing is bumped), the data-parallel slot
 * descriptor (always world 1) and the block counts.  No group form is reachable this way.
 *   RLREP_RL_INFONCE        ctrlsac InfoNCE on given scores S [B, ncols] (in place: dS out); rhat given, or Z / theta_w / theta_b given (ZM null)
 *   RLREP_RL_SCORE_INFONCE  the score matrix S = Z ZM^T and its InfoNCE in one launch (S out only); needs F % 64 == 0, ncols <= 256,
 *                           ldZ % 4 == 0, ldZM % 4 == 0 and Z, ZM, theta_w on 16-byte boundaries
 *   RLREP_RL_COLSUM         out[f] = sum_k w[k] X[k, f] (w null: plain); X2 given: a second set in the same launch (+ outb2 = sum of w2, optional)
 *   RLREP_RL_SPEDER_ROWS / RLREP_RL_SPEDER_GRADS   spedersac's spectral loss rows / its gradients ([2B, F] blocks)
 *   RLREP_RL_PERTURB / RLREP_RL_SCORE              diffsrsac's perturbation / denoising score matching (U [B, F, S] in, dU out in place)
 *   RLREP_RL_REG_STATS      diffsrsac's ELU-layer regulariser statistics of four (x [B, H], Gram matrix [H, H]) pairs; partial has
 *                           4 * (ceil(H*H / 1024) + ceil(B / 4)) floats
 *   RLREP_RL_COPY2          d1[i] = d2[i] = src[i] (d2 may be null)
 * partial of the InfoNCE / spectral rows kernels: 2 / 3 floats per block, min(ceil(B / 4), 128) blocks (row i in block (i / 4) % blocks);
 * of the fused form 2 per block of 16 rows; of score matching one per sample.
 * Refused with RLREP_ERR_ARG and a message starting "replearn:", before any GPU call: an unknown kernel, a null required pointer, a
 * non-positive extent, a row stride below the row's width, diag_off < 0 or diag_off + B > ncols, a regulariser batch below 2, the fused
 * form's preconditions above, and a score-matching S whose row kernel would need more than 64 KB of dynamic LDS (5 * S floats). */
enum { RLREP_RL_INFONCE = 0, RLREP_RL_SCORE_INFONCE = 1, RLREP_RL_COLSUM = 2, RLREP_RL_SPEDER_ROWS = 3, RLREP_RL_SPEDER_GRADS = 4,
       RLREP_RL_PERTURB = 5, RLREP_RL_SCORE = 6, RLREP_RL_REG_STATS = 7, RLREP_RL_COPY2 = 8 };
typedef union rlrep_replearn_args {
    struct { float* S; int32_t ldS, ncols, diag_off; const float* rhat; const float* r; float* drhat; float* partial; int32_t B; float inv_batch;
             const float* Z; int32_t ldZ, F; const float* theta_w; const float* theta_b; const float* ZM; int32_t ldZM; } infonce;
    struct { const float* X; int32_t ldX; const float* w; float* out; int32_t rows, F;
             const float* X2; int32_t ldX2; const float* w2; float* out2; float* outb2; int32_t rows2; } colsum;
    struct { const float* phi; const float* mu; const float* mu_r; const float* phibar; const float* theta_w; const float* theta_b; const float* r;
             float* c; float* drhat; float* partial; int32_t B, F; float inv_batch; } speder_rows;
    struct { const float* phi; const float* mu; const float* c; const float* drhat; const float* phibar; const float* v; const float* theta_w;
             float* Gphi; float* Gmu; int32_t B, F; float inv_batch; } speder_grads;
    struct { const float* alphabars; const int32_t* idx; const float* s2; int32_t ld_s2; const float* eps; float* XN; float* TGT; int32_t B, S; } perturb;
    struct { float* U; const float* PHI; const float* TGT; const float* alphabars; const int32_t* idx; float* GPHI; float* partial;
             int32_t B, F, S; float sigma, inv_batch; } score;
    struct { const float* X[4]; const float* C[4]; int32_t B, H; float lambda; float* partial; } reg_stats;
    struct { const float* src; float* d1; float* d2; int64_t n; } copy2;
} rlrep_replearn_args;
int32_t rlrep_replearn(int32_t kernel, const rlrep_replearn_args* args, void* stream);

/* Host-only (no GPU call): the kernel the score-matching launcher picks for a [F, S] block per sample whose U is (u_aligned16 != 0) or is not
 * on a 16-byte boundary, under the RLREP_ENABLE=score_ch / RLREP_DISABLE=score_small settings in force at the call.  *form:
 * one pass through LDS in column chunks of 32 / 64 / 128 floats, a thread per row with 1 / 2 / 4 rows per thread, the 16-byte two-pass
 * kernel, the lanes-over-columns two-pass kernel. */
enum { RLREP_SCORE_LDS32 = 0, RLREP_SCORE_LDS64 = 1, RLREP_SCORE_LDS128 = 2, RLREP_SCORE_SMALL1 = 3, RLREP_SCORE_SMALL2 = 4, RLREP_SCORE_SMALL4 = 5,
       RLREP_SCORE_VEC = 6, RLREP_SCORE_ROWS = 7 };
int32_t rlrep_diffsr_score_plan(int32_t S, int32_t F, int32_t u_aligned16, int32_t* form);

/* Host-only: the engine the builder picks for the vlsac noise critic's first layer (vlsac_agent.py:44-63) with `heads` heads in one
 * launch -- *engine 0 = fp32 MFMA, 1 = bf16x3 (needs F % 32 == 0 and 16-byte rows; RLREP_NC_X3=0 turns it off) -- and its
 * workgroup tile: *rows batch rows x *cols hidden units. */
int32_t rlrep_nc_fwd_plan(int32_t heads, int32_t batch, int32_t feature_dim, int32_t hidden_dim,
                          int32_t* engine, int32_t* rows, int32_t* cols);

/* Unit-test hook of the vlsac noise-critic kernels (csrc/noisecritic.hip; tests/test_noisecritic_kernels.py): ONE launch of one kernel of the
 * family on caller buffers, with no agent, through the launchers the step programs use (rl_launch_nc_fwd / _dx / _dw) and the tile numbering
 * the program builder uses.  The records carry the fields of the launch records (csrc/kparams.h NcFwdTask, NcDxTask, NcDwBatch) except the
 * tile fields; the number of noise rows is 20.  form (may be null) receives the form that was launched.
 *   RLREP_NC_FWD  Hm[b, j] = (1/20) sum_n elu(W[j, :] . (mean[b] + exp(clamp(lstd[b])) noise[n]) + bias[j]) for 1..4 tasks; U (the elu outputs
 *                 [B * 20, H]) and sigma_out ([B, F]) may be null per task.  w3 (may be null per task): device scratch of
 *                 rlrep_nc_w3_bytes(H, F) bytes that the hook fills with the bf16x3 images of W before the forward launch (the production
 *                 producer: the shadow launch, kind 1) and hands to the kernel; needs F % 32 == 0 and W on a 16-byte boundary.
 *                 g2 (0 = planner; 1, 2, 4 row groups of 4 batch rows a workgroup) and cols (0 = planner; 64, 128 hidden units a workgroup)
 *                 override the plan.  Engine and the K-chunked form follow RLREP_DISABLE=x3 / RLREP_ENABLE=nc_fwd_chunk as in production.
 *                 form[4]: engine (0 fp32 MFMA, 1 bf16x3), g2, cols, K-chunked.
 *   RLREP_NC_DX   G[b, k] = dmean, G[b, F + k] = dlog_std of one or two heads.  form[2]: engine, 16-byte loads of U / GH (fp32 engine).
 *   RLREP_NC_DW   gW [H, F], gb [H] of one or two tasks; sigma [B, F] dense is an input.  lean: the 128-register build of the fp32 kernel;
 *                 splits: 0 = the planner's count, else 1..16; slab (ntasks * splits * H * F floats) and bslab (ntasks * splits * H floats)
 *                 hold the split partials of the bf16x3 form, which nc_dw_fin_kernel adds in split order (never folded into an optimizer
 *                 launch here); the bf16x3 form steps by noise row unless RLREP_DISABLE=nc_dw_rows.  form[4]: engine, lean, splits, by noise row.
 * Refused with RLREP_ERR_ARG and a message starting "noisecritic:", before any GPU call: an unknown kernel, a null required pointer, a count of
 * tasks / heads outside its range, a non-positive extent, F % 4 != 0, a row stride below the row's width or no multiple of 4, mean / lstd /
 * noise / sigma / sigma_out off a 16-byte boundary (the kernels stage them with unconditional 16-byte accesses; rlrep_layout guarantees the
 * alignment to the step programs), tasks of one forward launch that differ in F (its LDS table is sized once) or, where the bf16x3 engine
 * would take them, in B or H; dW tasks that differ in B, F or H; an override the launcher cannot run (K-chunked with cols 64, a whole table
 * past 64 KB, g2 != 2 on bf16x3); w3 with F % 32 != 0 or a W / w3 off a 16-byte boundary; slabs that are missing or too small; a seed
 * group's call in progress. */
enum { RLREP_NC_FWD = 0, RLREP_NC_DX = 1, RLREP_NC_DW = 2 };
typedef struct rlrep_nc_fwd_task {
    const float* mean; const float* lstd; int32_t ld_ml; const float* noise; const float* W; const float* bias; void* w3;
    float* Hm; float* U; float* sigma_out; int32_t B, F, H;
} rlrep_nc_fwd_task;
typedef struct rlrep_nc_dw_task {
    const float* U; const float* GH; int32_t ldgh; const float* mean; const float* sigma; int32_t ld_ml; const float* noise;
    float* gW; float* gb; int32_t B, F, H;
} rlrep_nc_dw_task;
typedef union rlrep_noisecritic_args {
    struct { int32_t ntasks, g2, cols; int32_t* form; rlrep_nc_fwd_task t[4]; } fwd;
    struct { const float* GH[2]; int32_t ldgh; const float* U[2]; const float* W[2]; const float* noise; const float* lstd; int32_t ld_l;
             float* G; int32_t ldg; int32_t B, F, H, nheads; int32_t* form; } dx;
    struct { int32_t ntasks, lean, splits; float* slab; int64_t slab_floats; float* bslab; int64_t bslab_floats; int32_t* form;
             rlrep_nc_dw_task t[2]; } dw;
} rlrep_noisecritic_args;
int32_t rlrep_noisecritic(int32_t kernel, const rlrep_noisecritic_args* args, void* stream);

/* Host-only: bytes of the per-task w3 scratch of RLREP_NC_FWD (the three bf16 images of W [H, F] and the producer's table entry behind them);
 * 0 for a non-positive extent. */
int64_t rlrep_nc_w3_bytes(int32_t hidden_dim, int32_t feature_dim);

/* Host-only: whether the fp32 forward of width feature_dim runs K-chunked with g2 row groups a workgroup (*chunked; RLREP_ENABLE=nc_fwd_chunk
 * forces it), and the split count of the bf16x3 weight gradient (*splits) for `tasks` tasks of these dimensions.  Either out pointer may be null. */
int32_t rlrep_nc_forms(int32_t tasks, int32_t batch, int32_t feature_dim, int32_t hidden_dim, int32_t g2, int32_t* chunked, int32_t* splits);

/* Unit-test hook of the loss heads every agent shares (csrc/elementwise.hip policy_fwd / policy_bwd / vae_mid / heads_vae / vae_mse /
 * qhead_critic / qhead_actor kernels, csrc/per.hip qhead_critic_w_kernel, and the 16-row engine's epilogues that replace four of them:
 * csrc/gemm16_tile.h EPI_FWD_POLICY, EPI_DX_POLICYBWD, EPI_FWD_MSE, EPI_DX_REPARAM; tests/test_heads_kernels.py): ONE launch of one head on
 * caller buffers, with no agent, through the launchers the step programs use (rl_launch_policy_fwd ... rl_launch_qhead_actor,
 * rl_launch_qhead_critic_w; rl_launch_gemm16 with rl_gemm16_number_tiles for the fused forms, whose task records are filled by the functions
 * the program builder fills them with: engine_internal.h rl_task_*).  The records carry the fields of the launch records (csrc/kparams.h
 * PolicyFwd, PolicyBwd, VaeMid, HeadsVae, VaeMse, QHeadCritic(W), QHeadActor) except block / tile counts (the builder's helpers: qhead_blocks,
 * rl_vae_blocks, rl_heads_vae_tiles_c) and the group counter (always null: nothing is bumped).  alpha_state: the double the kernels read
 * log(alpha) from.  form (may be null) receives what was launched: form[0] = 0 the stand-alone kernel / 1 a gemm16 epilogue; form[1] =
 * HEADS_VAE: 1 the 16-byte loader copy, 0 the 4-byte one; QHEAD_CRITIC: 1 the weighted kernel; REPARAM_DX: pre.  Which gemm16 front end
 * a fused launch took: the difference of rlrep_front_end_counts around the call.
 *   fused = 1 (POLICY_FWD, POLICY_BWD, VAE_MSE; REPARAM_DX always): the head runs as the epilogue of its layer's product, and the record
 *   carries the layer's operands in rlrep_hd_layer: forward X [B, K] (row stride ldx) . W [N, K]^T (ldw) + bias [N]; backward
 *   G [B, K] (ldx) . W [K, N] (ldw), bias unused.  O / DH / dA, inputs of the stand-alone kernels, then are what the product leaves
 *   (POLICY_FWD: O [B, 2A] dense is an output; VAE_MSE: GDH is the product's output; POLICY_BWD: dA is not stored and may be null).
 *   POLICY_FWD fused: 1 or 2 policy tasks (t[0], t[1]: the hoisted "actor.head x2 + policy" stage) and one optional plain forward task
 *   (extra.l.X non-null: Y [rows, N] = act(X W^T + bias), act as rlrep_gemm) in the same launch.
 *   REPARAM_DX: G[b, c] += v[b, c], G[b, F + c] += v[b, c] EZ[b, c], v = A . W ([K, F], ldw).  pre = 0: A [B, K] (lda) is read; pre = 1: A =
 *   (X [B, K1] Wh [K1, K]) relu'(M [B, K]) is recomputed by every tile (the fused short product) and stored to A; pre = 2: X = dmse(M Wh^T + bh;
 *   s2, r) as well (the heads + mse launch riding along, K1 = S + 1 <= 32): X [B, K1] (ldx) and partial [2 ceil(B / 16)] are outputs.
 * Refused with RLREP_ERR_ARG and a message starting "heads:", before any GPU call: an unknown kind, a null required pointer, a non-positive
 * extent, a row stride below the row's width, fused outside {0, 1}, fused = 1 with 2A > 16 (forward) or A > 16 (backward) -- the kinds
 * that have no fused form, and REPARAM_DX, which has no other, carry no such switch --, a clamp or a null eps on the fused forward, a task
 * count outside 1..2, pre outside 0..2, K1 outside 1..32, an alpha_state off an 8-byte boundary, a
 * float pointer off a 4-byte boundary, the 16-byte rows the mse phase of pre = 2 loads (K % 4, ldm % 4, ldwh % 4, M or Wh off a 16-byte
 * boundary), a seed group's call in progress. */
enum { RLREP_HD_POLICY_FWD = 0, RLREP_HD_POLICY_BWD = 1, RLREP_HD_VAE_MID = 2, RLREP_HD_HEADS_VAE = 3, RLREP_HD_VAE_MSE = 4,
       RLREP_HD_REPARAM_DX = 5, RLREP_HD_QHEAD_CRITIC = 6, RLREP_HD_QHEAD_ACTOR = 7 };
typedef struct rlrep_hd_layer { const float* X; int32_t ldx; const float* W; int32_t ldw; const float* bias; int32_t K; } rlrep_hd_layer;
typedef struct rlrep_hd_policy_task { float* O; const float* eps; float* act; int32_t ld_act; float* logp; rlrep_hd_layer l; } rlrep_hd_policy_task;
typedef union rlrep_heads_args {
    struct { int32_t fused, ntasks, B, A, clamp; float lo, hi; int32_t* form; rlrep_hd_policy_task t[2];
             struct { rlrep_hd_layer l; float* Y; int32_t ldy, rows, N, act; } extra; } policy_fwd;
    struct { int32_t fused; const float* O; const float* eps; const float* act; int32_t ld_act; float* dA; int32_t ld_dA;
             const double* alpha_state; float inv_batch; float* G; int32_t B, A; int32_t* form; rlrep_hd_layer l; } policy_bwd;
    struct { const float* EH; const float* FH; const float* eps; float* Z; float* EZ; float* GEH; float* GFH; float* partial;
             int32_t B, F; float scale; int32_t* form; } vae_mid;
    struct { const float* Ae; const float* Af; int32_t lda; const float* We; const float* be; const float* Wf; const float* bf; const float* eps;
             float* Z; float* EZ; float* GEH; float* GFH; float* partial; float* EH; float* FH; int32_t B, F, K; float scale; int32_t* form; } heads_vae;
    struct { int32_t fused; const float* DH; const float* s2; int32_t ld_s2; const float* r; float* GDH; float* partial; int32_t B, S;
             float scale_s, scale_r; int32_t* form; rlrep_hd_layer l; } vae_mse;
    struct { int32_t pre; float* A; int32_t lda; const float* W; int32_t ldw; float* G; int32_t ldg; const float* EZ; int32_t ldez; int32_t B, F, K;
             float* X; int32_t ldx; const float* Wh; int32_t ldwh; int32_t K1; const float* M; int32_t ldm;
             const float* bh; const float* s2; int32_t ld_s2; const float* r; float scale_s, scale_r; float* partial; int32_t* form; } reparam_dx;
    struct { const float* Et[2]; const float* Ec[2]; const float* wt[2]; const float* bt[2]; const float* wc[2]; const float* bc[2];
             const float* logp; const float* R; const float* D; const double* alpha_state; float gamma, inv_batch;
             float* dq; float* GE[2]; float* partial; int32_t B, H, train, ldE; int32_t weighted; const float* w; float* td; int32_t* form; } qhead_critic;
    struct { const float* Ec[2]; const float* wc[2]; const float* bc[2]; const float* logp; const double* alpha_state; float inv_batch, target_entropy;
             float* GE[2]; float* partial_loss; float* partial_c; int32_t B, H, ldE; int32_t* form; } qhead_actor;
} rlrep_heads_args;
int32_t rlrep_heads(int32_t kind, const rlrep_heads_args* args, void* stream);
/* Host-only: every check of rlrep_heads on the record and the form it would launch (args' form), without any GPU call. */
int32_t rlrep_heads_plan(int32_t kind, const rlrep_heads_args* args);
/* Host-only: blocks (or tiles) of a head's launch and so the floats of its partial buffers: VAE_MID ceil(B F / 256); HEADS_VAE ceil(B / 16)
 * ceil(F / 16); VAE_MSE (n = S): fused = 0: 2 ceil(B (S + 1) / 256), fused = 1: 2 ceil(B / 16) ceil((S + 1) / 16); REPARAM_DX (n = unused):
 * 2 ceil(B / 16); QHEAD_CRITIC 4 qhead_blocks(B); QHEAD_ACTOR qhead_blocks(B) (each of its two); 0 for another kind or a non-positive extent. */
int32_t rlrep_heads_partials(int32_t kind, int32_t fused, int32_t B, int32_t n);

/* Chains (csrc/xchain.hip): consecutive row-local stages of a step program -- the forward and dX launches of the reference's
 * feature_step / critic_step / update_actor_and_alpha (agent/vlsac/vlsac_agent.py:126-237 and siblings) -- run as ONE persistent launch
 * whose workgroups synchronise per XCD.  The launch checks its own assumptions on the device: *status receives the error word
 * (0 = clean; bit 0: a wait inside a chain timed out; bit 1: the workgroups of one group did not share an XCD, i.e. the hand-offs
 * were not guaranteed to be seen).  SYNCHRONISES `stream`.  Returns RLREP_ERR_STATE (and sets the error text) when the word is not 0:
 * results of the affected steps are invalid; RLREP_XCHAIN=0 selects one launch per stage. */
int32_t rlrep_chain_status(rlrep_agent* agent, uint32_t* status, void* stream);

/* bit 0: this library was built with RLREP_BUILD_EXPERIMENTS=1 (the opt-in engines that were measured and not adopted: RLREP_ROWPROG,
 * RLREP_XCHAIN, RLREP_FUSE_L1, superseded noise-critic forward kernels).  0: they are not compiled in and their switches are ignored. */
int32_t rlrep_build_flags(void);

/* Metric history.  While on (rlrep_history(agent, 1)), the LAST optimizer launch of every train() -- the actor's, reference
 * agent/sac/sac_agent.py:157-166 -- also appends the 16 metric slots to a device ring of *records records of *record_floats floats: record
 * n % *records holds the metrics of the n-th such launch since the agent was created and n itself (int32 bit pattern) in word *tag_word; *seq is
 * the device counter n.  The reference returns the metrics of a train() as host floats (a device sync per value); a caller
 * that replays train() as a hipGraph reads record n when -- and if -- somebody looks at the returned dict, instead of paying a snapshot
 * launch per call.  A record is overwritten *records calls later: the tag says whether it still is the one asked for.  The switch is read
 * when a step is LAUNCHED (or captured), not on the device.  Not kept by the fused-optimizer variant (RLREP_FUSE_ADAM). */
int32_t rlrep_history(rlrep_agent* agent, int32_t on);
int32_t rlrep_history_dev(rlrep_agent* agent, const float** ring, const int32_t** seq, int32_t* records, int32_t* record_floats, int32_t* tag_word);

/* Diagnostics: one single-thread launch on `stream` that appends (100 MHz device wall clock << 8 | tag) to a ring of `cap` 64-bit words
 * after a running counter in ring[0] (ring: cap + 1 words of device memory, zeroed by the caller).  Captured between the launches of a
 * train() graph it dates the chains on the DEVICE (tools/exp/chain_stamps.py); it is not part of any step. */
int32_t rlrep_debug_stamp(int64_t* ring_dev, int32_t cap, int32_t tag, void* stream);

/* Number of kernel launches the last step program issued (for the latency model in DESIGN.md). */
int32_t rlrep_last_launch_count(rlrep_agent* agent);
/* process-wide number of kernel launches the library has issued so far (a captured train()'s launch count = the difference around its capture) */
int64_t rlrep_launch_counter(void);
/* process-wide launches of the 16-row tile engine per FRONT END so far: out4[0] = gemm16_fast_kernel, [1] = gemm16_fast4_kernel, [2] =
 * gemm16_fastpre_kernel (operand loads issued from preloaded scalars; a launch qualifies by its shapes and by all its operands lying within
 * 16 GiB of one base -- the caller's arenas should be slices of ONE allocation), [3] = the record front end (gemm16_kernel /
 * gemm16_duo_kernel).  Counted when a launch is issued or captured, like rlrep_launch_counter.  The layers these launches compute:
 * reference networks/vae.py:40-57,83-85,112-117 and the MLPs of agent/<alg>/<alg>_agent.py. */
int32_t rlrep_front_end_counts(int64_t* out4);

/* ---- seed groups: R independent sac or ctrlsac agents in the same launches (additive to ABI 4) -----------------------------------------
 * A group is R members of identical dims (and hyper, but for what rlrep_group_set_member_hyper may vary) whose blocks -- the seven arenas of rlrep_agent_create -- are laid out identically at a
 * constant byte stride in ONE allocation: member r's copy of any word is member 0's address + r * member_stride_bytes.  The step programs are
 * built once, against member 0's arenas; every launch of the agent then runs all members (grid y = member) and moves every pointer it
 * dereferences to the member's block.  Each member computes exactly what a standalone agent with its seed computes: same tiles, same
 * summation order, nothing shared between members.  The returned handle is used with the ordinary step entry points (rlrep_critic_step,
 * rlrep_actor_alpha_step, rlrep_update_target, rlrep_prefetch_policy, rlrep_end_train; ctrlsac: rlrep_feature_step, rlrep_sync_frozen and
 * rlrep_prefetch_batch(_slot 0) with indices inside member 0's block, with or without RLREP_FLAG_NO_FEATURE_TARGET), which then run every
 * member; the train prologue and select_action take their group forms below.
 * The entry points that have no group form -- rlrep_set_batch, rlrep_replay_sample (other than the gathers the group prologue or a group
 * optimizer launch already did), rlrep_prefetch_batch_slot 1, rlrep_prefetch_policy_early, the deferred-chain and image calls, rlrep_actor_forward, rlrep_select_action,
 * rlrep_run_stage, rlrep_chain_status -- refuse a group with RLREP_ERR_ARG and a message.  Every kernel launcher without a group form refuses
 * too while a group call is in progress (the persistent 256 x 128 bf16x3 tile, the opt-in fused score + InfoNCE kernel, the spedersac /
 * diffsrsac / noise-critic kernels, the data-parallel pulls, the experimental engines): a step whose program reaches one fails with
 * RLREP_ERR_HIP.  No entry point runs member 0 alone.
 * Rejected with RLREP_ERR_ARG and a message: alg other than sac and ctrlsac (checked first), members outside [1, rlrep_group_max_members()],
 * a stride that is not a positive multiple of 256 or is smaller than the member span (lowest arena pointer to the end of the highest arena),
 * world_size > 1.
 * On success members 1..R-1 start as byte copies of member 0's block (after its creation); the caller then writes each member's parameters.
 * Reference: main.py:63-68 (one run per seed) -- a group runs several seeds at once. */
int32_t rlrep_group_create(const rlrep_dims* dims, const rlrep_hyper* hyper, const rlrep_arenas* member0_arenas, int32_t members,
                           int64_t member_stride_bytes, void* stream, rlrep_agent** out);
int32_t rlrep_group_max_members(void);
/* members of a group agent; 0 for an ordinary agent */
int32_t rlrep_group_members(rlrep_agent* agent);
/* Sweeps: members may differ in the hyper-parameters that no launch's shape depends on.  Member `member`'s lr_feature, lr_critic, lr_actor
 * (its temperature optimizer's too), discount, tau, feature_tau, target_update_period and learn_alpha become `hyper`'s: its four optimizer
 * records' lr / tau words (rlrep_group_cfg_dev, the member's copy) and its record of the scalars the programs otherwise carry by value
 * (discount, target_update_period, the temperature lr and learn_alpha), read by the group launches from the member's block.  Stream-ordered on
 * `stream` and then synchronised; a captured graph reads the new values at its next replay (no re-capture).  The step counters, moments and
 * the temperature state are untouched: the initial temperature is the caller's alpha_state[0].
 * Rejected with RLREP_ERR_ARG and a message: an ordinary agent, a member outside [0, members), a structural field that differs from the
 * group's (target_entropy, sigma_scale, extra_feature_steps, world_size, beta1, beta2, adam_eps, critic_reg_lambda), a learning rate that is
 * not finite and positive, a non-finite discount, tau or feature_tau outside [0, 1], target_update_period < 1.  Until it is called a member
 * has rlrep_group_create's hyper.  rlrep_group_get_member_hyper reads a member's values back (world_size as the group normalises it). */
int32_t rlrep_group_set_member_hyper(rlrep_agent* agent, int32_t member, const rlrep_hyper* hyper, void* stream);
int32_t rlrep_group_get_member_hyper(rlrep_agent* agent, int32_t member, rlrep_hyper* out);
/* Exploit step of population-based training: for k < n, member dst[k] becomes member src[k] -- parameters, targets, Adam moments and
 * step counts, temperature state, train() counter -- and keeps its own hyper-parameters (rlrep_group_set_member_hyper), seed, replay
 * ring and metric history.  ONE launch, stream-ordered on `stream`; captured train() graphs read the new state at their next replay.
 * Copied, from src's block to dst's: the parameter, target, exp_avg and exp_avg_sq arenas, alpha_state and the batch-independent device
 * records (the train() counter block, the four optimizer records, the metric slots) except words 1..5 of every optimizer record (lr, beta1,
 * beta2, eps, tau: rlrep_group_cfg_dev), which stay dst's.  Gradients, activations and the index / noise pools are rewritten by every train().
 * Rejected with RLREP_ERR_ARG and a message, before anything is launched: an ordinary agent, n outside [1, members], a member outside
 * [0, members), src == dst in a pair, a destination named twice, a member that is a source of one pair and the destination of another (pairs
 * are independent: the launch orders nothing between them), a call between rlrep_group_train_prologue and the end of that train(). */
int32_t rlrep_group_clone_members(rlrep_agent* agent, const int32_t* src_host, const int32_t* dst_host, int32_t n, void* stream);
/* Successive halving: take members out of every group launch, keep their state, put them back.  live_host [members], 1 = live, 0 = retired.
 * The group's live table (device: n_live, then the live members in ascending order) is rebuilt from the mask in ONE launch, stream-ordered on
 * `stream`; grid y of the group launches stays `members`, and a workgroup whose slot lies at or behind n_live returns at once, so a captured
 * train() graph obeys the mask from its next replay (no re-capture).  Nothing of a retired member is read or written by rlrep_group_train_prologue,
 * the step programs or rlrep_group_select_action (its action row is left unwritten): parameters, moments, step counters, tickets, pools, slot
 * buffers, metric slots and history stand still until it is revived.  rlrep_group_clone_members, rlrep_group_set_member_hyper and
 * rlrep_group_replay_add_sized do not look at the mask.  After rlrep_group_create every member is live.
 * Rejected with RLREP_ERR_ARG and a message, before anything is launched: an ordinary agent, a mask with no live member, a value other than
 * 0 / 1, a call between rlrep_group_train_prologue and the end of that train().  rlrep_group_get_live reads the mask back. */
int32_t rlrep_group_set_live(rlrep_agent* agent, const int32_t* live_host, void* stream);
int32_t rlrep_group_get_live(rlrep_agent* agent, int32_t* live_out);
/* the Philox seed of every member (n = members): member r's index and noise pools are drawn as rlrep_train_prologue draws them with seeds[r] */
int32_t rlrep_group_set_seeds(rlrep_agent* agent, const uint64_t* seeds_host, int32_t n, void* stream);
/* rlrep_train_prologue for every member, in ONE launch: member r draws with its seed, gathers from ring_dev + r * ring_stride_bytes bounded
 * by size_dev[r], writes its pools at idx_pool_dev / eps_pool_dev + r * member stride (the pools must lie inside member 0's block) and counts its
 * own steps. */
int32_t rlrep_group_train_prologue(rlrep_agent* agent, const float* ring_dev, int64_t ring_stride_bytes, const int32_t* size_dev,
                                   int32_t* idx_pool_dev, int64_t n_idx, float* eps_pool_dev, int64_t n_eps, uint64_t idx_offset,
                                   uint64_t eps_offset, int32_t batch, void* stream);
/* size a group's step programs for `batch` (blocking table uploads when it changes: call it outside a graph capture).  Launches nothing. */
int32_t rlrep_group_prepare(rlrep_agent* agent, int32_t batch);
/* rlrep_select_action for every member in ONE launch: member r reads observation r of obs_host [members, state_dim] and writes action r of
 * action_host [members, action_dim] (both pinned host memory, read / written in place) with its own actor; explore: its draw is
 * rlrep_fill_normal(eps[A], 1, seeds[r], offset), as a standalone agent with seed seeds[r] draws it.  (reference agent/sac/sac_agent.py:89-96) */
int32_t rlrep_group_select_action(rlrep_agent* agent, const float* obs_host, int32_t explore, uint64_t offset, float lo, float hi,
                                  float* action_host, void* stream);
/* rlrep_group_select_action for `rows` observations per member in ONE launch (grid (rows, members); additive to ABI 4): member r's row e reads
 * obs_host[(r * rows + e) * S ..], writes action_host[(r * rows + e) * A ..] (both pinned) and draws rlrep_fill_normal(eps[A], 1, seeds[r],
 * offset + (e << 20)) -- what standalone agent r's e-th of `rows` successive select_action calls draws.  A retired member's rows are neither
 * read nor written.  rows in [1, RLREP_SELECT_MAX_ROWS]; refused before any launch, "group_select_action_n:" first: a null argument, rows
 * outside the range, a handle that is not a seed group, unpinned buffers. */
int32_t rlrep_group_select_action_n(rlrep_agent* agent, const float* obs_host, int32_t rows, int32_t explore, uint64_t offset, float lo, float hi,
                                    float* action_host, void* stream);
/* rlrep_replay_add_sized for `members` rings ring_dev + r * ring_stride_floats, in ONE launch: member r's nrows staged rows start at
 * rows_host + r * rows_stride_floats (pinned), its fill level goes to size_dev[r]. */
int32_t rlrep_group_replay_add_sized(float* ring_dev, int64_t ring_stride_floats, int32_t members, int64_t capacity, int32_t row_floats, int64_t ptr,
                                     const float* rows_host, int64_t rows_stride_floats, int64_t nrows, int32_t* size_dev, int32_t new_size, void* stream);

/* rlrep_act_device for a seed group in ONE launch (grid (ceil(rows / 16), members); additive to ABI 4): obs_dev [members, rows, S] and
 * action_dev [members, rows, A] are device tensors, member r acts with its own actor and draws with seeds[r] at offset + (e << 20): its plane is
 * bit for bit what rlrep_act_device gives the standalone agent with that seed.  A retired member's planes are neither read nor written.
 * Refused before any launch, "group_act_device:" first: a null argument, rows outside [1, RLREP_ACT_MAX_ROWS], a handle that is not a seed
 * group, the LDS limit. */
int32_t rlrep_group_act_device(rlrep_agent* agent, const float* obs_dev, int32_t rows, int32_t explore, uint64_t offset, float lo, float hi,
                               float* action_dev, void* stream);
/* rlrep_replay_add_cols for `members` rings ring_dev + r * ring_stride_floats in ONE launch: member r's n transitions are rows r * n .. of the
 * five arrays, its fill level goes to size_dev[r].  Like rlrep_group_replay_add_sized it does not look at the live mask. */
int32_t rlrep_group_replay_add_cols(float* ring_dev, int64_t max_size, int32_t row_floats, int64_t start, int32_t S, int32_t A, const float* s, int64_t ld_s,
                                    const float* a, int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n,
                                    int32_t members, int64_t ring_stride_floats, int32_t* size_dev, int32_t new_size, void* stream);

/* ---- the one-graph simulator loop of a seed group (additive to ABI 4) ---------------------------------------------------------
 * The counter-reading forms above, for every live member of a group in ONE launch each (grid y = a slot of the live table), stream-ordered and
 * capturable: no copy, no allocation, no synchronisation.  The loop record of a group is ctl_dev, int64[members][RLREP_LOOP_CTL_WORDS] in
 * caller-owned device memory, member r's row r * RLREP_LOOP_CTL_WORDS words behind member 0's:
 *   shared by the group, in row 0:  word 0 calls, 1 t_global (steps PER MEMBER: an iteration adds n), 2 iter, 6 warm -- one value for all
 *                                   members; they advance whenever at least one member is live
 *   per member, in row r:           word 3 next, 4 start, 5 size -- member r's cursor into its own ring (words 0, 1, 2, 6 of rows 1.. are unused)
 * In either launch no thread writes a word that a workgroup of the same launch reads: thread 0 of workgroup (0, slot) moves the cursor of member
 * slot_member[slot]; the one of slot 0 -- the first live member -- also writes the shared words.  A retired member's row, ring, size word and
 * planes are neither read nor written.
 *
 * rlrep_group_act_device_ctl: obs_dev [members, rows, S], action_dev [members, rows, A] (contiguous); plane r is bit for bit what
 * rlrep_act_device_ctl gives the standalone agent with seed seeds[r] (rlrep_group_set_seeds) at the same calls / t_global / iter -- seeds[r] is
 * the key of the head's draw and of the exploration mix.  Refused with RLREP_ERR_ARG before the launch ("group_act_device_ctl:"): a null
 * argument, rows outside [1, RLREP_ACT_MAX_ROWS] or above max_size, a handle that is not a seed group, eps_greedy outside [0, 1], a negative
 * start_timesteps, the LDS limit.
 *
 * rlrep_group_replay_add_cols_ctl: member r's n transitions are rows r * n .. of the five arrays; they go into ring ring_dev + r *
 * ring_stride_floats from ITS start, wrapping; ITS size goes to size_dev[r] (which may be NULL); iter += 1, t_global += n and calls += n unless
 * warm happen once.  Unlike rlrep_group_replay_add_cols it honours the live table.  Refused by name ("group_replay_add_cols_ctl:"): a null
 * argument, a handle that is not a seed group, n outside [1, RLREP_ACT_MAX_ROWS] or above max_size, row_floats != 2 S + A + 2, a row stride
 * below its width, a ring stride below a ring.
 *
 * rlrep_group_sim_start / _step / _step_append_ctl: rlrep_sim_start / _step / _step_append_ctl for members x n environments.  `sim` is a
 * rlrep_sim_state whose arrays are [members, n] planes (obs [members, n, S]); its `seed` field is ignored: member r's start states are keyed by
 * sim_seeds_dev[r] (uint64[members], device) with the environment's index WITHIN the member as counter word 2, so plane r is the single
 * simulator with that seed, word for word.  act is [members, n] rows at stride ld_act; next_obs [members, n, S], reward and done [members, n].
 * rlrep_group_sim_start resets every member and does not consult the live table; the two steps skip retired members.  The _ctl form does for
 * the group what rlrep_group_replay_add_cols_ctl's bookkeeping threads do.  Refused by name before the launch ("group_sim_start:",
 * "group_sim_step:", "group_sim_step_append_ctl:"): a null argument, a handle that is not a seed group, an unknown kind, n outside [1,
 * RLREP_SIM_MAX_ENVS] or above max_size, ld_act below the kind's A, row_floats != 2 S + A + 2, a ring stride below a ring. */
int32_t rlrep_group_act_device_ctl(rlrep_agent* agent, const float* obs_dev, int32_t rows, float lo, float hi, float* action_dev, int64_t* ctl_dev,
                                   int64_t max_size, float eps_greedy, int64_t start_timesteps, void* stream);
int32_t rlrep_group_replay_add_cols_ctl(rlrep_agent* agent, float* ring_dev, int64_t max_size, int32_t row_floats, int32_t S, int32_t A, const float* s,
                                        int64_t ld_s, const float* a, int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n,
                                        int64_t ring_stride_floats, int32_t* size_dev, int64_t* ctl_dev, void* stream);
int32_t rlrep_group_sim_start(rlrep_agent* agent, const rlrep_sim_state* sim, const uint64_t* sim_seeds_dev, void* stream);
int32_t rlrep_group_sim_step(rlrep_agent* agent, const rlrep_sim_state* sim, const uint64_t* sim_seeds_dev, const float* act, int64_t ld_act, float* next_obs,
                             float* reward, float* done, void* stream);
int32_t rlrep_group_sim_step_append_ctl(rlrep_agent* agent, const rlrep_sim_state* sim, const uint64_t* sim_seeds_dev, const float* act, int64_t ld_act,
                                        float* ring_dev, int64_t max_size, int32_t row_floats, int64_t ring_stride_floats, int32_t* size_dev,
                                        int64_t* ctl_dev, void* stream);

/* ---- device environments of a seed group (additive to ABI 4) ------------------------------------------------------------------------------
 * The launcher's group loop (main.py run_seeds) waits for select_action, steps R NumPy environments, draws the exploration actions and stages
 * R ring rows on the host every iteration, and every evaluation costs episodes x 200 further round trips per member.  A device environment
 * keeps one record per member on the device (an allocation of its own: the member stride, rlrep_group_clone_members' segments and the
 * checkpoint device records do not know it) and does all of that in ONE launch per iteration, capturable in front of the group's train()
 * graph, and one launch per evaluation.  kind 0 = Pendulum-v1 (S = 3), kind 2 = MountainCarContinuous-v0 (S = 2; the goal p >= 0.45 with
 * v >= 0 ends an episode, 999-step time limit) -- the public specifications as rlrep_amd/envs/pendulum.py and envs/mountain_car.py restate
 * them; fp64 dynamics in one lane, rounded to fp32 where the host environment rounds; any other kind is RLREP_ERR_ARG.  The kind lives in the
 * handle: step, evaluate and reset dispatch on it.  Below, "200" and "9 floats" are Pendulum's time limit and row: a kind has its own
 * (MountainCarContinuous-v0: 999 and 7).
 *
 * Record (256 bytes per member, csrc/group_env.h EnvRecord): double theta, theta_dot, episode_return; int64 ring_ptr, nsteps; int32 t,
 * ring_size, episodes_done, force; float force_action, act; float obs[4]; double returns[16] (finished episodes, entry episodes_done % 16
 * is written next); 48 bytes of padding.  Counters (16 bytes, group-wide): int64 t_global (steps since reset), uint64 calls (the
 * select_action call counter).  MountainCarContinuous-v0: theta / theta_dot hold position and velocity (fp32-representable values: that
 * environment rounds its state to fp32 at reset and after every step), obs[0..1] = (p, v).
 * Philox streams (counter word 3, where every other draw of the library has a value below 2^17): 0xE0000000 collection -- counter = the
 * member's nsteps, word 2 = 0 for a step's exploration draws (word 0: the epsilon-greedy test, word 1: the uniform action), word 2 = 1 for
 * an episode's start state; 0xE1000000 evaluation start states, counter = eval_index * episodes + episode.  Key = the member's seed
 * (rlrep_group_set_seeds).  The index, noise and select_action streams of train() are untouched.
 *
 * rlrep_group_env_step, per LIVE member (a retired member's record, ring and block are neither read nor written): the actor forward on the
 * record's observation and the exploring sample exactly as rlrep_group_select_action(explore = 1, offset = (calls + 1) << 20) computes them;
 * a uniform action in [lo, hi] instead while t_global < start_timesteps or with probability eps_greedy (or the record's force_action when
 * force is set: one shot); the dynamics; the row [s, a, s', r, done_bool = 0] at ring_ptr of ring_dev + member * ring_stride_floats
 * (rlrep_group_replay_add_sized's layout, row = 9 floats); ring_ptr and ring_size advance (wrap at `capacity`), size_dev[member] = ring_size;
 * on the 200th step the episode return is filed and a new episode starts.  MountainCarContinuous-v0: done_bool = 1 where the step reaches the
 * goal before the 999th step of its episode (a goal ON the 999th step is the time limit's and stays 0, the host loop's rule); the episode
 * ends at the goal or on the 999th step, and the new start is p = fp32(-0.6 + 0.2 u), v = 0 from words 0..1 of the start-state block.  The launch's last workgroup adds 1 to t_global and, past warm-up,
 * to calls.  rlrep_group_env_evaluate: workgroup (episode e, member) rolls out one 200-step episode with the mean action
 * (select_action(explore = 0), clamped to Pendulum's +-2) from its Philox start state and writes the fp64 sum of the fp32 rewards to
 * out_dev[member * episodes + e] (a retired member's entries are left unwritten); episodes in [1, 64].  MountainCarContinuous-v0: up to 999
 * steps, the action clamped to +-1, and the workgroup leaves the loop (uniformly) once the goal is reached.
 * rlrep_group_env_reset: every record starts a fresh episode (start state at counter 0), cursors, counters and returns zeroed.
 * rlrep_group_env_state: copy block `what` (RLREP_ENV_STATE_*) to (write = 0) or from (write = 1) host memory, `bytes` = the block's exact
 * size (records: 256 * members; counters: 16; the start states of the last evaluation, read only: 16 * members * episodes, [member, episode,
 * (theta, theta_dot)]); stream-ordered on `stream`, then synchronised.
 * All launches are stream-ordered and capturable; nothing is allocated after create.  Rejected with RLREP_ERR_ARG and a message, before any
 * launch: a null pointer, an ordinary agent, state / action dims other than the kind's (3 / 1, 2 / 1), an environment of another group, a call between
 * rlrep_group_train_prologue and the end of that train(), episodes outside [1, 64], a capacity below 1 or a ring stride that does not hold it. */
typedef struct rlrep_group_env rlrep_group_env;
#define RLREP_ENV_PENDULUM 0
#define RLREP_ENV_MOUNTAIN_CAR_CONTINUOUS 2
#define RLREP_ENV_STATE_RECORDS 0
#define RLREP_ENV_STATE_COUNTERS 1
#define RLREP_ENV_STATE_EVAL_STARTS 2
int32_t rlrep_group_env_create(rlrep_agent* agent, int32_t kind, rlrep_group_env** out);
void rlrep_group_env_destroy(rlrep_group_env* env);
int32_t rlrep_group_env_reset(rlrep_group_env* env, void* stream);
int32_t rlrep_group_env_step(rlrep_agent* agent, rlrep_group_env* env, float* ring_dev, int64_t ring_stride_floats, int64_t capacity, int32_t* size_dev,
                             float lo, float hi, float eps_greedy, int64_t start_timesteps, void* stream);
int32_t rlrep_group_env_evaluate(rlrep_agent* agent, rlrep_group_env* env, int32_t episodes, uint64_t eval_index, double* out_dev, void* stream);
int32_t rlrep_group_env_state(rlrep_group_env* env, int32_t what, void* host, int64_t bytes, int32_t write, void* stream);

/* ---- the device environment of a SINGLE agent (additive to ABI 4) ---------------------------------------------------------------------------
 * The same thing for an ordinary agent (rlrep_agent_create) of any of the five algorithms -- they carry the same actor trunk: one record, the
 * same kinds, record and counters layout, Philox streams, dynamics, row layout and done_bool rule as above (one code: csrc/env_step_body.h,
 * env_eval_body.h), with the member's seed replaced by `seed` of rlrep_env_create -- the seed rlrep_select_action is called with.
 * rlrep_env_step is ONE launch of one workgroup, capturable in front of the agent's train(): the action is bit for bit
 * rlrep_select_action(explore = 1, seed, offset = (calls + 1) << 20) on the record's observation; ring_dev holds `capacity` rows,
 * size_dev[0] receives the fill level.  rlrep_env_evaluate is ONE launch, grid (episodes, 1): out_dev[e] is episode e's return.
 * rlrep_env_state: as rlrep_group_env_state with one record (256 bytes; counters 16; start states 16 * episodes).
 * Rejected with RLREP_ERR_ARG and a message that names the entry point, before any launch: a null pointer, a seed group ("takes
 * rlrep_group_env_create"), a data-parallel agent, an unknown kind, dimensions other than the kind's, an environment of another agent, a call
 * inside a train(), episodes outside [1, 64], a capacity below 1.  rlrep_env_destroy(NULL) is a no-op.
 * rlrep_prepare: size an agent's step programs for `batch` (blocking table uploads when it changes: call it outside a graph capture); launches
 * nothing.  rlrep_group_prepare's twin for an ordinary agent. */
typedef struct rlrep_env rlrep_env;
int32_t rlrep_env_create(rlrep_agent* agent, int32_t kind, uint64_t seed, rlrep_env** out);
void rlrep_env_destroy(rlrep_env* env);
int32_t rlrep_env_reset(rlrep_env* env, void* stream);
int32_t rlrep_env_step(rlrep_agent* agent, rlrep_env* env, float* ring_dev, int64_t capacity, int32_t* size_dev, float lo, float hi, float eps_greedy,
                       int64_t start_timesteps, void* stream);
int32_t rlrep_env_evaluate(rlrep_agent* agent, rlrep_env* env, int32_t episodes, uint64_t eval_index, double* out_dev, void* stream);
int32_t rlrep_env_state(rlrep_env* env, int32_t what, void* host, int64_t bytes, int32_t write, void* stream);
int32_t rlrep_prepare(rlrep_agent* agent, int32_t batch);

/* ---- several environments per member / agent (additive to ABI 4) -----------------------------------------------------------------------------
 * rlrep_group_env_create_n / rlrep_env_create_n: as the create calls above (which are their num_envs = 1 forms), with num_envs = E in [1, 64]
 * environments per member resp. for the agent: [members][E] records, record (m, e) at index m * E + e.  The other entry points keep their
 * signatures and take E from the handle:
 *   reset     every record starts a fresh episode; record (m, e)'s ring cursor is row e.
 *   step      ONE launch, grid (E, members) resp. (E, 1): workgroup (e, slot) steps environment e of its member and writes ONE ring row, so a
 *             step writes E rows per live member, at (ptr + e) mod capacity in environment order where ptr is the member's next free row
 *             (every record carries its own cursor and advances it by E; record (m, 0)'s cursor is the next free row).  ring_size grows by
 *             E (capped at capacity) and environment 0 publishes it to size_dev.  t_global advances by E per launch and, past warm-up
 *             (decided once per launch: keep start_timesteps a multiple of E), calls by E.  capacity >= E.
 *   draws     key = the member's seed, counter = the record's nsteps, word 3 = the collection stream, word 2 = 2 e (exploration) resp.
 *             2 e + 1 (start state): environment 0 draws what the single environment draws.  The action of environment e is bit for bit
 *             select_action(explore = 1, offset = (calls + 1 + e) << 20) on its observation.
 *   evaluate  unchanged, per member: it does not depend on E.
 *   state     the records block holds 256 * members * E bytes (single: 256 * E), in index order; counters and start states as before.
 * rlrep_group_env_num_envs / rlrep_env_num_envs: E of a handle (0 for NULL).  With E = 1 every call launches the kernels it launched
 * before.  Rejected with RLREP_ERR_ARG and a message naming the entry point (group_env_create_n / env_create_n), before any launch: a kind
 * that is not built, num_envs outside [1, 64], a null pointer, and what the create calls reject. */
int32_t rlrep_group_env_create_n(rlrep_agent* agent, int32_t kind, int32_t num_envs, rlrep_group_env** out);
int32_t rlrep_group_env_num_envs(rlrep_group_env* env);
int32_t rlrep_env_create_n(rlrep_agent* agent, int32_t kind, uint64_t seed, int32_t num_envs, rlrep_env** out);
int32_t rlrep_env_num_envs(rlrep_env* env);

#ifdef __cplusplus
}
#endif
#endif /* RLREP_H */
