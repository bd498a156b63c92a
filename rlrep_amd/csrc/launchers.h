// Everything of librlrep_hip.so that one .hip file of csrc/ defines and another one uses: the kernel launchers with the planners, predicates
// and init functions beside them (C linkage), and the few plain C++ symbols shared the same way.  Declared HERE ONLY, and included by the file
// that defines a symbol as well as by the files that call it: a C-linkage definition whose parameter list differs from its prototype is a
// compile error in the defining file, instead of a wrong call at run time.  (rl_off / rl_opt: common.h.  Diagnostics entry points that only
// Python tools bind -- rl_timing_*, rl_nc_timing_fetch, rl_rowprog_timing, rl_xc_timing_* -- have no C++ caller and are not listed.)
// Declarations only: no device code, no inline functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"
#include "kparams.h"
#include "gemm_lds_tiles.h"
#include "group.h"
#include "group_env.h"
#include "rowprog.h"

struct DpPull; struct DpSlots; struct DpAttach;       // dp_pull.h
struct rlrep_agent;                                   // engine_internal.h
struct rlrep_comm;                                    // comm.hip

extern "C" {
// ---- engine.hip ----
const RlGrp* rl_grp_active();                         // the group of the library call in progress (group.h), null outside one
// rlrep_comm_attach (comm.hip) hands the comm's exchange block to the agent
int rl_agent_attach_dp(rlrep_agent* ag, const DpAttach* at, int* attached_mask);
// ---- gemm16.hip ----
void rl_gemm16_read_env();                            // RLREP_DISABLE=gemm16_fast / gemm16_spec, RLREP_ENABLE=gemm16_trace, read at agent creation
int rl_launch_gemm16(int la, int lb, int nf, const GemmBatch* gb, int total_tiles, hipStream_t st);
int rl_launch_gemm16_duo(int split, int nf2, const GemmBatch* gb, int total_tiles, hipStream_t st);
// ---- gemm_lds.hip ----
int rl_launch_gemm_lds(GlKind kind, int la, int lb, const GemmBatch* gb, int total_tiles, int fin_blocks, hipStream_t st);
int rl_gemm_lds_dims_ok(const GemmTask* t);
int rl_gemm_lds_dim_flags(const GemmTask* t, int la, int lb);
int rl_gemm_lds_ptr_flags(const GemmTask* t);
GlKind rl_gemm_lds_route(const GemmTask* t, int la, int lb, int extra_flags, int* splits, int* kchunk, int* flags);
void rl_gemm_lds_plan(const GemmTask* t, int* bt, int* splits, int* kchunk);
// ---- noisecritic.hip ----
int rl_launch_nc_fwd(const NcFwdBatch* nb, int total_tiles, int g2, int chunked, hipStream_t st);
int rl_nc_fwd_chunked(int F, int g2);
int rl_launch_nc_dx(const NcDxTask* t, hipStream_t st);
int rl_nc_dx_engine(const NcDxTask* t);
int rl_launch_nc_dw(const NcDwBatch* nb, int total_tiles, hipStream_t st);
int rl_nc_init();
int rl_nc_dw_engine();
int rl_nc_dw_splits(int B, int F, int H, int ntasks);
int rl_nc_fwd_cols();
void rl_nc_fwd_plan(const NcFwdTask* tasks, int ntasks, int* engine, int* g2, int* cols);
// ---- elementwise.hip ----
int rl_launch_fill_slot(const SlotFill* p, hipStream_t st);
int rl_launch_philox(const PhiloxFill* p, hipStream_t st);
int rl_launch_philox_raw(const uint32_t* ck, uint32_t* out, long long n, hipStream_t st);
int rl_launch_policy_fwd(const PolicyFwd* p, hipStream_t st);
int rl_launch_policy_bwd(const PolicyBwd* p, hipStream_t st);
int rl_launch_vae_mid(const VaeMid* p, hipStream_t st);
int rl_launch_heads_vae(const HeadsVae* p, hipStream_t st);
int rl_launch_vae_mse(const VaeMse* p, hipStream_t st);
int rl_launch_qhead_critic(const QHeadCritic* p, hipStream_t st);
int rl_launch_qhead_actor(const QHeadActor* p, hipStream_t st);
int rl_launch_counter_sync(int* c, int mirror, hipStream_t st);
int rl_launch_counter_inc(int* c, int mirror, hipStream_t st);
int rl_launch_adam(const AdamTask* task, int adam_blocks, const FinTask* fin, int nfin, const SlotFill* sf, const SlotFill* sf2, const AdamSnap* snap, const DpPull* dp, hipStream_t st);
int rl_launch_adam_l1(const AdamTask* task, int adam_blocks, const FinTask* fin, int nfin, const SlotFill* sf, const GemmTask* g0, const GemmTask* g1, hipStream_t st);
int rl_adam_dp_occupancy(int* one_shot, int* two_shot);
int rl_launch_train_prologue(TrainPrologue* p, hipStream_t st);
int rl_launch_polyak(const PolyakTask* t, hipStream_t st);
int rl_launch_copy(const float* src, float* dst, long long n, hipStream_t st);
int rl_launch_copy_segs(const CopySegs* p, hipStream_t st);
int rl_launch_shadow(const ShadowEnt* sh_dev, int nsh, int ntiles, const float* base, int target, hipStream_t st);
int rl_launch_select_action(const SelectAct* p, hipStream_t st);
int rl_launch_select_action_n(const SelectAct* p, int rows, hipStream_t st);      // `rows` observations (per member of an active group), one workgroup each
int rl_launch_replay_add(float* ring, long long capacity, int row, long long ptr, const float* rows, long long nrows, int* size_dev, int new_size, hipStream_t st);
int rl_launch_replay_add_grp(float* ring, long long ring_stride, int members, long long capacity, int row, long long ptr, const float* rows,
                             long long rows_stride, long long nrows, int* size_dev, int new_size, hipStream_t st);
int rl_launch_replay_add_cols(const ReplayCols* p, int members, hipStream_t st);  // members == 0: one ring; otherwise grid y = member
int rl_launch_replay_add_cols_ctl(const ReplayCols* p, long long* ctl, hipStream_t st);     // start and fill level from the loop record (RL_CTL_*)
int rl_launch_replay_add_cols_ctl_grp(const ReplayCols* p, long long* ctl, hipStream_t st); // an active group: its live members, each from its own row of the record
// ---- actor_tile.hip ----
long long rl_actor_tile_lds_bytes(int S, int Ha, int A);
int rl_launch_actor_tile(const ActTile* p, hipStream_t st);                        // p->rows observations (per member of an active group), 16 per workgroup
int rl_launch_actor_tile_ctl(const ActTile* p, const ActCtl* k, hipStream_t st);   // one agent; counters from the loop record, exploration mix behind the head
int rl_launch_actor_tile_ctl_grp(const ActTile* p, const ActCtl* k, hipStream_t st);        // an active group; k->ctl: the group's record, int64[members][8]
// ---- per.hip (prioritized replay of a single agent: one workgroup each; the weighted sac critic head; sample + slot gather in one launch) ----
int rl_launch_per_add(const PerAdd* p, hipStream_t st);
int rl_launch_per_rebuild(float* tree, long long P, hipStream_t st);
int rl_launch_per_sample(const PerSample* p, hipStream_t st);
int rl_launch_per_update(const PerUpdate* p, hipStream_t st);
int rl_launch_qhead_critic_w(const QHeadCriticW* p, hipStream_t st);                // its group form (per_group.hip) while a group is active
// (prioritized replay of the representation agents' critic minibatch: sample + slot gather, workgroup 0 samples, the rest gather)
int rl_launch_per_sample_fill(PerSampleFill* p, hipStream_t st);                    // sets p->rows
// ---- per_group.hip (prioritized replay of a sac seed group: one workgroup per member; all but per_add need an active group) ----
int rl_launch_per_add_grp(const PerAdd* p, int members, hipStream_t st);                                    // member m: tree + m * 2P, scal + 4 m
int rl_launch_per_sample_grp(const PerSample* p, hipStream_t st);
int rl_launch_per_gather_grp(const SlotFill* fill, const int* idx, long long ring_rows, hipStream_t st);      // ring row idx[m][b] of member m's ring -> its slot 0, grid (blocks, R)
int rl_launch_per_update_grp(const PerUpdate* p, long long td_stride, hipStream_t st);                      // td_stride < 0: td moves by the member stride
int rl_launch_qhead_critic_w_grp(const QHeadCriticW* p, hipStream_t st);
// (prioritized critic replay of a ctrlsac seed group: the group form of rl_launch_per_sample_fill, grid (1 + G, R); the weighted head with a [R, B] td)
int rl_launch_per_sample_fill_grp(PerSampleFill* p, hipStream_t st);                 // sets p->rows; needs an active group
int rl_launch_qhead_critic_wtd_grp(const QHeadCriticW* p, hipStream_t st);          // w and td: the buffer group's [R, B] arrays
// ---- nstep.hip (n-step returns: the chain-following replay gather, one wave per sample) ----
int rl_launch_nstep_gather(const NStepGather* p, hipStream_t st);
int rl_launch_nstep_gather_grp(const NStepGather* p, int idx_rows, hipStream_t st);       // grid (x, R); idx_rows == 0: the indices move by the member stride, else int32[R, idx_rows]
// ---- nstep_targets.hip (n-step critic targets of the representation agents: the same walk, writing XF2[:, 0:S], Rn and D only) ----
int rl_launch_nstep_targets(const NStepTargets* p, hipStream_t st);
// ---- replearn.hip ----
int rl_replearn_init();
int rl_launch_infonce(const InfoNce* p, hipStream_t st);
int rl_launch_colsum(const ColSum* p, hipStream_t st);
int rl_launch_reg_stats(const RegStats* p, hipStream_t st);
int rl_launch_speder_rows(const SpederRows* p, hipStream_t st);
int rl_launch_speder_grads(const SpederGrads* p, hipStream_t st);
int rl_launch_diffsr_perturb(const DiffsrPerturb* p, hipStream_t st);
DsForm rl_diffsr_score_form(const DiffsrScore* p);   // host only: the kernel rl_launch_diffsr_score picks (reads the switches in force)
int rl_launch_diffsr_score(const DiffsrScore* p, hipStream_t st);
int rl_launch_copy2(const float* src, float* d1, float* d2, long long n, hipStream_t st);
// ---- comm.hip: the comm's pull descriptor; ctrlsac's batch-coupled exchanges as launches of the step program (attached agents) ----
void rl_comm_fill_pull(const rlrep_comm* c, DpPull* d);
int rl_launch_xchg_gather(const DpPull* proto, int channel, long long off, long long n, int no_done, hipStream_t st);
int rl_launch_xchg_reduce(const DpPull* proto, int channel, long long off, long long n, float* out, int two_shot, int no_done, hipStream_t st);
int rl_launch_slots_sum(const DpSlots* d, float* out, hipStream_t st);
// ---- group_clone.hip ----
int rl_launch_group_clone(const CloneTab* tab, const ClonePairs* pairs, int npairs, hipStream_t st);
int rl_launch_group_live(int* table_dev, const LiveTab* tab, int members, hipStream_t st);
// ---- group_env.hip ----
int rl_launch_group_env_reset(int kind, EnvRecord* recs, EnvCtl* ctl, const unsigned long long* seeds, int members, int num_envs, hipStream_t st);
int rl_launch_group_env_step(int kind, const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y,
                             int num_envs, EnvRecord* recs, EnvCtl* ctl, float* ring, long long ring_stride, long long capacity, int* size_dev, float eps_greedy,
                             long long start_timesteps, hipStream_t st);
int rl_launch_group_env_eval(int kind, const SelectAct* p, long long mstride, const unsigned long long* seeds, const int* live, int grid_y,
                             unsigned long long counter0, int episodes, double* out, double* starts, hipStream_t st);
int rl_launch_env_reset(int kind, EnvRecord* rec, EnvCtl* ctl, unsigned long long seed, int num_envs, hipStream_t st);
int rl_launch_env_step(int kind, const SelectAct* p, int num_envs, EnvRecord* rec, EnvCtl* ctl, float* ring, long long capacity, int* size_dev, float eps_greedy,
                       long long start_timesteps, hipStream_t st);
int rl_launch_env_eval(int kind, const SelectAct* p, unsigned long long counter0, int episodes, double* out, double* starts, hipStream_t st);
// ---- sim_step.hip (fused simulators: one thread per environment, grid ceil(n / 256); an unknown kind or n outside [1, RL_SIM_MAX_ENVS]: -7) ----
int rl_launch_sim_start(const SimState* s, hipStream_t st);
int rl_launch_sim_step(const SimState* s, const float* act, long long ld_act, float* next_obs, float* reward, float* done, hipStream_t st);
int rl_launch_sim_step_ctl(const SimState* s, const float* act, long long ld_act, float* ring, long long capacity, int* size_dev, long long* ctl,
                           hipStream_t st);                                        // + the ring rows and the append launch's one thread (RL_CTL_*)
// (their group forms: [members, n] planes, member m keyed by seeds[m], grid (ceil(n / 256), y); all need an active group, the steps its live table)
int rl_launch_sim_start_grp(const SimState* s, const unsigned long long* seeds, hipStream_t st);
int rl_launch_sim_step_grp(const SimState* s, const unsigned long long* seeds, const float* act, long long ld_act, float* next_obs, float* reward, float* done,
                           hipStream_t st);
int rl_launch_sim_step_ctl_grp(const SimState* s, const unsigned long long* seeds, const float* act, long long ld_act, float* ring, long long ring_stride,
                               long long capacity, int* size_dev, long long* ctl, hipStream_t st);       // the group's loop record: int64[members][8]
// ---- rowprog.hip / xchain.hip (experiments build); experiments_off.hip (product build: stubs) ----
int rl_launch_rowprog(const RpLaunch* L, int total_blocks, hipStream_t st);
int rl_rowprog_init();
int rl_launch_xchain(const XcLaunch* L, hipStream_t st);
}

// ---- plain C++ (engine.hip; g_rl_front: gemm16.hip) ----
void rl_set_error(const char* fmt, ...);
void rl_switches_read();                              // parses RLREP_DISABLE / RLREP_ENABLE at a library entry (what rl_off / rl_opt of common.h then answer)
// process-wide count of kernel launches issued by the library (rlrep_launch_counter: bench.py counts the launches a captured train() holds)
extern long long g_rl_launches;
extern long long g_rl_front[4];                       // launches per front end of the 16-row tile engine (fast, fast4, fastpre, record)
