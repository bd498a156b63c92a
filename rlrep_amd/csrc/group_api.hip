// C ABI of seed groups and of device environments -- a group's and a single agent's (include/rlrep.h rlrep_group_*, rlrep_group_env_*, rlrep_env_*): host side; the group forms of the
// kernels live beside the single-agent kernels, group_clone.hip and group_env.hip hold the kernels only groups have.
#include "engine_internal.h"
#include <cmath>
#include <cstddef>

// [p, p + bytes) inside member 0's block [grp_lo, grp_lo + stride): what a group launch moves by r * stride must stay in member r's block
bool in_member0(const rlrep_agent* ag, const void* p, long long bytes) {
    const char* q = (const char*)p;
    return q && bytes >= 0 && q >= ag->grp_lo && q + bytes <= ag->grp_lo + ag->grp_stride;
}

extern "C" {

// ---- seed groups ------------------------------------------------------------------------------------------------------------------------------
// byte extent of the seven arenas of one member: [lowest arena pointer, end of the highest)
static long long member_span(const rlrep_layout_info& info, const rlrep_arenas* a) {
    const char* p[7] = {(const char*)a->param_dev, (const char*)a->target_dev, (const char*)a->grad_dev, (const char*)a->exp_avg_dev,
                        (const char*)a->exp_avg_sq_dev, (const char*)a->workspace_dev, (const char*)a->alpha_state_dev};
    const long long n[7] = {4 * info.param_floats, 4 * info.target_floats, 4 * info.grad_floats, 4 * info.param_floats, 4 * info.param_floats,
                            (long long)info.workspace_bytes, 4 * 8};
    const char* lo = p[0]; const char* hi = p[0] + n[0];
    for (int q = 1; q < 7; ++q) { lo = std::min(lo, p[q]); hi = std::max(hi, p[q] + n[q]); }
    return (long long)(hi - lo);
}
int32_t rlrep_group_max_members(void) { return RLREP_GROUP_MAX_MEMBERS; }
// what the step programs carry by value from rlrep_hyper, as a group member's record holds it (kparams.h MemberHyper; agents1.hip actor_fins,
// critic_apply_folded and the qhead critic stages read the same fields)
static MemberHyper member_hyper_of(const rlrep_hyper& h) {
    MemberHyper m;
    m.gamma = h.discount; m.pol_period = h.target_update_period; m.alpha_lr = h.lr_actor; m.learn = h.learn_alpha;
    return m;
}

int32_t rlrep_group_create(const rlrep_dims* dims, const rlrep_hyper* hyper, const rlrep_arenas* arenas, int32_t members, int64_t member_stride_bytes,
                           void* stream, rlrep_agent** out) {
    if (!dims || !hyper || !arenas || !out) { rl_set_error("group_create: null argument"); return RLREP_ERR_ARG; }
    if (dims->alg != RLREP_ALG_SAC && dims->alg != RLREP_ALG_CTRLSAC) {
        rl_set_error("group_create: seed groups are built for sac and ctrlsac only (alg %d)", dims->alg); return RLREP_ERR_ARG;
    }
    if (members < 1 || members > RLREP_GROUP_MAX_MEMBERS) { rl_set_error("group_create: members %d outside [1, %d]", members, RLREP_GROUP_MAX_MEMBERS); return RLREP_ERR_ARG; }
    if (dims->world_size > 1 || hyper->world_size > 1) { rl_set_error("group_create: a seed group does not attach to data parallel (world_size %d)", std::max(dims->world_size, hyper->world_size)); return RLREP_ERR_ARG; }
    if (member_stride_bytes <= 0 || (member_stride_bytes & 255)) { rl_set_error("group_create: member stride %lld is not a positive multiple of 256 bytes", (long long)member_stride_bytes); return RLREP_ERR_ARG; }
    if (!arenas->param_dev || !arenas->grad_dev || !arenas->exp_avg_dev || !arenas->exp_avg_sq_dev || !arenas->workspace_dev ||
        !arenas->alpha_state_dev || !arenas->target_dev) { rl_set_error("group_create: null arena pointer"); return RLREP_ERR_ARG; }
    rlrep_layout_info info;
    if (!check_dims(dims) || rlrep_layout(dims, &info, nullptr, 0) != 0) return RLREP_ERR_ARG;
    const long long span = member_span(info, arenas);
    if (member_stride_bytes < span) { rl_set_error("group_create: member stride %lld is smaller than the member span %lld", (long long)member_stride_bytes, span); return RLREP_ERR_ARG; }
    rlrep_agent* ag = nullptr;
    int rc = rlrep_agent_create(dims, hyper, arenas, stream, &ag);
    if (rc) return rc;
    ag->members = members; ag->grp_stride = member_stride_bytes;
    // every member starts as a byte copy of member 0's block (step counters, optimizer records, metric slots; the caller then writes each
    // member's parameters): the programs' device records are member 0's, and a group launch moves every pointer it finds in them
    hipError_t e = hipMalloc((void**)&ag->grp_seeds, sizeof(unsigned long long) * members);
    if (e == hipSuccess) e = hipMemsetAsync(ag->grp_seeds, 0, sizeof(unsigned long long) * members, (hipStream_t)stream);
    // the live table: everybody live (n_live = members, slot r = member r)
    LiveTab live0; memset(&live0, 0, sizeof(live0));
    live0.n_live = members;
    for (int m = 0; m < members; ++m) live0.slot_member[m] = m;
    if (e == hipSuccess) e = hipMalloc((void**)&ag->grp_live, sizeof(int) * (1 + members));
    if (e == hipSuccess) e = hipMemcpyAsync(ag->grp_live, &live0, sizeof(int) * (1 + members), hipMemcpyHostToDevice, (hipStream_t)stream);   // (synchronised below)
    ag->grp_live_mask.assign(members, 1);
    ag->grp_compact = rl_opt("grp_compact") != nullptr; ag->grp_grid_y = members;
    const char* lo = (const char*)arenas->param_dev;
    for (const void* q : {(const void*)arenas->target_dev, (const void*)arenas->grad_dev, (const void*)arenas->exp_avg_dev, (const void*)arenas->exp_avg_sq_dev,
                          (const void*)arenas->workspace_dev, (const void*)arenas->alpha_state_dev}) lo = std::min(lo, (const char*)q);
    ag->grp_lo = lo;
    ag->grp_hyper.assign(members, ag->h);
    const MemberHyper mh0 = member_hyper_of(ag->h);
    if (e == hipSuccess) e = hipMemcpyAsync(ag->mhyp, &mh0, sizeof(mh0), hipMemcpyHostToDevice, (hipStream_t)stream);
    for (int m = 1; m < members && e == hipSuccess; ++m)
        e = hipMemcpyAsync((char*)lo + (long long)m * member_stride_bytes, lo, (size_t)span, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { rl_set_error("group_create: %s", hipGetErrorString(e)); rlrep_agent_destroy(ag); return RLREP_ERR_HIP; }
    *out = ag;
    return 0;
}
int32_t rlrep_group_members(rlrep_agent* ag) { return ag ? ag->members : RLREP_ERR_ARG; }
int32_t rlrep_group_set_seeds(rlrep_agent* ag, const uint64_t* seeds, int32_t n, void* stream) {
    if (!ag || ag->members <= 0 || !seeds || n != ag->members) { rl_set_error("group_set_seeds: need one seed per member of a group"); return RLREP_ERR_ARG; }
    const hipError_t e = hipMemcpyAsync(ag->grp_seeds, seeds, sizeof(uint64_t) * n, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) (void)hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { rl_set_error("group_set_seeds: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_set_member_hyper(rlrep_agent* ag, int32_t member, const rlrep_hyper* hyper, void* stream) {
    GROUP_ONLY("group_set_member_hyper")
    if (member < 0 || member >= ag->members) { rl_set_error("group_set_member_hyper: member %d outside [0, %d)", member, ag->members); return RLREP_ERR_ARG; }
    if (!hyper) { rl_set_error("group_set_member_hyper: null hyper"); return RLREP_ERR_ARG; }
    const rlrep_hyper& g = ag->h;
    // structural: these shape the step programs (or are shared by every member's launches) -- equal to the group's or refused
    const int ws = hyper->world_size > 0 ? hyper->world_size : 1;
    const struct { const char* name; double have, want; } st[] = {
        {"target_entropy", hyper->target_entropy, g.target_entropy}, {"sigma_scale", hyper->sigma_scale, g.sigma_scale},
        {"extra_feature_steps", (double)hyper->extra_feature_steps, (double)g.extra_feature_steps}, {"world_size", (double)ws, (double)g.world_size},
        {"beta1", hyper->beta1, g.beta1}, {"beta2", hyper->beta2, g.beta2}, {"adam_eps", hyper->adam_eps, g.adam_eps},
        {"critic_reg_lambda", hyper->critic_reg_lambda, g.critic_reg_lambda}};
    for (const auto& f : st)
        if (!(f.have == f.want)) {
            rl_set_error("group_set_member_hyper: %s is structural and must equal the group's (%g, the group has %g)", f.name, f.have, f.want);
            return RLREP_ERR_ARG;
        }
    const struct { const char* name; float v; } lrs[] = {{"lr_feature", hyper->lr_feature}, {"lr_critic", hyper->lr_critic}, {"lr_actor", hyper->lr_actor}};
    for (const auto& f : lrs)
        if (!std::isfinite(f.v) || !(f.v > 0.f)) { rl_set_error("group_set_member_hyper: %s %g is not a finite positive learning rate", f.name, (double)f.v); return RLREP_ERR_ARG; }
    if (!std::isfinite(hyper->discount)) { rl_set_error("group_set_member_hyper: discount %g is not finite", (double)hyper->discount); return RLREP_ERR_ARG; }
    if (!(hyper->tau >= 0.f && hyper->tau <= 1.f)) { rl_set_error("group_set_member_hyper: tau %g outside [0, 1]", (double)hyper->tau); return RLREP_ERR_ARG; }
    if (!(hyper->feature_tau >= 0.f && hyper->feature_tau <= 1.f)) { rl_set_error("group_set_member_hyper: feature_tau %g outside [0, 1]", (double)hyper->feature_tau); return RLREP_ERR_ARG; }
    if (hyper->target_update_period < 1) { rl_set_error("group_set_member_hyper: target_update_period %d is below 1", hyper->target_update_period); return RLREP_ERR_ARG; }
    rlrep_hyper h = *hyper;
    h.world_size = ws;
    // the member's optimizer records: lr, beta1, beta2, eps, tau of each of the four groups -- as rlrep_agent_create writes them (the step
    // counters and the running powers stay); then its by-value record.  Both are read at the next launch: captured graphs need no re-capture.
    struct Words { float lr, b1, b2, eps, tau; } w[4];
    static_assert(offsetof(GroupCfg, tau) - offsetof(GroupCfg, lr) == 4 * sizeof(float), "GroupCfg words lr .. tau");
    for (int q = 0; q < 4; ++q) {
        w[q].lr = q == 1 ? h.lr_critic : q == 2 ? h.lr_actor : h.lr_feature;
        w[q].b1 = h.beta1; w[q].b2 = h.beta2; w[q].eps = h.adam_eps;
        w[q].tau = (q == 0) ? h.feature_tau : (q == 1) ? h.tau : 0.f;
    }
    const MemberHyper mh = member_hyper_of(h);
    const long long d = (long long)member * ag->grp_stride;
    hipStream_t sm = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    for (int q = 0; q < 4 && e == hipSuccess; ++q)
        e = hipMemcpyAsync((char*)&ag->adam_step[q].lr + d, &w[q], sizeof(Words), hipMemcpyHostToDevice, sm);
    if (e == hipSuccess) e = hipMemcpyAsync((char*)ag->mhyp + d, &mh, sizeof(mh), hipMemcpyHostToDevice, sm);
    if (e == hipSuccess) e = hipStreamSynchronize(sm);          // (the host words above live on this stack frame)
    if (e != hipSuccess) { rl_set_error("group_set_member_hyper: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    ag->grp_hyper[member] = h;
    return 0;
}
int32_t rlrep_group_get_member_hyper(rlrep_agent* ag, int32_t member, rlrep_hyper* out) {
    GROUP_ONLY("group_get_member_hyper")
    if (member < 0 || member >= ag->members) { rl_set_error("group_get_member_hyper: member %d outside [0, %d)", member, ag->members); return RLREP_ERR_ARG; }
    if (!out) { rl_set_error("group_get_member_hyper: null output"); return RLREP_ERR_ARG; }
    *out = ag->grp_hyper[member];
    return 0;
}
// what changes a group between two train() calls refuses to run inside one: `what` names the caller in the message
static bool in_train_refused(const char* what, const rlrep_agent* ag) {
    if (ag->in_train) rl_set_error("%s: inside a train() (between rlrep_group_train_prologue and the end of that train())", what);
    return ag->in_train;
}
int32_t rlrep_group_clone_members(rlrep_agent* ag, const int32_t* src_host, const int32_t* dst_host, int32_t n, void* stream) {
    GROUP_ONLY("group_clone_members")
    if (!src_host || !dst_host) { rl_set_error("group_clone_members: null member list"); return RLREP_ERR_ARG; }
    if (n < 1 || n > ag->members) { rl_set_error("group_clone_members: n %d outside [1, %d]", n, ag->members); return RLREP_ERR_ARG; }
    // pairs must be independent of each other (one launch serves all of them, in no order): role 1 = a source, 2 = a destination
    char role[RLREP_GROUP_MAX_MEMBERS] = {0};
    ClonePairs pairs; memset(&pairs, 0, sizeof(pairs));
    for (int k = 0; k < n; ++k) {
        const int s = src_host[k], d = dst_host[k];
        if (s < 0 || s >= ag->members || d < 0 || d >= ag->members) {
            rl_set_error("group_clone_members: pair %d (%d -> %d) names a member outside [0, %d)", k, s, d, ag->members); return RLREP_ERR_ARG;
        }
        if (s == d) { rl_set_error("group_clone_members: pair %d copies member %d onto itself", k, s); return RLREP_ERR_ARG; }
        if (role[d] == 2) { rl_set_error("group_clone_members: member %d is a destination twice", d); return RLREP_ERR_ARG; }
        if (role[d] == 1 || role[s] == 2) {
            rl_set_error("group_clone_members: member %d is both a source and a destination", role[d] == 1 ? d : s); return RLREP_ERR_ARG;
        }
        role[s] = 1; role[d] = 2;
        pairs.src[k] = s; pairs.dst[k] = d;
    }
    if (in_train_refused("group_clone_members", ag)) return RLREP_ERR_ARG;
    // what a standalone agent's load(snapshot) restores: four arenas, the temperature state, the device records (static_state: the train()
    // counter block, the optimizer records, the metric slots -- the head of the workspace, up to the end of the metric slots)
    CloneTab tab; memset(&tab, 0, sizeof(tab));
    tab.base = const_cast<char*>(ag->grp_lo); tab.stride = ag->grp_stride;
    const long long pf = 4ll * ag->L.cur[RLREP_ARENA_PARAM], tf = 4ll * ag->L.cur[RLREP_ARENA_TARGET];
    const char* ws0 = (const char*)ag->a.workspace_dev;
    const struct { const void* p; long long bytes; } segs[] = {
        {ag->a.param_dev, pf}, {ag->a.target_dev, tf}, {ag->a.exp_avg_dev, pf}, {ag->a.exp_avg_sq_dev, pf}, {ag->a.alpha_state_dev, 4 * 8},
        {ws0, (long long)((const char*)(ag->metrics + M_COUNT) - ws0)}};
    static_assert(sizeof(segs) / sizeof(segs[0]) <= RL_CLONE_MAX_SEGS, "CloneTab segments");
    for (const auto& g : segs) {
        if (g.bytes <= 0) continue;
        const long long off = (const char*)g.p - ag->grp_lo;
        if (off < 0 || (off & 3) || (g.bytes & 3) || off + g.bytes > ag->grp_stride) {
            rl_set_error("group_clone_members: a segment [%lld, %lld) leaves the member block of %lld bytes", off, off + g.bytes, ag->grp_stride); return RLREP_ERR_ARG;
        }
        if (g.p == ws0) {
            tab.rec_seg = tab.nseg;
            tab.rec_w0 = (int)(((const char*)ag->adam_step - ws0) >> 2); tab.rec_nw = 4 * RLREP_GROUP_CFG_WORDS; tab.rec_words = RLREP_GROUP_CFG_WORDS;
            if ((const char*)ag->steps != ws0 || (const char*)(ag->adam_step + 4) > (const char*)ag->metrics) {
                rl_set_error("group_clone_members: the device records are not laid out as static_state lays them out"); return RLREP_ERR_ARG;
            }
        }
        tab.seg[tab.nseg].off = off; tab.seg[tab.nseg].bytes = g.bytes; ++tab.nseg;
    }
    ++g_rl_launches;
    const int rc = rl_launch_group_clone(&tab, &pairs, n, (hipStream_t)stream);
    if (rc) { rl_set_error("group_clone_members: launch failed (%d)", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_set_live(rlrep_agent* ag, const int32_t* live_host, void* stream) {
    GROUP_ONLY("group_set_live")
    if (!live_host) { rl_set_error("group_set_live: null mask"); return RLREP_ERR_ARG; }
    LiveTab tab; memset(&tab, 0, sizeof(tab));
    for (int m = 0; m < ag->members; ++m) {
        if (live_host[m] != 0 && live_host[m] != 1) { rl_set_error("group_set_live: mask[%d] = %d is neither 0 nor 1", m, live_host[m]); return RLREP_ERR_ARG; }
        if (live_host[m]) tab.slot_member[tab.n_live++] = m;
    }
    if (tab.n_live < 1) { rl_set_error("group_set_live: no live member (at least one member of a group stays live)"); return RLREP_ERR_ARG; }
    if (in_train_refused("group_set_live", ag)) return RLREP_ERR_ARG;
    // the slots behind n_live name no member (0): a launch never reads them
    ++g_rl_launches;
    const int rc = rl_launch_group_live(ag->grp_live, &tab, ag->members, (hipStream_t)stream);
    if (rc) { rl_set_error("group_set_live: launch failed (%d)", rc); return RLREP_ERR_HIP; }
    ag->grp_live_mask.assign(live_host, live_host + ag->members);
    ag->grp_grid_y = ag->grp_compact ? tab.n_live : ag->members;
    return 0;
}
int32_t rlrep_group_get_live(rlrep_agent* ag, int32_t* live_out) {
    GROUP_ONLY("group_get_live")
    if (!live_out) { rl_set_error("group_get_live: null output"); return RLREP_ERR_ARG; }
    for (int m = 0; m < ag->members; ++m) live_out[m] = ag->grp_live_mask[m];
    return 0;
}
int32_t rlrep_group_train_prologue(rlrep_agent* ag, const float* ring_dev, int64_t ring_stride_bytes, const int32_t* size_dev, int32_t* idx_pool_dev, int64_t n_idx,
                                   float* eps_pool_dev, int64_t n_eps, uint64_t idx_offset, uint64_t eps_offset, int32_t batch, void* stream) {
    GROUP_ONLY("group_train_prologue")
    if (ring_stride_bytes < 0 || (ring_stride_bytes & 3) || (ag->members > 1 && ring_stride_bytes < 4ll * batch)) {
        rl_set_error("group_train_prologue: bad ring stride %lld", (long long)ring_stride_bytes); return RLREP_ERR_ARG;
    }
    if (!in_member0(ag, idx_pool_dev, 4 * n_idx) || !in_member0(ag, eps_pool_dev, 4 * n_eps)) {
        rl_set_error("group_train_prologue: the index / noise pools must lie inside member 0's block (they are written at every member's stride)");
        return RLREP_ERR_ARG;
    }
    ag->grp_ring_stride = ring_stride_bytes;          // (also what a later optimizer launch's ring gather moves by)
    GrpScope grp_scope_(ag);
    return rlrep_train_prologue(ag, ring_dev, size_dev, idx_pool_dev, n_idx, eps_pool_dev, n_eps, 0, idx_offset, eps_offset, batch, stream);
}
int32_t rlrep_group_prepare(rlrep_agent* ag, int32_t batch) {
    GROUP_ONLY("group_prepare")
    return ensure_batch(ag, batch);
}
// the actor part of a SelectAct (member 0's weights, the dimensions, the action range); everything else zero
static void group_actor(rlrep_agent* ag, SelectAct& p, float lo, float hi) {
    memset(&p, 0, sizeof(p));
    p.W1 = ag->P("actor.trunk.0.weight"); p.b1 = ag->P("actor.trunk.0.bias"); p.W2 = ag->P("actor.trunk.2.weight"); p.b2 = ag->P("actor.trunk.2.bias");
    p.W3 = ag->P("actor.trunk.4.weight"); p.b3 = ag->P("actor.trunk.4.bias");
    p.S = ag->d.state_dim; p.Ha = ag->d.actor_hidden_dim; p.A = ag->d.action_dim; p.lo = lo; p.hi = hi;
}
int32_t rlrep_group_select_action(rlrep_agent* ag, const float* obs_host, int32_t explore, uint64_t offset, float lo, float hi, float* action_host, void* stream) {
    if (!ag || ag->members <= 0 || !obs_host || !action_host) { rl_set_error("group_select_action: bad argument (needs a seed group)"); return RLREP_ERR_ARG; }
    SelectAct p; group_actor(ag, p, lo, hi);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<float*>(obs_host), 0) != hipSuccess || !d) { rl_set_error("group_select_action: the observations are not mapped (pinned) host memory"); return RLREP_ERR_ARG; }
    p.obs = (const float*)d;
    if (hipHostGetDevicePointer(&d, action_host, 0) != hipSuccess || !d) { rl_set_error("group_select_action: the action buffer is not mapped (pinned) host memory"); return RLREP_ERR_ARG; }
    p.act = (float*)d;
    p.explore = explore ? 1 : 0; p.seed = 0; p.offset = offset;
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_select_action(&p, (hipStream_t)stream);
    if (rc) { rl_set_error("group_select_action: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
// `rows` observations per member in ONE launch (select_action_kernel_grp_n): obs_host [members, rows, S], action_host [members, rows, A]
int32_t rlrep_group_select_action_n(rlrep_agent* ag, const float* obs_host, int32_t rows, int32_t explore, uint64_t offset, float lo, float hi, float* action_host,
                                    void* stream) {
    if (!ag || !obs_host || !action_host) { rl_set_error("group_select_action_n: bad argument (null agent, observations or actions)"); return RLREP_ERR_ARG; }
    if (rows < 1 || rows > RLREP_SELECT_MAX_ROWS) { rl_set_error("group_select_action_n: rows %d outside [1, %d]", rows, RLREP_SELECT_MAX_ROWS); return RLREP_ERR_ARG; }
    GROUP_ONLY("group_select_action_n")
    SelectAct p; group_actor(ag, p, lo, hi);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<float*>(obs_host), 0) != hipSuccess || !d) { (void)hipGetLastError(); rl_set_error("group_select_action_n: the observations are not mapped (pinned) host memory"); return RLREP_ERR_ARG; }
    p.obs = (const float*)d;
    if (hipHostGetDevicePointer(&d, action_host, 0) != hipSuccess || !d) { (void)hipGetLastError(); rl_set_error("group_select_action_n: the action buffer is not mapped (pinned) host memory"); return RLREP_ERR_ARG; }
    p.act = (float*)d;
    p.explore = explore ? 1 : 0; p.seed = 0; p.offset = offset;
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_select_action_n(&p, rows, (hipStream_t)stream);
    if (rc) { rl_set_error("group_select_action_n: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_replay_add_sized(float* ring_dev, int64_t ring_stride_floats, int32_t members, int64_t capacity, int32_t row_floats, int64_t ptr,
                                     const float* rows_host, int64_t rows_stride_floats, int64_t nrows, int32_t* size_dev, int32_t new_size, void* stream) {
    if (!ring_dev || !rows_host || members < 1 || members > RLREP_GROUP_MAX_MEMBERS || capacity <= 0 || row_floats <= 0 || ring_stride_floats < capacity * row_floats ||
        rows_stride_floats < nrows * row_floats ||
        ptr < 0 || ptr >= capacity || nrows < 0 || nrows > capacity || new_size < 0 || new_size > capacity) {
        rl_set_error("group_replay_add_sized: bad argument"); return RLREP_ERR_ARG;
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<float*>(rows_host), 0) != hipSuccess || !d) { rl_set_error("group_replay_add_sized: the staging rows are not mapped (pinned) host memory"); return RLREP_ERR_ARG; }
    ++g_rl_launches;
    const int rc = rl_launch_replay_add_grp(ring_dev, ring_stride_floats, members, capacity, row_floats, ptr, (const float*)d, rows_stride_floats, nrows, size_dev, new_size, (hipStream_t)stream);
    if (rc) { rl_set_error("group_replay_add_sized: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// `rows` device-resident observations per member in ONE launch (actor_tile_kernel_grp, grid (ceil(rows / 16), members)): obs_dev [members, rows, S],
// action_dev [members, rows, A]; member r draws with seeds[r].  A retired member's planes are neither read nor written.
int32_t rlrep_group_act_device(rlrep_agent* ag, const float* obs_dev, int32_t rows, int32_t explore, uint64_t offset, float lo, float hi, float* action_dev,
                               void* stream) {
    if (!ag || !obs_dev || !action_dev) { rl_set_error("group_act_device: bad argument (null agent, observations or actions)"); return RLREP_ERR_ARG; }
    if (rows < 1 || rows > RLREP_ACT_MAX_ROWS) { rl_set_error("group_act_device: rows %d outside [1, %d]", rows, RLREP_ACT_MAX_ROWS); return RLREP_ERR_ARG; }
    GROUP_ONLY("group_act_device")
    SelectAct q; group_actor(ag, q, lo, hi);
    if (rl_actor_tile_lds_bytes(q.S, q.Ha, q.A) > RL_ACT_TILE_LDS_MAX) {
        rl_set_error("group_act_device: the activation tiles of S %d, Ha %d, A %d need %lld bytes of LDS, a workgroup has %d", q.S, q.Ha, q.A,
                     rl_actor_tile_lds_bytes(q.S, q.Ha, q.A), RL_ACT_TILE_LDS_MAX);
        return RLREP_ERR_ARG;
    }
    ActTile p; memset(&p, 0, sizeof(p));
    p.obs = obs_dev; p.act = action_dev; p.W1 = q.W1; p.b1 = q.b1; p.W2 = q.W2; p.b2 = q.b2; p.W3 = q.W3; p.b3 = q.b3;
    p.S = q.S; p.Ha = q.Ha; p.A = q.A; p.explore = explore ? 1 : 0; p.lo = lo; p.hi = hi; p.seed = 0; p.offset = offset;
    p.rows = rows; p.ld_obs = q.S; p.ld_act = q.A;
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_actor_tile(&p, (hipStream_t)stream);
    if (rc) { rl_set_error("group_act_device: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
// rlrep_replay_add_cols for `members` rings in ONE launch: member r's plane of the five arrays lies n rows behind member r - 1's
int32_t rlrep_group_replay_add_cols(float* ring_dev, int64_t max_size, int32_t row_floats, int64_t start, int32_t S, int32_t A, const float* s, int64_t ld_s,
                                    const float* a, int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n,
                                    int32_t members, int64_t ring_stride_floats, int32_t* size_dev, int32_t new_size, void* stream) {
    if (!ring_dev || !s || !a || !s2 || !r || !d) { rl_set_error("group_replay_add_cols: bad argument (null ring or array)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || n < 1 || n > max_size) { rl_set_error("group_replay_add_cols: n %lld outside [1, max_size %lld]", (long long)n, (long long)max_size); return RLREP_ERR_ARG; }
    if (S < 1 || A < 1 || row_floats != 2 * S + A + 2) { rl_set_error("group_replay_add_cols: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, S, A); return RLREP_ERR_ARG; }
    if (start < 0 || start >= max_size) { rl_set_error("group_replay_add_cols: start %lld outside the ring of %lld rows", (long long)start, (long long)max_size); return RLREP_ERR_ARG; }
    if (members < 1 || members > RLREP_GROUP_MAX_MEMBERS || ring_stride_floats < max_size * row_floats || ld_s < S || ld_a < A || ld_s2 < S || new_size < 0 || new_size > max_size) {
        rl_set_error("group_replay_add_cols: bad argument (members, the ring stride, a row stride below its width, or new_size outside the ring)"); return RLREP_ERR_ARG;
    }
    ReplayCols p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.capacity = max_size; p.start = start; p.ring_stride = ring_stride_floats; p.row = row_floats; p.S = S; p.A = A; p.new_size = new_size;
    p.s = s; p.a = a; p.s2 = s2; p.r = r; p.d = d; p.ld_s = ld_s; p.ld_a = ld_a; p.ld_s2 = ld_s2; p.n = n; p.size_dev = size_dev;
    ++g_rl_launches;
    const int rc = rl_launch_replay_add_cols(&p, members, (hipStream_t)stream);
    if (rc) { rl_set_error("group_replay_add_cols: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// ---- the one-graph simulator loop of a seed group (kparams.h "the loop record of a GROUP": int64[members][8]) ----------------
// rlrep_act_device_ctl for every live member in ONE launch (actor_tile_kernel_ctl_grp): the group's CALLS / T / ITER, member r's key seeds[r],
// its cursor moved by `rows` in its own row of the record
int32_t rlrep_group_act_device_ctl(rlrep_agent* ag, const float* obs_dev, int32_t rows, float lo, float hi, float* action_dev, int64_t* ctl_dev,
                                   int64_t max_size, float eps_greedy, int64_t start_timesteps, void* stream) {
    if (!ag || !obs_dev || !action_dev || !ctl_dev) { rl_set_error("group_act_device_ctl: bad argument (null agent, observations, actions or loop record)"); return RLREP_ERR_ARG; }
    if (rows < 1 || rows > RLREP_ACT_MAX_ROWS) { rl_set_error("group_act_device_ctl: rows %d outside [1, %d]", rows, RLREP_ACT_MAX_ROWS); return RLREP_ERR_ARG; }
    if (max_size < rows) { rl_set_error("group_act_device_ctl: rows %d outside [1, max_size %lld] (the rings the cursors move in)", rows, (long long)max_size); return RLREP_ERR_ARG; }
    if (!(eps_greedy >= 0.f && eps_greedy <= 1.f) || start_timesteps < 0) {
        rl_set_error("group_act_device_ctl: bad argument (eps_greedy outside [0, 1] or a negative start_timesteps)"); return RLREP_ERR_ARG;
    }
    GROUP_ONLY("group_act_device_ctl")                  // (what needs no handle is checked first)
    SelectAct q; group_actor(ag, q, lo, hi);
    if (rl_actor_tile_lds_bytes(q.S, q.Ha, q.A) > RL_ACT_TILE_LDS_MAX) {
        rl_set_error("group_act_device_ctl: the activation tiles of S %d, Ha %d, A %d need %lld bytes of LDS, a workgroup has %d", q.S, q.Ha, q.A,
                     rl_actor_tile_lds_bytes(q.S, q.Ha, q.A), RL_ACT_TILE_LDS_MAX);
        return RLREP_ERR_ARG;
    }
    ActTile p; memset(&p, 0, sizeof(p));
    p.obs = obs_dev; p.act = action_dev; p.W1 = q.W1; p.b1 = q.b1; p.W2 = q.W2; p.b2 = q.b2; p.W3 = q.W3; p.b3 = q.b3;
    p.S = q.S; p.Ha = q.Ha; p.A = q.A; p.explore = 1; p.lo = lo; p.hi = hi; p.seed = 0;
    p.rows = rows; p.ld_obs = q.S; p.ld_act = q.A;
    ActCtl k; memset(&k, 0, sizeof(k));
    k.ctl = (long long*)ctl_dev; k.capacity = max_size; k.start_timesteps = start_timesteps; k.eps_greedy = eps_greedy;
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_actor_tile_ctl_grp(&p, &k, (hipStream_t)stream);
    if (rc) { rl_set_error("group_act_device_ctl: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
// rlrep_replay_add_cols_ctl for every live member in ONE launch (replay_add_cols_kernel_ctl_grp): member r's plane of the five arrays into its
// ring from its own start row, its fill level into size_dev[r], the group's counters advanced once
int32_t rlrep_group_replay_add_cols_ctl(rlrep_agent* ag, float* ring_dev, int64_t max_size, int32_t row_floats, int32_t S, int32_t A, const float* s, int64_t ld_s,
                                        const float* a, int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n,
                                        int64_t ring_stride_floats, int32_t* size_dev, int64_t* ctl_dev, void* stream) {
    if (!ag || !ring_dev || !s || !a || !s2 || !r || !d || !ctl_dev) { rl_set_error("group_replay_add_cols_ctl: bad argument (null agent, ring, array or loop record)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || max_size > INT32_MAX || n < 1 || n > max_size || n > RLREP_ACT_MAX_ROWS) {
        rl_set_error("group_replay_add_cols_ctl: n %lld outside [1, min(max_size %lld, %d)]", (long long)n, (long long)max_size, RLREP_ACT_MAX_ROWS); return RLREP_ERR_ARG;
    }
    if (S < 1 || A < 1 || row_floats != 2 * S + A + 2) { rl_set_error("group_replay_add_cols_ctl: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, S, A); return RLREP_ERR_ARG; }
    if (ld_s < S || ld_a < A || ld_s2 < S) { rl_set_error("group_replay_add_cols_ctl: bad argument (a row stride below its width)"); return RLREP_ERR_ARG; }
    if (ring_stride_floats < max_size * row_floats) {
        rl_set_error("group_replay_add_cols_ctl: ring stride %lld below a ring's %lld floats", (long long)ring_stride_floats, (long long)(max_size * row_floats)); return RLREP_ERR_ARG;
    }
    GROUP_ONLY("group_replay_add_cols_ctl")             // (what needs no handle is checked first)
    ReplayCols p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.capacity = max_size; p.ring_stride = ring_stride_floats; p.row = row_floats; p.S = S; p.A = A;
    p.s = s; p.a = a; p.s2 = s2; p.r = r; p.d = d; p.ld_s = ld_s; p.ld_a = ld_a; p.ld_s2 = ld_s2; p.n = n; p.size_dev = size_dev;
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_replay_add_cols_ctl_grp(&p, (long long*)ctl_dev, (hipStream_t)stream);
    if (rc) { rl_set_error("group_replay_add_cols_ctl: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// ---- fused simulators of a seed group (sim_step.hip, the group forms): the state's arrays are [members, n] planes, member r keyed by sim_seeds_dev[r] ----
// what the three entry points refuse alike without looking into the handle, by the entry point's name `who`; the kind's row of rl_env_kinds,
// or null with the error set.  The handle is looked at last (GROUP_ONLY), as in the entry points above.
static const EnvKindInfo* group_sim_check(const char* who, const rlrep_agent* ag, const rlrep_sim_state* s, const uint64_t* seeds) {
    if (!ag || !s || !seeds || !s->x0 || !s->x1 || !s->ep_return || !s->last_return || !s->t || !s->episodes || !s->starts || !s->obs) {
        rl_set_error("%s: bad argument (null agent, simulator state, array or seeds)", who); return nullptr;
    }
    const EnvKindInfo* k = rl_env_kind(s->kind);
    if (!k) { rl_set_error("%s: kind %d is not built (0 = Pendulum-v1, 2 = MountainCarContinuous-v0)", who, s->kind); return nullptr; }
    if (s->n < 1 || s->n > RLREP_SIM_MAX_ENVS) { rl_set_error("%s: n %d outside [1, %d]", who, s->n, RLREP_SIM_MAX_ENVS); return nullptr; }
    return k;
}
int32_t rlrep_group_sim_start(rlrep_agent* ag, const rlrep_sim_state* sim, const uint64_t* sim_seeds_dev, void* stream) {
    if (!group_sim_check("group_sim_start", ag, sim, sim_seeds_dev)) return RLREP_ERR_ARG;
    GROUP_ONLY("group_sim_start")
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_sim_start_grp((const SimState*)sim, (const unsigned long long*)sim_seeds_dev, (hipStream_t)stream);
    if (rc) { rl_set_error("group_sim_start: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_sim_step(rlrep_agent* ag, const rlrep_sim_state* sim, const uint64_t* sim_seeds_dev, const float* act, int64_t ld_act, float* next_obs,
                             float* reward, float* done, void* stream) {
    const EnvKindInfo* k = group_sim_check("group_sim_step", ag, sim, sim_seeds_dev);
    if (!k) return RLREP_ERR_ARG;
    if (!act || !next_obs || !reward || !done) { rl_set_error("group_sim_step: bad argument (null actions or output array)"); return RLREP_ERR_ARG; }
    if (ld_act < k->A) { rl_set_error("group_sim_step: ld_act %lld below the kind's A %d", (long long)ld_act, k->A); return RLREP_ERR_ARG; }
    GROUP_ONLY("group_sim_step")
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_sim_step_grp((const SimState*)sim, (const unsigned long long*)sim_seeds_dev, act, ld_act, next_obs, reward, done, (hipStream_t)stream);
    if (rc) { rl_set_error("group_sim_step: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_sim_step_append_ctl(rlrep_agent* ag, const rlrep_sim_state* sim, const uint64_t* sim_seeds_dev, const float* act, int64_t ld_act,
                                        float* ring_dev, int64_t max_size, int32_t row_floats, int64_t ring_stride_floats, int32_t* size_dev, int64_t* ctl_dev,
                                        void* stream) {
    const EnvKindInfo* k = group_sim_check("group_sim_step_append_ctl", ag, sim, sim_seeds_dev);
    if (!k) return RLREP_ERR_ARG;
    if (!act || !ring_dev || !ctl_dev) { rl_set_error("group_sim_step_append_ctl: bad argument (null actions, ring or loop record)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || max_size > INT32_MAX || sim->n > max_size) {
        rl_set_error("group_sim_step_append_ctl: n %d outside [1, max_size %lld]", sim->n, (long long)max_size); return RLREP_ERR_ARG;
    }
    if (ld_act < k->A) { rl_set_error("group_sim_step_append_ctl: ld_act %lld below the kind's A %d", (long long)ld_act, k->A); return RLREP_ERR_ARG; }
    if (row_floats != k->row) { rl_set_error("group_sim_step_append_ctl: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, k->S, k->A); return RLREP_ERR_ARG; }
    if (ring_stride_floats < max_size * row_floats) {
        rl_set_error("group_sim_step_append_ctl: ring stride %lld below a ring's %lld floats", (long long)ring_stride_floats, (long long)(max_size * row_floats)); return RLREP_ERR_ARG;
    }
    GROUP_ONLY("group_sim_step_append_ctl")
    GrpScope grp_scope_(ag);
    ++g_rl_launches;
    const int rc = rl_launch_sim_step_ctl_grp((const SimState*)sim, (const unsigned long long*)sim_seeds_dev, act, ld_act, ring_dev, ring_stride_floats, max_size,
                                              size_dev, (long long*)ctl_dev, (hipStream_t)stream);
    if (rc) { rl_set_error("group_sim_step_append_ctl: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// ---- prioritized replay of a sac seed group (per_group.hip) ---------------------------------------------------------------------
// trees_dev float32[members, 2P], scal_dev float32[members, 4], idx_dev int32[members, batch], w_dev float32[members, batch]: the buffer group's
static bool per_group_tree_ok(const char* what, const float* trees, int64_t P, const float* scal, int members) {
    if (!per_tree_ok(what, trees, P, scal)) return false;
    if (members < 1 || members > RLREP_GROUP_MAX_MEMBERS) { rl_set_error("%s: members %d outside [1, %d]", what, members, RLREP_GROUP_MAX_MEMBERS); return false; }
    return true;
}
// the entry points that take an agent work for a sac seed group on one GPU, and refuse everything else by name
static int per_group_ok(const char* what, const rlrep_agent* ag) {
    if (!ag) { rl_set_error("%s: null agent", what); return RLREP_ERR_ARG; }
    if (ag->members <= 0) { rl_set_error("%s: not a seed group (a single sac agent takes rlrep_per_* / rlrep_critic_step_weighted)", what); return RLREP_ERR_ARG; }
    if (ag->d.alg != RLREP_ALG_SAC) { rl_set_error("%s: prioritized replay is built for sac seed groups only (a ctrlsac group reuses its last feature minibatch: it takes rlrep_group_per_sample_fill / rlrep_group_critic_weights_arm / rlrep_group_per_update_td)", what); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("%s: prioritized replay runs on one GPU (world_size = %d)", what, ag->h.world_size); return RLREP_ERR_ARG; }
    return 0;
}
int32_t rlrep_group_per_add(float* trees_dev, int64_t P, const float* scal_dev, int32_t members, int64_t capacity, int64_t start, int64_t n, void* stream) {
    if (!per_group_tree_ok("group_per_add", trees_dev, P, scal_dev, members)) return RLREP_ERR_ARG;
    if (capacity < 1 || capacity > P || start < 0 || start >= capacity || n < 1 || n > capacity) {
        rl_set_error("group_per_add: rows [%lld, +%lld) of rings of %lld rows (trees of %lld leaves)", (long long)start, (long long)n, (long long)capacity, (long long)P); return RLREP_ERR_ARG;
    }
    PerAdd p; memset(&p, 0, sizeof(p));
    p.tree = trees_dev; p.scal = scal_dev; p.P = P; p.capacity = capacity; p.start = start; p.n = n;
    const int rc = (++g_rl_launches, rl_launch_per_add_grp(&p, members, (hipStream_t)stream));
    if (rc) { rl_set_error("group_per_add: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_per_sample(rlrep_agent* ag, const float* trees_dev, int64_t P, const float* scal_dev, int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given,
                               uint64_t offset, int32_t use_counter, const float* ring_dev, int64_t ring_stride_bytes, int64_t capacity, void* stream) {
    if (int rc = per_group_ok("group_per_sample", ag)) return rc;
    if (!per_group_tree_ok("group_per_sample", trees_dev, P, scal_dev, ag->members)) return RLREP_ERR_ARG;
    if (!idx_dev || !w_dev || batch < 1) { rl_set_error("group_per_sample: bad argument (null idx / w, or batch %d)", batch); return RLREP_ERR_ARG; }
    PerSample p; memset(&p, 0, sizeof(p));
    p.tree = trees_dev; p.scal = scal_dev; p.idx = idx_dev; p.w = w_dev; p.P = P; p.B = batch; p.given = given ? 1 : 0;
    p.seed = 0; p.offset = offset; p.step_dev = use_counter ? ag->steps : nullptr;          // (member m: its seed, its counter)
    SlotFill f; memset(&f, 0, sizeof(f));
    if (ring_dev) {         // the gather of the drawn rows into every live member's slot 0: a second launch behind the sampler
        if (capacity < 1 || capacity > P || ring_stride_bytes < 0 || (ring_stride_bytes & 3) ||
            (ag->members > 1 && ring_stride_bytes < capacity * 4ll * (2 * ag->d.state_dim + ag->d.action_dim + 2))) {
            rl_set_error("group_per_sample: rings of %lld rows at a stride of %lld bytes (trees of %lld leaves)", (long long)capacity, (long long)ring_stride_bytes, (long long)P);
            return RLREP_ERR_ARG;
        }
        if (batch != ag->B) { rl_set_error("group_per_sample: batch %d is not the batch the step programs are built for (%d): rlrep_group_prepare first", batch, ag->B); return RLREP_ERR_ARG; }
        Slot& s = ag->slot[0];
        f.ring = ring_dev; f.B = ag->B; f.S = ag->d.state_dim; f.A = ag->d.action_dim;
        f.XE = s.XE; f.XF = s.XF; f.XF2 = s.XF2; f.XFpi = s.XFpi; f.R = s.R; f.D = s.D;
        ag->grp_ring_stride = ring_stride_bytes;
        // a new batch: what rlrep_replay_sample invalidates
        ag->pf_done = false; ag->pi_ready = nullptr; ag->hoist_req = nullptr;
        s.filled = true;
    }
    GrpScope grp_scope_(ag);
    int rc = (++g_rl_launches, rl_launch_per_sample_grp(&p, (hipStream_t)stream));
    if (rc == 0 && ring_dev) rc = (++g_rl_launches, rl_launch_per_gather_grp(&f, idx_dev, capacity, (hipStream_t)stream));
    if (rc) { rl_set_error("group_per_sample: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_per_update(rlrep_agent* ag, float* trees_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch, void* stream) {
    if (int rc = per_group_ok("group_per_update", ag)) return rc;
    if (!per_group_tree_ok("group_per_update", trees_dev, P, scal_dev, ag->members)) return RLREP_ERR_ARG;
    if (!idx_dev || batch < 1 || (!td_dev && batch != ag->B)) { rl_set_error("group_per_update: bad argument (null idx, or batch %d is not the batch of the last weighted critic step)", batch); return RLREP_ERR_ARG; }
    PerUpdate p; memset(&p, 0, sizeof(p));
    p.tree = trees_dev; p.scal = scal_dev; p.idx = idx_dev; p.td = td_dev ? td_dev : ag->per_td; p.P = P; p.B = batch;
    if (!p.td) { rl_set_error("group_per_update: no weighted critic step has run"); return RLREP_ERR_STATE; }
    GrpScope grp_scope_(ag);
    // td_dev given: float32[members, batch]; otherwise every member's |TD| buffer in its workspace
    const int rc = (++g_rl_launches, rl_launch_per_update_grp(&p, td_dev ? (long long)batch : -1ll, (hipStream_t)stream));
    if (rc) { rl_set_error("group_per_update: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
const float* rlrep_group_per_td_dev(rlrep_agent* ag) { return (ag && ag->members > 0 && ag->d.alg == RLREP_ALG_SAC) ? ag->per_td : nullptr; }
// rlrep_critic_step of every live member with per-sample weights w_dev[members, B]; leaves every member's |TD| in its workspace
int32_t rlrep_group_critic_step_weighted(rlrep_agent* ag, const float* eps, const float* w_dev, void* stream) {
    if (int rc = per_group_ok("group_critic_step_weighted", ag)) return rc;
    if (!eps || !w_dev) { rl_set_error("group_critic_step_weighted: needs eps[B,A] (member 0's) and w[members,B]"); return RLREP_ERR_ARG; }
    if (ag->critic_bwd_w.stages.empty()) { rl_set_error("group_critic_step_weighted: no weighted critic program was built for this group"); return RLREP_ERR_STATE; }
    const int rc = critic_backward_dispatch(ag, eps, w_dev, stream);
    return rc ? rc : rlrep_critic_apply(ag, stream);
}

// ---- prioritized replay of the critic's minibatch for a ctrlsac seed group (per_group.hip) --------------------------------
// the three entry points work for a ctrlsac seed group on one GPU, and refuse everything else by name
static int cper_group_ok(const char* what, const rlrep_agent* ag) {
    if (!ag) { rl_set_error("%s: null agent", what); return RLREP_ERR_ARG; }
    if (ag->members <= 0) { rl_set_error("%s: not a seed group (a single agent takes rlrep_per_sample_fill / rlrep_critic_weights_arm / rlrep_per_update_td)", what); return RLREP_ERR_ARG; }
    if (ag->d.alg == RLREP_ALG_SAC) {
        rl_set_error("%s: a sac seed group owns its whole minibatch: use rlrep_group_per_sample / rlrep_group_critic_step_weighted / rlrep_group_per_update", what);
        return RLREP_ERR_ARG;
    }
    if (ag->h.world_size > 1) { rl_set_error("%s: prioritized critic replay runs on one GPU (world_size = %d)", what, ag->h.world_size); return RLREP_ERR_ARG; }
    return 0;
}
static bool cper_group_batch_ok(const char* what, const rlrep_agent* ag, int32_t batch) {
    if (batch < 1 || batch != ag->B) {
        rl_set_error("%s: batch %d is not the batch the step programs are built for (%d): rlrep_group_prepare first", what, batch, ag->B); return false;
    }
    return true;
}
// rlrep_per_sample_fill of every live member in ONE launch.  Never skipped: it overwrites whatever gather the train prologue ran.
int32_t rlrep_group_per_sample_fill(rlrep_agent* ag, const float* rings_dev, int64_t ring_stride_bytes, int64_t capacity, const float* trees_dev, int64_t P,
                                    const float* scal_dev, int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given, uint64_t offset, int32_t use_counter,
                                    void* stream) {
    const char* what = "group_per_sample_fill";
    if (int rc = cper_group_ok(what, ag)) return rc;
    if (!per_group_tree_ok(what, trees_dev, P, scal_dev, ag->members)) return RLREP_ERR_ARG;
    if (!rings_dev || !idx_dev || !w_dev) { rl_set_error("%s: bad argument (null rings / idx / w)", what); return RLREP_ERR_ARG; }
    if (capacity < 1 || capacity > P) { rl_set_error("%s: rings of %lld rows under trees of %lld leaves", what, (long long)capacity, (long long)P); return RLREP_ERR_ARG; }
    if (ring_stride_bytes < 0 || (ring_stride_bytes & 3) ||
        (ag->members > 1 && ring_stride_bytes < capacity * 4ll * (2 * ag->d.state_dim + ag->d.action_dim + 2))) {
        rl_set_error("%s: rings of %lld rows at a stride of %lld bytes", what, (long long)capacity, (long long)ring_stride_bytes); return RLREP_ERR_ARG;
    }
    if (!cper_group_batch_ok(what, ag, batch)) return RLREP_ERR_ARG;
    Slot& s = ag->slot[0];
    PerSampleFill p; memset(&p, 0, sizeof(p));
    p.s.tree = trees_dev; p.s.scal = scal_dev; p.s.idx = idx_dev; p.s.w = w_dev; p.s.P = P; p.s.B = batch; p.s.given = given ? 1 : 0;
    p.s.seed = 0; p.s.offset = offset; p.s.step_dev = use_counter ? ag->steps : nullptr;          // (member m: its seed, its counter)
    p.f.ring = rings_dev; p.f.B = ag->B; p.f.S = ag->d.state_dim; p.f.A = ag->d.action_dim;
    p.f.XE = s.XE; p.f.XF = s.XF; p.f.XF2 = s.XF2; p.f.XFpi = s.XFpi; p.f.R = s.R; p.f.D = s.D;
    p.capacity = capacity;
    ag->grp_ring_stride = ring_stride_bytes;
    // a new batch: what rlrep_replay_sample invalidates
    ag->pf_done = false; ag->pi_ready = nullptr; ag->hoist_req = nullptr;
    s.filled = true;
    GrpScope grp_scope_(ag);
    const int rc = (++g_rl_launches, rl_launch_per_sample_fill_grp(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("%s: hip error %d", what, rc); return RLREP_ERR_HIP; }
    return 0;
}
// The next rlrep_critic_step / rlrep_critic_backward of the group is the weighted one: w[members, B] in the members' losses, their |TD| into the
// caller's td[members, B] (critic_head_launch picks the group head of per_group.hip).  That step disarms (critic_backward_dispatch); so
// does passing null.
int32_t rlrep_group_critic_weights_arm(rlrep_agent* ag, const float* w_dev, float* td_dev) {
    if (int rc = cper_group_ok("group_critic_weights_arm", ag)) return rc;
    if ((w_dev == nullptr) != (td_dev == nullptr)) { rl_set_error("group_critic_weights_arm: needs w[members,B] and td[members,B] (or neither, to disarm)"); return RLREP_ERR_ARG; }
    ag->arm_w = w_dev; ag->arm_td = td_dev;
    return w_dev ? 1 : 0;
}
// rlrep_per_update_td of every live member: per_update_grp_kernel with the caller's |TD| array, `batch` floats per member
int32_t rlrep_group_per_update_td(rlrep_agent* ag, float* trees_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch,
                                  void* stream) {
    const char* what = "group_per_update_td";
    if (int rc = cper_group_ok(what, ag)) return rc;
    if (!per_group_tree_ok(what, trees_dev, P, scal_dev, ag->members)) return RLREP_ERR_ARG;
    if (!idx_dev || !td_dev) { rl_set_error("%s: bad argument (null idx / td)", what); return RLREP_ERR_ARG; }
    if (!cper_group_batch_ok(what, ag, batch)) return RLREP_ERR_ARG;
    PerUpdate p; memset(&p, 0, sizeof(p));
    p.tree = trees_dev; p.scal = scal_dev; p.idx = idx_dev; p.td = td_dev; p.P = P; p.B = batch;
    GrpScope grp_scope_(ag);
    const int rc = (++g_rl_launches, rl_launch_per_update_grp(&p, (long long)batch, (hipStream_t)stream));
    if (rc) { rl_set_error("%s: hip error %d", what, rc); return RLREP_ERR_HIP; }
    return 0;
}

// ---- n-step returns of a sac seed group (nstep.hip) ------------------------------------------------------------------------------
// The chain-following gather of every live member into its slot 0, one launch on grid (x, members): member m's ring, fill level size_dev[m]
// and discount (its hyper record, read on the device).  idx_per_member == 0: idx_dev lies in member 0's block (the index pool the group train
// prologue wrote) and moves by the member stride; otherwise idx_dev is int32[members, batch] (a prioritized buffer group's draw buffers).
int32_t rlrep_group_replay_gather_nstep(rlrep_agent* ag, const float* rings_dev, int64_t ring_stride_bytes, const int32_t* idx_dev, int32_t idx_per_member,
                                        int32_t batch, int64_t max_size, const int32_t* size_dev, int32_t n, int32_t stride, void* stream) {
    const char* what = "group_replay_gather_nstep";
    if (!ag) { rl_set_error("%s: null agent", what); return RLREP_ERR_ARG; }
    if (ag->members <= 0) { rl_set_error("%s: not a seed group (a single sac agent takes rlrep_replay_sample_nstep)", what); return RLREP_ERR_ARG; }
    if (ag->d.alg != RLREP_ALG_SAC) { rl_set_error("%s: n-step replay is built for sac seed groups only (a ctrlsac group's feature step models one-step dynamics)", what); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("%s: n-step replay runs on one GPU (world_size = %d)", what, ag->h.world_size); return RLREP_ERR_ARG; }
    if (!rings_dev || !idx_dev || !size_dev || batch < 1) { rl_set_error("%s: bad argument (null rings / idx / size_dev, or batch %d)", what, batch); return RLREP_ERR_ARG; }
    if (max_size < 1 || max_size > 0x7fffffffll || ring_stride_bytes < 0 || (ring_stride_bytes & 3) ||
        (ag->members > 1 && ring_stride_bytes < max_size * 4ll * (2 * ag->d.state_dim + ag->d.action_dim + 2))) {
        rl_set_error("%s: rings of %lld rows at a stride of %lld bytes", what, (long long)max_size, (long long)ring_stride_bytes); return RLREP_ERR_ARG;
    }
    if (n < 1 || n > RLREP_NSTEP_MAX) { rl_set_error("%s: n %d outside [1, %d]", what, n, RLREP_NSTEP_MAX); return RLREP_ERR_ARG; }
    if (stride < 1) { rl_set_error("%s: stride %d (the number of interleaved environments) must be >= 1", what, stride); return RLREP_ERR_ARG; }
    if (!idx_per_member && !in_member0(ag, idx_dev, 4ll * batch)) { rl_set_error("%s: indices that move by the member stride must lie inside member 0's block", what); return RLREP_ERR_ARG; }
    if (batch != ag->B) { rl_set_error("%s: batch %d is not the batch the step programs are built for (%d): rlrep_group_prepare first", what, batch, ag->B); return RLREP_ERR_ARG; }
    Slot& s = ag->slot[0];
    NStepGather p; memset(&p, 0, sizeof(p));
    p.fill.ring = rings_dev; p.fill.idx = idx_dev; p.fill.B = ag->B; p.fill.S = ag->d.state_dim; p.fill.A = ag->d.action_dim;
    p.fill.XE = s.XE; p.fill.XF = s.XF; p.fill.XF2 = s.XF2; p.fill.XFpi = s.XFpi; p.fill.R = s.R; p.fill.D = s.D;
    p.size_dev = size_dev; p.capacity = max_size; p.n = n; p.stride = stride; p.gamma = ag->h.discount;      // (the kernel takes every member's own)
    ag->grp_ring_stride = ring_stride_bytes;
    // a new batch: what rlrep_replay_sample invalidates
    ag->pf_done = false; ag->l1_done = false; ag->chain_next = false; ag->pi_ready = nullptr; ag->hoist_req = nullptr;
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    s.filled = true;
    GrpScope grp_scope_(ag);
    const int rc = (++g_rl_launches, rl_launch_nstep_gather_grp(&p, idx_per_member ? batch : 0, (hipStream_t)stream));
    if (rc) { rl_set_error("%s: hip error %d", what, rc); return RLREP_ERR_HIP; }
    return 0;
}

// ---- device environments of a seed group (group_env.hip) --------------------------------------------------------------------------------------
static_assert(EnvPendulum::KIND == RLREP_ENV_PENDULUM && EnvMountainCar::KIND == RLREP_ENV_MOUNTAIN_CAR_CONTINUOUS, "group_env.h kinds are include/rlrep.h RLREP_ENV_*");
struct rlrep_group_env {
    rlrep_agent* ag; int kind, members, num_envs;
    EnvRecord* recs; EnvCtl* ctl;                     // [members][num_envs] records and the group's counters: allocations of their own
    double* starts;                                   // [members, RL_ENV_MAX_EPISODES, 2] start states of the last evaluation
    int last_episodes;
};
// what every entry point that launches checks first: `what` names the caller in the message
static int group_env_check(const char* what, rlrep_agent* ag, rlrep_group_env* env) {
    if (!ag || !env) { rl_set_error("%s: null agent or environment", what); return RLREP_ERR_ARG; }
    if (ag->members <= 0) { rl_set_error("%s: not a seed group (device environments are built for rlrep_group_create agents)", what); return RLREP_ERR_ARG; }
    if (env->ag != ag || env->members != ag->members) { rl_set_error("%s: the environment was created for another group", what); return RLREP_ERR_ARG; }
    if (in_train_refused(what, ag)) return RLREP_ERR_ARG;
    return 0;
}
// rlrep_group_env_create (`what` = "group_env_create", num_envs = 1) and rlrep_group_env_create_n: one code, the message names the caller
static int32_t group_env_create(const char* what, rlrep_agent* ag, int32_t kind, int32_t num_envs, rlrep_group_env** out) {
    const EnvKindInfo* k = rl_env_kind(kind);
    if (!k) { rl_set_error("%s: kind %d is not built (0 = Pendulum-v1, 2 = MountainCarContinuous-v0)", what, kind); return RLREP_ERR_ARG; }
    if (num_envs < 1 || num_envs > RL_ENV_MAX_ENVS) { rl_set_error("%s: num_envs %d outside [1, %d]", what, num_envs, RL_ENV_MAX_ENVS); return RLREP_ERR_ARG; }
    if (!ag || !out) { rl_set_error("%s: null argument", what); return RLREP_ERR_ARG; }
    if (ag->members <= 0) { rl_set_error("%s: not a seed group (device environments are built for rlrep_group_create agents)", what); return RLREP_ERR_ARG; }
    if (ag->d.state_dim != k->S || ag->d.action_dim != k->A) {
        rl_set_error("%s: %s has %d observations and %d action (the group has %d and %d)", what, k->name, k->S, k->A, ag->d.state_dim, ag->d.action_dim); return RLREP_ERR_ARG;
    }
    rlrep_group_env* env = new rlrep_group_env();
    env->ag = ag; env->kind = kind; env->members = ag->members; env->num_envs = num_envs; env->last_episodes = 0;
    env->recs = nullptr; env->ctl = nullptr; env->starts = nullptr;
    const size_t rec_bytes = sizeof(EnvRecord) * (size_t)env->members * (size_t)num_envs;
    hipError_t e = hipMalloc((void**)&env->recs, rec_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&env->ctl, sizeof(EnvCtl));
    if (e == hipSuccess) e = hipMalloc((void**)&env->starts, sizeof(double) * 2 * RL_ENV_MAX_EPISODES * env->members);
    if (e == hipSuccess) e = hipMemset(env->recs, 0, rec_bytes);
    if (e == hipSuccess) e = hipMemset(env->ctl, 0, sizeof(EnvCtl));
    if (e == hipSuccess) e = hipMemset(env->starts, 0, sizeof(double) * 2 * RL_ENV_MAX_EPISODES * env->members);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { rl_set_error("%s: %s", what, hipGetErrorString(e)); rlrep_group_env_destroy(env); return RLREP_ERR_HIP; }
    *out = env;
    return 0;
}
int32_t rlrep_group_env_create(rlrep_agent* ag, int32_t kind, rlrep_group_env** out) { return group_env_create("group_env_create", ag, kind, 1, out); }
int32_t rlrep_group_env_create_n(rlrep_agent* ag, int32_t kind, int32_t num_envs, rlrep_group_env** out) {
    return group_env_create("group_env_create_n", ag, kind, num_envs, out);
}
int32_t rlrep_group_env_num_envs(rlrep_group_env* env) { return env ? env->num_envs : 0; }
void rlrep_group_env_destroy(rlrep_group_env* env) {
    if (!env) return;
    if (env->recs) (void)hipFree(env->recs);
    if (env->ctl) (void)hipFree(env->ctl);
    if (env->starts) (void)hipFree(env->starts);
    delete env;
}
int32_t rlrep_group_env_reset(rlrep_group_env* env, void* stream) {
    if (const int rc = group_env_check("group_env_reset", env ? env->ag : nullptr, env)) return rc;
    ++g_rl_launches;
    const int rc = rl_launch_group_env_reset(env->kind, env->recs, env->ctl, env->ag->grp_seeds, env->members, env->num_envs, (hipStream_t)stream);
    if (rc) { rl_set_error("group_env_reset: launch failed (%d)", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_env_step(rlrep_agent* ag, rlrep_group_env* env, float* ring_dev, int64_t ring_stride_floats, int64_t capacity, int32_t* size_dev,
                             float lo, float hi, float eps_greedy, int64_t start_timesteps, void* stream) {
    if (const int rc = group_env_check("group_env_step", ag, env)) return rc;
    if (!ring_dev || !size_dev) { rl_set_error("group_env_step: null ring or size pointer"); return RLREP_ERR_ARG; }
    const int row = 2 * ag->d.state_dim + ag->d.action_dim + 2;
    if (capacity < env->num_envs) { rl_set_error("group_env_step: capacity %lld is below the %d rows of one step (num_envs)", (long long)capacity, env->num_envs); return RLREP_ERR_ARG; }
    if (capacity < 1 || ring_stride_floats < capacity * row) {
        rl_set_error("group_env_step: capacity %lld / ring stride %lld floats do not hold %lld rows of %d floats", (long long)capacity, (long long)ring_stride_floats, (long long)capacity, row);
        return RLREP_ERR_ARG;
    }
    if (!(lo <= hi) || !(eps_greedy >= 0.f && eps_greedy <= 1.f)) { rl_set_error("group_env_step: bad action range [%g, %g] or eps_greedy %g", (double)lo, (double)hi, (double)eps_greedy); return RLREP_ERR_ARG; }
    SelectAct p; group_actor(ag, p, lo, hi);
    ++g_rl_launches;
    const int rc = rl_launch_group_env_step(env->kind, &p, ag->grp_stride, ag->grp_seeds, ag->grp_live, ag->grp_grid_y, env->num_envs, env->recs, env->ctl, ring_dev, ring_stride_floats, capacity,
                                            size_dev, eps_greedy, start_timesteps, (hipStream_t)stream);
    if (rc) { rl_set_error("group_env_step: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_env_evaluate(rlrep_agent* ag, rlrep_group_env* env, int32_t episodes, uint64_t eval_index, double* out_dev, void* stream) {
    if (const int rc = group_env_check("group_env_evaluate", ag, env)) return rc;
    if (episodes < 1 || episodes > RL_ENV_MAX_EPISODES) { rl_set_error("group_env_evaluate: episodes %d outside [1, %d]", episodes, RL_ENV_MAX_EPISODES); return RLREP_ERR_ARG; }
    if (!out_dev) { rl_set_error("group_env_evaluate: null output"); return RLREP_ERR_ARG; }
    const EnvKindInfo* k = rl_env_kind(env->kind);
    SelectAct p; group_actor(ag, p, k->lo, k->hi);       // the environment's own action range (Pendulum-v1: its max_torque)
    ++g_rl_launches;
    const int rc = rl_launch_group_env_eval(env->kind, &p, ag->grp_stride, ag->grp_seeds, ag->grp_live, ag->grp_grid_y, eval_index * (uint64_t)episodes, episodes, out_dev,
                                            env->starts, (hipStream_t)stream);
    if (rc) { rl_set_error("group_env_evaluate: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    env->last_episodes = episodes;
    return 0;
}
// rlrep_group_env_state / rlrep_env_state: copy one block of an environment of `n` agents with `num_envs` records each to or from the host;
// `what_fn` names the caller
static int32_t env_state_copy(const char* what_fn, rlrep_agent* ag, EnvRecord* recs, int n, int num_envs, EnvCtl* ctl, double* starts, int last_episodes, int32_t what,
                              void* host, int64_t bytes, int32_t write, void* stream) {
    void* dev = nullptr; int64_t have = 0;
    if (what == RLREP_ENV_STATE_RECORDS) { dev = recs; have = (int64_t)sizeof(EnvRecord) * n * num_envs; }
    else if (what == RLREP_ENV_STATE_COUNTERS) { dev = ctl; have = 16; }
    else if (what == RLREP_ENV_STATE_EVAL_STARTS && !write) { dev = starts; have = (int64_t)sizeof(double) * 2 * last_episodes * n; }
    else { rl_set_error("%s: what = %d (write %d) is not a block of the environment", what_fn, what, write); return RLREP_ERR_ARG; }
    if (bytes != have) { rl_set_error("%s: block %d holds %lld bytes, the buffer %lld", what_fn, what, (long long)have, (long long)bytes); return RLREP_ERR_ARG; }
    if (in_train_refused(what_fn, ag)) return RLREP_ERR_ARG;
    hipError_t e = hipSuccess;
    if (bytes > 0) e = write ? hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream)
                             : hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { rl_set_error("%s: %s", what_fn, hipGetErrorString(e)); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_group_env_state(rlrep_group_env* env, int32_t what, void* host, int64_t bytes, int32_t write, void* stream) {
    if (!env || !host) { rl_set_error("group_env_state: null argument"); return RLREP_ERR_ARG; }
    return env_state_copy("group_env_state", env->ag, env->recs, env->members, env->num_envs, env->ctl, env->starts, env->last_episodes, what, host, bytes, write, stream);
}

// ---- the device environment of a SINGLE agent (group_env.hip env_*_kernel): any of the five algorithms, they carry the same actor trunk --------
struct rlrep_env {
    rlrep_agent* ag; int kind, num_envs; uint64_t seed;
    EnvRecord* rec; EnvCtl* ctl;                      // [num_envs] records and their counters: allocations of their own
    double* starts;                                   // [RL_ENV_MAX_EPISODES, 2] start states of the last evaluation
    int last_episodes;
};
static int env_check(const char* what, rlrep_agent* ag, rlrep_env* env) {
    if (!ag || !env) { rl_set_error("%s: null agent or environment", what); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("%s: a seed group takes rlrep_group_env_*", what); return RLREP_ERR_ARG; }
    if (env->ag != ag) { rl_set_error("%s: the environment was created for another agent", what); return RLREP_ERR_ARG; }
    if (in_train_refused(what, ag)) return RLREP_ERR_ARG;
    return 0;
}
static int32_t env_create(const char* what, rlrep_agent* ag, int32_t kind, uint64_t seed, int32_t num_envs, rlrep_env** out) {
    const EnvKindInfo* k = rl_env_kind(kind);
    if (!k) { rl_set_error("%s: kind %d is not built (0 = Pendulum-v1, 2 = MountainCarContinuous-v0)", what, kind); return RLREP_ERR_ARG; }
    if (num_envs < 1 || num_envs > RL_ENV_MAX_ENVS) { rl_set_error("%s: num_envs %d outside [1, %d]", what, num_envs, RL_ENV_MAX_ENVS); return RLREP_ERR_ARG; }
    if (!ag || !out) { rl_set_error("%s: null argument", what); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("%s: a seed group of %d members takes rlrep_group_env_create", what, ag->members); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1 || ag->dp_proto.world > 1) {
        rl_set_error("%s: a data-parallel agent (world_size %d) has no device environment", what, std::max(ag->h.world_size, ag->dp_proto.world)); return RLREP_ERR_ARG;
    }
    if (ag->d.state_dim != k->S || ag->d.action_dim != k->A) {
        rl_set_error("%s: %s has %d observations and %d action (the agent has %d and %d)", what, k->name, k->S, k->A, ag->d.state_dim, ag->d.action_dim); return RLREP_ERR_ARG;
    }
    rlrep_env* env = new rlrep_env();
    env->ag = ag; env->kind = kind; env->num_envs = num_envs; env->seed = seed; env->last_episodes = 0; env->rec = nullptr; env->ctl = nullptr; env->starts = nullptr;
    hipError_t e = hipMalloc((void**)&env->rec, sizeof(EnvRecord) * (size_t)num_envs);
    if (e == hipSuccess) e = hipMalloc((void**)&env->ctl, sizeof(EnvCtl));
    if (e == hipSuccess) e = hipMalloc((void**)&env->starts, sizeof(double) * 2 * RL_ENV_MAX_EPISODES);
    if (e == hipSuccess) e = hipMemset(env->rec, 0, sizeof(EnvRecord) * (size_t)num_envs);
    if (e == hipSuccess) e = hipMemset(env->ctl, 0, sizeof(EnvCtl));
    if (e == hipSuccess) e = hipMemset(env->starts, 0, sizeof(double) * 2 * RL_ENV_MAX_EPISODES);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { rl_set_error("%s: %s", what, hipGetErrorString(e)); rlrep_env_destroy(env); return RLREP_ERR_HIP; }
    *out = env;
    return 0;
}
int32_t rlrep_env_create(rlrep_agent* ag, int32_t kind, uint64_t seed, rlrep_env** out) { return env_create("env_create", ag, kind, seed, 1, out); }
int32_t rlrep_env_create_n(rlrep_agent* ag, int32_t kind, uint64_t seed, int32_t num_envs, rlrep_env** out) {
    return env_create("env_create_n", ag, kind, seed, num_envs, out);
}
int32_t rlrep_env_num_envs(rlrep_env* env) { return env ? env->num_envs : 0; }
void rlrep_env_destroy(rlrep_env* env) {
    if (!env) return;
    if (env->rec) (void)hipFree(env->rec);
    if (env->ctl) (void)hipFree(env->ctl);
    if (env->starts) (void)hipFree(env->starts);
    delete env;
}
int32_t rlrep_env_reset(rlrep_env* env, void* stream) {
    if (const int rc = env_check("env_reset", env ? env->ag : nullptr, env)) return rc;
    ++g_rl_launches;
    const int rc = rl_launch_env_reset(env->kind, env->rec, env->ctl, env->seed, env->num_envs, (hipStream_t)stream);
    if (rc) { rl_set_error("env_reset: launch failed (%d)", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_env_step(rlrep_agent* ag, rlrep_env* env, float* ring_dev, int64_t capacity, int32_t* size_dev, float lo, float hi, float eps_greedy,
                       int64_t start_timesteps, void* stream) {
    if (const int rc = env_check("env_step", ag, env)) return rc;
    if (!ring_dev || !size_dev) { rl_set_error("env_step: null ring or size pointer"); return RLREP_ERR_ARG; }
    if (capacity < 1) { rl_set_error("env_step: capacity %lld is below one row", (long long)capacity); return RLREP_ERR_ARG; }
    if (capacity < env->num_envs) { rl_set_error("env_step: capacity %lld is below the %d rows of one step (num_envs)", (long long)capacity, env->num_envs); return RLREP_ERR_ARG; }
    if (!(lo <= hi) || !(eps_greedy >= 0.f && eps_greedy <= 1.f)) { rl_set_error("env_step: bad action range [%g, %g] or eps_greedy %g", (double)lo, (double)hi, (double)eps_greedy); return RLREP_ERR_ARG; }
    SelectAct p; group_actor(ag, p, lo, hi);
    p.seed = env->seed;
    ++g_rl_launches;
    const int rc = rl_launch_env_step(env->kind, &p, env->num_envs, env->rec, env->ctl, ring_dev, capacity, size_dev, eps_greedy, start_timesteps, (hipStream_t)stream);
    if (rc) { rl_set_error("env_step: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_env_evaluate(rlrep_agent* ag, rlrep_env* env, int32_t episodes, uint64_t eval_index, double* out_dev, void* stream) {
    if (const int rc = env_check("env_evaluate", ag, env)) return rc;
    if (episodes < 1 || episodes > RL_ENV_MAX_EPISODES) { rl_set_error("env_evaluate: episodes %d outside [1, %d]", episodes, RL_ENV_MAX_EPISODES); return RLREP_ERR_ARG; }
    if (!out_dev) { rl_set_error("env_evaluate: null output"); return RLREP_ERR_ARG; }
    const EnvKindInfo* k = rl_env_kind(env->kind);
    SelectAct p; group_actor(ag, p, k->lo, k->hi);       // the environment's own action range
    p.seed = env->seed;
    ++g_rl_launches;
    const int rc = rl_launch_env_eval(env->kind, &p, eval_index * (uint64_t)episodes, episodes, out_dev, env->starts, (hipStream_t)stream);
    if (rc) { rl_set_error("env_evaluate: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    env->last_episodes = episodes;
    return 0;
}
int32_t rlrep_env_state(rlrep_env* env, int32_t what, void* host, int64_t bytes, int32_t write, void* stream) {
    if (!env || !host) { rl_set_error("env_state: null argument"); return RLREP_ERR_ARG; }
    return env_state_copy("env_state", env->ag, env->rec, 1, env->num_envs, env->ctl, env->starts, env->last_episodes, what, host, bytes, write, stream);
}
// size a single agent's step programs for `batch` outside a capture (rlrep_group_prepare's twin): SACAgent.iterate captures its graph while
// the DEVICE owns the ring cursor, where the eager gather a train() capture sizes them with would sample by a stale host fill level
int32_t rlrep_prepare(rlrep_agent* ag, int32_t batch) {
    GROUP_REFUSE("prepare")
    if (!ag) { rl_set_error("prepare: null agent"); return RLREP_ERR_ARG; }
    return ensure_batch(ag, batch);
}

}  // extern "C"
