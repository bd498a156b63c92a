// librlrep_hip.so host side: error and switch state, tensor layouts, (re)building an agent's step programs, the C ABI of single agents
// (include/rlrep.h) with its diagnostics, the data-parallel attach.  The step programs themselves: agents1.hip (sac, vlsac), agents2.hip (ctrlsac,
// spedersac, diffsrsac); the seed-group ABI: group_api.hip.
//
// A step program is a short, fixed list of kernel launches (stages).  Each stage executes a TABLE of
// independent tasks (grouped GEMMs, see gemm16.hip), so the number of dependent launches equals the depth
// of the agent's computation graph.  Tables live in the caller-provided workspace and are uploaded when
// the batch size changes; the hot path performs no allocation, no host<->device copy and no sync.
#include "engine_internal.h"
#include <cstdarg>
#include <cmath>
#include <cstddef>
#include <memory>

static thread_local char g_err[512] = "";
long long g_rl_launches = 0;
void rl_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}

// ---- diagnostic switches (common.h: rl_off / rl_opt) ---------------------------------------------------------------------------------
// TWO environment variables, comma-separated tokens, parsed when the library is entered through rlrep_layout / rlrep_agent_create / rlrep_gemm*
// (never on a launch path): RLREP_DISABLE lists default mechanisms to switch off (every one of them has an equivalence test that compares the two
// forms), RLREP_ENABLE lists opt-in ones, optionally with a value (token=value).  INTEGRATION.md has the table.
// the group of the library call in progress (group.h): launchers issue their group forms while it is set
static thread_local RlGrp g_grp;
static thread_local bool g_grp_on = false;
extern "C" const RlGrp* rl_grp_active() { return g_grp_on ? &g_grp : nullptr; }
GrpScope::GrpScope(const rlrep_agent* ag) {
    if (!ag || ag->members <= 0) return;
    prev = g_grp; prev_on = g_grp_on;          // (nesting-safe: the enclosing call's group comes back on exit)
    g_grp.members = ag->members; g_grp.stride = ag->grp_stride; g_grp.ring_stride = ag->grp_ring_stride; g_grp.seeds = ag->grp_seeds; g_grp.hyp = ag->mhyp; g_grp.live = ag->grp_live; g_grp.grid_y = ag->grp_grid_y;
    g_grp_on = set = true;
}
GrpScope::~GrpScope() { if (set) { g_grp = prev; g_grp_on = prev_on; } }
static std::map<std::string, std::string> g_sw_off, g_sw_on;
static void sw_parse(const char* env, std::map<std::string, std::string>& m) {
    m.clear();
    const char* e = getenv(env);
    if (!e) return;
    std::string s(e), tok;
    s.push_back(',');
    for (char ch : s) {
        if (ch == ',' || ch == ' ' || ch == ';') {
            if (!tok.empty()) {
                const size_t eq = tok.find('=');
                if (eq == std::string::npos) m[tok] = "1"; else m[tok.substr(0, eq)] = tok.substr(eq + 1);
                tok.clear();
            }
        } else tok.push_back(ch);
    }
}
void rl_switches_read() { sw_parse("RLREP_DISABLE", g_sw_off); sw_parse("RLREP_ENABLE", g_sw_on); rl_gemm16_read_env(); }
bool rl_off(const char* token) { return g_sw_off.count(token) != 0; }
const char* rl_opt(const char* token) { auto it = g_sw_on.find(token); return it == g_sw_on.end() ? nullptr : it->second.c_str(); }

// ================================================================================================
// layout (names = reference state_dict keys; see oracle/shapes.py for the reference order)
// ================================================================================================
void lay_actor(Layout& L, int S, int A, int Ha, int arena, int group) {
    L.lin("actor.trunk.0", Ha, S, arena, group);          // agent/sac/actor.py:63-74
    L.lin("actor.trunk.2", Ha, Ha, arena, group);
    L.lin("actor.trunk.4", 2 * A, Ha, arena, group);
}
static void lay_doubleq(Layout& L, const std::string& m, int SA, int H, int arena, int group) {
    // agent/sac/critic.py:15-36; the two heads' first layers are stored as one [2H, S+A] matrix
    L.lin_pair(m + ".Q1.0", H, m + ".Q2.0", H, SA, arena, group);
    L.lin(m + ".Q1.2", H, H, arena, group);
    L.lin(m + ".Q2.2", H, H, arena, group);
    L.lin(m + ".Q1.4", 1, H, arena, group);
    L.lin(m + ".Q2.4", 1, H, arena, group);
}
void lay_six(Layout& L, const std::string& m, int in_f, int H, int arena, int group) {
    // l1..l6 critics (vlsac_agent.py:33-41, spedersac_agent.py:26-34, diffsrsac_agent.py:51-59); l1|l4 glued
    L.lin_pair(m + ".l1", H, m + ".l4", H, in_f, arena, group);
    L.lin(m + ".l2", H, H, arena, group);
    L.lin(m + ".l5", H, H, arena, group);
    L.lin(m + ".l3", 1, H, arena, group);
    L.lin(m + ".l6", 1, H, arena, group);
}
static void lay_gauss(Layout& L, const std::string& m, int in_f, int Hv, int F, int arena, int group) {
    // networks/vae.py:28-35 / 104-109; mean|log_std heads glued into one [2F, Hv] matrix
    L.lin(m + ".l1", Hv, in_f, arena, group);
    L.lin(m + ".l2", Hv, Hv, arena, group);
    L.lin_pair(m + ".mean_linear", F, m + ".log_std_linear", F, Hv, arena, group);
}

bool build_layout(const rlrep_dims& d, Layout& L) {
    const int S = d.state_dim, A = d.action_dim, H = d.hidden_dim, Ha = d.actor_hidden_dim, F = d.feature_dim;
    const int P = RLREP_ARENA_PARAM, T = RLREP_ARENA_TARGET;
    switch (d.alg) {
    case RLREP_ALG_SAC:
        L.begin_group(1); lay_doubleq(L, "critic", S + A, H, P, 1); L.end_group(1);
        L.begin_group(2); lay_actor(L, S, A, Ha, P, 2); L.end_group(2);
        lay_doubleq(L, "critic_target", S + A, H, T, -1);
        return true;
    case RLREP_ALG_VLSAC: {
        const int Hv = d.vae_hidden_dim;
        L.begin_group(0);
        lay_gauss(L, "encoder", 2 * S + A, Hv, F, P, 0);
        L.lin("decoder.l1", Hv, F, P, 0);                                   // networks/vae.py:74-77
        L.lin_pair("decoder.state_linear", S, "decoder.reward_linear", 1, Hv, P, 0);
        lay_gauss(L, "f", S + A, Hv, F, P, 0);
        L.end_group(0);
        L.begin_group(1); lay_six(L, "critic", F, H, P, 1); L.end_group(1);
        L.begin_group(2); lay_actor(L, S, A, Ha, P, 2); L.end_group(2);
        lay_gauss(L, "f_target", S + A, Hv, F, T, -1);
        lay_six(L, "critic_target", F, H, T, -1);
        L.add("critic.noise", d.num_noise, F, T, -1);                      // quirk Q3: plain attribute
        return true;
    }
    case RLREP_ALG_CTRLSAC: lay_ctrlsac(d, L); return true;
    case RLREP_ALG_SPEDERSAC: lay_spedersac(d, L); return true;
    case RLREP_ALG_DIFFSRSAC: lay_diffsrsac(d, L); return true;
    default:
        rl_set_error("unknown algorithm %d", d.alg);
        return false;
    }
}

// ================================================================================================
// (re)build for a batch size
// ================================================================================================
static int build_programs(rlrep_agent* ag, int B) {
    ag->B = B;
    ag->ws.used = ag->ws_static;
    for (Program* p : {&ag->feat_bwd, &ag->feat_apply, &ag->critic_bwd, &ag->critic_apply, &ag->actor_bwd, &ag->actor_apply, &ag->upd_target, &ag->infer, &ag->sync_prog, &ag->critic_bwd_h, &ag->critic_bwd_w, &ag->critic_bwd_wh, &ag->critic_apply_f, &ag->feat_bwd_h, &ag->critic_bwd_h2, &ag->feat_bwd_m, &ag->feat_apply_m})
        p->stages.clear();
    for (auto& D : ag->dset) for (Program* p : {&D.critic_bwd, &D.critic_apply, &D.actor_bwd}) p->stages.clear();
    ag->infer_n = 0; ag->actor_resume = 0; ag->pi_ready = ag->hoist_req = nullptr; ag->in_train = ag->target_done = false;
    ag->pf_armed = ag->pf_done = false; ag->pf2_armed = ag->pf2_done = false;
    ag->chain_next = ag->chain_bwd_done = ag->l1_done = false;
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    ag->feat_cuts.clear();
    Builder b(ag);
    const int S = ag->d.state_dim, A = ag->d.action_dim;
    {
        // spedersac steps on two minibatches; their [s,a,s'] / [s,a] matrices are allocated back to back so
        // that phi/mu run as ONE 2B-row GEMM per layer
        const int ns = (ag->d.alg == RLREP_ALG_SPEDERSAC) ? 2 : 1;
        float* XE = b.ws.f((size_t)ns * B * (2 * S + A));
        float* XF = b.ws.f((size_t)ns * B * (S + A));
        for (int i = 0; i < ns; ++i) {
            Slot& s = ag->slot[i];
            s.XE = XE ? XE + (size_t)i * B * (2 * S + A) : nullptr;
            s.XF = XF ? XF + (size_t)i * B * (S + A) : nullptr;
            s.XF2 = b.ws.f((size_t)B * (S + A)); s.XFpi = b.ws.f((size_t)B * (S + A)); s.R = b.ws.f(B); s.D = b.ws.f(B); s.filled = false;
            s.Rn = (i == 0 && ag->critic_nstep && ag->cn_block) ? ag->cn_block : s.R;          // (the critic heads read slot 0 only)
        }
    }
    switch (ag->d.alg) {
    case RLREP_ALG_SAC: build_sac(b, ag); break;
    case RLREP_ALG_VLSAC: build_vlsac(b, ag); break;
    case RLREP_ALG_CTRLSAC: build_ctrlsac(b, ag); break;
    case RLREP_ALG_SPEDERSAC: build_spedersac(b, ag); break;
    case RLREP_ALG_DIFFSRSAC: build_diffsrsac(b, ag); break;
    default: rl_set_error("unknown algorithm %d", ag->d.alg); return RLREP_ERR_ARG;
    }
    ag->prog_end = ag->ws.used;
    // room for the B<=max_batch inference program (rlrep_actor_forward)
    const size_t infer_bytes = (size_t)ag->d.max_batch * (2 * ag->d.actor_hidden_dim + 2 * ag->d.action_dim) * sizeof(float) + 8192;
    if (!ag->ws.dry && ag->ws.used + infer_bytes > ag->ws.cap) { rl_set_error("workspace too small: need %zu bytes, have %zu", ag->ws.used + infer_bytes, ag->ws.cap); return RLREP_ERR_NOMEM; }
    if (ag->ws.dry) ag->ws.used += infer_bytes;
    return 0;
}

bool check_dims(const rlrep_dims* d) {
    if (!d || d->state_dim <= 0 || d->action_dim <= 0 || d->hidden_dim <= 0 || d->actor_hidden_dim <= 0 || d->max_batch <= 0) {
        rl_set_error("bad dimensions"); return false;
    }
    if (d->alg == RLREP_ALG_VLSAC) {
        if (d->num_noise != 4 * NC_NF_HOST) { rl_set_error("vlsac: num_noise must be %d", 4 * NC_NF_HOST); return false; }
        if (d->feature_dim <= 0 || d->vae_hidden_dim <= 0 || (d->feature_dim & 3)) { rl_set_error("vlsac: feature_dim must be a positive multiple of 4"); return false; }
    }
    if (d->alg == RLREP_ALG_CTRLSAC || d->alg == RLREP_ALG_SPEDERSAC || d->alg == RLREP_ALG_DIFFSRSAC) {
        if (d->feature_dim <= 0 || d->phi_hidden_dim <= 0 || d->mu_hidden_dim <= 0 || d->phi_hidden_depth < 0 || d->mu_hidden_depth < 0 ||
            d->phi_hidden_depth > 3 || d->mu_hidden_depth > 3) { rl_set_error("bad representation-network dimensions"); return false; }
        if (d->alg == RLREP_ALG_DIFFSRSAC && d->num_noise <= 0) { rl_set_error("diffsrsac: num_noise must be positive"); return false; }
    }
    return true;
}

static void static_state(rlrep_agent* ag) {
    Workspace& ws = ag->ws;
    ws.used = 0;
    ag->steps = (int*)ws.alloc(sizeof(int) * 8);
    ag->adam_step = (GroupCfg*)ws.alloc(sizeof(GroupCfg) * 4);     // [4] optimizer groups
    ag->metrics = ws.f(M_COUNT);
    const int S = ag->d.state_dim, A = ag->d.action_dim;
    ag->obs_in = ws.f((size_t)ag->d.max_batch * S);
    ag->act_out = ws.f((size_t)ag->d.max_batch * A);
    ag->rp_epoch = (int*)ws.alloc(sizeof(int) * 4);
    ag->hist = ws.f((size_t)RL_HIST_N * RL_HIST_REC);
    ag->hist_seq = (int*)ws.alloc(sizeof(int) * 4);
    if (!ws.dry && ws.ok()) { (void)hipMemset(ag->hist, 0xff, sizeof(float) * RL_HIST_N * RL_HIST_REC); (void)hipMemset(ag->hist_seq, 0, sizeof(int) * 4); }
    ag->xc_err = (unsigned*)ws.alloc(256);
    if (!ws.dry && ws.ok()) (void)hipMemset(ag->xc_err, 0, 256);
    // a seed group member's by-value hyper-parameters (group kernel forms only; written by rlrep_group_create / _set_member_hyper).  Behind the
    // metric slots: not part of the device records a checkpoint carries (HipCore.device_state)
    ag->mhyp = (MemberHyper*)ws.alloc(sizeof(MemberHyper));
    if (!ws.dry && ws.ok()) { const int one[4] = {1, 0, 0, 0}; (void)hipMemcpy(ag->rp_epoch, one, sizeof(one), hipMemcpyHostToDevice); }
    // transposed weight shadows (see rlrep_agent::sh_dev): vlsac's feature group, read by the feature step's row programs
    ag->shadow_of.clear();
    for (int g = 0; g < 4; ++g) { ag->sh_dev[g] = nullptr; ag->nsh[g] = ag->sh_tiles[g] = 0; }
    // ... and, with RLREP_ENABLE=fuse_l1, the two FIRST layers of its feature nets (K = 2S+A / S+A) for the variant in which they ride in the
    // second layers' launch (Builder::fwd_stage12 reads W1 transposed).  OPT-IN: measured 11.2 us for the fused launch against 3.7 + 4.9 us
    // for the pair (every one of the 512 tiles re-reads W1^T and X: twice the L2 traffic, three times the load instructions): 2 763 vs
    // 2 865 train()/s.
    const char* fl1 = rl_opt("fuse_l1");
#ifdef RL_EXPERIMENTS
    const bool sh_all = rl_rowprog_enabled(), sh_l1 = fl1 && fl1[0] == '1';
#else
    const bool sh_all = false, sh_l1 = false; (void)fl1;       // (the fused-first-layers launch is an experiments-build kernel)
#endif
    if (ag->d.alg == RLREP_ALG_VLSAC && (sh_all || sh_l1) && !rl_off("shadows")) {
        std::vector<ShadowEnt> tab; std::vector<std::string> first;
        const auto& T = ag->L.t;
        for (size_t q = 0; q < T.size(); ++q) {
            const LT& e = T[q];
            if (e.arena != RLREP_ARENA_PARAM || e.group != 0 || e.cols <= 1 || e.name.find(".weight") == std::string::npos) continue;
            if (!sh_all && e.name != "encoder.l1.weight" && e.name != "f.l1.weight") continue;
            // a glued pair (mean | log_std heads, state | reward heads: Layout::lin_pair) is two consecutive blocks [o1, in], [o2, in] = ONE
            // [o1 + o2, in] matrix for the kernels: one shadow, reachable under the first tensor's name
            if (!tab.empty() && q > 0 && T[q - 1].name.find(".weight") != std::string::npos && tab.back().off + tab.back().n == e.off - ag->L.group_off[0] && tab.back().cols == e.cols) {
                tab.back().rows += e.rows; tab.back().n += (long long)e.rows * e.cols;
                continue;
            }
            ShadowEnt se; memset(&se, 0, sizeof(se));
            // offsets RELATIVE to the group's start: the group's Adam launch indexes its arena slice from 0, and the refresh launches are
            // given param_dev + group_off[0] as their base (one table serves both, wherever the group sits in the arena)
            se.off = e.off - ag->L.group_off[0]; se.n = (long long)e.rows * e.cols; se.rows = e.rows; se.cols = e.cols;
            tab.push_back(se); first.push_back(e.name);
        }
        int tiles = 0;
        for (size_t k = 0; k < tab.size(); ++k) {
            tab[k].sp = ws.f((size_t)tab[k].n);
            ag->shadow_of[first[k]] = tab[k].sp;
            tiles += ((tab[k].rows + 31) / 32) * ((tab[k].cols + 31) / 32);
        }
        ShadowEnt* dev = (ShadowEnt*)ws.alloc(tab.size() * sizeof(ShadowEnt));
        if (!ws.dry && ws.ok() && !tab.empty()) (void)hipMemcpy(dev, tab.data(), tab.size() * sizeof(ShadowEnt), hipMemcpyHostToDevice);
        ag->sh_dev[0] = dev; ag->nsh[0] = (int)tab.size(); ag->sh_tiles[0] = tiles;
    }
    // bf16x3 images of the noise critic's first layers (vlsac): see rlrep_agent::x3_refresh.  (Where the shape rules them out -- F not a
    // multiple of 32 -- the kernels split W themselves, as in round 1.)
    ag->x3_refresh = nullptr; ag->x3_n = ag->x3_tiles = 0; ag->x3_of.clear();
    {
        const int F = ag->d.feature_dim, H = ag->d.hidden_dim;
        if (ag->d.alg == RLREP_ALG_VLSAC && !rl_off("x3") && F > 0 && (F % 32) == 0 && ag->L.index.count("critic.l1.weight") && ag->L.index.count("critic_target.l1.weight")) {
            std::vector<ShadowEnt> all, live;
            const char* names[4] = {"critic.l1.weight", "critic.l4.weight", "critic_target.l1.weight", "critic_target.l4.weight"};
            for (int q = 0; q < 4; ++q) {
                const LT& t = ag->L.get(names[q]);
                ShadowEnt se; memset(&se, 0, sizeof(se));
                se.off = t.off; se.n = (long long)t.rows * t.cols; se.rows = t.rows; se.cols = t.cols; se.kind = 1;
                unsigned char* img = (unsigned char*)ws.alloc((size_t)3 * t.rows * t.cols * 2);
                se.sp = reinterpret_cast<float*>(img);
                se.src = q < 2 ? (ag->a.param_dev ? ag->a.param_dev + t.off : nullptr) : (ag->a.target_dev ? ag->a.target_dev + t.off : nullptr);
                ag->x3_of[names[q]] = img;
                all.push_back(se);
                ag->x3_tiles += ((t.rows + 31) / 32) * ((t.cols + 31) / 32);
                if (q < 2) { ShadowEnt lv = se; lv.src = nullptr; lv.off = t.off - ag->L.group_off[1]; live.push_back(lv); }     // (the Adam launch indexes from the group's start)
                (void)H;
            }
            // the critic's Adam launch carries the critic -> critic_target Polyak inside a train(): its lanes then keep the TARGET images current too
            for (size_t q = 0; q < live.size(); ++q) live[q].st = all[q + 2].sp;
            ShadowEnt* dev = (ShadowEnt*)ws.alloc(all.size() * sizeof(ShadowEnt));
            ShadowEnt* dev_live = (ShadowEnt*)ws.alloc(live.size() * sizeof(ShadowEnt));
            if (!ws.dry && ws.ok()) {
                (void)hipMemcpy(dev, all.data(), all.size() * sizeof(ShadowEnt), hipMemcpyHostToDevice);
                (void)hipMemcpy(dev_live, live.data(), live.size() * sizeof(ShadowEnt), hipMemcpyHostToDevice);
            }
            ag->x3_refresh = dev; ag->x3_n = (int)all.size();
            // the critic group's Adam launch keeps the live images current (the actor step reads them right after the critic update)
            ag->sh_dev[1] = dev_live; ag->nsh[1] = (int)live.size(); ag->sh_tiles[1] = 0;      // (no tiles: group 1 is refreshed through x3_refresh)
        }
    }
    ag->ws_static = ws.used;
}

// regenerate the shadows of group g from the parameters as they stand (a launch of its own: the eager entry points)
static int refresh_shadows(rlrep_agent* ag, void* stream) {
    for (int g = 0; g < 4; ++g) {
        if (!ag->nsh[g] || !ag->sh_tiles[g]) continue;
        const int rc = rl_launch_shadow(ag->sh_dev[g], ag->nsh[g], ag->sh_tiles[g], ag->a.param_dev + ag->L.group_off[g], 0, (hipStream_t)stream); ++g_rl_launches;
        if (rc) { rl_set_error("shadow refresh: hip error %d", rc); return RLREP_ERR_HIP; }
    }
    return 0;
}

// regenerate the bf16x3 images of the noise critic's first layers, live and target, from the tensors as they stand (one launch)
static int refresh_x3(rlrep_agent* ag, void* stream) {
    if (!ag->x3_n) return 0;
    const int rc = rl_launch_shadow(ag->x3_refresh, ag->x3_n, ag->x3_tiles, nullptr, 0, (hipStream_t)stream); ++g_rl_launches;
    if (rc) { rl_set_error("x3 shadow refresh: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

// ================================================================================================
// C ABI
// ================================================================================================
// floats of exchange scratch the batch-coupled feature exchanges of this agent need once attached (rlrep_layout_info.exchange_floats)
static long long exchange_floats(const rlrep_dims& d, int world) {
    if (world <= 1) return 0;
    const long long F = d.feature_dim, B = d.max_batch, W = world;
    if (d.alg == RLREP_ALG_SPEDERSAC) return F <= RL_SLOTS_MAX_F ? 2 * (2 * W * ((F + 63) & ~63ll)) : 0;      // Phibar and v: [2 parities][world][F] each
    if (d.alg == RLREP_ALG_CTRLSAC) return 2 * W * B * F;                                                      // mu(s') of all ranks + its partial gradients
    return 0;
}

int ensure_batch(rlrep_agent* ag, int B) {
    if (B <= 0 || B > ag->d.max_batch) { rl_set_error("batch %d outside (0, max_batch=%d]", B, ag->d.max_batch); return RLREP_ERR_ARG; }
    if (B != ag->B) {
        // table re-upload uses blocking copies: quiesce the device first (rare path: batch size changed)
        (void)hipDeviceSynchronize();
        return build_programs(ag, B);
    }
    return 0;
}

extern "C" {

int32_t rlrep_abi_version(void) { return RLREP_ABI_VERSION; }
const char* rlrep_last_error(void) { return g_err; }

int32_t rlrep_layout(const rlrep_dims* dims, rlrep_layout_info* info, rlrep_tensor_desc* descs, int32_t cap) {
    rl_switches_read();
    if (!check_dims(dims) || !info) return RLREP_ERR_ARG;
    rlrep_agent tmp;
    tmp.d = *dims; memset(&tmp.h, 0, sizeof(tmp.h)); memset(&tmp.a, 0, sizeof(tmp.a));
    tmp.h.world_size = dims->world_size > 1 ? dims->world_size : 1;       // (sizes the workspace of the batch-coupled feature steps: ctrlsac's [B, W B] score matrix)
    if (!build_layout(*dims, tmp.L)) return RLREP_ERR_ARG;
    tmp.L.align(RLREP_ARENA_PARAM); tmp.L.align(RLREP_ARENA_TARGET);
    tmp.ws.dry = true;
    static_state(&tmp);
    if (build_programs(&tmp, dims->max_batch) != 0) return RLREP_ERR_ARG;
    if (tmp.h.world_size > 1 && exchange_floats(*dims, tmp.h.world_size) > 0) {
        // ... and the ATTACHED form (rl_agent_attach_dp: exchanges inside the launches, deferred step programs kept): the larger of the two
        const size_t plain = tmp.ws.used;
        tmp.xfold = true; tmp.xscratch_floats = exchange_floats(*dims, tmp.h.world_size); tmp.dp_proto.world = tmp.h.world_size; tmp.dp_proto.rank = dims->rank;
        if (build_programs(&tmp, dims->max_batch) != 0) return RLREP_ERR_ARG;
        if (tmp.ws.used < plain) tmp.ws.used = plain;
    }
    memset(info, 0, sizeof(*info));
    info->param_floats = tmp.L.cur[RLREP_ARENA_PARAM];
    info->target_floats = tmp.L.cur[RLREP_ARENA_TARGET] > 0 ? tmp.L.cur[RLREP_ARENA_TARGET] : 4;
    info->grad_floats = info->param_floats + RLREP_GRAD_TAIL;
    info->workspace_bytes = (int64_t)tmp.ws.used + 4096;
    info->exchange_floats = exchange_floats(*dims, tmp.h.world_size);
    for (int g = 0; g < 4; ++g) { info->group_offset[g] = tmp.L.group_off[g]; info->group_floats[g] = tmp.L.group_n[g]; }
    info->n_tensors = (int32_t)tmp.L.t.size();
    info->n_metrics = M_COUNT;
    if (descs) {
        for (int i = 0; i < (int)tmp.L.t.size() && i < cap; ++i) {
            const LT& e = tmp.L.t[i];
            memset(&descs[i], 0, sizeof(descs[i]));
            snprintf(descs[i].name, sizeof(descs[i].name), "%s", e.name.c_str());
            descs[i].arena = e.arena; descs[i].group = e.group; descs[i].offset = e.off; descs[i].rows = e.rows; descs[i].cols = e.cols;
        }
    }
    return 0;
}

int32_t rlrep_metric_names(int32_t alg, char (*names)[32], int32_t cap) {
    const char* n[M_COUNT];
    for (int i = 0; i < M_COUNT; ++i) n[i] = "";
    n[M_ACTOR_LOSS] = "actor_loss"; n[M_ALPHA_LOSS] = "alpha_loss"; n[M_ALPHA] = "alpha"; n[M_Q1] = "q1"; n[M_Q2] = "q2";
    switch (alg) {
    case RLREP_ALG_SAC: n[M_Q1_LOSS] = "q_loss"; break;
    case RLREP_ALG_VLSAC:
        n[M_FEAT_TOTAL] = "vae_loss"; n[M_FEAT_A] = "ml_loss"; n[M_KL] = "kl_loss"; n[M_S_LOSS] = "s_loss"; n[M_R_LOSS] = "r_loss";
        n[M_Q1_LOSS] = "q1_loss"; n[M_Q2_LOSS] = "q2_loss"; break;
    case RLREP_ALG_CTRLSAC: case RLREP_ALG_SPEDERSAC:
        n[M_FEAT_TOTAL] = "total_loss"; n[M_FEAT_A] = "model_loss"; n[M_R_LOSS] = "r_loss"; n[M_Q1_LOSS] = "q1_loss"; n[M_Q2_LOSS] = "q2_loss"; break;
    case RLREP_ALG_DIFFSRSAC:
        n[M_FEAT_TOTAL] = "score_loss"; n[M_Q1_LOSS] = "q_loss_reg"; n[M_Q2_LOSS] = "q_loss_noreg"; break;
    default: return RLREP_ERR_ARG;
    }
    for (int i = 0; i < M_COUNT && i < cap; ++i) snprintf(names[i], 32, "%s", n[i]);
    return M_COUNT;
}

int32_t rlrep_agent_create(const rlrep_dims* dims, const rlrep_hyper* hyper, const rlrep_arenas* arenas, void* stream, rlrep_agent** out) {
    if (!check_dims(dims) || !hyper || !arenas || !out) return RLREP_ERR_ARG;
    if (!arenas->param_dev || !arenas->grad_dev || !arenas->exp_avg_dev || !arenas->exp_avg_sq_dev || !arenas->workspace_dev ||
        !arenas->alpha_state_dev || !arenas->target_dev) { rl_set_error("null arena pointer"); return RLREP_ERR_ARG; }
    rlrep_layout_info info;
    if (rlrep_layout(dims, &info, nullptr, 0) != 0) return RLREP_ERR_ARG;
    rl_switches_read();            // RLREP_DISABLE / RLREP_ENABLE are read here, once per agent, never per launch
    std::unique_ptr<rlrep_agent> ag(new rlrep_agent());
    ag->d = *dims; ag->h = *hyper; ag->a = *arenas;
    if (ag->h.world_size <= 0) ag->h.world_size = 1;
    if (!build_layout(*dims, ag->L)) return RLREP_ERR_ARG;
    ag->L.align(RLREP_ARENA_PARAM); ag->L.align(RLREP_ARENA_TARGET);
    ag->ws.base = (char*)arenas->workspace_dev; ag->ws.cap = (size_t)info.workspace_bytes; ag->ws.dry = false;
    static_state(ag.get());
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ag->steps, 0, sizeof(int) * 8 + 0, st);
    {
        GroupCfg gc[4]; memset(gc, 0, sizeof(gc));
        for (int g = 0; g < 4; ++g) {
            gc[g].lr = g == 1 ? hyper->lr_critic : g == 2 ? hyper->lr_actor : hyper->lr_feature;
            gc[g].b1 = hyper->beta1; gc[g].b2 = hyper->beta2; gc[g].eps = hyper->adam_eps;
            gc[g].tau = (g == 0) ? hyper->feature_tau : (g == 1) ? hyper->tau : 0.f;    // Polyak rate of the group's target copy
        }
        if (e == hipSuccess) e = hipMemcpy(ag->adam_step, gc, sizeof(gc), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemsetAsync(ag->metrics, 0, sizeof(float) * M_COUNT, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { rl_set_error("create: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    if (rl_nc_init() != 0) { rl_set_error("create: cannot reserve LDS for the noise-critic kernels"); return RLREP_ERR_HIP; }
    if (rl_rowprog_init() != 0) { rl_set_error("create: cannot reserve LDS for the row-program kernel"); return RLREP_ERR_HIP; }
    if (rl_replearn_init() != 0) { rl_set_error("create: cannot reserve LDS for the score-matching kernel"); return RLREP_ERR_HIP; }
    int rc = build_programs(ag.get(), dims->max_batch);
    if (rc != 0) return rc;
    *out = ag.release();
    return 0;
}

void rlrep_agent_destroy(rlrep_agent* agent) {
    if (agent && agent->grp_seeds) (void)hipFree(agent->grp_seeds);
    if (agent && agent->grp_live) (void)hipFree(agent->grp_live);
    if (agent && agent->cn_block) (void)hipFree(agent->cn_block);
    delete agent;
}

int32_t rlrep_set_batch(rlrep_agent* ag, int32_t slot, const rlrep_batch* bt, void* stream) {
    GROUP_REFUSE("set_batch")
    if (!ag || !bt || slot < 0 || slot > 1 || (slot == 1 && ag->d.alg != RLREP_ALG_SPEDERSAC)) { rl_set_error("set_batch: bad argument"); return RLREP_ERR_ARG; }
    if (slot == 0) { ag->pf_done = false; ag->pf_armed = false; } else { ag->pf2_done = false; ag->pf2_armed = false; }
    ag->pi_ready = nullptr; ag->hoist_req = nullptr;           // a new batch invalidates any prefetched policy forward
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    int rc = ensure_batch(ag, bt->batch);
    if (rc) return rc;
    Slot& s = ag->slot[slot];
    SlotFill p; memset(&p, 0, sizeof(p));
    p.s = bt->state_dev; p.a = bt->action_dev; p.r = bt->reward_dev; p.s2 = bt->next_state_dev; p.d = bt->done_dev;
    p.B = ag->B; p.S = ag->d.state_dim; p.A = ag->d.action_dim;
    p.XE = s.XE; p.XF = s.XF; p.XF2 = s.XF2; p.XFpi = s.XFpi; p.R = s.R; p.D = s.D;
    s.filled = true;
    rc = (++g_rl_launches, rl_launch_fill_slot(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("fill_slot: hip error %d", rc); return RLREP_ERR_HIP; }
    if (s.Rn != s.R && s.Rn && bt->reward_dev) {           // (rlrep_set_critic_nstep: a caller's batch is what it is -- the critic heads read its rewards)
        const hipError_t e = hipMemcpyAsync(s.Rn, bt->reward_dev, sizeof(float) * (size_t)ag->B, hipMemcpyDeviceToDevice, (hipStream_t)stream);
        if (e != hipSuccess) { rl_set_error("set_batch: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    }
    return 0;
}

int32_t rlrep_replay_row_floats(const rlrep_dims* d) { return d ? 2 * d->state_dim + d->action_dim + 2 : RLREP_ERR_ARG; }

int32_t rlrep_replay_add(float* ring_dev, int64_t capacity, int32_t row_floats, int64_t ptr, const float* rows_host, int64_t nrows, void* stream) {
    if (!ring_dev || !rows_host || capacity <= 0 || row_floats <= 0 || ptr < 0 || ptr >= capacity || nrows < 0 || nrows > capacity) {
        rl_set_error("replay_add: bad argument"); return RLREP_ERR_ARG;
    }
    const int64_t first = nrows < capacity - ptr ? nrows : capacity - ptr;
    hipError_t e = hipSuccess;
    if (first > 0) e = hipMemcpyAsync(ring_dev + ptr * row_floats, rows_host, sizeof(float) * first * row_floats, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess && first < nrows)        // across the wrap-around
        e = hipMemcpyAsync(ring_dev, rows_host + first * row_floats, sizeof(float) * (nrows - first) * row_floats, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) { rl_set_error("replay_add: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    return 0;
}

// ... the same in ONE launch that also writes the ring's new fill level into `size_dev` (the scalar the device index generator reads): the rows are
// read in place from PINNED (mapped) host memory -- RLREP_ERR_ARG if `rows_host` is not.
int32_t rlrep_replay_add_sized(float* ring_dev, int64_t capacity, int32_t row_floats, int64_t ptr, const float* rows_host, int64_t nrows,
                               int32_t* size_dev, int32_t new_size, void* stream) {
    if (!ring_dev || !rows_host || capacity <= 0 || row_floats <= 0 || ptr < 0 || ptr >= capacity || nrows < 0 || nrows > capacity || new_size < 0 || new_size > capacity) {
        rl_set_error("replay_add_sized: bad argument"); return RLREP_ERR_ARG;
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, const_cast<float*>(rows_host), 0) != hipSuccess || !d) { rl_set_error("replay_add_sized: the staging rows are not mapped (pinned) host memory"); return RLREP_ERR_ARG; }
    ++g_rl_launches;
    const int rc = rl_launch_replay_add(ring_dev, capacity, row_floats, ptr, (const float*)d, nrows, size_dev, new_size, (hipStream_t)stream);
    if (rc) { rl_set_error("replay_add_sized: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

// n device-resident transitions (five arrays with row strides) into the ring in ONE launch, the new fill level with them (replay_add_cols_kernel)
int32_t rlrep_replay_add_cols(float* ring_dev, int64_t max_size, int32_t row_floats, int64_t start, int32_t S, int32_t A, const float* s, int64_t ld_s,
                              const float* a, int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n, int32_t* size_dev,
                              int32_t new_size, void* stream) {
    if (!ring_dev || !s || !a || !s2 || !r || !d) { rl_set_error("replay_add_cols: bad argument (null ring or array)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || n < 1 || n > max_size) { rl_set_error("replay_add_cols: n %lld outside [1, max_size %lld]", (long long)n, (long long)max_size); return RLREP_ERR_ARG; }
    if (S < 1 || A < 1 || row_floats != 2 * S + A + 2) { rl_set_error("replay_add_cols: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, S, A); return RLREP_ERR_ARG; }
    if (start < 0 || start >= max_size) { rl_set_error("replay_add_cols: start %lld outside the ring of %lld rows", (long long)start, (long long)max_size); return RLREP_ERR_ARG; }
    if (ld_s < S || ld_a < A || ld_s2 < S || new_size < 0 || new_size > max_size) { rl_set_error("replay_add_cols: bad argument (a row stride below its width, or new_size outside the ring)"); return RLREP_ERR_ARG; }
    ReplayCols p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.capacity = max_size; p.start = start; p.row = row_floats; p.S = S; p.A = A; p.new_size = new_size;
    p.s = s; p.a = a; p.s2 = s2; p.r = r; p.d = d; p.ld_s = ld_s; p.ld_a = ld_a; p.ld_s2 = ld_s2; p.n = n; p.size_dev = size_dev;
    ++g_rl_launches;
    const int rc = rl_launch_replay_add_cols(&p, 0, (hipStream_t)stream);
    if (rc) { rl_set_error("replay_add_cols: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

static_assert(RL_LOOP_CTL_WORDS == RLREP_LOOP_CTL_WORDS && RL_CTL_WARM < RL_LOOP_CTL_WORDS, "include/rlrep.h documents the loop record (kparams.h RL_CTL_*)");
// rlrep_replay_add_cols with `start` and the fill level read from the loop record on the device (replay_add_cols_kernel_ctl): capturable
int32_t rlrep_replay_add_cols_ctl(float* ring_dev, int64_t max_size, int32_t row_floats, int32_t S, int32_t A, const float* s, int64_t ld_s, const float* a,
                                  int64_t ld_a, const float* s2, int64_t ld_s2, const float* r, const float* d, int64_t n, int32_t* size_dev, int64_t* ctl_dev,
                                  void* stream) {
    if (!ring_dev || !s || !a || !s2 || !r || !d || !ctl_dev) { rl_set_error("replay_add_cols_ctl: bad argument (null ring, array or loop record)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || max_size > INT32_MAX || n < 1 || n > max_size) { rl_set_error("replay_add_cols_ctl: n %lld outside [1, max_size %lld]", (long long)n, (long long)max_size); return RLREP_ERR_ARG; }
    if (S < 1 || A < 1 || row_floats != 2 * S + A + 2) { rl_set_error("replay_add_cols_ctl: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, S, A); return RLREP_ERR_ARG; }
    if (ld_s < S || ld_a < A || ld_s2 < S) { rl_set_error("replay_add_cols_ctl: bad argument (a row stride below its width)"); return RLREP_ERR_ARG; }
    ReplayCols p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.capacity = max_size; p.row = row_floats; p.S = S; p.A = A;
    p.s = s; p.a = a; p.s2 = s2; p.r = r; p.d = d; p.ld_s = ld_s; p.ld_a = ld_a; p.ld_s2 = ld_s2; p.n = n; p.size_dev = size_dev;
    ++g_rl_launches;
    const int rc = rl_launch_replay_add_cols_ctl(&p, (long long*)ctl_dev, (hipStream_t)stream);
    if (rc) { rl_set_error("replay_add_cols_ctl: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

// ---- fused simulators (sim_step.hip): rlrep_sim_state is kparams.h SimState, field for field ----
static_assert(sizeof(SimState) == sizeof(rlrep_sim_state) && offsetof(SimState, t) == offsetof(rlrep_sim_state, t) && offsetof(SimState, obs) == offsetof(rlrep_sim_state, obs) &&
              offsetof(SimState, kind) == offsetof(rlrep_sim_state, kind) && offsetof(SimState, n) == offsetof(rlrep_sim_state, n) &&
              offsetof(SimState, seed) == offsetof(rlrep_sim_state, seed) && offsetof(SimState, auto_restart) == offsetof(rlrep_sim_state, auto_restart) &&
              RL_SIM_MAX_ENVS == RLREP_SIM_MAX_ENVS, "include/rlrep.h rlrep_sim_state (kparams.h SimState)");
int32_t rlrep_sim_state_bytes(void) { return (int32_t)sizeof(rlrep_sim_state); }
// what the three entry points refuse alike, by the entry point's name `who`; the kind's row of rl_env_kinds, or null with the error set
static const EnvKindInfo* sim_check(const char* who, const rlrep_sim_state* s) {
    if (!s || !s->x0 || !s->x1 || !s->ep_return || !s->last_return || !s->t || !s->episodes || !s->starts || !s->obs) {
        rl_set_error("%s: bad argument (null simulator state or array)", who); return nullptr;
    }
    const EnvKindInfo* k = rl_env_kind(s->kind);
    if (!k) { rl_set_error("%s: kind %d is not built (0 = Pendulum-v1, 2 = MountainCarContinuous-v0)", who, s->kind); return nullptr; }
    if (s->n < 1 || s->n > RLREP_SIM_MAX_ENVS) { rl_set_error("%s: n %d outside [1, %d]", who, s->n, RLREP_SIM_MAX_ENVS); return nullptr; }
    return k;
}
int32_t rlrep_sim_start(const rlrep_sim_state* sim, void* stream) {
    if (!sim_check("sim_start", sim)) return RLREP_ERR_ARG;
    ++g_rl_launches;
    const int rc = rl_launch_sim_start((const SimState*)sim, (hipStream_t)stream);
    if (rc) { rl_set_error("sim_start: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_sim_step(const rlrep_sim_state* sim, const float* act, int64_t ld_act, float* next_obs, float* reward, float* done, void* stream) {
    const EnvKindInfo* k = sim_check("sim_step", sim);
    if (!k) return RLREP_ERR_ARG;
    if (!act || !next_obs || !reward || !done) { rl_set_error("sim_step: bad argument (null actions or output array)"); return RLREP_ERR_ARG; }
    if (ld_act < k->A) { rl_set_error("sim_step: ld_act %lld below the kind's A %d", (long long)ld_act, k->A); return RLREP_ERR_ARG; }
    ++g_rl_launches;
    const int rc = rl_launch_sim_step((const SimState*)sim, act, ld_act, next_obs, reward, done, (hipStream_t)stream);
    if (rc) { rl_set_error("sim_step: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_sim_step_append_ctl(const rlrep_sim_state* sim, const float* act, int64_t ld_act, float* ring_dev, int64_t max_size, int32_t row_floats,
                                  int32_t* size_dev, int64_t* ctl_dev, void* stream) {
    const EnvKindInfo* k = sim_check("sim_step_append_ctl", sim);
    if (!k) return RLREP_ERR_ARG;
    if (!act || !ring_dev || !ctl_dev) { rl_set_error("sim_step_append_ctl: bad argument (null actions, ring or loop record)"); return RLREP_ERR_ARG; }
    if (max_size <= 0 || max_size > INT32_MAX || sim->n > max_size) {
        rl_set_error("sim_step_append_ctl: n %d outside [1, max_size %lld]", sim->n, (long long)max_size); return RLREP_ERR_ARG;
    }
    if (ld_act < k->A) { rl_set_error("sim_step_append_ctl: ld_act %lld below the kind's A %d", (long long)ld_act, k->A); return RLREP_ERR_ARG; }
    if (row_floats != k->row) { rl_set_error("sim_step_append_ctl: row %d is not 2 S + A + 2 (S %d, A %d)", row_floats, k->S, k->A); return RLREP_ERR_ARG; }
    ++g_rl_launches;
    const int rc = rl_launch_sim_step_ctl((const SimState*)sim, act, ld_act, ring_dev, max_size, size_dev, (long long*)ctl_dev, (hipStream_t)stream);
    if (rc) { rl_set_error("sim_step_append_ctl: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

static void slot_fill_params(rlrep_agent* ag, int slot, const float* ring_dev, const int32_t* idx_dev, SlotFill& p) {
    Slot& s = ag->slot[slot];
    memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.idx = idx_dev; p.B = ag->B; p.S = ag->d.state_dim; p.A = ag->d.action_dim;
    p.XE = s.XE; p.XF = s.XF; p.XF2 = s.XF2; p.XFpi = s.XFpi; p.R = s.R; p.D = s.D;
}

int32_t rlrep_prefetch_batch(rlrep_agent* ag, const float* ring_dev, const int32_t* idx_dev, int32_t batch) {
    if (!ag || !ring_dev || !idx_dev) { rl_set_error("prefetch_batch: bad argument"); return RLREP_ERR_ARG; }
    // a seed group's gather rides in its group optimizer launch: member r reads ring r (the stride its train prologue was given) through ITS
    // index stream, which must therefore lie in member 0's block (it is read at every member's stride)
    if (ag->members > 0 && !in_member0(ag, idx_dev, 4ll * batch)) {
        rl_set_error("prefetch_batch: a seed group's indices must lie inside member 0's block"); return RLREP_ERR_ARG;
    }
    ag->pf_armed = false;
    if (batch != ag->B || rl_off("prefetch_batch")) return 0;      // would need a rebuild: let replay_sample do it
    slot_fill_params(ag, 0, ring_dev, idx_dev, ag->pf_fill);
    ag->pf_ring = ring_dev; ag->pf_idx = idx_dev; ag->pf_armed = true;
    return 1;
}

int32_t rlrep_prefetch_batch_slot(rlrep_agent* ag, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch) {
    if (slot == 0) return rlrep_prefetch_batch(ag, ring_dev, idx_dev, batch);
    GROUP_REFUSE("prefetch_batch_slot")
    if (!ag || !ring_dev || !idx_dev || slot != 1 || ag->d.alg != RLREP_ALG_SPEDERSAC) { rl_set_error("prefetch_batch_slot: bad argument"); return RLREP_ERR_ARG; }
    ag->pf2_armed = false;
    if (batch != ag->B || rl_off("prefetch_batch")) return 0;
    slot_fill_params(ag, 1, ring_dev, idx_dev, ag->pf2_fill);
    ag->pf2_ring = ring_dev; ag->pf2_idx = idx_dev; ag->pf2_armed = true;
    return 1;
}

int32_t rlrep_train_prologue(rlrep_agent* ag, const float* ring_dev, const int32_t* size_dev, int32_t* idx_pool_dev, int64_t n_idx,
                             float* eps_pool_dev, int64_t n_eps, uint64_t seed, uint64_t idx_offset, uint64_t eps_offset,
                             int32_t batch, void* stream) {
    if (!ag || !ring_dev || !size_dev || !idx_pool_dev || !eps_pool_dev || n_idx < batch || n_eps <= 0 || batch <= 0) {
        rl_set_error("train_prologue: bad argument"); return RLREP_ERR_ARG;
    }
    if (ag->members > 0 && !g_grp_on) { rl_set_error("train_prologue: a seed group takes rlrep_group_train_prologue"); return RLREP_ERR_ARG; }
    ag->pi_ready = nullptr; ag->hoist_req = nullptr; ag->pf_armed = false; ag->pf_done = false; ag->pf2_armed = false; ag->pf2_done = false;
    ag->chain_next = ag->chain_bwd_done = ag->l1_done = false;
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    int rc = ensure_batch(ag, batch);
    if (rc) return rc;
    if (ag->mirror_pending) {      // the previous prologue was followed by no optimizer launch that refreshes the counter's mirror: catch up (rare path)
        rc = (++g_rl_launches, rl_launch_counter_sync(ag->steps, 2, (hipStream_t)stream));
        if (rc) { rl_set_error("train_prologue: hip error %d", rc); return RLREP_ERR_HIP; }
    }
    TrainPrologue tp; memset(&tp, 0, sizeof(tp));
    tp.idx.dst_i = idx_pool_dev; tp.idx.n = n_idx; tp.idx.kind = 1; tp.idx.hi = 1; tp.idx.hi_dev = size_dev;
    tp.idx.seed = seed; tp.idx.offset = idx_offset; tp.idx.step_dev = ag->steps + 2; tp.idx.step_add = 1;
    tp.eps.dst_f = eps_pool_dev; tp.eps.n = n_eps; tp.eps.kind = 0; tp.eps.std = 1.0f;
    tp.eps.seed = seed; tp.eps.offset = eps_offset; tp.eps.step_dev = ag->steps + 2; tp.eps.step_add = 1;
    slot_fill_params(ag, 0, ring_dev, nullptr, tp.fill);
    tp.counter = ag->steps; tp.ticket = nullptr;          // (word 2 of the counter block is what the prologue's blocks read: train_prologue_kernel)
    tp.sh = ag->sh_dev[0]; tp.nsh = ag->nsh[0]; tp.nb_tr = ag->sh_tiles[0]; tp.sh_base = ag->a.param_dev + ag->L.group_off[0];
    rc = (++g_rl_launches, rl_launch_train_prologue(&tp, (hipStream_t)stream));
    if (rc) { rl_set_error("train_prologue: hip error %d", rc); return RLREP_ERR_HIP; }
    ag->slot[0].filled = true;
    ag->pf_done = true; ag->pf_ring = ring_dev; ag->pf_idx = idx_pool_dev;     // the first `batch` pool entries are in slot 0
    ag->in_train = true; ag->target_done = false;
    ag->mirror_pending = true;          // cleared by the optimizer launch that refreshes the mirror (engine_internal.h Builder::adam)
    return 0;
}

int32_t rlrep_replay_sample(rlrep_agent* ag, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch, void* stream) {
    if (!ag || !ring_dev || !idx_dev || slot < 0 || slot > 1 || (slot == 1 && ag->d.alg != RLREP_ALG_SPEDERSAC)) { rl_set_error("replay_sample: bad argument"); return RLREP_ERR_ARG; }
    if (slot == 0 && ag->pf_done && ring_dev == ag->pf_ring && idx_dev == ag->pf_idx && batch == ag->B && ag->slot[0].filled) {
        ag->pf_done = false;                                   // this very gather already ran (train prologue / optimizer launch)
        return 0;
    }
    if (slot == 1 && ag->pf2_done && ring_dev == ag->pf2_ring && idx_dev == ag->pf2_idx && batch == ag->B && ag->slot[1].filled) {
        ag->pf2_done = false;                                  // gathered by the previous optimizer launch (rlrep_prefetch_batch_slot)
        return 0;
    }
    GROUP_REFUSE("replay_sample")                              // (a group's gathers are its train prologue's)
    if (slot == 0) { ag->pf_done = false; ag->l1_done = false; ag->chain_next = false; } else ag->pf2_done = false;
    ag->pi_ready = nullptr; ag->hoist_req = nullptr;           // a new batch invalidates any prefetched policy forward
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    int rc = ensure_batch(ag, batch);
    if (rc) return rc;
    Slot& s = ag->slot[slot];
    SlotFill p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.idx = idx_dev; p.B = ag->B; p.S = ag->d.state_dim; p.A = ag->d.action_dim;
    p.XE = s.XE; p.XF = s.XF; p.XF2 = s.XF2; p.XFpi = s.XFpi; p.R = s.R; p.D = s.D;
    s.filled = true;
    rc = (++g_rl_launches, rl_launch_fill_slot(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("fill_slot: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

// ---- n-step returns (nstep.hip) ------------------------------------------------------------------------------------------------
static int nstep_args_ok(const char* what, const float* ring, const int32_t* idx, int32_t batch, int64_t max_size, const int32_t* size_dev, int32_t n, int32_t stride) {
    if (!ring || !idx || !size_dev || batch < 1) { rl_set_error("%s: bad argument (null ring / idx / size_dev, or batch %d)", what, batch); return RLREP_ERR_ARG; }
    if (max_size < 1 || max_size > 0x7fffffffll) { rl_set_error("%s: a ring of %lld rows (int32 indices address [1, 2^31) rows)", what, (long long)max_size); return RLREP_ERR_ARG; }
    if (n < 1 || n > RLREP_NSTEP_MAX) { rl_set_error("%s: n %d outside [1, %d]", what, n, RLREP_NSTEP_MAX); return RLREP_ERR_ARG; }
    if (stride < 1) { rl_set_error("%s: stride %d (the number of interleaved environments) must be >= 1", what, stride); return RLREP_ERR_ARG; }
    return 0;
}
// rlrep_replay_sample(slot 0) with n-step rows: never skipped (the gather the train prologue ran is overwritten), discount = the agent's
int32_t rlrep_replay_sample_nstep(rlrep_agent* ag, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch, int64_t max_size,
                                  const int32_t* size_dev, int32_t n, int32_t stride, void* stream) {
    if (!ag) { rl_set_error("replay_sample_nstep: null agent"); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("replay_sample_nstep: not available on a seed group (rlrep_group_create): n-step replay is built for one sac agent"); return RLREP_ERR_ARG; }
    if (ag->d.alg != RLREP_ALG_SAC) { rl_set_error("replay_sample_nstep: n-step replay is built for sac only (the representation agents' feature step models one-step dynamics)"); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("replay_sample_nstep: n-step replay runs on one GPU (world_size = %d)", ag->h.world_size); return RLREP_ERR_ARG; }
    if (slot != 0) { rl_set_error("replay_sample_nstep: slot %d (sac has slot 0 only)", slot); return RLREP_ERR_ARG; }
    if (int rc = nstep_args_ok("replay_sample_nstep", ring_dev, idx_dev, batch, max_size, size_dev, n, stride)) return rc;
    // a new batch: what rlrep_replay_sample invalidates
    ag->pf_done = false; ag->l1_done = false; ag->chain_next = false;
    ag->pi_ready = nullptr; ag->hoist_req = nullptr;
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    int rc = ensure_batch(ag, batch);
    if (rc) return rc;
    NStepGather p; memset(&p, 0, sizeof(p));
    slot_fill_params(ag, 0, ring_dev, idx_dev, p.fill);
    p.size_dev = size_dev; p.capacity = max_size; p.n = n; p.stride = stride; p.gamma = ag->h.discount;
    ag->slot[0].filled = true;
    rc = (++g_rl_launches, rl_launch_nstep_gather(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("replay_sample_nstep: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// the same gather into caller-owned arrays, no agent: xe [batch, 2 S + A] = [s, a, s'], r [batch], d [batch] (ReplayBuffer.gather_nstep)
int32_t rlrep_replay_gather_nstep(const float* ring_dev, const int32_t* idx_dev, int32_t batch, int32_t S, int32_t A, int64_t max_size, const int32_t* size_dev,
                                  int32_t n, int32_t stride, float gamma, float* xe_dev, float* xf_dev, float* xf2_dev, float* xfpi_dev, float* r_dev, float* d_dev,
                                  void* stream) {
    if (int rc = nstep_args_ok("replay_gather_nstep", ring_dev, idx_dev, batch, max_size, size_dev, n, stride)) return rc;
    if (S < 1 || A < 1 || !xe_dev || !xf_dev || !xf2_dev || !xfpi_dev || !r_dev || !d_dev) { rl_set_error("replay_gather_nstep: bad argument (S %d, A %d, or a null output)", S, A); return RLREP_ERR_ARG; }
    NStepGather p; memset(&p, 0, sizeof(p));
    p.fill.ring = ring_dev; p.fill.idx = idx_dev; p.fill.B = batch; p.fill.S = S; p.fill.A = A;
    p.fill.XE = xe_dev; p.fill.XF = xf_dev; p.fill.XF2 = xf2_dev; p.fill.XFpi = xfpi_dev; p.fill.R = r_dev; p.fill.D = d_dev;
    p.size_dev = size_dev; p.capacity = max_size; p.n = n; p.stride = stride; p.gamma = gamma;
    const int rc = (++g_rl_launches, rl_launch_nstep_gather(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("replay_gather_nstep: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

// ---- n-step critic targets of the representation agents (nstep_targets.hip) ----------------------------------------------------
// on: the critic heads of vlsac / ctrlsac / spedersac / diffsrsac read a reward array of their own (Slot::Rn), which
// rlrep_replay_sample_nstep_targets fills; the feature programs keep reading R.  Outside any capture: allocates (once) and rebuilds the programs.
int32_t rlrep_set_critic_nstep(rlrep_agent* ag, int32_t on) {
    if (!ag) { rl_set_error("set_critic_nstep: null agent"); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("set_critic_nstep: not available on a seed group (rlrep_group_create): n-step critic targets are built for one agent"); return RLREP_ERR_ARG; }
    if (ag->d.alg == RLREP_ALG_SAC) { rl_set_error("set_critic_nstep: sac has n_step (rlrep_replay_sample_nstep): its critic owns the whole minibatch"); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("set_critic_nstep: n-step critic targets run on one GPU (world_size = %d)", ag->h.world_size); return RLREP_ERR_ARG; }
    const bool want = on != 0;
    if (want == ag->critic_nstep) return 0;
    hipError_t e = hipDeviceSynchronize();                 // (the programs are rebuilt with blocking table uploads, as when the batch size changes)
    if (e != hipSuccess) { rl_set_error("set_critic_nstep: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    if (want && !ag->cn_block) {
        const size_t bytes = sizeof(float) * (size_t)(((long long)ag->d.max_batch + 63) & ~63ll) * (1 + rlrep_agent::NSETS);
        float* block = nullptr;
        e = hipMalloc((void**)&block, bytes);
        if (e != hipSuccess) { rl_set_error("set_critic_nstep: %s", hipGetErrorString(e)); return RLREP_ERR_NOMEM; }
        e = hipMemset(block, 0, bytes);
        if (e != hipSuccess) { (void)hipFree(block); rl_set_error("set_critic_nstep: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
        ag->cn_block = block; ag->cn_stride = ((long long)ag->d.max_batch + 63) & ~63ll;
    }
    ag->critic_nstep = want;
    return ag->B > 0 ? build_programs(ag, ag->B) : 0;
}
// The target gather behind rlrep_replay_sample(slot 0) of the minibatch the critic and actor steps reuse: XF2[:, 0:S], Rn and D of slot 0 become
// the n-step ones (discount = the agent's); XE, XF, XFpi and R -- what the feature step reads -- stay.  Never skipped.
int32_t rlrep_replay_sample_nstep_targets(rlrep_agent* ag, int32_t slot, const float* ring_dev, const int32_t* idx_dev, int32_t batch, int64_t max_size,
                                          const int32_t* size_dev, int32_t n, int32_t stride, void* stream) {
    const char* what = "replay_sample_nstep_targets";
    if (!ag) { rl_set_error("%s: null agent", what); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("%s: not available on a seed group (rlrep_group_create): n-step critic targets are built for one agent", what); return RLREP_ERR_ARG; }
    if (ag->d.alg == RLREP_ALG_SAC) { rl_set_error("%s: sac takes rlrep_replay_sample_nstep (its critic owns the whole minibatch)", what); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("%s: n-step critic targets run on one GPU (world_size = %d)", what, ag->h.world_size); return RLREP_ERR_ARG; }
    if (slot != 0) { rl_set_error("%s: slot %d (the critic and actor steps read slot 0)", what, slot); return RLREP_ERR_ARG; }
    if (int rc = nstep_args_ok(what, ring_dev, idx_dev, batch, max_size, size_dev, n, stride)) return rc;
    if (!ag->critic_nstep || ag->slot[0].Rn == ag->slot[0].R) { rl_set_error("%s: rlrep_set_critic_nstep(agent, 1) has not been called (the critic heads still read R)", what); return RLREP_ERR_STATE; }
    if (batch != ag->B || !ag->slot[0].filled) { rl_set_error("%s: batch %d behind no rlrep_replay_sample of that size (slot 0 holds %d rows)", what, batch, ag->slot[0].filled ? ag->B : 0); return RLREP_ERR_STATE; }
    ag->early_ready_crit = nullptr;                        // (a policy forward on the one-step s' that already ran is stale; one that is armed runs behind this launch)
    const Slot& s = ag->slot[0];
    NStepTargets p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.idx = idx_dev; p.XF2 = s.XF2; p.Rn = s.Rn; p.D = s.D; p.size_dev = size_dev; p.capacity = max_size;
    p.B = ag->B; p.S = ag->d.state_dim; p.A = ag->d.action_dim; p.n = n; p.stride = stride; p.gamma = ag->h.discount;
    const int rc = (++g_rl_launches, rl_launch_nstep_targets(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("%s: hip error %d", what, rc); return RLREP_ERR_HIP; }
    return 0;
}
// the same gather into caller-owned arrays, no agent: xf2 [batch, S + A] (columns [0, S) written), rn [batch], d [batch]
int32_t rlrep_replay_gather_nstep_targets(const float* ring_dev, const int32_t* idx_dev, int32_t batch, int32_t S, int32_t A, int64_t max_size,
                                          const int32_t* size_dev, int32_t n, int32_t stride, float gamma, float* xf2_dev, float* rn_dev, float* d_dev, void* stream) {
    const char* what = "replay_gather_nstep_targets";
    if (int rc = nstep_args_ok(what, ring_dev, idx_dev, batch, max_size, size_dev, n, stride)) return rc;
    if (S < 1 || A < 1 || !xf2_dev || !rn_dev || !d_dev) { rl_set_error("%s: bad argument (S %d, A %d, or a null output)", what, S, A); return RLREP_ERR_ARG; }
    NStepTargets p; memset(&p, 0, sizeof(p));
    p.ring = ring_dev; p.idx = idx_dev; p.XF2 = xf2_dev; p.Rn = rn_dev; p.D = d_dev; p.size_dev = size_dev; p.capacity = max_size;
    p.B = batch; p.S = S; p.A = A; p.n = n; p.stride = stride; p.gamma = gamma;
    const int rc = (++g_rl_launches, rl_launch_nstep_targets(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("%s: hip error %d", what, rc); return RLREP_ERR_HIP; }
    return 0;
}

// the arrays of minibatch slot `slot` (which = 0 .. 6: XE, XF, XF2, XFpi, R, D, Rn), for read-back by tests and tools; a group: member 0's
const float* rlrep_slot_dev(rlrep_agent* ag, int32_t slot, int32_t which) {
    if (!ag || slot < 0 || slot > 1 || which < 0 || which > 6) return nullptr;
    const Slot& s = ag->slot[slot];
    const float* const arr[7] = {s.XE, s.XF, s.XF2, s.XFpi, s.R, s.D, s.Rn};
    return arr[which];
}

static int philox(float* df, int32_t* di, int64_t n, int kind, float std, int hi, const int* hi_dev, uint64_t seed, uint64_t off,
                  const int* step_dev, void* stream) {
    if (n <= 0) return 0;
    PhiloxFill p; memset(&p, 0, sizeof(p));
    p.dst_f = df; p.dst_i = di; p.n = n; p.kind = kind; p.std = std; p.hi = hi; p.hi_dev = hi_dev; p.seed = seed; p.offset = off;
    p.step_dev = step_dev; p.stream_id = 0;
    int rc = (++g_rl_launches, rl_launch_philox(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("philox: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_fill_indices(int32_t* dst, int64_t n, int32_t hi, uint64_t seed, uint64_t offset, void* stream) {
    if (!dst || hi <= 0) { rl_set_error("fill_indices: bad argument"); return RLREP_ERR_ARG; }
    return philox(nullptr, dst, n, 1, 0.f, hi, nullptr, seed, offset, nullptr, stream);
}
int32_t rlrep_fill_normal(float* dst, int64_t n, float std, uint64_t seed, uint64_t offset, void* stream) {
    if (!dst) { rl_set_error("fill_normal: bad argument"); return RLREP_ERR_ARG; }
    return philox(dst, nullptr, n, 0, std, 0, nullptr, seed, offset, nullptr, stream);
}
int32_t rlrep_fill_indices_dev(int32_t* dst, int64_t n, const int32_t* hi_dev, uint64_t seed, uint64_t offset, const int32_t* counter_dev, void* stream) {
    if (!dst || !hi_dev) { rl_set_error("fill_indices_dev: bad argument"); return RLREP_ERR_ARG; }
    return philox(nullptr, dst, n, 1, 0.f, 1, hi_dev, seed, offset, counter_dev, stream);
}
int32_t rlrep_fill_normal_dev(float* dst, int64_t n, float std, uint64_t seed, uint64_t offset, const int32_t* counter_dev, void* stream) {
    if (!dst) { rl_set_error("fill_normal_dev: bad argument"); return RLREP_ERR_ARG; }
    return philox(dst, nullptr, n, 0, std, 0, nullptr, seed, offset, counter_dev, stream);
}
int32_t rlrep_philox_raw(const uint32_t* ctr_key_dev, uint32_t* out_dev, int64_t n, void* stream) {
    if (!ctr_key_dev || !out_dev || n <= 0 || n > (1ll << 30)) { rl_set_error("philox_raw: bad argument"); return RLREP_ERR_ARG; }
    const int rc = rl_launch_philox_raw(ctr_key_dev, out_dev, n, (hipStream_t)stream);
    if (rc) { rl_set_error("philox_raw: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
const int32_t* rlrep_steps_dev(rlrep_agent* ag) { return ag ? ag->steps : nullptr; }
static_assert(sizeof(GroupCfg) == 4 * RLREP_GROUP_CFG_WORDS, "include/rlrep.h documents the GroupCfg layout");
const void* rlrep_group_cfg_dev(rlrep_agent* ag) { return ag ? ag->adam_step : nullptr; }

static int run(rlrep_agent* ag, const Program& p, void* stream) {
    if (!ag->slot[0].filled) { rl_set_error("step before set_batch / replay_sample"); return RLREP_ERR_STATE; }
    ag->last_launches += (int)p.stages.size();
    return p.run((hipStream_t)stream);
}
#define STEP_PROLOGUE(needs_feature) \
    if (!ag) { rl_set_error("null agent"); return RLREP_ERR_ARG; } \
    GrpScope grp_scope_(ag); \
    if ((needs_feature) && ag->d.alg == RLREP_ALG_SAC) { rl_set_error("sac has no feature step"); return RLREP_ERR_ARG; }

int32_t rlrep_feature_backward(rlrep_agent* ag, const float* eps, const int32_t* idx, void* stream) {
    STEP_PROLOGUE(true)
    if (ag->d.alg == RLREP_ALG_VLSAC && !eps) { rl_set_error("vlsac feature step needs eps[B,F]"); return RLREP_ERR_ARG; }
    if (ag->d.alg == RLREP_ALG_DIFFSRSAC && (!eps || !idx)) { rl_set_error("diffsrsac feature step needs noise_idx[B] and eps[B,S]"); return RLREP_ERR_ARG; }
    if (ag->d.alg == RLREP_ALG_SPEDERSAC && !ag->slot[1].filled) { rl_set_error("spedersac feature step needs batch slot 1"); return RLREP_ERR_STATE; }
    ag->cur_eps = eps; ag->cur_idx = idx; ag->last_launches = 0;
    if (!ag->in_train && ag->has_shadows()) { const int rs = refresh_shadows(ag, stream); if (rs) return rs; }     // parameters may have been written by the caller
    if (!ag->in_train && rl_rowprog_enabled() && ag->rp_epoch) (void)(++g_rl_launches, rl_launch_counter_inc(ag->rp_epoch, 0, (hipStream_t)stream));   // a fresh epoch whatever ran before
    ag->pi_ready = nullptr;                                       // f_target is about to change
    ag->early_ready_crit = ag->early_ready_act = nullptr;
    // chained feature steps: the previous step's optimizer launch already ran this step's first stage (encoder.l1 / f.l1)
    const size_t first = ag->l1_done ? 1 : 0;
    const bool chain = ag->chain_next;
    ag->l1_done = false; ag->chain_next = false; ag->chain_bwd_done = false;
    if (ag->early_crit && !ag->feat_bwd_h.stages.empty()) {
        if (first || chain) { rl_set_error("feature step: rlrep_feature_chain_next cannot be combined with rlrep_prefetch_policy_early"); return RLREP_ERR_STATE; }
        ag->cur_eps3 = ag->early_crit; ag->cur_eps2 = ag->early_act;
        ag->early_crit = ag->early_act = nullptr;
        const int rc = run(ag, ag->feat_bwd_h, stream);
        if (rc == 0) { ag->early_ready_crit = ag->cur_eps3; ag->early_ready_act = ag->cur_eps2; }
        return rc;
    }
    ag->early_crit = ag->early_act = nullptr;
    if (!ag->slot[0].filled) { rl_set_error("step before set_batch / replay_sample"); return RLREP_ERR_STATE; }
    const Program& p = chain ? ag->feat_bwd_m : ag->feat_bwd;
    ag->last_launches += (int)(p.stages.size() - first);
    const int rc = p.run((hipStream_t)stream, first);
    if (rc == 0 && chain) ag->chain_bwd_done = true;
    return rc;
}
int32_t rlrep_feature_apply(rlrep_agent* ag, void* stream) {
    STEP_PROLOGUE(true)
    if (ag->chain_bwd_done) {          // the first layers' optimizer already ran (weight-gradient epilogues): the launch that skips them and runs the next step's head
        ag->chain_bwd_done = false;
        const int rc = run(ag, ag->feat_apply_m, stream);
        if (rc == 0) ag->l1_done = true;
        return rc;
    }
    return run(ag, ag->feat_apply, stream);
}
// The NEXT feature step will follow this one directly, on the minibatch armed by rlrep_prefetch_batch: chain them (rlrep_agent::feat_bwd_m).
// Call between rlrep_prefetch_batch and this step's rlrep_feature_backward / rlrep_feature_step.  1: armed; 0: not available for this agent
// (the step then runs as usual).  The caller must indeed run that next step next, with plain rlrep_feature_backward (no early policy).
int32_t rlrep_feature_chain_next(rlrep_agent* ag) {
    if (!ag) { rl_set_error("null agent"); return RLREP_ERR_ARG; }
    ag->chain_next = false;
    if (ag->feat_bwd_m.stages.empty() || ag->feat_apply_m.stages.empty() || !ag->pf_armed || ag->snap_armed) return 0;
    ag->chain_next = true;
    return 1;
}
int32_t rlrep_prefetch_policy_early(rlrep_agent* ag, const float* eps_critic, const float* eps_actor) {
    GROUP_REFUSE("prefetch_policy_early")
    if (!ag) { rl_set_error("null agent"); return RLREP_ERR_ARG; }
    ag->early_crit = ag->early_act = nullptr;
    if (!eps_critic || !eps_actor || ag->feat_bwd_h.stages.empty() || ag->critic_bwd_h2.stages.empty()) return 0;
    ag->early_crit = eps_critic; ag->early_act = eps_actor;
    return 1;
}
int32_t rlrep_prefetch_policy(rlrep_agent* ag, const float* eps_actor) {
    if (!ag) { rl_set_error("null agent"); return RLREP_ERR_ARG; }
    ag->hoist_req = nullptr;
    if (!eps_actor || ag->critic_bwd_h.stages.empty()) return 0;      // not supported for this agent / shape: nothing armed
    ag->hoist_req = eps_actor;
    return 1;
}
// The critic step's backward half, shared by rlrep_critic_backward (w == nullptr) and rlrep_critic_step_weighted (w = per-sample weights, sac
// only: the program pair whose head stage is the weighted kernel, per.hip): one dispatch, so the two cannot drift apart.
int critic_backward_dispatch(rlrep_agent* ag, const float* eps, const float* w, void* stream) {
    STEP_PROLOGUE(false)
    if (!eps) { rl_set_error("critic step needs eps[B,A]"); return RLREP_ERR_ARG; }
    // rlrep_critic_weights_arm (never sac): this backward is the weighted one, whichever of the agent's programs it takes -- their head stage
    // looks at cur_w when it launches (critic_head_launch) -- and it disarms
    const bool armed = !w && ag->arm_w;
    if (armed) { w = ag->arm_w; ag->cur_td = ag->arm_td; }
    ag->arm_w = nullptr; ag->arm_td = nullptr;
    struct Disarm { rlrep_agent* a; ~Disarm() { a->cur_w = nullptr; a->cur_td = nullptr; } } disarm_{ag};      // (a deferred chain's head must find none)
    ag->cur_eps = eps; ag->cur_w = w; ag->last_launches = 0;
    ag->pi_ready = nullptr;
    // the images of critic.l1 / l4 and of their targets, from the tensors as they are now: the target copies have no other writer, and a
    // caller may have written any of them since the last step (the launch rides on the chain that has slack in the pipelined train())
    if (!ag->images_managed) { const int rs = refresh_x3(ag, stream); if (rs) return rs; }
    if ((!w || armed) && ag->early_ready_crit && ag->early_ready_crit == eps) {      // both policy forwards already ran (last feature step; never for sac)
        const float* act_eps = ag->early_ready_act;
        ag->early_ready_crit = ag->early_ready_act = nullptr; ag->hoist_req = nullptr;
        const int rc = run(ag, ag->critic_bwd_h2, stream);
        if (rc == 0) ag->pi_ready = act_eps;
        return rc;
    }
    ag->early_ready_crit = ag->early_ready_act = nullptr;
    const bool own = w && !armed;             // sac's weighted programs (rlrep_critic_step_weighted); an armed step runs the agent's own
    const Program& hoisted = own ? ag->critic_bwd_wh : ag->critic_bwd_h;
    if (ag->hoist_req && !hoisted.stages.empty()) {
        ag->cur_eps2 = ag->hoist_req; ag->hoist_req = nullptr;
        const int rc = run(ag, hoisted, stream);
        if (rc == 0) ag->pi_ready = ag->cur_eps2;
        return rc;
    }
    ag->hoist_req = nullptr;
    return run(ag, own ? ag->critic_bwd_w : ag->critic_bwd, stream);
}
int32_t rlrep_critic_backward(rlrep_agent* ag, const float* eps, void* stream) { return critic_backward_dispatch(ag, eps, nullptr, stream); }
int32_t rlrep_critic_apply(rlrep_agent* ag, void* stream) {
    STEP_PROLOGUE(false)
    if (ag->in_train && !ag->target_done && !ag->critic_apply_f.stages.empty()) {
        ag->target_done = true;
        return run(ag, ag->critic_apply_f, stream);
    }
    return run(ag, ag->critic_apply, stream);
}
int32_t rlrep_actor_backward(rlrep_agent* ag, const float* eps, void* stream) {
    STEP_PROLOGUE(false)
    if (!eps) { rl_set_error("actor step needs eps[B,A]"); return RLREP_ERR_ARG; }
    ag->cur_eps = eps; ag->last_launches = 0;
    // resume after the forward half iff the critic step of this train() ran it with exactly this noise
    const size_t first = (ag->pi_ready && ag->pi_ready == eps) ? (size_t)ag->actor_resume : 0;
    ag->pi_ready = nullptr;
    if (!ag->slot[0].filled) { rl_set_error("step before set_batch / replay_sample"); return RLREP_ERR_STATE; }
    if (!ag->in_train && !ag->images_managed) { const int rs = refresh_x3(ag, stream); if (rs) return rs; }        // (inside a train() the critic's Adam launch kept the live images current)
    ag->last_launches += (int)(ag->actor_bwd.stages.size() - first);
    return ag->actor_bwd.run((hipStream_t)stream, first);
}
int32_t rlrep_actor_apply(rlrep_agent* ag, void* stream) { STEP_PROLOGUE(false) return run(ag, ag->actor_apply, stream); }

int32_t rlrep_feature_step(rlrep_agent* ag, const float* eps, const int32_t* idx, void* stream) {
    int rc = rlrep_feature_backward(ag, eps, idx, stream);
    return rc ? rc : rlrep_feature_apply(ag, stream);
}
int32_t rlrep_critic_step(rlrep_agent* ag, const float* eps, void* stream) {
    int rc = rlrep_critic_backward(ag, eps, stream);
    return rc ? rc : rlrep_critic_apply(ag, stream);
}
// ---- prioritized replay (per.hip) -------------------------------------------------------------------------------------
bool per_tree_ok(const char* what, const float* tree, int64_t P, const float* scal) {
    if (!tree || !scal || P < 1 || P > (1ll << 30) || (P & (P - 1)) != 0) { rl_set_error("%s: bad argument (null tree / scalars, or P %lld is not a power of two in [1, 2^30])", what, (long long)P); return false; }
    return true;
}
// the entry points that work for ONE sac agent on ONE GPU
static int per_agent_ok(const char* what, const rlrep_agent* ag) {
    if (!ag) { rl_set_error("%s: null agent", what); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("%s: not available on a seed group (rlrep_group_create): prioritized replay is built for one sac agent", what); return RLREP_ERR_ARG; }
    if (ag->d.alg != RLREP_ALG_SAC) { rl_set_error("%s: prioritized replay is built for sac only (the representation agents reuse their last feature minibatch)", what); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("%s: prioritized replay runs on one GPU (world_size = %d)", what, ag->h.world_size); return RLREP_ERR_ARG; }
    return 0;
}
int32_t rlrep_per_add(float* tree_dev, int64_t P, const float* scal_dev, int64_t capacity, int64_t start, int64_t n, void* stream) {
    if (!per_tree_ok("per_add", tree_dev, P, scal_dev)) return RLREP_ERR_ARG;
    if (capacity < 1 || capacity > P || start < 0 || start >= capacity || n < 1 || n > capacity) {
        rl_set_error("per_add: rows [%lld, +%lld) of a ring of %lld rows (tree of %lld leaves)", (long long)start, (long long)n, (long long)capacity, (long long)P); return RLREP_ERR_ARG;
    }
    PerAdd p; memset(&p, 0, sizeof(p));
    p.tree = tree_dev; p.scal = scal_dev; p.P = P; p.capacity = capacity; p.start = start; p.n = n;
    const int rc = (++g_rl_launches, rl_launch_per_add(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("per_add: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_per_rebuild(float* tree_dev, int64_t P, void* stream) {
    if (!per_tree_ok("per_rebuild", tree_dev, P, tree_dev)) return RLREP_ERR_ARG;
    const int rc = (++g_rl_launches, rl_launch_per_rebuild(tree_dev, P, (hipStream_t)stream));
    if (rc) { rl_set_error("per_rebuild: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
int32_t rlrep_per_sample(rlrep_agent* ag, const float* tree_dev, int64_t P, const float* scal_dev, int32_t* idx_dev, float* w_dev, int32_t batch, int32_t given,
                         uint64_t seed, uint64_t offset, const int32_t* counter_dev, void* stream) {
    if (int rc = per_agent_ok("per_sample", ag)) return rc;
    if (!per_tree_ok("per_sample", tree_dev, P, scal_dev)) return RLREP_ERR_ARG;
    if (!idx_dev || !w_dev || batch < 1) { rl_set_error("per_sample: bad argument (null idx / w, or batch %d)", batch); return RLREP_ERR_ARG; }
    PerSample p; memset(&p, 0, sizeof(p));
    p.tree = tree_dev; p.scal = scal_dev; p.idx = idx_dev; p.w = w_dev; p.P = P; p.B = batch; p.given = given ? 1 : 0;
    p.seed = seed; p.offset = offset; p.step_dev = counter_dev;
    const int rc = (++g_rl_launches, rl_launch_per_sample(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("per_sample: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
const float* rlrep_per_td_dev(rlrep_agent* ag) { return (ag && ag->members == 0 && ag->d.alg == RLREP_ALG_SAC) ? ag->per_td : nullptr; }
int32_t rlrep_per_update(rlrep_agent* ag, float* tree_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch, void* stream) {
    if (int rc = per_agent_ok("per_update", ag)) return rc;
    if (!per_tree_ok("per_update", tree_dev, P, scal_dev)) return RLREP_ERR_ARG;
    if (!idx_dev || batch < 1 || (!td_dev && batch != ag->B)) { rl_set_error("per_update: bad argument (null idx, or batch %d is not the batch of the last weighted critic step)", batch); return RLREP_ERR_ARG; }
    PerUpdate p; memset(&p, 0, sizeof(p));
    p.tree = tree_dev; p.scal = scal_dev; p.idx = idx_dev; p.td = td_dev ? td_dev : ag->per_td; p.P = P; p.B = batch;
    if (!p.td) { rl_set_error("per_update: no weighted critic step has run"); return RLREP_ERR_STATE; }
    const int rc = (++g_rl_launches, rl_launch_per_update(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("per_update: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// rlrep_critic_step with per-sample weights w[B]: the same launches, the head stage replaced by the weighted kernel, which also leaves
// td[b] = 0.5 (|q1 - y| + |q2 - y|) in the agent's workspace (rlrep_per_td_dev) for rlrep_per_update
int32_t rlrep_critic_step_weighted(rlrep_agent* ag, const float* eps, const float* w, void* stream) {
    if (int rc = per_agent_ok("critic_step_weighted", ag)) return rc;
    if (!eps || !w) { rl_set_error("critic_step_weighted: needs eps[B,A] and w[B]"); return RLREP_ERR_ARG; }
    if (ag->critic_bwd_w.stages.empty()) { rl_set_error("critic_step_weighted: no weighted critic program was built for this agent"); return RLREP_ERR_STATE; }
    const int rc = critic_backward_dispatch(ag, eps, w, stream);
    return rc ? rc : rlrep_critic_apply(ag, stream);
}

// ---- prioritized replay of the critic's minibatch for vlsac / ctrlsac / spedersac / diffsrsac (per.hip) ------------
// the entry points that work for ONE representation agent on ONE GPU
static int cper_agent_ok(const char* what, const rlrep_agent* ag) {
    if (!ag) { rl_set_error("%s: null agent", what); return RLREP_ERR_ARG; }
    if (ag->members > 0) { rl_set_error("%s: not available on a seed group (rlrep_group_create): prioritized critic replay is built for one agent", what); return RLREP_ERR_ARG; }
    if (ag->d.alg == RLREP_ALG_SAC) { rl_set_error("%s: a sac agent owns its whole minibatch: use rlrep_per_sample / rlrep_critic_step_weighted", what); return RLREP_ERR_ARG; }
    if (ag->h.world_size > 1) { rl_set_error("%s: prioritized critic replay runs on one GPU (world_size = %d)", what, ag->h.world_size); return RLREP_ERR_ARG; }
    return 0;
}
// rlrep_per_sample and rlrep_replay_sample(slot 0) of the drawn rows in ONE launch.  Never skipped: it overwrites whatever gather the train
// prologue or an optimizer launch ran.
int32_t rlrep_per_sample_fill(rlrep_agent* ag, const float* ring_dev, int64_t capacity, const float* tree_dev, int64_t P, const float* scal_dev, int32_t* idx_dev,
                              float* w_dev, int32_t batch, int32_t given, uint64_t seed, uint64_t offset, const int32_t* counter_dev, void* stream) {
    if (int rc = cper_agent_ok("per_sample_fill", ag)) return rc;
    if (!per_tree_ok("per_sample_fill", tree_dev, P, scal_dev)) return RLREP_ERR_ARG;
    if (!ring_dev || !idx_dev || !w_dev || batch < 1) { rl_set_error("per_sample_fill: bad argument (null ring / idx / w, or batch %d)", batch); return RLREP_ERR_ARG; }
    if (capacity < 1 || capacity > P) { rl_set_error("per_sample_fill: a ring of %lld rows under a tree of %lld leaves", (long long)capacity, (long long)P); return RLREP_ERR_ARG; }
    // a new batch: what rlrep_replay_sample invalidates
    ag->pf_done = false; ag->l1_done = false; ag->chain_next = false;
    ag->pi_ready = nullptr; ag->hoist_req = nullptr;
    ag->early_crit = ag->early_act = ag->early_ready_crit = ag->early_ready_act = nullptr;
    int rc = ensure_batch(ag, batch);
    if (rc) return rc;
    PerSampleFill p; memset(&p, 0, sizeof(p));
    p.s.tree = tree_dev; p.s.scal = scal_dev; p.s.idx = idx_dev; p.s.w = w_dev; p.s.P = P; p.s.B = batch; p.s.given = given ? 1 : 0;
    p.s.seed = seed; p.s.offset = offset; p.s.step_dev = counter_dev;
    slot_fill_params(ag, 0, ring_dev, nullptr, p.f);
    p.capacity = capacity;
    ag->slot[0].filled = true;
    rc = (++g_rl_launches, rl_launch_per_sample_fill(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("per_sample_fill: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}
// The next rlrep_critic_step / rlrep_critic_backward is the weighted one: w[B] in the loss, td[b] = 0.5 (|q1 - y| + |q2 - y|) into the
// caller's td_dev.  That step disarms; so does passing null.
int32_t rlrep_critic_weights_arm(rlrep_agent* ag, const float* w_dev, float* td_dev) {
    if (int rc = cper_agent_ok("critic_weights_arm", ag)) return rc;
    if ((w_dev == nullptr) != (td_dev == nullptr)) { rl_set_error("critic_weights_arm: needs w[B] and td[B] (or neither, to disarm)"); return RLREP_ERR_ARG; }
    ag->arm_w = w_dev; ag->arm_td = td_dev;
    return w_dev ? 1 : 0;
}
// rlrep_per_update with the caller's |TD| array and no agent (as rlrep_per_add has none)
int32_t rlrep_per_update_td(float* tree_dev, int64_t P, float* scal_dev, const int32_t* idx_dev, const float* td_dev, int32_t batch, void* stream) {
    if (!per_tree_ok("per_update_td", tree_dev, P, scal_dev)) return RLREP_ERR_ARG;
    if (!idx_dev || !td_dev || batch < 1) { rl_set_error("per_update_td: bad argument (null idx / td, or batch %d)", batch); return RLREP_ERR_ARG; }
    PerUpdate p; memset(&p, 0, sizeof(p));
    p.tree = tree_dev; p.scal = scal_dev; p.idx = idx_dev; p.td = td_dev; p.P = P; p.B = batch;
    const int rc = (++g_rl_launches, rl_launch_per_update(&p, (hipStream_t)stream));
    if (rc) { rl_set_error("per_update_td: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

int32_t rlrep_actor_alpha_step(rlrep_agent* ag, const float* eps, void* stream) {
    int rc = rlrep_actor_backward(ag, eps, stream);
    return rc ? rc : rlrep_actor_apply(ag, stream);
}
int32_t rlrep_update_target(rlrep_agent* ag, void* stream) {
    if (!ag) return RLREP_ERR_ARG;
    GrpScope grp_scope_(ag);
    const bool done = ag->target_done;
    ag->in_train = ag->target_done = false;
    if (done) return 0;                                  // already folded into this train()'s critic Adam launch
    ag->last_launches += (int)ag->upd_target.stages.size();
    return ag->upd_target.run((hipStream_t)stream);
}
int32_t rlrep_begin_train(rlrep_agent* ag, void* stream) {
    if (!ag) return RLREP_ERR_ARG;
    GrpScope grp_scope_(ag);
    int rc = (++g_rl_launches, rl_launch_counter_inc(ag->steps, 2, (hipStream_t)stream));
    if (rc) { rl_set_error("begin_train: hip error %d", rc); return RLREP_ERR_HIP; }
    if (ag->has_shadows() && (rc = refresh_shadows(ag, stream)) != 0) return rc;
    ag->in_train = true; ag->target_done = false;
    return 0;
}
int32_t rlrep_defer_supported(rlrep_agent* ag) {
    if (!ag) return 0;
    int n = 0;
    for (int k = 0; k < rlrep_agent::NSETS; ++k) if (!ag->dset[k].critic_bwd.stages.empty() && !ag->dset[k].actor_bwd.stages.empty()) ++n;
    return n == rlrep_agent::NSETS ? n : 0;
}
// Arm the folded snapshot: the NEXT feature optimizer launch (rlrep_feature_apply) also writes snapshot set `set` -- the minibatch slices
// and the two noise blocks by extra blocks, the f_target (or live f) block by the lanes that produce its new values -- and the
// rlrep_defer_snapshot that follows with the same arguments launches nothing.  To be called before the LAST feature step of a train().
// Returns 1 if armed, 0 if this agent / configuration has no folded form (the caller proceeds as before).
int32_t rlrep_defer_arm(rlrep_agent* ag, int32_t set, const float* eps_critic, const float* eps_actor) {
    GROUP_REFUSE("defer_arm")
    if (!ag || set < 0 || set >= rlrep_agent::NSETS) return 0;
    ag->snap_armed = false; ag->snap_done = -1;
    if (!eps_critic || !eps_actor || !rlrep_defer_supported(ag) || ag->dset[set].block_which < 0 || !ag->dset[set].block) return 0;
    if (!ag->sync_prog.stages.empty()) return 0;
    ag->snap_armed = true; ag->snap_set = set; ag->snap_ec = eps_critic; ag->snap_ea = eps_actor;
    return 1;
}
int32_t rlrep_defer_snapshot(rlrep_agent* ag, int32_t set, const float* eps_critic, const float* eps_actor, void* stream) {
    GROUP_REFUSE("defer_snapshot")
    if (!ag || !eps_critic || !eps_actor || set < 0 || set >= rlrep_agent::NSETS) { rl_set_error("defer_snapshot: bad argument"); return RLREP_ERR_ARG; }
    if (!rlrep_defer_supported(ag)) { rl_set_error("deferred critic/actor steps are not built for this agent"); return RLREP_ERR_STATE; }
    if (!ag->slot[0].filled) { rl_set_error("defer_snapshot before set_batch / replay_sample"); return RLREP_ERR_STATE; }
    if (!ag->sync_prog.stages.empty()) {          // ctrlsac: frozen_phi, frozen_phi_target <- phi (ctrlsac_agent.py:344-346) belongs to the end of the feature steps
        const int rs = ag->sync_prog.run((hipStream_t)stream);
        if (rs) return rs;
    }
    if (ag->snap_done == set && ag->snap_ec == eps_critic && ag->snap_ea == eps_actor) {      // the last feature optimizer launch already wrote this set
        ag->snap_done = -1; ag->snap_armed = false;
        ag->dset[set].valid = true;
        return 0;
    }
    ag->snap_done = -1; ag->snap_armed = false;
    CopySegs cs = ag->dset[set].segs;
    cs.src[cs.n - 2] = eps_critic; cs.src[cs.n - 1] = eps_actor;
    const int rc = (++g_rl_launches, rl_launch_copy_segs(&cs, (hipStream_t)stream));
    if (rc) { rl_set_error("defer_snapshot: hip error %d", rc); return RLREP_ERR_HIP; }
    ag->dset[set].valid = true;
    return 0;
}
// part: 0 critic backward, 1 critic apply (+ period-gated critic-target Polyak), 2 actor backward, 3 actor + temperature apply; -1 all.
// Data parallel callers all-reduce the critic / actor gradient slices between 0 and 1 and between 2 and 3.
int32_t rlrep_deferred_part(rlrep_agent* ag, int32_t set, int32_t part, void* stream) {
    GROUP_REFUSE("deferred_part")
    if (!ag || set < 0 || set >= rlrep_agent::NSETS || part < -1 || part > 3 || !rlrep_defer_supported(ag)) { rl_set_error("deferred critic/actor steps are not built for this agent"); return RLREP_ERR_STATE; }
    rlrep_agent::DeferSet& D = ag->dset[set];
    if (!D.valid) { rl_set_error("deferred critic/actor steps before rlrep_defer_snapshot of this set"); return RLREP_ERR_STATE; }
    const float* e_crit = D.eps; const float* e_act = D.eps + (size_t)ag->B * ag->d.action_dim;
    const float* keep1 = ag->cur_eps; const float* keep2 = ag->cur_eps2;
    int rc = 0;
    if (part == -1 || part == 0) {
        ag->cur_eps = e_crit; ag->cur_eps2 = e_act; ag->last_launches = 0;
        if (!ag->images_managed) rc = refresh_x3(ag, stream);                 // as in rlrep_critic_backward
        if (!rc) rc = run(ag, D.critic_bwd, stream);
    }
    if (!rc && (part == -1 || part == 1)) rc = run(ag, D.critic_apply, stream);
    if (!rc && (part == -1 || part == 2)) {
        ag->cur_eps = e_act;
        ag->last_launches += (int)(D.actor_bwd.stages.size() - D.actor_resume);
        rc = D.actor_bwd.run((hipStream_t)stream, (size_t)D.actor_resume);
    }
    if (!rc && (part == -1 || part == 3)) rc = run(ag, ag->actor_apply, stream);
    ag->cur_eps = keep1; ag->cur_eps2 = keep2;
    return rc;
}
int32_t rlrep_deferred_critic_actor(rlrep_agent* ag, int32_t set, void* stream) { return rlrep_deferred_part(ag, set, -1, stream); }
// Weight images of the vlsac noise critic (bf16x3).  By default every critic step regenerates them from the tensors with a launch
// of its own (a caller may have written parameters; the target copies have no other writer outside a train()).  A caller that replays
// captured train() graphs can take that launch off the chain: between rlrep_images_managed(agent, 1) and (agent, 0) the step entry points do
// NOT launch it -- inside a train() bracket the critic group's optimizer launch keeps the live AND (with the folded Polyak) the target images
// current -- and the caller runs rlrep_refresh_images itself whenever anything else may have written critic / critic_target (an eager step
// method, rlrep_update_target outside a bracket, a torch write into the arenas).  Returns 1 if the agent keeps such images (else 0: nothing to manage).
int32_t rlrep_images_managed(rlrep_agent* ag, int32_t on) {
    if (!ag) { rl_set_error("null agent"); return RLREP_ERR_ARG; }
    if (!ag->x3_n || ag->critic_apply_f.stages.empty()) { ag->images_managed = false; return 0; }
    ag->images_managed = on != 0;
    return 1;
}
int32_t rlrep_refresh_images(rlrep_agent* ag, void* stream) {
    GROUP_REFUSE("refresh_images")
    if (!ag) { rl_set_error("null agent"); return RLREP_ERR_ARG; }
    return refresh_x3(ag, stream);
}
int32_t rlrep_end_train(rlrep_agent* ag) {
    if (!ag) return RLREP_ERR_ARG;
    ag->in_train = ag->target_done = false;
    return 0;
}
int32_t rlrep_feature_exchange_count(rlrep_agent* ag) { return ag ? (int32_t)ag->feat_cuts.size() : RLREP_ERR_ARG; }
int32_t rlrep_feature_exchange(rlrep_agent* ag, int32_t k, int32_t* kind, float** ptr, int64_t* count, int64_t* local_off) {
    if (!ag || k < 0 || k >= (int)ag->feat_cuts.size() || !kind || !ptr || !count || !local_off) { rl_set_error("feature_exchange: bad argument"); return RLREP_ERR_ARG; }
    const Exchange& e = ag->feat_cuts[k];
    *kind = e.kind; *ptr = e.ptr; *count = e.count; *local_off = e.local_off;
    return 0;
}
int32_t rlrep_feature_backward_part(rlrep_agent* ag, int32_t part, const float* eps, const int32_t* idx, void* stream) {
    STEP_PROLOGUE(true)
    const int ncut = (int)ag->feat_cuts.size();
    if (part < 0 || part > ncut) { rl_set_error("feature_backward_part: part %d of %d", part, ncut + 1); return RLREP_ERR_ARG; }
    if (!ag->slot[0].filled) { rl_set_error("step before set_batch / replay_sample"); return RLREP_ERR_STATE; }
    ag->cur_eps = eps; ag->cur_idx = idx; ag->pi_ready = nullptr;
    const int lo = part == 0 ? 0 : ag->feat_cuts[part - 1].after_stage + 1;
    const int hi = part == ncut ? (int)ag->feat_bwd.stages.size() : ag->feat_cuts[part].after_stage + 1;
    if (part == 0) ag->last_launches = 0;
    for (int i = lo; i < hi; ++i) {
        int rc = ag->feat_bwd.stages[i].run((hipStream_t)stream); ++g_rl_launches;
        if (rc) { rl_set_error("stage '%s' failed: hip error %d", ag->feat_bwd.stages[i].what, rc); return RLREP_ERR_HIP; }
    }
    ag->last_launches += hi - lo;
    return 0;
}

int32_t rlrep_sync_frozen(rlrep_agent* ag, void* stream) {
    if (!ag) return RLREP_ERR_ARG;
    GrpScope grp_scope_(ag);                   // (a seed group: every member's copy, in one launch)
    ag->last_launches += (int)ag->sync_prog.stages.size();
    return ag->sync_prog.run((hipStream_t)stream);
}

int32_t rlrep_actor_forward(rlrep_agent* ag, const float* obs, int32_t n, const float* eps, float lo, float hi, float* action, void* stream) {
    GROUP_REFUSE("actor_forward")
    if (!ag || !obs || !action || n <= 0 || n > ag->d.max_batch) { rl_set_error("actor_forward: bad argument"); return RLREP_ERR_ARG; }
    const int S = ag->d.state_dim, A = ag->d.action_dim, Ha = ag->d.actor_hidden_dim;
    hipStream_t st = (hipStream_t)stream;
    if (ag->infer_n != n) {
        (void)hipDeviceSynchronize();
        ag->infer.stages.clear();
        // inference scratch lives behind the step programs' buffers
        ag->ws.used = ag->prog_end;
        Builder b(ag);
        float* A1 = b.ws.f((size_t)n * Ha); float* A2 = b.ws.f((size_t)n * Ha); float* AO = b.ws.f((size_t)n * 2 * A);
        b.fwd_stage(ag->infer, {Builder::fwd(ag->obs_in, S, n, S, ag->P("actor.trunk.0.weight"), S, ag->P("actor.trunk.0.bias"), Ha, A1, Ha, ACT_ELU)}, "infer l1");
        b.fwd_stage(ag->infer, {Builder::fwd(A1, Ha, n, Ha, ag->P("actor.trunk.2.weight"), Ha, ag->P("actor.trunk.2.bias"), Ha, A2, Ha, ACT_ELU)}, "infer l2");
        b.fwd_stage(ag->infer, {Builder::fwd(A2, Ha, n, Ha, ag->P("actor.trunk.4.weight"), Ha, ag->P("actor.trunk.4.bias"), 2 * A, AO, 2 * A, ACT_NONE)}, "infer head");
        PolicyFwd pf; memset(&pf, 0, sizeof(pf));
        pf.O = AO; pf.B = n; pf.A = A; pf.act = ag->act_out; pf.ld_act = A; pf.logp = nullptr; pf.clamp = 1;
        rlrep_agent* a2 = ag;
        ag->infer.stages.push_back({[=](hipStream_t s2) { PolicyFwd q = pf; q.eps = a2->cur_eps; q.lo = a2->infer_lo; q.hi = a2->infer_hi; return rl_launch_policy_fwd(&q, s2); }, "infer policy"});
        if (!ag->ws.ok()) { ag->ws.used = ag->prog_end; ag->infer.stages.clear(); rl_set_error("workspace too small for inference"); return RLREP_ERR_NOMEM; }
        ag->infer_n = n;
    }
    int rc = rl_launch_copy(obs, ag->obs_in, (long long)n * S, st);
    if (rc) { rl_set_error("actor_forward copy-in: hip error %d", rc); return RLREP_ERR_HIP; }
    ag->cur_eps = eps; ag->infer_lo = lo; ag->infer_hi = hi;
    rc = ag->infer.run(st);
    if (rc) return rc;
    rc = rl_launch_copy(ag->act_out, action, (long long)n * A, st);
    if (rc) { rl_set_error("actor_forward copy-out: hip error %d", rc); return RLREP_ERR_HIP; }
    return 0;
}

// One observation -> one action in ONE launch.  obs / action: device pointers, or pinned (mapped) host buffers -- resolved here with
// hipHostGetDevicePointer, so that the kernel reads the observation and writes the action in place and no copy launch stands on either side.
int32_t rlrep_select_action(rlrep_agent* ag, const float* obs, int32_t obs_on_host, int32_t explore, uint64_t seed, uint64_t offset,
                            float lo, float hi, float* action, int32_t action_on_host, void* stream) {
    GROUP_REFUSE("select_action")
    if (!ag || !obs || !action) { rl_set_error("select_action: bad argument"); return RLREP_ERR_ARG; }
    SelectAct p; memset(&p, 0, sizeof(p));
    void* d = nullptr;
    if (obs_on_host) { if (hipHostGetDevicePointer(&d, const_cast<float*>(obs), 0) != hipSuccess || !d) { rl_set_error("select_action: the observation buffer is not mapped (pinned) host memory"); return RLREP_ERR_ARG; } p.obs = (const float*)d; }
    else p.obs = obs;
    if (action_on_host) { if (hipHostGetDevicePointer(&d, action, 0) != hipSuccess || !d) { rl_set_error("select_action: the action buffer is not mapped (pinned) host memory"); return RLREP_ERR_ARG; } p.act = (float*)d; }
    else p.act = action;
    p.W1 = ag->P("actor.trunk.0.weight"); p.b1 = ag->P("actor.trunk.0.bias"); p.W2 = ag->P("actor.trunk.2.weight"); p.b2 = ag->P("actor.trunk.2.bias");
    p.W3 = ag->P("actor.trunk.4.weight"); p.b3 = ag->P("actor.trunk.4.bias");
    p.S = ag->d.state_dim; p.Ha = ag->d.actor_hidden_dim; p.A = ag->d.action_dim; p.explore = explore ? 1 : 0; p.lo = lo; p.hi = hi; p.seed = seed; p.offset = offset;
    ++g_rl_launches;
    const int rc = rl_launch_select_action(&p, (hipStream_t)stream);
    if (rc) { rl_set_error("select_action: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}

// `rows` observations -> `rows` actions in ONE launch (select_action_kernel_n: one workgroup per row).  Everything is refused before the launch;
// rlrep_select_action and its launcher stay as they are.
int32_t rlrep_select_action_n(rlrep_agent* ag, const float* obs, int32_t obs_on_host, int32_t rows, int32_t explore, uint64_t seed, uint64_t offset,
                              float lo, float hi, float* action, int32_t action_on_host, void* stream) {
    if (!ag || !obs || !action) { rl_set_error("select_action_n: bad argument (null agent, observations or actions)"); return RLREP_ERR_ARG; }
    if (rows < 1 || rows > RLREP_SELECT_MAX_ROWS) { rl_set_error("select_action_n: rows %d outside [1, %d]", rows, RLREP_SELECT_MAX_ROWS); return RLREP_ERR_ARG; }
    GROUP_REFUSE("select_action_n")
    SelectAct p; memset(&p, 0, sizeof(p));
    void* d = nullptr;
    if (obs_on_host) { if (hipHostGetDevicePointer(&d, const_cast<float*>(obs), 0) != hipSuccess || !d) { (void)hipGetLastError(); rl_set_error("select_action_n: the observation buffer is not mapped (pinned) host memory"); return RLREP_ERR_ARG; } p.obs = (const float*)d; }
    else p.obs = obs;
    if (action_on_host) { if (hipHostGetDevicePointer(&d, action, 0) != hipSuccess || !d) { (void)hipGetLastError(); rl_set_error("select_action_n: the action buffer is not mapped (pinned) host memory"); return RLREP_ERR_ARG; } p.act = (float*)d; }
    else p.act = action;
    p.W1 = ag->P("actor.trunk.0.weight"); p.b1 = ag->P("actor.trunk.0.bias"); p.W2 = ag->P("actor.trunk.2.weight"); p.b2 = ag->P("actor.trunk.2.bias");
    p.W3 = ag->P("actor.trunk.4.weight"); p.b3 = ag->P("actor.trunk.4.bias");
    p.S = ag->d.state_dim; p.Ha = ag->d.actor_hidden_dim; p.A = ag->d.action_dim; p.explore = explore ? 1 : 0; p.lo = lo; p.hi = hi; p.seed = seed; p.offset = offset;
    ++g_rl_launches;
    const int rc = rl_launch_select_action_n(&p, rows, (hipStream_t)stream);
    if (rc) { rl_set_error("select_action_n: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}

// `rows` device-resident observations -> `rows` actions in ONE launch (actor_tile_kernel: 16 rows per workgroup share every weight they fetch).
// Stream-ordered: no copy, no allocation, no synchronisation, and nothing is rebuilt when `rows` changes.  What needs no handle is checked first.
int32_t rlrep_act_device(rlrep_agent* ag, const float* obs_dev, int64_t ld_obs, int32_t rows, int32_t explore, uint64_t seed, uint64_t offset,
                         float lo, float hi, float* action_dev, int64_t ld_act, void* stream) {
    if (!ag || !obs_dev || !action_dev) { rl_set_error("act_device: bad argument (null agent, observations or actions)"); return RLREP_ERR_ARG; }
    if (rows < 1 || rows > RLREP_ACT_MAX_ROWS) { rl_set_error("act_device: rows %d outside [1, %d]", rows, RLREP_ACT_MAX_ROWS); return RLREP_ERR_ARG; }
    GROUP_REFUSE("act_device")
    const int S = ag->d.state_dim, Ha = ag->d.actor_hidden_dim, A = ag->d.action_dim;
    if (ld_obs < S || ld_act < A || ld_obs > INT32_MAX || ld_act > INT32_MAX) {
        rl_set_error("act_device: row strides (%lld, %lld) below the row widths (%d, %d)", (long long)ld_obs, (long long)ld_act, S, A); return RLREP_ERR_ARG;
    }
    if (rl_actor_tile_lds_bytes(S, Ha, A) > RL_ACT_TILE_LDS_MAX) {
        rl_set_error("act_device: the activation tiles of S %d, Ha %d, A %d need %lld bytes of LDS, a workgroup has %d", S, Ha, A, rl_actor_tile_lds_bytes(S, Ha, A), RL_ACT_TILE_LDS_MAX);
        return RLREP_ERR_ARG;
    }
    ActTile p; memset(&p, 0, sizeof(p));
    p.obs = obs_dev; p.act = action_dev;
    p.W1 = ag->P("actor.trunk.0.weight"); p.b1 = ag->P("actor.trunk.0.bias"); p.W2 = ag->P("actor.trunk.2.weight"); p.b2 = ag->P("actor.trunk.2.bias");
    p.W3 = ag->P("actor.trunk.4.weight"); p.b3 = ag->P("actor.trunk.4.bias");
    p.S = S; p.Ha = Ha; p.A = A; p.explore = explore ? 1 : 0; p.lo = lo; p.hi = hi; p.seed = seed; p.offset = offset;
    p.rows = rows; p.ld_obs = (int)ld_obs; p.ld_act = (int)ld_act;
    ++g_rl_launches;
    const int rc = rl_launch_actor_tile(&p, (hipStream_t)stream);
    if (rc) { rl_set_error("act_device: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}

// rlrep_act_device(explore = 1) with the call counter read from the loop record on the device, the exploration mix behind the head and the
// ring cursor moved by `rows` (actor_tile_kernel_ctl): ONE launch, capturable -- nothing that changes between two replays rides by value
int32_t rlrep_act_device_ctl(rlrep_agent* ag, const float* obs_dev, int64_t ld_obs, int32_t rows, uint64_t seed, float lo, float hi, float* action_dev,
                             int64_t ld_act, int64_t* ctl_dev, int64_t max_size, float eps_greedy, int64_t start_timesteps, void* stream) {
    if (!ag || !obs_dev || !action_dev || !ctl_dev) { rl_set_error("act_device_ctl: bad argument (null agent, observations, actions or loop record)"); return RLREP_ERR_ARG; }
    if (rows < 1 || rows > RLREP_ACT_MAX_ROWS) { rl_set_error("act_device_ctl: rows %d outside [1, %d]", rows, RLREP_ACT_MAX_ROWS); return RLREP_ERR_ARG; }
    GROUP_REFUSE("act_device_ctl")
    const int S = ag->d.state_dim, Ha = ag->d.actor_hidden_dim, A = ag->d.action_dim;
    if (ld_obs < S || ld_act < A || ld_obs > INT32_MAX || ld_act > INT32_MAX) {
        rl_set_error("act_device_ctl: row strides (%lld, %lld) below the row widths (%d, %d)", (long long)ld_obs, (long long)ld_act, S, A); return RLREP_ERR_ARG;
    }
    if (max_size < rows) { rl_set_error("act_device_ctl: rows %d outside [1, max_size %lld] (the ring the cursor moves in)", rows, (long long)max_size); return RLREP_ERR_ARG; }
    if (!(eps_greedy >= 0.f && eps_greedy <= 1.f) || start_timesteps < 0) {
        rl_set_error("act_device_ctl: bad argument (eps_greedy outside [0, 1] or a negative start_timesteps)"); return RLREP_ERR_ARG;
    }
    if (rl_actor_tile_lds_bytes(S, Ha, A) > RL_ACT_TILE_LDS_MAX) {
        rl_set_error("act_device_ctl: the activation tiles of S %d, Ha %d, A %d need %lld bytes of LDS, a workgroup has %d", S, Ha, A, rl_actor_tile_lds_bytes(S, Ha, A), RL_ACT_TILE_LDS_MAX);
        return RLREP_ERR_ARG;
    }
    ActTile p; memset(&p, 0, sizeof(p));
    p.obs = obs_dev; p.act = action_dev;
    p.W1 = ag->P("actor.trunk.0.weight"); p.b1 = ag->P("actor.trunk.0.bias"); p.W2 = ag->P("actor.trunk.2.weight"); p.b2 = ag->P("actor.trunk.2.bias");
    p.W3 = ag->P("actor.trunk.4.weight"); p.b3 = ag->P("actor.trunk.4.bias");
    p.S = S; p.Ha = Ha; p.A = A; p.explore = 1; p.lo = lo; p.hi = hi; p.seed = seed;
    p.rows = rows; p.ld_obs = (int)ld_obs; p.ld_act = (int)ld_act;
    ActCtl k; memset(&k, 0, sizeof(k));
    k.ctl = (long long*)ctl_dev; k.capacity = max_size; k.start_timesteps = start_timesteps; k.eps_greedy = eps_greedy;
    ++g_rl_launches;
    const int rc = rl_launch_actor_tile_ctl(&p, &k, (hipStream_t)stream);
    if (rc) { rl_set_error("act_device_ctl: launch failed (%d)", rc); return rc == -7 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}

static Program* prog_of(rlrep_agent* ag, int id) {
    switch (id) {
    case 0: return &ag->feat_bwd; case 1: return &ag->feat_apply; case 2: return &ag->critic_bwd; case 3: return &ag->critic_apply;
    case 4: return &ag->actor_bwd; case 5: return &ag->actor_apply; case 6: return &ag->upd_target; case 7: return &ag->critic_bwd_h;
    case 8: return &ag->feat_bwd_h; case 9: return &ag->critic_bwd_h2;
    default: return nullptr;
    }
}
int32_t rlrep_stage_count(rlrep_agent* ag, int32_t program) {
    Program* p = ag ? prog_of(ag, program) : nullptr;
    return p ? (int32_t)p->stages.size() : RLREP_ERR_ARG;
}
const char* rlrep_stage_name(rlrep_agent* ag, int32_t program, int32_t stage) {
    Program* p = ag ? prog_of(ag, program) : nullptr;
    if (!p || stage < 0 || stage >= (int)p->stages.size()) return nullptr;
    return p->stages[stage].what;
}
int32_t rlrep_stage_info(rlrep_agent* ag, int32_t program, int32_t stage, int32_t* engine, double* flops, double* bytes) {
    Program* p = ag ? prog_of(ag, program) : nullptr;
    if (!p || stage < 0 || stage >= (int)p->stages.size()) { rl_set_error("stage_info: bad program/stage"); return RLREP_ERR_ARG; }
    const Stage& s = p->stages[stage];
    if (engine) *engine = s.engine;
    if (flops) *flops = s.flops;
    if (bytes) *bytes = s.bytes;
    return 0;
}
int32_t rlrep_run_stage(rlrep_agent* ag, int32_t program, int32_t stage, void* stream) {
    GROUP_REFUSE("run_stage")
    Program* p = ag ? prog_of(ag, program) : nullptr;
    if (!p || stage < 0 || stage >= (int)p->stages.size()) { rl_set_error("run_stage: bad program/stage"); return RLREP_ERR_ARG; }
    if (!ag->slot[0].filled) { rl_set_error("run_stage before a full step"); return RLREP_ERR_STATE; }
    int rc = p->stages[stage].run((hipStream_t)stream); ++g_rl_launches;
    if (rc) { rl_set_error("stage '%s' failed: hip error %d", p->stages[stage].what, rc); return RLREP_ERR_HIP; }
    return 0;
}

int32_t rlrep_gemm(int32_t engine, int32_t la, int32_t lb, const float* A, int32_t lda, const float* B, int32_t ldb,
                   float* Cm, int32_t ldc, int32_t R, int32_t Cn, int32_t K, int32_t epi, int32_t act, int32_t flags,
                   const float* bias, const float* aux, int32_t ldaux, float* out2, int32_t bt, int32_t splits,
                   float* wsp, int64_t ws_floats, void* stream) {
    rl_switches_read();
    if (!A || !B || !Cm || R <= 0 || Cn <= 0 || K <= 0 || (epi != EPI_FWD && epi != EPI_DX && epi != EPI_DW)) { rl_set_error("gemm: bad argument"); return RLREP_ERR_ARG; }
    GemmTask t; memset(&t, 0, sizeof(t));
    t.scale = 1.f; t.A = A; t.lda = lda; t.B = B; t.ldb = ldb; t.C = Cm; t.ldc = ldc; t.R = R; t.Cn = Cn; t.K = K;
    t.epi = epi; t.act = act; t.flags = flags & FLAG_ACCUM;
    if (epi == EPI_FWD) { t.bias = bias; t.out2 = out2; t.ldout2 = ldc; }
    if (epi == EPI_DX) { t.aux = aux; t.ldaux = ldaux; }
    if (epi == EPI_DW && (flags & FLAG_BIASGRAD) && out2) { t.flags |= FLAG_BIASGRAD; t.out2 = out2; }
    GemmBatch gb; memset(&gb, 0, sizeof(gb)); gb.ntasks = 1;
    int rc;
    if (engine == 0) {
        rl_gemm16_number_tiles(&t, 1, 1);
        gb.t[0] = t;
        rc = rl_launch_gemm16(la, lb, 1, &gb, t.ntiles, (hipStream_t)stream);
    } else {
        t.flags |= rl_gemm_lds_dim_flags(&t, la, lb) | rl_gemm_lds_ptr_flags(&t);
        // (the 64-wide bf16x3 tile has any-alignment loaders; the 128-wide one needs 16-byte-regular operands)
        if (engine == 2 && (t.flags & (FLAG_SCALAR_A | FLAG_SCALAR_B)) && (bt != 64 || !gl_x3s_unaligned_can_run(&t))) { rl_set_error("gemm: shape/alignment not eligible for the bf16x3 tile"); return RLREP_ERR_ARG; }
        if (engine == 2 && bt != 64 && bt != 32 && (t.flags & FLAG_SCALAR_C)) { rl_set_error("gemm: shape/alignment not eligible for the bf16x3 tile"); return RLREP_ERR_ARG; }
        int pbt = 0, psp = 1, pkc = 0;
        rl_gemm_lds_plan(&t, &pbt, &psp, &pkc);
        if (bt == 64 || bt == 128) pbt = bt;
        // bt names the tile: bf16x3 (engine 2) 32 / 64 / 256, anything else its 128-wide tile; fp32 MFMA 64 / 128, anything else the planner's width
        const GlKind kind = engine == 2 ? (bt == 32 ? GL_X3Q32 : bt == 64 ? GL_X3S64 : bt == 256 ? GL_X3W256 : GL_X3_128) : pbt == 64 ? GL_T64 : GL_T128;
        if (!GL_KINDS[kind].split_k) { psp = 1; pkc = K; }
        else if (splits > 0) { psp = splits; pkc = ((K + psp - 1) / psp + 31) / 32 * 32; psp = (K + pkc - 1) / pkc; }
        t.splits = psp; t.kchunk = pkc;
        // the 32 x 32 tile whose four waves split K (gemm_x3q.h): row-major A, K % 16 == 0, no slabs
        if (kind == GL_X3Q32 && !gl_x3q_can_run(&t, la, lb, t.flags, t.splits)) { rl_set_error("gemm: shape/alignment not eligible for the 32 x 32 bf16x3 tile"); return RLREP_ERR_ARG; }
        if (psp > 1) {
            if (!wsp || ws_floats < (int64_t)psp * R * (((Cn + 3) & ~3) + 1)) { rl_set_error("gemm: workspace too small for %d splits", psp); return RLREP_ERR_ARG; }
            t.slab = wsp; t.bslab = wsp + (size_t)psp * R * ((Cn + 3) & ~3);
            if ((flags & 4) && GL_KINDS[kind].fin_inline) {
                // flags & 4: the 64-wide bf16x3 tile finishes its split-K products inside the launch (FLAG_FIN_INLINE: one ticket word per output
                // tile behind the slabs, zero between launches) -- no finishing launch
                const size_t ticks = (size_t)((R + 63) / 64) * ((Cn + 63) / 64);
                if (ws_floats < (int64_t)psp * R * (((Cn + 3) & ~3) + 1) + (int64_t)ticks) { rl_set_error("gemm: workspace too small for %d splits", psp); return RLREP_ERR_ARG; }
                if (hipMemsetAsync(t.bslab, 0, ticks * sizeof(int), (hipStream_t)stream) != hipSuccess) return RLREP_ERR_HIP;
                t.bslab += ticks; t.flags |= FLAG_FIN_INLINE;
            }
        }
        if (kind == GL_X3W256 && (act == ACT_SIN || act == ACT_TANH)) { rl_set_error("gemm: the 256 x 128 tile has no sin / tanh epilogue"); return RLREP_ERR_ARG; }
        int fin = 0;
        const int total = gl_number_tiles(&t, 1, kind, &fin);
        gb.t[0] = t;
        rc = rl_launch_gemm_lds(kind, la, lb, &gb, total, fin, (hipStream_t)stream);
    }
    if (rc != 0) { rl_set_error("gemm: launch failed (%d)", rc); return rc < 0 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}

// Unit-test hook of the 16-row tile engine: a whole task TABLE through the launchers the step programs use, numbered by the builder's own helpers
// (engine_internal.h rl_gemm16_number_tiles*), so that tile widths, multi-task directories, the fast front ends and the duo form can be reached
// without an agent (tests/test_gemm16_engine.py).
int32_t rlrep_gemm16_table(int32_t la, int32_t lb, int32_t nf, const rlrep_gemm16_task* tasks, int32_t ntasks, int32_t duo_split, int32_t nf2,
                           int32_t low_prio, void* stream) {
    rl_switches_read();
    if (!tasks || ntasks < 1 || ntasks > GEMM_MAX_TASKS) { rl_set_error("gemm16_table: ntasks %d outside 1..%d", ntasks, GEMM_MAX_TASKS); return RLREP_ERR_ARG; }
    if (nf != 1 && nf != 2 && nf != 4) { rl_set_error("gemm16_table: nf %d not in {1, 2, 4}", nf); return RLREP_ERR_ARG; }
    if (duo_split < 0 || (duo_split > 0 && (duo_split >= ntasks || (nf2 != 1 && nf2 != 4)))) { rl_set_error("gemm16_table: bad duo split %d / nf2 %d", duo_split, nf2); return RLREP_ERR_ARG; }
    GemmBatch gb; memset(&gb, 0, sizeof(gb));
    gb.ntasks = ntasks; gb.low_prio = low_prio ? 1 : 0;
    for (int q = 0; q < ntasks; ++q) {
        const rlrep_gemm16_task& s = tasks[q];
        if (!s.a || !s.b || !s.c) { rl_set_error("gemm16_table: task %d has a null operand or output", q); return RLREP_ERR_ARG; }
        if (s.rows <= 0 || s.cols <= 0 || s.inner <= 0 || s.lda <= 0 || s.ldb <= 0 || s.ldc <= 0) { rl_set_error("gemm16_table: task %d has a non-positive extent", q); return RLREP_ERR_ARG; }
        if (s.epi != EPI_FWD && s.epi != EPI_DX && s.epi != EPI_DW) { rl_set_error("gemm16_table: task %d: epilogue %d not in {0, 1, 3}", q, s.epi); return RLREP_ERR_ARG; }
        if (s.act < ACT_NONE || s.act > ACT_TANH) { rl_set_error("gemm16_table: task %d: activation %d outside 0..4", q, s.act); return RLREP_ERR_ARG; }
        if ((s.r1u != nullptr) != (s.r1v != nullptr)) { rl_set_error("gemm16_table: task %d: the rank-1 term needs both vectors", q); return RLREP_ERR_ARG; }
        if (s.epi == EPI_FWD && s.act == ACT_SIN && !s.out2) { rl_set_error("gemm16_table: task %d: the sin epilogue stores its pre-activation to out2", q); return RLREP_ERR_ARG; }
        if (s.epi == EPI_DX && s.act != ACT_NONE && !s.aux) { rl_set_error("gemm16_table: task %d: dX with an activation needs aux", q); return RLREP_ERR_ARG; }
        GemmTask& t = gb.t[q];
        t.scale = s.scale; t.A = s.a; t.lda = s.lda; t.B = s.b; t.ldb = s.ldb; t.C = s.c; t.ldc = s.ldc; t.R = s.rows; t.Cn = s.cols; t.K = s.inner;
        t.epi = s.epi; t.act = s.act; t.flags = s.flags & FLAG_ACCUM;
        if (s.epi == EPI_FWD) { t.bias = s.bias; t.out2 = s.out2; t.ldout2 = s.ldc; }
        if (s.epi == EPI_DX) { t.aux = s.aux; t.ldaux = s.ldaux; t.r1u = s.r1u; t.r1v = s.r1v; }
        if (s.epi == EPI_DW && (s.flags & FLAG_BIASGRAD) && s.out2) { t.flags |= FLAG_BIASGRAD; t.out2 = s.out2; }
    }
    int rc;
    if (duo_split > 0) {
        const int total = rl_gemm16_number_tiles_duo(gb.t, duo_split, gb.t + duo_split, ntasks - duo_split, nf2);
        rc = rl_launch_gemm16_duo(duo_split, nf2, &gb, total, (hipStream_t)stream);
    } else {
        const int total = rl_gemm16_number_tiles(gb.t, ntasks, nf);
        rc = rl_launch_gemm16(la, lb, nf, &gb, total, (hipStream_t)stream);
    }
    if (rc != 0) { rl_set_error("gemm16_table: launch failed (%d)", rc); return rc < 0 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}

int32_t rlrep_gemm_plan(int32_t la, int32_t lb, int32_t R, int32_t Cn, int32_t K, int32_t lda, int32_t ldb, int32_t ldc,
                        int32_t* engine, int32_t* tile, int32_t* splits, int32_t* kchunk, int32_t* scalar_sides) {
    rl_switches_read();
    if (R <= 0 || Cn <= 0 || K <= 0 || !engine) { rl_set_error("gemm_plan: bad argument"); return RLREP_ERR_ARG; }
    GemmTask t; memset(&t, 0, sizeof(t));
    t.R = R; t.Cn = Cn; t.K = K; t.lda = lda; t.ldb = ldb; t.ldc = ldc; t.epi = la == LD_COL ? EPI_DW : EPI_FWD;
    int sp = 1, kc = 0, fl = 0;
    const GlKind kind = rl_gemm_lds_route(&t, la, lb, 0, &sp, &kc, &fl);
    const bool lds = kind != GL_GEMM16;
    *engine = GL_KINDS[kind].plan_engine;
    if (tile) *tile = GL_KINDS[kind].rows;
    if (splits) *splits = lds ? sp : 1;
    if (kchunk) *kchunk = lds ? kc : K;
    if (scalar_sides) *scalar_sides = lds ? (((fl & FLAG_SCALAR_A) ? 1 : 0) | ((fl & FLAG_SCALAR_B) ? 2 : 0) | ((fl & FLAG_SCALAR_C) ? 4 : 0)) : 0;
    return 0;
}

// Unit-test hook of the representation-loss kernels (replearn.hip): one launch on caller buffers through the launcher the step programs use, with the
// block counts of the builder's own helpers (qhead_blocks, infonce_fused_blocks, reg_gram_blocks / reg_row_blocks).  Every shape is checked
// HERE, before any GPU call: nothing a test hands in can make a kernel index outside the extents its record states.
static_assert(RLREP_SCORE_LDS32 == DS_LDS32 && RLREP_SCORE_LDS64 == DS_LDS64 && RLREP_SCORE_LDS128 == DS_LDS128 && RLREP_SCORE_SMALL1 == DS_SMALL1 &&
              RLREP_SCORE_SMALL2 == DS_SMALL2 && RLREP_SCORE_SMALL4 == DS_SMALL4 && RLREP_SCORE_VEC == DS_VEC && RLREP_SCORE_ROWS == DS_ROWS, "rlrep.h names the forms of kparams.h");
#define RLR_REFUSE(...) { rl_set_error("replearn: " __VA_ARGS__); return RLREP_ERR_ARG; }
int32_t rlrep_replearn(int32_t kernel, const rlrep_replearn_args* a, void* stream) {
    rl_switches_read();
    if (!a) RLR_REFUSE("null argument record")
    if (kernel < RLREP_RL_INFONCE || kernel > RLREP_RL_COPY2) RLR_REFUSE("unknown kernel %d", kernel)
    const hipStream_t st = (hipStream_t)stream;
    const char* what = "";
    auto al16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    // (the record of the launch is built first, the GPU is touched after every check has passed)
    InfoNce nc; ColSum cs; SpederRows sr; SpederGrads sg; DiffsrPerturb dp; DiffsrScore ds; RegStats rs;
    switch (kernel) {
    case RLREP_RL_INFONCE: case RLREP_RL_SCORE_INFONCE: {
        const auto& s = a->infonce;
        const bool fused = kernel == RLREP_RL_SCORE_INFONCE;
        what = fused ? "score matrix + infonce" : "infonce";
        if (!s.S || !s.r || !s.drhat || !s.partial) RLR_REFUSE("%s: null S, r, drhat or partial", what)
        if (s.B <= 0 || s.ncols <= 0 || s.ldS < s.ncols) RLR_REFUSE("%s: B %d, ncols %d, ldS %d: non-positive extent or row stride below the width", what, s.B, s.ncols, s.ldS)
        if (s.diag_off < 0 || (long long)s.diag_off + s.B > s.ncols) RLR_REFUSE("%s: diagonal columns [%d, %d + %d) outside the %d columns", what, s.diag_off, s.diag_off, s.B, s.ncols)
        if (fused) {
            if (!s.Z || !s.ZM || !s.theta_w || !s.theta_b) RLR_REFUSE("%s: null Z, ZM or theta", what)
            if (s.F <= 0 || s.ldZ < s.F || s.ldZM < s.F) RLR_REFUSE("%s: F %d, ldZ %d, ldZM %d: non-positive extent or row stride below the width", what, s.F, s.ldZ, s.ldZM)
            if (s.F & 63) RLR_REFUSE("%s: F %d is no multiple of 64", what, s.F)
            if (s.ncols > 256) RLR_REFUSE("%s: %d columns, at most 256", what, s.ncols)
            if ((s.ldZ & 3) || (s.ldZM & 3)) RLR_REFUSE("%s: ldZ %d / ldZM %d is no multiple of 4", what, s.ldZ, s.ldZM)
            if (!al16(s.Z) || !al16(s.ZM) || !al16(s.theta_w)) RLR_REFUSE("%s: Z, ZM or theta_w not on a 16-byte boundary", what)
        } else {
            if (s.ZM) RLR_REFUSE("%s: ZM given (the one-launch form is RLREP_RL_SCORE_INFONCE)", what)
            if (s.Z) {
                if (!s.theta_w || !s.theta_b) RLR_REFUSE("%s: Z given without theta", what)
                if (s.F <= 0 || s.ldZ < s.F) RLR_REFUSE("%s: F %d, ldZ %d: non-positive extent or row stride below the width", what, s.F, s.ldZ)
            } else if (!s.rhat) RLR_REFUSE("%s: neither rhat nor Z given", what)
        }
        memset(&nc, 0, sizeof(nc));
        nc.S = s.S; nc.ldS = s.ldS; nc.ncols = s.ncols; nc.diag_off = s.diag_off; nc.rhat = s.rhat; nc.r = s.r; nc.drhat = s.drhat; nc.partial = s.partial;
        nc.B = s.B; nc.nblk = fused ? infonce_fused_blocks(s.B) : qhead_blocks(s.B); nc.inv_batch = s.inv_batch;
        if (s.Z) { nc.Z = s.Z; nc.ldZ = s.ldZ; nc.F = s.F; nc.theta_w = s.theta_w; nc.theta_b = s.theta_b; }
        if (fused) { nc.ZM = s.ZM; nc.ldZM = s.ldZM; }
    } break;
    case RLREP_RL_COLSUM: {
        const auto& s = a->colsum;
        what = "column sum";
        if (!s.X || !s.out) RLR_REFUSE("%s: null X or out", what)
        if (s.rows <= 0 || s.F <= 0 || s.ldX < s.F) RLR_REFUSE("%s: rows %d, F %d, ldX %d: non-positive extent or row stride below the width", what, s.rows, s.F, s.ldX)
        if (s.X2 && !s.out2) RLR_REFUSE("%s: second set without out2", what)
        if (s.X2 && (s.rows2 <= 0 || s.ldX2 < s.F)) RLR_REFUSE("%s: rows2 %d, ldX2 %d: non-positive extent or row stride below the width", what, s.rows2, s.ldX2)
        memset(&cs, 0, sizeof(cs));
        cs.X = s.X; cs.ldX = s.ldX; cs.w = s.w; cs.out = s.out; cs.rows = s.rows; cs.F = s.F;
        if (s.X2) { cs.X2 = s.X2; cs.ldX2 = s.ldX2; cs.w2 = s.w2; cs.out2 = s.out2; cs.outb2 = s.outb2; cs.rows2 = s.rows2; }
    } break;
    case RLREP_RL_SPEDER_ROWS: {
        const auto& s = a->speder_rows;
        what = "spectral rows";
        if (!s.phi || !s.mu || !s.mu_r || !s.phibar || !s.theta_w || !s.theta_b || !s.r || !s.c || !s.drhat || !s.partial) RLR_REFUSE("%s: null pointer", what)
        if (s.B <= 0 || s.F <= 0) RLR_REFUSE("%s: B %d, F %d: non-positive extent", what, s.B, s.F)
        memset(&sr, 0, sizeof(sr));
        sr.phi = s.phi; sr.mu = s.mu; sr.mu_r = s.mu_r; sr.phibar = s.phibar; sr.theta_w = s.theta_w; sr.theta_b = s.theta_b; sr.r = s.r;
        sr.c = s.c; sr.drhat = s.drhat; sr.partial = s.partial; sr.B = s.B; sr.F = s.F; sr.nblk = qhead_blocks(s.B); sr.inv_batch = s.inv_batch;
    } break;
    case RLREP_RL_SPEDER_GRADS: {
        const auto& s = a->speder_grads;
        what = "spectral gradients";
        if (!s.phi || !s.mu || !s.c || !s.drhat || !s.phibar || !s.v || !s.theta_w || !s.Gphi || !s.Gmu) RLR_REFUSE("%s: null pointer", what)
        if (s.B <= 0 || s.F <= 0) RLR_REFUSE("%s: B %d, F %d: non-positive extent", what, s.B, s.F)
        memset(&sg, 0, sizeof(sg));
        sg.phi = s.phi; sg.mu = s.mu; sg.c = s.c; sg.drhat = s.drhat; sg.phibar = s.phibar; sg.v = s.v; sg.theta_w = s.theta_w;
        sg.Gphi = s.Gphi; sg.Gmu = s.Gmu; sg.B = s.B; sg.F = s.F; sg.inv_batch = s.inv_batch;
    } break;
    case RLREP_RL_PERTURB: {
        const auto& s = a->perturb;
        what = "perturb";
        if (!s.alphabars || !s.idx || !s.s2 || !s.eps || !s.XN || !s.TGT) RLR_REFUSE("%s: null pointer", what)
        if (s.B <= 0 || s.S <= 0 || s.ld_s2 < s.S) RLR_REFUSE("%s: B %d, S %d, ld_s2 %d: non-positive extent or row stride below the width", what, s.B, s.S, s.ld_s2)
        memset(&dp, 0, sizeof(dp));
        dp.alphabars = s.alphabars; dp.idx = s.idx; dp.s2 = s.s2; dp.ld_s2 = s.ld_s2; dp.eps = s.eps; dp.XN = s.XN; dp.TGT = s.TGT; dp.B = s.B; dp.S = s.S;
    } break;
    case RLREP_RL_SCORE: {
        const auto& s = a->score;
        what = "score matching";
        if (!s.U || !s.PHI || !s.TGT || !s.alphabars || !s.idx || !s.GPHI || !s.partial) RLR_REFUSE("%s: null pointer", what)
        if (s.B <= 0 || s.F <= 0 || s.S <= 0) RLR_REFUSE("%s: B %d, F %d, S %d: non-positive extent", what, s.B, s.F, s.S)
        memset(&ds, 0, sizeof(ds));
        ds.U = s.U; ds.PHI = s.PHI; ds.TGT = s.TGT; ds.alphabars = s.alphabars; ds.idx = s.idx; ds.GPHI = s.GPHI; ds.partial = s.partial;
        ds.B = s.B; ds.F = s.F; ds.S = s.S; ds.sigma = s.sigma; ds.inv_batch = s.inv_batch;
        const DsForm f = rl_diffsr_score_form(&ds);
        if ((f == DS_ROWS || f == DS_VEC) && (long long)5 * s.S * (long long)sizeof(float) > 65536)
            RLR_REFUSE("%s: S %d: the two-pass kernel's %lld bytes of dynamic LDS exceed the 65536 a launch may have", what, s.S, (long long)5 * s.S * (long long)sizeof(float))
    } break;
    case RLREP_RL_REG_STATS: {
        const auto& s = a->reg_stats;
        what = "regulariser statistics";
        for (int k = 0; k < 4; ++k) if (!s.X[k] || !s.C[k]) RLR_REFUSE("%s: null X[%d] or C[%d]", what, k, k)
        if (!s.partial) RLR_REFUSE("%s: null partial", what)
        if (s.H <= 0) RLR_REFUSE("%s: H %d: non-positive extent", what, s.H)
        if (s.B < 2) RLR_REFUSE("%s: batch %d below 2 (the statistic divides by (B - 1) B)", what, s.B)
        memset(&rs, 0, sizeof(rs));
        for (int k = 0; k < 4; ++k) { rs.X[k] = s.X[k]; rs.C[k] = s.C[k]; }
        rs.B = s.B; rs.H = s.H; rs.nbc = reg_gram_blocks(s.H); rs.nbr = reg_row_blocks(s.B); rs.lambda = s.lambda; rs.partial = s.partial;
    } break;
    case RLREP_RL_COPY2: {
        const auto& s = a->copy2;
        what = "copy2";
        if (!s.src || !s.d1) RLR_REFUSE("%s: null src or d1", what)
        if (s.n <= 0) RLR_REFUSE("%s: n %lld: non-positive extent", what, (long long)s.n)
    } break;
    }
    int rc = rl_replearn_init();                  // (the LDS reservations of the one-pass score-matching kernels: 69 888 bytes at F = 256)
    if (rc != 0) { rl_set_error("replearn: %s: rl_replearn_init failed (%d)", what, rc); return RLREP_ERR_HIP; }
    switch (kernel) {
    case RLREP_RL_INFONCE: case RLREP_RL_SCORE_INFONCE: rc = rl_launch_infonce(&nc, st); break;
    case RLREP_RL_COLSUM: rc = rl_launch_colsum(&cs, st); break;
    case RLREP_RL_SPEDER_ROWS: rc = rl_launch_speder_rows(&sr, st); break;
    case RLREP_RL_SPEDER_GRADS: rc = rl_launch_speder_grads(&sg, st); break;
    case RLREP_RL_PERTURB: rc = rl_launch_diffsr_perturb(&dp, st); break;
    case RLREP_RL_SCORE: rc = rl_launch_diffsr_score(&ds, st); break;
    case RLREP_RL_REG_STATS: rc = rl_launch_reg_stats(&rs, st); break;
    case RLREP_RL_COPY2: rc = rl_launch_copy2(a->copy2.src, a->copy2.d1, a->copy2.d2, (long long)a->copy2.n, st); break;
    }
    if (rc != 0) { rl_set_error("replearn: %s: launch failed (%d)", what, rc); return rc < 0 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
#undef RLR_REFUSE

int32_t rlrep_diffsr_score_plan(int32_t S, int32_t F, int32_t u_aligned16, int32_t* form) {
    rl_switches_read();
    if (S <= 0 || F <= 0 || !form) { rl_set_error("diffsr_score_plan: bad argument"); return RLREP_ERR_ARG; }
    DiffsrScore p; memset(&p, 0, sizeof(p));
    p.S = S; p.F = F; p.U = (float*)(uintptr_t)(u_aligned16 ? 64 : 68);        // (only its alignment is read)
    *form = (int32_t)rl_diffsr_score_form(&p);
    return 0;
}

int32_t rlrep_nc_fwd_plan(int32_t heads, int32_t B, int32_t F, int32_t H, int32_t* engine, int32_t* rows, int32_t* cols) {
    rl_switches_read();
    if (heads <= 0 || heads > NC_MAX_TASKS || B <= 0 || F <= 0 || H <= 0 || !engine) { rl_set_error("nc_fwd_plan: bad argument"); return RLREP_ERR_ARG; }
    NcFwdTask t[NC_MAX_TASKS]; memset(t, 0, sizeof(t));
    for (int q = 0; q < heads; ++q) { t[q].B = B; t[q].F = F; t[q].H = H; t[q].N = 20; t[q].ld_ml = 2 * F; }
    int e = 0, g2 = 1, c = 128;
    rl_nc_fwd_plan(t, heads, &e, &g2, &c);
    *engine = e;
    if (rows) *rows = 4 * g2;
    if (cols) *cols = c;
    return 0;
}

// Unit-test hook of the noise-critic kernels (noisecritic.hip): one launch on caller buffers through the launchers the step programs use, numbered
// by the builder's own helpers (engine_internal.h rl_nc_*_number_tiles).  Every shape, stride and alignment the kernels take for granted is
// checked HERE, before any GPU call -- rl_nc_init() included (the raised dynamic-LDS attribute of the fp32 dW kernel and the bf16x3 forwards,
// which an agent's creation sets in production).
static int64_t nc_w3_image_bytes(int H, int F) { return (((int64_t)6 * H * F) + 15) & ~(int64_t)15; }
int64_t rlrep_nc_w3_bytes(int32_t H, int32_t F) {
    if (H <= 0 || F <= 0) return 0;
    return nc_w3_image_bytes(H, F) + (int64_t)((sizeof(ShadowEnt) + 15) & ~(size_t)15);
}
int32_t rlrep_nc_forms(int32_t tasks, int32_t B, int32_t F, int32_t H, int32_t g2, int32_t* chunked, int32_t* splits) {
    rl_switches_read();
    if (tasks <= 0 || B <= 0 || F <= 0 || H <= 0 || (g2 != 1 && g2 != 2 && g2 != 4)) { rl_set_error("nc_forms: bad argument"); return RLREP_ERR_ARG; }
    if (chunked) *chunked = rl_nc_fwd_chunked(F, g2);
    if (splits) *splits = rl_nc_dw_splits(B, F, H, tasks);
    return 0;
}
#define NCR_REFUSE(...) { rl_set_error("noisecritic: " __VA_ARGS__); return RLREP_ERR_ARG; }
int32_t rlrep_noisecritic(int32_t kernel, const rlrep_noisecritic_args* a, void* stream) {
    rl_switches_read();
    if (!a) NCR_REFUSE("null argument record")
    if (kernel < RLREP_NC_FWD || kernel > RLREP_NC_DW) NCR_REFUSE("unknown kernel %d", kernel)
    if (rl_grp_active()) NCR_REFUSE("a seed group's call is in progress (the family has no group form)")
    const hipStream_t st = (hipStream_t)stream;
    constexpr int N = 4 * NC_NF_HOST;
    auto al16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
    auto ld_ok = [](int ld, int width) { return ld >= width && (ld & 3) == 0; };
    const char* what = "";
    NcFwdBatch fb; NcDxTask dx; NcDwBatch wb;
    int total = 0, g2 = 1, chunked = 0;
    switch (kernel) {
    case RLREP_NC_FWD: {
        const auto& s = a->fwd;
        what = "forward";
        if (s.ntasks < 1 || s.ntasks > NC_MAX_TASKS) NCR_REFUSE("%s: ntasks %d outside 1..%d", what, s.ntasks, NC_MAX_TASKS)
        if (s.g2 != 0 && s.g2 != 1 && s.g2 != 2 && s.g2 != 4) NCR_REFUSE("%s: g2 %d not in {0, 1, 2, 4}", what, s.g2)
        if (s.cols != 0 && s.cols != 64 && s.cols != 128) NCR_REFUSE("%s: cols %d not in {0, 64, 128}", what, s.cols)
        memset(&fb, 0, sizeof(fb));
        bool same = true;
        for (int q = 0; q < s.ntasks; ++q) {
            const rlrep_nc_fwd_task& u = s.t[q];
            if (!u.mean || !u.lstd || !u.noise || !u.W || !u.bias || !u.Hm) NCR_REFUSE("%s: task %d: null mean, lstd, noise, W, bias or Hm", what, q)
            if (u.B <= 0 || u.F <= 0 || u.H <= 0) NCR_REFUSE("%s: task %d: B %d, F %d, H %d: non-positive extent", what, q, u.B, u.F, u.H)
            if (u.F & 3) NCR_REFUSE("%s: task %d: F %d is no multiple of 4", what, q, u.F)
            if (!ld_ok(u.ld_ml, u.F)) NCR_REFUSE("%s: task %d: ld_ml %d below F %d or no multiple of 4", what, q, u.ld_ml, u.F)
            if (!al16(u.mean) || !al16(u.lstd) || !al16(u.noise) || !al16(u.sigma_out)) NCR_REFUSE("%s: task %d: mean, lstd, noise or sigma_out not on a 16-byte boundary", what, q)
            if (u.w3 && ((u.F & 31) || !al16(u.W) || !al16(u.w3))) NCR_REFUSE("%s: task %d: w3 needs F %% 32 == 0 and W, w3 on 16-byte boundaries", what, q)
            if (u.F != s.t[0].F) NCR_REFUSE("%s: task %d: F %d differs from task 0's %d (one LDS table size per launch)", what, q, u.F, s.t[0].F)
            same = same && u.B == s.t[0].B && u.H == s.t[0].H;
            NcFwdTask& t = fb.t[q];
            t.mean = u.mean; t.lstd = u.lstd; t.ld_ml = u.ld_ml; t.noise = u.noise; t.W = u.W; t.bias = u.bias; t.W3 = (const unsigned char*)u.w3;
            t.Hm = u.Hm; t.U = u.U; t.sigma_out = u.sigma_out; t.B = u.B; t.F = u.F; t.H = u.H; t.N = N;
        }
        const int F = s.t[0].F;
        if (!same && !rl_off("x3") && (F % 32) == 0 && F >= 64) NCR_REFUSE("%s: tasks of a bf16x3 launch differ in B or H", what)
        int engine = 0, cols = 128;
        rl_nc_fwd_plan(fb.t, s.ntasks, &engine, &g2, &cols);
        if (s.g2) g2 = s.g2;
        if (s.cols) cols = s.cols;
        if (engine == 1 && g2 != 2) NCR_REFUSE("%s: g2 %d on the bf16x3 engine (8 batch rows a workgroup: g2 = 2)", what, g2)
        chunked = (engine == 0 && rl_nc_fwd_chunked(F, g2)) ? 1 : 0;
        if (chunked && cols != 128) NCR_REFUSE("%s: the K-chunked form has 128 hidden units a workgroup, not %d", what, cols)
        if (engine == 0 && !chunked && (size_t)(8 * g2 + N) * (size_t)(((F + 15) & ~15) + 16) * sizeof(float) > 64 * 1024)
            NCR_REFUSE("%s: the whole table of F %d at g2 %d is past 64 KB of LDS", what, F, g2)
        fb.ntasks = s.ntasks; fb.engine = engine; fb.cols = cols; fb.nt_u = rl_opt("nc_u_nt") ? 1 : 0;
        total = rl_nc_fwd_number_tiles(fb.t, s.ntasks, g2, cols);
        if (s.form) { s.form[0] = engine; s.form[1] = g2; s.form[2] = cols; s.form[3] = chunked; }
    } break;
    case RLREP_NC_DX: {
        const auto& s = a->dx;
        what = "dX";
        if (s.nheads < 1 || s.nheads > 2) NCR_REFUSE("%s: nheads %d outside 1..2", what, s.nheads)
        for (int h = 0; h < s.nheads; ++h) if (!s.GH[h] || !s.U[h] || !s.W[h]) NCR_REFUSE("%s: head %d: null GH, U or W", what, h)
        if (!s.noise || !s.lstd || !s.G) NCR_REFUSE("%s: null noise, lstd or G", what)
        if (s.B <= 0 || s.F <= 0 || s.H <= 0) NCR_REFUSE("%s: B %d, F %d, H %d: non-positive extent", what, s.B, s.F, s.H)
        if (s.F & 3) NCR_REFUSE("%s: F %d is no multiple of 4", what, s.F)
        if (!ld_ok(s.ldgh, s.H) || !ld_ok(s.ld_l, s.F) || !ld_ok(s.ldg, 2 * s.F))
            NCR_REFUSE("%s: ldgh %d / ld_l %d / ldg %d below the row's width (H %d, F %d, 2 F) or no multiple of 4", what, s.ldgh, s.ld_l, s.ldg, s.H, s.F)
        if (!al16(s.lstd) || !al16(s.noise)) NCR_REFUSE("%s: lstd or noise not on a 16-byte boundary", what)
        memset(&dx, 0, sizeof(dx));
        for (int h = 0; h < s.nheads; ++h) { dx.GH[h] = s.GH[h]; dx.U[h] = s.U[h]; dx.W[h] = s.W[h]; }
        dx.ldgh = s.ldgh; dx.noise = s.noise; dx.lstd = s.lstd; dx.ld_l = s.ld_l; dx.G = s.G; dx.ldg = s.ldg;
        dx.B = s.B; dx.F = s.F; dx.H = s.H; dx.N = N; dx.nheads = s.nheads;
        total = rl_nc_dx_number_tiles(&dx);
        if (s.form) {
            bool vec = ((s.H & 3) == 0) && ((s.ldgh & 3) == 0);                  // (rl_launch_nc_dx's own rule)
            for (int h = 0; h < s.nheads; ++h) vec = vec && al16(s.U[h]) && al16(s.GH[h]);
            s.form[0] = rl_nc_dx_engine(&dx); s.form[1] = vec ? 1 : 0;
        }
    } break;
    case RLREP_NC_DW: {
        const auto& s = a->dw;
        what = "dW";
        if (s.ntasks < 1 || s.ntasks > 2) NCR_REFUSE("%s: ntasks %d outside 1..2", what, s.ntasks)
        if (s.lean != 0 && s.lean != 1) NCR_REFUSE("%s: lean %d not 0 or 1", what, s.lean)
        if (s.splits < 0 || s.splits > 16) NCR_REFUSE("%s: splits %d outside 0..16", what, s.splits)
        memset(&wb, 0, sizeof(wb));
        for (int q = 0; q < s.ntasks; ++q) {
            const rlrep_nc_dw_task& u = s.t[q];
            if (!u.U || !u.GH || !u.mean || !u.sigma || !u.noise || !u.gW || !u.gb) NCR_REFUSE("%s: task %d: null pointer", what, q)
            if (u.B <= 0 || u.F <= 0 || u.H <= 0) NCR_REFUSE("%s: task %d: B %d, F %d, H %d: non-positive extent", what, q, u.B, u.F, u.H)
            if (u.F & 3) NCR_REFUSE("%s: task %d: F %d is no multiple of 4", what, q, u.F)
            if (!ld_ok(u.ldgh, u.H) || !ld_ok(u.ld_ml, u.F)) NCR_REFUSE("%s: task %d: ldgh %d / ld_ml %d below the row's width (H %d, F %d) or no multiple of 4", what, q, u.ldgh, u.ld_ml, u.H, u.F)
            if (!al16(u.mean) || !al16(u.sigma) || !al16(u.noise)) NCR_REFUSE("%s: task %d: mean, sigma or noise not on a 16-byte boundary", what, q)
            if (u.B != s.t[0].B || u.F != s.t[0].F || u.H != s.t[0].H) NCR_REFUSE("%s: task %d differs from task 0 in B, F or H", what, q)
            NcDwTask& t = wb.t[q];
            t.U = u.U; t.GH = u.GH; t.ldgh = u.ldgh; t.mean = u.mean; t.sigma = u.sigma; t.ld_ml = u.ld_ml; t.noise = u.noise; t.gW = u.gW; t.gb = u.gb;
            t.B = u.B; t.F = u.F; t.H = u.H; t.N = N;
        }
        const rlrep_nc_dw_task& u0 = s.t[0];
        wb.ntasks = s.ntasks; wb.lean = s.lean; wb.engine = rl_nc_dw_engine();
        wb.splits = s.splits ? s.splits : rl_nc_dw_splits(u0.B, u0.F, u0.H, s.ntasks);
        wb.fin_in_adam = 0; wb.rows = rl_off("nc_dw_rows") ? 0 : 1;
        if (wb.engine == 1) {
            const long long need = (long long)s.ntasks * wb.splits * u0.H;
            if (!s.slab || !s.bslab || s.slab_floats < need * u0.F || s.bslab_floats < need)
                NCR_REFUSE("%s: the bf16x3 form with %d splits needs a slab of %lld and a bias slab of %lld floats", what, wb.splits, need * u0.F, need)
            wb.slab = s.slab; wb.bslab = s.bslab;
        }
        total = rl_nc_dw_number_tiles(&wb);
        if (s.form) { s.form[0] = wb.engine; s.form[1] = wb.lean; s.form[2] = wb.splits; s.form[3] = wb.engine == 1 ? wb.rows : 0; }
    } break;
    }
    int rc = rl_nc_init();
    if (rc != 0) { rl_set_error("noisecritic: %s: rl_nc_init failed (%d)", what, rc); return RLREP_ERR_HIP; }
    switch (kernel) {
    case RLREP_NC_FWD:
        for (int q = 0; q < fb.ntasks && rc == 0; ++q) {
            NcFwdTask& t = fb.t[q];
            if (!t.W3) continue;
            // the production producer of the images (shadow launch, ShadowEnt kind 1); its one-entry table sits behind the images in the scratch
            unsigned char* img = const_cast<unsigned char*>(t.W3);
            ShadowEnt se; memset(&se, 0, sizeof(se));
            se.n = (long long)t.H * t.F; se.rows = t.H; se.cols = t.F; se.kind = 1; se.sp = reinterpret_cast<float*>(img); se.src = t.W;
            ShadowEnt* dev = reinterpret_cast<ShadowEnt*>(img + nc_w3_image_bytes(t.H, t.F));
            hipError_t e = hipStreamSynchronize(st);
            if (e == hipSuccess) e = hipMemcpy(dev, &se, sizeof(se), hipMemcpyHostToDevice);
            if (e != hipSuccess) { rl_set_error("noisecritic: %s: table upload failed: %s", what, hipGetErrorString(e)); return RLREP_ERR_HIP; }
            rc = rl_launch_shadow(dev, 1, ((t.H + 31) / 32) * (t.F / 32), nullptr, 0, st);
        }
        if (rc == 0) rc = rl_launch_nc_fwd(&fb, total, g2, chunked, st);
        break;
    case RLREP_NC_DX: rc = rl_launch_nc_dx(&dx, st); break;
    case RLREP_NC_DW: rc = rl_launch_nc_dw(&wb, total, st); break;
    }
    if (rc != 0) { rl_set_error("noisecritic: %s: launch failed (%d)", what, rc); return rc < 0 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
#undef NCR_REFUSE

// Unit-test hook of the loss heads (elementwise.hip / per.hip kernels and the gemm16 epilogues that replace four of them): one launch on caller
// buffers through the launchers the step programs use.  Block and tile counts come from the builder's helpers (qhead_blocks, rl_vae_blocks,
// rl_heads_vae_tiles_c, rl_gemm16_pick_nf / rl_gemm16_number_tiles), the fused task records from the functions the builder fills them with
// (engine_internal.h rl_task_*).  Every shape is checked HERE, before any GPU call: nothing a test hands in can make a kernel index outside
// the extents its record states.
int32_t rlrep_heads_partials(int32_t kind, int32_t fused, int32_t B, int32_t n) {
    if (B <= 0) return 0;
    switch (kind) {
    case RLREP_HD_VAE_MID: return n > 0 ? rl_vae_blocks(B, n) : 0;
    case RLREP_HD_HEADS_VAE: return n > 0 ? ((B + 15) / 16) * rl_heads_vae_tiles_c(n) : 0;
    case RLREP_HD_VAE_MSE: return n > 0 ? 2 * (fused ? ((B + 15) / 16) * ((n + 1 + 15) / 16) : rl_vae_blocks(B, n + 1)) : 0;
    case RLREP_HD_REPARAM_DX: return 2 * ((B + 15) / 16);
    case RLREP_HD_QHEAD_CRITIC: return 4 * qhead_blocks(B);
    case RLREP_HD_QHEAD_ACTOR: return qhead_blocks(B);
    default: return 0;
    }
}
#define HD_REFUSE(...) { rl_set_error("heads: " __VA_ARGS__); return RLREP_ERR_ARG; }
static int32_t heads_impl(int32_t kind, const rlrep_heads_args* a, void* stream, bool launch);
int32_t rlrep_heads(int32_t kind, const rlrep_heads_args* a, void* stream) { return heads_impl(kind, a, stream, true); }
int32_t rlrep_heads_plan(int32_t kind, const rlrep_heads_args* a) { return heads_impl(kind, a, nullptr, false); }
static int32_t heads_impl(int32_t kind, const rlrep_heads_args* a, void* stream, bool launch) {
    rl_switches_read();
    if (!a) HD_REFUSE("null argument record")
    if (kind < RLREP_HD_POLICY_FWD || kind > RLREP_HD_QHEAD_ACTOR) HD_REFUSE("unknown kind %d", kind)
    if (rl_grp_active()) HD_REFUSE("a seed group's call is in progress (the group forms are not reachable here)")
    const hipStream_t st = (hipStream_t)stream;
    auto al = [](const void* p, uintptr_t n) { return (((uintptr_t)p) & (n - 1)) == 0; };
    auto al4 = [&](std::initializer_list<const void*> ps) { for (const void* p : ps) if (!al(p, 4)) return false; return true; };
    // the layer of a fused form: forward X [rows, K] . W [N, K]^T + bias [N]; backward G [rows, K] . W [K, N]
    auto layer_bad = [&](const rlrep_hd_layer& l, bool fwd, int N) -> const char* {
        if (!l.X || !l.W || (fwd && !l.bias)) return "null X, W or bias of the layer";
        if (l.K <= 0) return "non-positive inner length of the layer";
        if (l.ldx < l.K || l.ldw < (fwd ? l.K : N)) return "row stride of the layer's X or W below the row's width";
        if (!al4({l.X, l.W, l.bias})) return "a pointer of the layer off a 4-byte boundary";
        return nullptr;
    };
    const char* what = "";
    PolicyFwd pf; PolicyBwd pb; VaeMid vm; HeadsVae hv; VaeMse ms; QHeadCriticW qw; QHeadActor qa;
    GemmBatch gb; memset(&gb, 0, sizeof(gb));
    int la = LD_ROW, lb = LD_ROW;
    bool gemm = false;
    int32_t* form = nullptr; int form1 = 0;
    switch (kind) {
    case RLREP_HD_POLICY_FWD: {
        const auto& s = a->policy_fwd;
        what = "policy forward"; form = s.form;
        if (s.fused != 0 && s.fused != 1) HD_REFUSE("%s: fused %d not 0 or 1", what, s.fused)
        if (s.B <= 0 || s.A <= 0) HD_REFUSE("%s: B %d, A %d: non-positive extent", what, s.B, s.A)
        const int nt = s.fused ? s.ntasks : 1;
        if (nt < 1 || nt > 2) HD_REFUSE("%s: ntasks %d outside 1..2", what, s.ntasks)
        if (s.fused && 2 * s.A > 16) HD_REFUSE("%s: fused with 2 A = %d > 16 (the [mu | rho] row must fit one 16-column tile)", what, 2 * s.A)
        if (s.fused && s.clamp) HD_REFUSE("%s: the fused form has no clamp", what)
        for (int q = 0; q < nt; ++q) {
            const rlrep_hd_policy_task& u = s.t[q];
            if (!u.O || !u.act) HD_REFUSE("%s: task %d: null O or act", what, q)
            if (u.ld_act < s.A) HD_REFUSE("%s: task %d: ld_act %d below A %d", what, q, u.ld_act, s.A)
            if (!al4({u.O, u.eps, u.act, u.logp})) HD_REFUSE("%s: task %d: a pointer off a 4-byte boundary", what, q)
            if (s.fused) {
                if (!u.eps) HD_REFUSE("%s: task %d: the fused form needs eps", what, q)
                if (const char* bad = layer_bad(u.l, true, 2 * s.A)) HD_REFUSE("%s: task %d: %s", what, q, bad)
            }
        }
        if (!s.fused) {
            memset(&pf, 0, sizeof(pf));
            pf.O = s.t[0].O; pf.eps = s.t[0].eps; pf.B = s.B; pf.A = s.A; pf.act = s.t[0].act; pf.ld_act = s.t[0].ld_act; pf.logp = s.t[0].logp;
            pf.clamp = s.clamp ? 1 : 0; pf.lo = s.lo; pf.hi = s.hi;
            break;
        }
        gemm = true;
        for (int q = 0; q < nt; ++q) {
            const rlrep_hd_policy_task& u = s.t[q];
            GemmTask head = Builder::fwd(u.l.X, u.l.ldx, s.B, u.l.K, u.l.W, u.l.ldw, u.l.bias, 2 * s.A, u.O, 2 * s.A, ACT_NONE);
            rl_task_policy_head(head, s.A, u.act, u.ld_act, u.logp, 0);
            head.x2 = u.eps;
            gb.t[gb.ntasks++] = head;
        }
        if (s.extra.l.X) {
            const auto& e = s.extra;
            if (e.rows <= 0 || e.N <= 0 || !e.Y || e.ldy < e.N) HD_REFUSE("%s: extra task: rows %d, N %d, ldy %d: non-positive extent, null Y or row stride below the width", what, e.rows, e.N, e.ldy)
            if (e.act < ACT_NONE || e.act > ACT_TANH || e.act == ACT_SIN) HD_REFUSE("%s: extra task: activation %d not in {0, 1, 2, 4}", what, e.act)
            if (const char* bad = layer_bad(e.l, true, e.N)) HD_REFUSE("%s: extra task: %s", what, bad)
            if (!al4({e.Y})) HD_REFUSE("%s: extra task: Y off a 4-byte boundary", what)
            gb.t[gb.ntasks++] = Builder::fwd(e.l.X, e.l.ldx, e.rows, e.l.K, e.l.W, e.l.ldw, e.l.bias, e.N, e.Y, e.ldy, e.act);
        }
    } break;
    case RLREP_HD_POLICY_BWD: {
        const auto& s = a->policy_bwd;
        what = "policy backward"; form = s.form;
        if (s.fused != 0 && s.fused != 1) HD_REFUSE("%s: fused %d not 0 or 1", what, s.fused)
        if (s.B <= 0 || s.A <= 0) HD_REFUSE("%s: B %d, A %d: non-positive extent", what, s.B, s.A)
        if (!s.O || !s.eps || !s.act || !s.alpha_state || !s.G) HD_REFUSE("%s: null O, eps, act, alpha_state or G", what)
        if (s.ld_act < s.A) HD_REFUSE("%s: ld_act %d below A %d", what, s.ld_act, s.A)
        if (!al(s.alpha_state, 8)) HD_REFUSE("%s: alpha_state off an 8-byte boundary", what)
        if (!al4({s.O, s.eps, s.act, s.dA, s.G})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        if (!s.fused) {
            if (!s.dA || s.ld_dA < s.A) HD_REFUSE("%s: null dA or ld_dA %d below A %d", what, s.ld_dA, s.A)
            memset(&pb, 0, sizeof(pb));
            pb.O = s.O; pb.eps = s.eps; pb.act = s.act; pb.ld_act = s.ld_act; pb.dA = s.dA; pb.ld_dA = s.ld_dA;
            pb.alpha_state = s.alpha_state; pb.inv_batch = s.inv_batch; pb.G = s.G; pb.B = s.B; pb.A = s.A;
            break;
        }
        if (s.A > 16) HD_REFUSE("%s: fused with A = %d > 16", what, s.A)
        if (const char* bad = layer_bad(s.l, false, s.A)) HD_REFUSE("%s: %s", what, bad)
        gemm = true; lb = LD_COL;
        GemmTask dxa = Builder::dx(s.l.X, s.l.ldx, s.B, s.l.K, s.l.W, s.l.ldw, s.dA, s.A, s.A, ACT_NONE, nullptr, 0);
        rl_task_policy_bwd(dxa, s.A, s.O, s.act, s.ld_act, s.G, s.alpha_state, s.inv_batch, 0);
        dxa.x2 = s.eps;
        gb.t[gb.ntasks++] = dxa;
    } break;
    case RLREP_HD_VAE_MID: {
        const auto& s = a->vae_mid;
        what = "vae_mid"; form = s.form;
        if (s.B <= 0 || s.F <= 0) HD_REFUSE("%s: B %d, F %d: non-positive extent", what, s.B, s.F)
        if (!s.EH || !s.FH || !s.eps || !s.Z || !s.EZ || !s.GEH || !s.GFH || !s.partial) HD_REFUSE("%s: null pointer", what)
        if (!al4({s.EH, s.FH, s.eps, s.Z, s.EZ, s.GEH, s.GFH, s.partial})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        memset(&vm, 0, sizeof(vm));
        vm.EH = s.EH; vm.FH = s.FH; vm.eps = s.eps; vm.Z = s.Z; vm.EZ = s.EZ; vm.GEH = s.GEH; vm.GFH = s.GFH; vm.partial = s.partial;
        vm.B = s.B; vm.F = s.F; vm.nblk = rl_vae_blocks(s.B, s.F); vm.scale = s.scale;
    } break;
    case RLREP_HD_HEADS_VAE: {
        const auto& s = a->heads_vae;
        what = "heads_vae"; form = s.form;
        if (s.B <= 0 || s.F <= 0 || s.K <= 0) HD_REFUSE("%s: B %d, F %d, K %d: non-positive extent", what, s.B, s.F, s.K)
        if (!s.Ae || !s.Af || !s.We || !s.be || !s.Wf || !s.bf || !s.eps || !s.Z || !s.EZ || !s.GEH || !s.GFH || !s.partial) HD_REFUSE("%s: null pointer", what)
        if (s.lda < s.K) HD_REFUSE("%s: lda %d below K %d", what, s.lda, s.K)
        if (!al4({s.Ae, s.Af, s.We, s.be, s.Wf, s.bf, s.eps, s.Z, s.EZ, s.GEH, s.GFH, s.partial, s.EH, s.FH})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        memset(&hv, 0, sizeof(hv));
        hv.Ae = s.Ae; hv.Af = s.Af; hv.lda = s.lda; hv.We = s.We; hv.be = s.be; hv.Wf = s.Wf; hv.bf = s.bf; hv.eps = s.eps;
        hv.Z = s.Z; hv.EZ = s.EZ; hv.GEH = s.GEH; hv.GFH = s.GFH; hv.partial = s.partial; hv.EH = s.EH; hv.FH = s.FH;
        hv.B = s.B; hv.F = s.F; hv.K = s.K; hv.tiles_c = rl_heads_vae_tiles_c(s.F); hv.scale = s.scale;
        // (heads_vae_tile's own rule for its 16-byte loader copy)
        form1 = (!(s.K & 3) && !(s.lda & 3) && al(s.Ae, 16) && al(s.Af, 16) && al(s.We, 16) && al(s.Wf, 16)) ? 1 : 0;
    } break;
    case RLREP_HD_VAE_MSE: {
        const auto& s = a->vae_mse;
        what = "vae_mse"; form = s.form;
        if (s.fused != 0 && s.fused != 1) HD_REFUSE("%s: fused %d not 0 or 1", what, s.fused)
        if (s.B <= 0 || s.S <= 0) HD_REFUSE("%s: B %d, S %d: non-positive extent", what, s.B, s.S)
        if (!s.s2 || !s.r || !s.GDH || !s.partial) HD_REFUSE("%s: null s2, r, GDH or partial", what)
        if (s.ld_s2 < s.S) HD_REFUSE("%s: ld_s2 %d below S %d", what, s.ld_s2, s.S)
        if (!al4({s.DH, s.s2, s.r, s.GDH, s.partial})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        if (!s.fused) {
            if (!s.DH) HD_REFUSE("%s: null DH", what)
            memset(&ms, 0, sizeof(ms));
            ms.DH = s.DH; ms.s2 = s.s2; ms.ld_s2 = s.ld_s2; ms.r = s.r; ms.GDH = s.GDH; ms.partial = s.partial; ms.B = s.B; ms.S = s.S;
            ms.nblk = rl_vae_blocks(s.B, s.S + 1); ms.scale_s = s.scale_s; ms.scale_r = s.scale_r;
            break;
        }
        if (const char* bad = layer_bad(s.l, true, s.S + 1)) HD_REFUSE("%s: %s", what, bad)
        gemm = true;
        GemmTask t = Builder::fwd(s.l.X, s.l.ldx, s.B, s.l.K, s.l.W, s.l.ldw, s.l.bias, s.S + 1, s.GDH, s.S + 1, ACT_NONE);
        rl_task_mse(t, s.S, s.s2, s.ld_s2, s.r, s.scale_s, s.scale_r, s.partial);
        gb.t[gb.ntasks++] = t;
    } break;
    case RLREP_HD_REPARAM_DX: {
        const auto& s = a->reparam_dx;
        what = "reparameterisation dX"; form = s.form; form1 = s.pre;
        if (s.pre < 0 || s.pre > 2) HD_REFUSE("%s: pre %d outside 0..2", what, s.pre)
        if (s.B <= 0 || s.F <= 0 || s.K <= 0) HD_REFUSE("%s: B %d, F %d, K %d: non-positive extent", what, s.B, s.F, s.K)
        if (!s.A || !s.W || !s.G || !s.EZ) HD_REFUSE("%s: null A, W, G or EZ", what)
        if (s.lda < s.K || s.ldw < s.F || s.ldg < 2 * s.F || s.ldez < s.F) HD_REFUSE("%s: lda %d / ldw %d / ldg %d / ldez %d below the row's width (K %d, F %d, 2 F, F)", what, s.lda, s.ldw, s.ldg, s.ldez, s.K, s.F)
        if (!al4({s.A, s.W, s.G, s.EZ, s.X, s.Wh, s.M, s.bh, s.s2, s.r, s.partial})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        gemm = true; lb = LD_COL;
        GemmTask t = Builder::dx(s.A, s.lda, s.B, s.K, s.W, s.ldw, s.G, s.ldg, s.F, ACT_NONE, nullptr, 0);
        rl_task_reparam(t, s.EZ, s.ldez, s.F);
        if (s.pre) {
            if (!s.X || !s.Wh || !s.M) HD_REFUSE("%s: null X, Wh or M of the fused short product", what)
            if (s.K1 <= 0 || s.K1 > 32) HD_REFUSE("%s: K1 %d outside 1..32", what, s.K1)
            if (s.ldx < s.K1 || s.ldwh < s.K || s.ldm < s.K) HD_REFUSE("%s: ldx %d / ldwh %d / ldm %d below the row's width (K1 %d, K %d, K)", what, s.ldx, s.ldwh, s.ldm, s.K1, s.K)
        }
        if (s.pre == 1) {
            // (the dec.heads dX task whose output the tiles recompute: agents1.hip build_vlsac, Builder::dx_stage12)
            const GemmTask d1 = Builder::dx(s.X, s.ldx, s.B, s.K1, s.Wh, s.ldwh, s.A, s.lda, s.K, ACT_RELU, s.M, s.ldm);
            rl_task_pre_dx(t, d1);
        } else if (s.pre == 2) {
            if (!s.bh || !s.s2 || !s.r || !s.partial) HD_REFUSE("%s: null bh, s2, r or partial of the mse phase", what)
            if (s.K1 < 2 || s.ld_s2 < s.K1 - 1) HD_REFUSE("%s: K1 %d below 2 (S + 1) or ld_s2 %d below S", what, s.K1, s.ld_s2)
            if ((s.K & 3) || (s.ldm & 3) || (s.ldwh & 3) || !al(s.M, 16) || !al(s.Wh, 16))
                HD_REFUSE("%s: the mse phase loads 16 bytes at a time: K %d, ldm %d, ldwh %d must be multiples of 4, M and Wh on 16-byte boundaries", what, s.K, s.ldm, s.ldwh)
            rl_task_pre_mse(t, s.X, s.ldx, s.Wh, s.ldwh, s.bh, s.K1 - 1, s.M, s.ldm, s.A, s.lda, s.s2, s.ld_s2, s.r, s.scale_s, s.scale_r, s.partial);
        }
        gb.t[gb.ntasks++] = t;
    } break;
    case RLREP_HD_QHEAD_CRITIC: {
        const auto& s = a->qhead_critic;
        what = "qhead critic"; form = s.form; form1 = s.weighted ? 1 : 0;
        if (s.B <= 0 || s.H <= 0) HD_REFUSE("%s: B %d, H %d: non-positive extent", what, s.B, s.H)
        for (int h = 0; h < 2; ++h) {
            if (!s.Et[h] || !s.Ec[h] || !s.wt[h] || !s.bt[h] || !s.wc[h] || !s.bc[h]) HD_REFUSE("%s: head %d: null Et, Ec, wt, bt, wc or bc", what, h)
            if (s.train && !s.GE[h]) HD_REFUSE("%s: head %d: null GE", what, h)
            if (!al4({s.Et[h], s.Ec[h], s.wt[h], s.bt[h], s.wc[h], s.bc[h], s.GE[h]})) HD_REFUSE("%s: head %d: a pointer off a 4-byte boundary", what, h)
        }
        if (!s.logp || !s.R || !s.D || !s.alpha_state || !s.partial || (s.train && !s.dq)) HD_REFUSE("%s: null logp, R, D, alpha_state, partial or dq", what)
        if (s.ldE != 0 && s.ldE < s.H) HD_REFUSE("%s: ldE %d below H %d (0: dense)", what, s.ldE, s.H)
        if (s.weighted && (!s.w || !s.td)) HD_REFUSE("%s: the weighted form needs w and td", what)
        if (!al(s.alpha_state, 8)) HD_REFUSE("%s: alpha_state off an 8-byte boundary", what)
        if (!al4({s.logp, s.R, s.D, s.partial, s.dq, s.w, s.td})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        memset(&qw, 0, sizeof(qw));
        QHeadCritic& q = qw.q;
        for (int h = 0; h < 2; ++h) { q.Et[h] = s.Et[h]; q.Ec[h] = s.Ec[h]; q.wt[h] = s.wt[h]; q.bt[h] = s.bt[h]; q.wc[h] = s.wc[h]; q.bc[h] = s.bc[h]; q.GE[h] = s.GE[h]; }
        q.logp = s.logp; q.R = s.R; q.D = s.D; q.alpha_state = s.alpha_state; q.gamma = s.gamma; q.inv_batch = s.inv_batch; q.dq = s.dq; q.partial = s.partial;
        q.B = s.B; q.H = s.H; q.nblk = qhead_blocks(s.B); q.train = s.train ? 1 : 0; q.ldE = s.ldE;
        qw.w = s.w; qw.td = s.td;
    } break;
    case RLREP_HD_QHEAD_ACTOR: {
        const auto& s = a->qhead_actor;
        what = "qhead actor"; form = s.form;
        if (s.B <= 0 || s.H <= 0) HD_REFUSE("%s: B %d, H %d: non-positive extent", what, s.B, s.H)
        for (int h = 0; h < 2; ++h) {
            if (!s.Ec[h] || !s.wc[h] || !s.bc[h] || !s.GE[h]) HD_REFUSE("%s: head %d: null Ec, wc, bc or GE", what, h)
            if (!al4({s.Ec[h], s.wc[h], s.bc[h], s.GE[h]})) HD_REFUSE("%s: head %d: a pointer off a 4-byte boundary", what, h)
        }
        if (!s.logp || !s.alpha_state || !s.partial_loss || !s.partial_c) HD_REFUSE("%s: null logp, alpha_state, partial_loss or partial_c", what)
        if (s.ldE != 0 && s.ldE < s.H) HD_REFUSE("%s: ldE %d below H %d (0: dense)", what, s.ldE, s.H)
        if (!al(s.alpha_state, 8)) HD_REFUSE("%s: alpha_state off an 8-byte boundary", what)
        if (!al4({s.logp, s.partial_loss, s.partial_c})) HD_REFUSE("%s: a pointer off a 4-byte boundary", what)
        memset(&qa, 0, sizeof(qa));
        for (int h = 0; h < 2; ++h) { qa.Ec[h] = s.Ec[h]; qa.wc[h] = s.wc[h]; qa.bc[h] = s.bc[h]; qa.GE[h] = s.GE[h]; }
        qa.logp = s.logp; qa.alpha_state = s.alpha_state; qa.inv_batch = s.inv_batch; qa.target_entropy = s.target_entropy;
        qa.partial_loss = s.partial_loss; qa.partial_c = s.partial_c; qa.B = s.B; qa.H = s.H; qa.nblk = qhead_blocks(s.B); qa.ldE = s.ldE;
    } break;
    }
    if (form) { form[0] = gemm ? 1 : 0; form[1] = form1; }
    if (!launch) return 0;
    int rc = 0;
    if (gemm) {
        const int nf = rl_gemm16_pick_nf(gb.t, gb.ntasks);
        const int total = rl_gemm16_number_tiles(gb.t, gb.ntasks, nf);
        rc = rl_launch_gemm16(la, lb, nf, &gb, total, st);
    } else switch (kind) {
        case RLREP_HD_POLICY_FWD: rc = rl_launch_policy_fwd(&pf, st); break;
        case RLREP_HD_POLICY_BWD: rc = rl_launch_policy_bwd(&pb, st); break;
        case RLREP_HD_VAE_MID: rc = rl_launch_vae_mid(&vm, st); break;
        case RLREP_HD_HEADS_VAE: rc = rl_launch_heads_vae(&hv, st); break;
        case RLREP_HD_VAE_MSE: rc = rl_launch_vae_mse(&ms, st); break;
        case RLREP_HD_QHEAD_CRITIC: rc = a->qhead_critic.weighted ? rl_launch_qhead_critic_w(&qw, st) : rl_launch_qhead_critic(&qw.q, st); break;
        case RLREP_HD_QHEAD_ACTOR: rc = rl_launch_qhead_actor(&qa, st); break;
    }
    if (rc != 0) { rl_set_error("heads: %s: launch failed (%d)", what, rc); return rc < 0 ? RLREP_ERR_ARG : RLREP_ERR_HIP; }
    return 0;
}
#undef HD_REFUSE

int32_t rlrep_chain_status(rlrep_agent* ag, uint32_t* status, void* stream) {
    GROUP_REFUSE("chain_status")
    if (!ag || !ag->xc_err) { rl_set_error("chain_status: bad argument"); return RLREP_ERR_ARG; }
    unsigned w = 0;
    hipError_t e = hipMemcpyAsync(&w, ag->xc_err, sizeof(w), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { rl_set_error("chain_status: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    if (status) *status = w;
    if (w) {
        rl_set_error("a persistent chain launch failed its run-time checks (word %u:%s%s); results are invalid -- leaving xchain out of RLREP_ENABLE runs one launch per stage",
                     w, (w & 5u) ? " wait timed out" : "", (w & 2u) ? " workgroups of a group on different XCDs" : "");
        return RLREP_ERR_STATE;
    }
    return 0;
}

__global__ void debug_stamp_kernel(long long* ring, int cap, int tag) {
    const unsigned long long i = atomicAdd((unsigned long long*)ring, 1ull);
    ring[1 + (long long)(i % (unsigned long long)cap)] = (long long)((wall_clock64() << 8) | (unsigned long long)(tag & 255));
}
int32_t rlrep_debug_stamp(int64_t* ring, int32_t cap, int32_t tag, void* stream) {
    if (!ring || cap <= 0) { rl_set_error("debug_stamp: bad argument"); return RLREP_ERR_ARG; }
    hipLaunchKernelGGL(debug_stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)ring, (int)cap, (int)tag);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { rl_set_error("debug_stamp: %s", hipGetErrorString(e)); return RLREP_ERR_HIP; }
    return 0;
}

int32_t rlrep_history(rlrep_agent* ag, int32_t on) {
    if (!ag) { rl_set_error("history: bad argument"); return RLREP_ERR_ARG; }
    ag->hist_on = on != 0;
    return 0;
}
int32_t rlrep_history_dev(rlrep_agent* ag, const float** ring, const int32_t** seq, int32_t* records, int32_t* record_floats, int32_t* tag_word) {
    if (!ag || !ag->hist) { rl_set_error("history_dev: bad argument"); return RLREP_ERR_ARG; }
    if (ring) *ring = ag->hist;
    if (seq) *seq = ag->hist_seq;
    if (records) *records = RL_HIST_N;
    if (record_floats) *record_floats = RL_HIST_REC;
    if (tag_word) *tag_word = RL_HIST_TAG;
    return 0;
}

int32_t rlrep_build_flags(void) {
#ifdef RL_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

const float* rlrep_metrics_dev(rlrep_agent* ag) { return ag ? ag->metrics : nullptr; }
int64_t rlrep_launch_counter(void) { return g_rl_launches; }
// rlrep_comm_attach (comm.hip): from now on the optimizer launches of the attached groups carry the data-parallel exchange, and -- with
// exchange scratch -- the feature step carries its batch-coupled exchanges (the programs are rebuilt)
extern "C" int rl_agent_attach_dp(rlrep_agent* ag, const DpAttach* at, int* attached_mask) {
    GROUP_REFUSE("attach_dp")
    if (!ag || !at) return RLREP_ERR_ARG;
    const DpPull* proto = &at->proto;
    if (proto->world != ag->h.world_size) { rl_set_error("comm_attach: the comm spans %d ranks, the agent was created with world_size = %d", proto->world, ag->h.world_size); return RLREP_ERR_ARG; }
    if (proto->world > 1 && proto->rank != ag->d.rank) { rl_set_error("comm_attach: the comm's rank is %d, the agent's dims.rank %d", proto->rank, ag->d.rank); return RLREP_ERR_ARG; }
    if (ag->a.grad_dev != proto->base[proto->rank]) { rl_set_error("comm_attach: the agent's gradient arena is not the comm's arena (create the agent with rlrep_comm_arena() as grad_dev)"); return RLREP_ERR_ARG; }
    rlrep_layout_info info;
    if (rlrep_layout(&ag->d, &info, nullptr, 0) != 0) return RLREP_ERR_ARG;
    if (at->arena_floats < info.grad_floats) { rl_set_error("comm_attach: the comm's arena holds %lld floats, the gradient arena needs %lld", at->arena_floats, (long long)info.grad_floats); return RLREP_ERR_ARG; }
    // Co-residency (dp_pull.h, "Progress with SEVERAL channels in flight"): the blocks of the two largest attached optimizer launches (riders
    // included: two minibatch gathers of at most 2048 blocks are NOT counted -- they wait for nothing and drain) must fit the chip together.
    int occ1 = 0, occ2 = 0, cus = 0, dev = 0;
    if (proto->world > 1) {
        if (rl_adam_dp_occupancy(&occ1, &occ2) != 0 || hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
            rl_set_error("comm_attach: cannot query the occupancy of the optimizer kernels"); return RLREP_ERR_HIP;
        }
    }
    ag->dp_proto = *proto;
    int mask = 0;
    long long blocks[4] = {0, 0, 0, 0};
    for (int g = 0; g < 4; ++g) {
        const bool on = proto->world > 1 && ag->L.group_n[g] > 0 && ag->L.group_n[g] <= at->max_floats;
        ag->dp_on[g] = on;
        ag->dp_two[g] = on && proto->world >= 3 && at->two_shot_floats > 0 && ag->L.group_n[g] >= at->two_shot_floats && proto->red[proto->rank] != nullptr;
        if (on) { mask |= 1 << g; blocks[g] = (ag->L.group_n[g] + 1023) / 1024 + 1 + 256; }       // optimizer blocks + trailing block + a folded snapshot's segments
    }
    // the two largest attached launches must fit the chip together; a group that does not leave room for a second one is NOT attached (its
    // gradients stay with the caller's all-reduce, as for every group above max_floats) -- largest first, until the bound holds
    const long long slots = (long long)cus * std::min(occ1, occ2 > 0 ? occ2 : occ1);
    while (mask) {
        int g0 = -1, g1 = -1;
        for (int g = 0; g < 4; ++g) if (mask & (1 << g)) { if (g0 < 0 || blocks[g] > blocks[g0]) { g1 = g0; g0 = g; } else if (g1 < 0 || blocks[g] > blocks[g1]) g1 = g; }
        if (blocks[g0] + (g1 >= 0 ? blocks[g1] : 0) <= slots) break;
        mask &= ~(1 << g0); ag->dp_on[g0] = ag->dp_two[g0] = false;
    }
    // batch-coupled exchanges: only when the feature group itself is attached (a train() is then one uninterrupted sequence of launches)
    const long long need = exchange_floats(ag->d, proto->world);
    const bool was = ag->xfold;
    ag->xfold = proto->world > 1 && ag->dp_on[0] && need > 0 && at->scratch_floats >= need && at->scratch[proto->rank] != nullptr && !rl_off("dp_fold_exchanges");
    ag->xscratch_floats = at->scratch_floats; ag->xarena_floats = at->arena_floats;
    for (int q = 0; q < RL_DP_MAX_WORLD; ++q) ag->xscratch[q] = q < proto->world ? at->scratch[q] : nullptr;
    if (attached_mask) *attached_mask = mask;
    if ((ag->xfold || was) && ag->B > 0) {
        (void)hipDeviceSynchronize();                      // (table re-upload uses blocking copies: rare path, once per attachment)
        return build_programs(ag, ag->B);
    }
    return 0;
}
int32_t rlrep_front_end_counts(int64_t* out4) {
    if (!out4) return RLREP_ERR_ARG;
    for (int q = 0; q < 4; ++q) out4[q] = g_rl_front[q];
    return 0;
}
int32_t rlrep_last_launch_count(rlrep_agent* ag) { return ag ? ag->last_launches : 0; }

}  // extern "C"
