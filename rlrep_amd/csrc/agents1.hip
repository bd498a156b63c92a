// Step programs of sac and vlsac and the actor / critic stages every agent shares (host side; kernels in gemm16.hip / noisecritic.hip /
// elementwise.hip): a short list of grouped launches per step.  ctrlsac, spedersac and diffsrsac: agents2.hip.
#include "engine_internal.h"

// ================================================================================================
// agent
// ================================================================================================
// rows processed per qhead block loop: grid <= 128 blocks of 4 waves
int qhead_blocks(int B) { int g = (B + 3) / 4; return g > 128 ? 128 : g; }

// ------------------------------------------------------------------------------------------------
// shared fragments: actor forward / backward, actor+alpha apply
// ------------------------------------------------------------------------------------------------

ActorBufs alloc_actor(Builder& b, int B, int A, int Ha) {
    ActorBufs r;
    r.A1 = b.ws.f((size_t)B * Ha); r.A2 = b.ws.f((size_t)B * Ha); r.AO = b.ws.f((size_t)B * 2 * A);
    r.logp = b.ws.f(B); r.dA = b.ws.f((size_t)B * A); r.Ghead = b.ws.f((size_t)B * 2 * A);
    r.GA2 = b.ws.f((size_t)B * Ha); r.GA1 = b.ws.f((size_t)B * Ha);
    return r;
}

// GEMM tasks of the three actor trunk layers on input X[B, S] (row stride ldx)
GemmTask actor_l(rlrep_agent* ag, int layer, const float* X, int ldx, const ActorBufs& ab) {
    const int S = ag->d.state_dim, A = ag->d.action_dim, Ha = ag->d.actor_hidden_dim, B = ag->B;
    if (layer == 0) return Builder::fwd(X, ldx, B, S, ag->P("actor.trunk.0.weight"), S, ag->P("actor.trunk.0.bias"), Ha, ab.A1, Ha, ACT_ELU);
    if (layer == 1) return Builder::fwd(ab.A1, Ha, B, Ha, ag->P("actor.trunk.2.weight"), Ha, ag->P("actor.trunk.2.bias"), Ha, ab.A2, Ha, ACT_ELU);
    return Builder::fwd(ab.A2, Ha, B, Ha, ag->P("actor.trunk.4.weight"), Ha, ag->P("actor.trunk.4.bias"), 2 * A, ab.AO, 2 * A, ACT_NONE);
}

void policy_fwd_stage(Program& p, rlrep_agent* ag, const ActorBufs& ab, float* act, int ld_act, const char* what) {
    PolicyFwd pf; memset(&pf, 0, sizeof(pf));
    pf.O = ab.AO; pf.B = ag->B; pf.A = ag->d.action_dim; pf.act = act; pf.ld_act = ld_act; pf.logp = ab.logp;
    p.stages.push_back({[=](hipStream_t st) { PolicyFwd q = pf; q.eps = ag->cur_eps; return rl_launch_policy_fwd(&q, st); }, what});
}

// the tanh-Gaussian sampling runs in the head GEMM's epilogue when [mu | rho] fits one 16-column tile
bool policy_fusable(const rlrep_agent* ag) { return 2 * ag->d.action_dim <= 16 && !rl_off("fuse_policy"); }
GemmTask policy_head_task(rlrep_agent* ag, const ActorBufs& ab, float* act, int ld_act, int dyn_flag) {
    GemmTask head = actor_l(ag, 2, nullptr, 0, ab);
    rl_task_policy_head(head, ag->d.action_dim, act, ld_act, ab.logp, dyn_flag);
    return head;
}

void actor_head_stage(Builder& b, Program& p, rlrep_agent* ag, const ActorBufs& ab, float* act, int ld_act, std::vector<GemmTask> extra, const char* what) {
    GemmTask head = actor_l(ag, 2, nullptr, 0, ab);
    if (policy_fusable(ag)) {
        extra.insert(extra.begin(), policy_head_task(ag, ab, act, ld_act, FLAG_DYN_EPS));
        b.fwd_stage(p, extra, what);
    } else {
        extra.insert(extra.begin(), head);
        b.fwd_stage(p, extra, what);
        policy_fwd_stage(p, ag, ab, act, ld_act, "policy");
    }
}

// policy head backward + trunk backward + weight gradients (X = actor input with row stride ldx)
void actor_backward(Builder& b, Program& p, rlrep_agent* ag, const ActorBufs& ab, const float* X, int ldx,
                           const float* act, int ld_act, GemmTask action_dx) {
    const int S = ag->d.state_dim, A = ag->d.action_dim, Ha = ag->d.actor_hidden_dim, B = ag->B;
    if (A <= 16 && !rl_off("fuse_policy")) {
        rl_task_policy_bwd(action_dx, A, ab.AO, act, ld_act, ab.Ghead, ag->a.alpha_state_dev, ag->inv_batch(), FLAG_DYN_EPS);
        b.dx_stage(p, {action_dx}, "dx(action) -> dL/d[mu|rho]");
    } else {
        b.dx_stage(p, {action_dx}, "dx(action)");
        PolicyBwd pb; memset(&pb, 0, sizeof(pb));
        pb.O = ab.AO; pb.act = act; pb.ld_act = ld_act; pb.dA = ab.dA; pb.ld_dA = A;
        pb.alpha_state = ag->a.alpha_state_dev; pb.inv_batch = ag->inv_batch(); pb.G = ab.Ghead; pb.B = B; pb.A = A;
        p.stages.push_back({[=](hipStream_t st) { PolicyBwd q = pb; q.eps = ag->cur_eps; return rl_launch_policy_bwd(&q, st); }, "policy_bwd"});
    }
    // the head's dX (inner length 2A <= 32) is recomputed by every tile of the second layer's dX launch (FLAG_PRE | FLAG_PRE_ELU): one launch less
    b.dx_stage12(p, Builder::dx(ab.Ghead, 2 * A, B, 2 * A, ag->P("actor.trunk.4.weight"), Ha, ab.GA2, Ha, Ha, ACT_ELU, ab.A2, Ha),
                 Builder::dx(ab.GA2, Ha, B, Ha, ag->P("actor.trunk.2.weight"), Ha, ab.GA1, Ha, Ha, ACT_ELU, ab.A1, Ha), "actor.head dx", "actor.head dx + actor.l2 dx");
    b.dw_stage(p, {Builder::dw(ab.Ghead, 2 * A, 2 * A, ab.A2, Ha, Ha, B, ag->G("actor.trunk.4.weight"), Ha, ag->G("actor.trunk.4.bias")),
                   Builder::dw(ab.GA2, Ha, Ha, ab.A1, Ha, Ha, B, ag->G("actor.trunk.2.weight"), Ha, ag->G("actor.trunk.2.bias")),
                   Builder::dw(ab.GA1, Ha, Ha, X, ldx, S, B, ag->G("actor.trunk.0.weight"), S, ag->G("actor.trunk.0.bias"))},
               "actor dW");
}

std::vector<FinTask> actor_fins(rlrep_agent* ag, const float* partial_loss, int nblk) {
    FinTask fa; memset(&fa, 0, sizeof(fa));
    fa.kind = FIN_ALPHA; fa.partials = ag->Gtail(); fa.count = nblk; fa.stride = 1; fa.scale = ag->inv_batch();
    fa.out = ag->metrics + M_ALPHA_LOSS; fa.out2 = ag->metrics + M_ALPHA; fa.alpha_state = ag->a.alpha_state_dev;
    fa.lr = ag->h.lr_actor; fa.beta1 = ag->h.beta1; fa.beta2 = ag->h.beta2; fa.eps = ag->h.adam_eps; fa.learn = ag->h.learn_alpha;
    // the actor's optimizer launch is the last one of a train(): it also files the call's metrics in the history ring (rlrep_history)
    return {Builder::fin_sum(partial_loss, nblk, 1, 1.0f / (float)ag->B, ag->metrics + M_ACTOR_LOSS), fa, Builder::fin_history(ag)};
}
void actor_apply_program(Builder& b, rlrep_agent* ag, const float* partial_loss, int nblk) {
    b.adam(ag->actor_apply, 2, ag->h.lr_actor, nullptr, 0, 0, 0.f, actor_fins(ag, partial_loss, nblk), "adam actor + alpha");
}

void update_target_program(rlrep_agent* ag, const std::string& first_src, const std::string& first_dst) {
    // critic -> critic_target over the whole critic group (identical internal layouts)
    PolyakTask t; memset(&t, 0, sizeof(t));
    t.src = ag->a.param_dev ? ag->a.param_dev + ag->L.group_off[1] : nullptr;
    t.dst = ag->a.target_dev ? ag->a.target_dev + ag->L.get(first_dst).off : nullptr;
    (void)first_src;
    t.n = ag->L.group_n[1]; t.tau = ag->h.tau; t.steps = ag->steps; t.period = ag->h.target_update_period;
    ag->upd_target.stages.push_back({[=](hipStream_t st) { return rl_launch_polyak(&t, st); }, "polyak critic"});
}
// critic Adam with the target update folded in (same Polyak, same period gate, run by the Adam launch's own lanes)
void critic_apply_folded(Builder& b, rlrep_agent* ag, const std::string& first_dst, std::vector<FinTask> fins, Program* into, const int* steps) {
    if (!into && rl_off("fold_target")) return;
    float* dst = ag->a.target_dev ? ag->a.target_dev + ag->L.get(first_dst).off : nullptr;
    b.adam(into ? *into : ag->critic_apply_f, 1, ag->h.lr_critic, dst, ag->L.group_off[1], ag->L.group_n[1], ag->h.tau, fins, "adam critic + polyak critic",
           steps ? steps : ag->steps, ag->h.target_update_period);
}

// ================================================================================================
// SAC   (agent/sac/sac_agent.py:105-166)
// ================================================================================================
void build_sac(Builder& b, rlrep_agent* ag) {
    const int S = ag->d.state_dim, A = ag->d.action_dim, H = ag->d.hidden_dim, Ha = ag->d.actor_hidden_dim, B = ag->B;
    const int SA = S + A;
    Slot& s0 = ag->slot[0];
    ActorBufs ab = alloc_actor(b, B, A, Ha);               // policy on s' (critic step)
    ActorBufs ab_pi = alloc_actor(b, B, A, Ha);            // policy on s  (actor step)
    float* E1t = b.ws.f((size_t)B * 2 * H);       // target first-layer activations [B, 2H] (Q1|Q2)
    float* E1c = b.ws.f((size_t)B * 2 * H);
    float* Et = b.ws.f((size_t)2 * B * H);        // second-layer activations, heads stacked [2][B,H]
    float* Ec = b.ws.f((size_t)2 * B * H);
    float* GE = b.ws.f((size_t)2 * B * H);
    float* G1 = b.ws.f((size_t)B * 2 * H);
    float* dq = b.ws.f((size_t)2 * B);
    const int nblk = qhead_blocks(B);
    float* part_q = b.ws.f((size_t)4 * nblk);
    float* part_l = b.ws.f(nblk);
    ag->per_td = b.ws.f(B);                       // |TD| of the weighted critic head (prioritized replay: rlrep_per_update reads it)
    auto Pw = [&](const char* n) { return ag->P(n); };
    auto Tw = [&](const char* n) { return ag->T(n); };

    // ---- critic step ----
    // hoist: the variant that also carries the forward half of the FOLLOWING actor step (policy on s): its three layers read nothing the
    // critic update writes, and as extra tasks of launches that exist anyway they take three launches off train() (rlrep_prefetch_policy)
    const bool can_hoist = policy_fusable(ag) && !rl_off("hoist");
    // weighted (prioritized replay, rlrep_critic_step_weighted): the head stage is the kernel that takes per-sample weights and leaves |TD|
    // (per.hip); every other stage, the partials and the apply programs are the unweighted ones
    auto critic_program = [&](Program& p, bool hoist, bool emit_apply, bool weighted = false) {
        if (hoist) {
            b.fwd_stage(p, {actor_l(ag, 0, s0.XF2, SA, ab), actor_l(ag, 0, s0.XFpi, SA, ab_pi)}, "actor.l1(s') actor.l1(s)");
            b.fwd_stage(p, {actor_l(ag, 1, nullptr, 0, ab), actor_l(ag, 1, nullptr, 0, ab_pi)}, "actor.l2 x2");
            b.fwd_stage(p, {policy_head_task(ag, ab, s0.XF2 + S, SA, FLAG_DYN_EPS), policy_head_task(ag, ab_pi, s0.XFpi + S, SA, FLAG_DYN_EPS2)},
                        "actor.head x2 + policy");
        } else {
            b.fwd_stage(p, {actor_l(ag, 0, s0.XF2, SA, ab)}, "actor.l1(s')");
            b.fwd_stage(p, {actor_l(ag, 1, nullptr, 0, ab)}, "actor.l2");
            actor_head_stage(b, p, ag, ab, s0.XF2 + S, SA, {}, "actor.head + policy");
        }
        b.fwd_stage(p, {Builder::fwd(s0.XF2, SA, B, SA, Tw("critic_target.Q1.0.weight"), SA, Tw("critic_target.Q1.0.bias"), 2 * H, E1t, 2 * H, ACT_ELU),
                        Builder::fwd(s0.XF, SA, B, SA, Pw("critic.Q1.0.weight"), SA, Pw("critic.Q1.0.bias"), 2 * H, E1c, 2 * H, ACT_ELU)}, "Q l1");
        b.fwd_stage(p, {Builder::fwd(E1t, 2 * H, B, H, Tw("critic_target.Q1.2.weight"), H, Tw("critic_target.Q1.2.bias"), H, Et, H, ACT_ELU),
                        Builder::fwd(E1t + H, 2 * H, B, H, Tw("critic_target.Q2.2.weight"), H, Tw("critic_target.Q2.2.bias"), H, Et + (size_t)B * H, H, ACT_ELU),
                        Builder::fwd(E1c, 2 * H, B, H, Pw("critic.Q1.2.weight"), H, Pw("critic.Q1.2.bias"), H, Ec, H, ACT_ELU),
                        Builder::fwd(E1c + H, 2 * H, B, H, Pw("critic.Q2.2.weight"), H, Pw("critic.Q2.2.bias"), H, Ec + (size_t)B * H, H, ACT_ELU)}, "Q l2");
        QHeadCritic q; memset(&q, 0, sizeof(q));
        q.Et[0] = Et; q.Et[1] = Et + (size_t)B * H; q.Ec[0] = Ec; q.Ec[1] = Ec + (size_t)B * H;
        q.wt[0] = Tw("critic_target.Q1.4.weight"); q.wt[1] = Tw("critic_target.Q2.4.weight");
        q.bt[0] = Tw("critic_target.Q1.4.bias"); q.bt[1] = Tw("critic_target.Q2.4.bias");
        q.wc[0] = Pw("critic.Q1.4.weight"); q.wc[1] = Pw("critic.Q2.4.weight");
        q.bc[0] = Pw("critic.Q1.4.bias"); q.bc[1] = Pw("critic.Q2.4.bias");
        q.logp = ab.logp; q.R = s0.R; q.D = s0.D; q.alpha_state = ag->a.alpha_state_dev; q.gamma = ag->h.discount;
        q.inv_batch = ag->inv_batch(); q.dq = dq; q.GE[0] = GE; q.GE[1] = GE + (size_t)B * H; q.partial = part_q;
        q.B = B; q.H = H; q.nblk = nblk; q.train = 1; q.step = ag->adam_step + 1;
        if (weighted) {
            float* td = ag->per_td;
            p.stages.push_back({[=](hipStream_t st) { QHeadCriticW qw; qw.q = q; qw.w = ag->cur_w; qw.td = td; return rl_launch_qhead_critic_w(&qw, st); },
                                "qhead critic (weighted)"});
        } else
        p.stages.push_back({[=](hipStream_t st) { return rl_launch_qhead_critic(&q, st); }, "qhead critic"});
        b.dx_stage(p, {Builder::dx(GE, H, B, H, Pw("critic.Q1.2.weight"), H, G1, 2 * H, H, ACT_ELU, E1c, 2 * H),
                       Builder::dx(GE + (size_t)B * H, H, B, H, Pw("critic.Q2.2.weight"), H, G1 + H, 2 * H, H, ACT_ELU, E1c + H, 2 * H)}, "Q l2 dx");
        b.dw_stage(p, {Builder::dw(dq, 1, 1, Ec, H, H, B, ag->G("critic.Q1.4.weight"), H, ag->G("critic.Q1.4.bias")),
                       Builder::dw(dq + B, 1, 1, Ec + (size_t)B * H, H, H, B, ag->G("critic.Q2.4.weight"), H, ag->G("critic.Q2.4.bias")),
                       Builder::dw(GE, H, H, E1c, 2 * H, H, B, ag->G("critic.Q1.2.weight"), H, ag->G("critic.Q1.2.bias")),
                       Builder::dw(GE + (size_t)B * H, H, H, E1c + H, 2 * H, H, B, ag->G("critic.Q2.2.weight"), H, ag->G("critic.Q2.2.bias")),
                       Builder::dw(G1, 2 * H, 2 * H, s0.XF, SA, SA, B, ag->G("critic.Q1.0.weight"), SA, ag->G("critic.Q1.0.bias"))}, "Q dW");
        // sac reports q_loss = mse1+mse2 and q2 := q1 (quirk Q13)
        const float ib = 1.0f / (float)B;
        const std::vector<FinTask> cfins = {Builder::fin_sum(part_q + 0, nblk, 4, ib, ag->metrics + M_TMP0),
                Builder::fin_sum(part_q + 1, nblk, 4, ib, ag->metrics + M_TMP1),
                Builder::fin_combine(ag->metrics + M_TMP0, 1.f, ag->metrics + M_TMP1, 1.f, ag->metrics + M_Q1_LOSS),
                Builder::fin_sum(part_q + 2, nblk, 4, ib, ag->metrics + M_Q1),
                Builder::fin_copy(ag->metrics + M_Q1, ag->metrics + M_Q2)};
        if (emit_apply) {
            b.adam(ag->critic_apply, 1, ag->h.lr_critic, nullptr, 0, 0, 0.f, cfins, "adam critic");
            critic_apply_folded(b, ag, "critic_target.Q1.0.weight", cfins);
        }
    };
    critic_program(ag->critic_bwd, false, true);
    if (can_hoist) critic_program(ag->critic_bwd_h, true, false);
    if (ag->h.world_size <= 1) {          // (one GPU; a seed group's head stage launches its group form, per_group.hip)
        critic_program(ag->critic_bwd_w, false, false, true);
        if (can_hoist) critic_program(ag->critic_bwd_wh, true, false, true);
    }
    // ---- actor step ----
    {
        Program& p = ag->actor_bwd;
        b.fwd_stage(p, {actor_l(ag, 0, s0.XFpi, SA, ab_pi)}, "actor.l1(s)");
        b.fwd_stage(p, {actor_l(ag, 1, nullptr, 0, ab_pi)}, "actor.l2");
        actor_head_stage(b, p, ag, ab_pi, s0.XFpi + S, SA, {}, "actor.head + policy");
        ag->actor_resume = (int)p.stages.size();              // everything above is what critic_bwd_h already did
        b.fwd_stage(p, {Builder::fwd(s0.XFpi, SA, B, SA, Pw("critic.Q1.0.weight"), SA, Pw("critic.Q1.0.bias"), 2 * H, E1c, 2 * H, ACT_ELU)}, "Q l1");
        b.fwd_stage(p, {Builder::fwd(E1c, 2 * H, B, H, Pw("critic.Q1.2.weight"), H, Pw("critic.Q1.2.bias"), H, Ec, H, ACT_ELU),
                        Builder::fwd(E1c + H, 2 * H, B, H, Pw("critic.Q2.2.weight"), H, Pw("critic.Q2.2.bias"), H, Ec + (size_t)B * H, H, ACT_ELU)}, "Q l2");
        QHeadActor q; memset(&q, 0, sizeof(q));
        q.Ec[0] = Ec; q.Ec[1] = Ec + (size_t)B * H;
        q.wc[0] = Pw("critic.Q1.4.weight"); q.wc[1] = Pw("critic.Q2.4.weight");
        q.bc[0] = Pw("critic.Q1.4.bias"); q.bc[1] = Pw("critic.Q2.4.bias");
        q.logp = ab_pi.logp; q.alpha_state = ag->a.alpha_state_dev; q.inv_batch = ag->inv_batch(); q.target_entropy = ag->h.target_entropy;
        q.GE[0] = GE; q.GE[1] = GE + (size_t)B * H; q.partial_loss = part_l; q.partial_c = ag->Gtail();
        q.B = B; q.H = H; q.nblk = nblk; q.step = ag->adam_step + 2;
        p.stages.push_back({[=](hipStream_t st) { return rl_launch_qhead_actor(&q, st); }, "qhead actor"});
        b.dx_stage(p, {Builder::dx(GE, H, B, H, Pw("critic.Q1.2.weight"), H, G1, 2 * H, H, ACT_ELU, E1c, 2 * H),
                       Builder::dx(GE + (size_t)B * H, H, B, H, Pw("critic.Q2.2.weight"), H, G1 + H, 2 * H, H, ACT_ELU, E1c + H, 2 * H)}, "Q l2 dx");
        // both heads at once: [G1_1 | G1_2] [B,2H] x [W_Q1.0 ; W_Q2.0][:, S:S+A]
        actor_backward(b, p, ag, ab_pi, s0.XFpi, SA, s0.XFpi + S, SA, Builder::dx(G1, 2 * H, B, 2 * H, Pw("critic.Q1.0.weight") ? Pw("critic.Q1.0.weight") + S : nullptr, SA, ab_pi.dA, A, A, ACT_NONE, nullptr, 0));
        actor_apply_program(b, ag, part_l, nblk);
    }
    update_target_program(ag, "critic.Q1.0.weight", "critic_target.Q1.0.weight");
}

// ================================================================================================
// VLSAC   (agent/vlsac/vlsac_agent.py:126-273)
// ================================================================================================
struct GaussBufs { float *H1, *H2, *HH; };

static void gauss_tasks(rlrep_agent* ag, bool target, const std::string& m, const float* X, int ldx, int K, const GaussBufs& g,
                        GemmTask (&out)[3]) {
    const int Hv = ag->d.vae_hidden_dim, F = ag->d.feature_dim, B = ag->B;
    auto W = [&](const std::string& n) { return target ? ag->T(m + n) : ag->P(m + n); };
    out[0] = Builder::fwd(X, ldx, B, K, W(".l1.weight"), K, W(".l1.bias"), Hv, g.H1, Hv, ACT_RELU);
    out[1] = Builder::fwd(g.H1, Hv, B, Hv, W(".l2.weight"), Hv, W(".l2.bias"), Hv, g.H2, Hv, ACT_RELU);
    out[2] = Builder::fwd(g.H2, Hv, B, Hv, W(".mean_linear.weight"), Hv, W(".mean_linear.bias"), 2 * F, g.HH, 2 * F, ACT_NONE);
}

void build_vlsac(Builder& b, rlrep_agent* ag) {
    const int S = ag->d.state_dim, A = ag->d.action_dim, H = ag->d.hidden_dim, Ha = ag->d.actor_hidden_dim, B = ag->B;
    const int F = ag->d.feature_dim, Hv = ag->d.vae_hidden_dim, N = ag->d.num_noise;
    const int SA = S + A, KE = 2 * S + A;
    Slot& s0 = ag->slot[0];
    Workspace& ws = b.ws;
    // use_feature_target=False (vlsac_agent.py:176-179, 214-219, 257-258): critic and actor steps read the LIVE f, no Polyak into f_target
    const bool nft = (ag->d.flags & RLREP_FLAG_NO_FEATURE_TARGET) != 0;
    const std::string fnet = nft ? "f" : "f_target";
    auto FT = [&](const char* n) { return nft ? ag->P(std::string("f.") + n) : ag->T(std::string("f_target.") + n); };
    auto Pw = [&](const char* n) { return ag->P(n); };
    auto Tw = [&](const char* n) { return ag->T(n); };
    auto Gw = [&](const char* n) { return ag->G(n); };

    // ---- feature step buffers ----
    GaussBufs ge{ws.f((size_t)B * Hv), ws.f((size_t)B * Hv), ws.f((size_t)B * 2 * F)};
    GaussBufs gf{ws.f((size_t)B * Hv), ws.f((size_t)B * Hv), ws.f((size_t)B * 2 * F)};
    float* Z = ws.f((size_t)B * F); float* EZ = ws.f((size_t)B * F);
    float* D1 = ws.f((size_t)B * Hv);
    float* GDH = ws.f((size_t)B * (S + 1)); float* GD1 = ws.f((size_t)B * Hv);
    float* GEH = ws.f((size_t)B * 2 * F); float* GFH = ws.f((size_t)B * 2 * F);
    float* GH2e = ws.f((size_t)B * Hv); float* GH1e = ws.f((size_t)B * Hv);
    float* GH2f = ws.f((size_t)B * Hv); float* GH1f = ws.f((size_t)B * Hv);
    // the Gaussian heads of encoder and f and vae_mid as ONE launch (heads_vae_kernel: a 16 x 16 tile per workgroup, one KL partial each;
    // +3 % against the heads launch + an elementwise vae_mid launch, which is gone)
    // dec.heads + mse inside the dec.l1 dX launch (FLAG_PRE_MSE): needs the 16-byte-aligned rows its first phase loads, K1 = S + 1 <= 32
    const bool fold_mse = !rl_rowprog_enabled() && !Builder::chain_enabled() && (Hv & 3) == 0 && S + 1 <= 32 && !rl_off("fold_mse") && !rl_off("fuse_dx") &&
                          ((B + 15) / 16) * ((F + 15) / 16) < 384 * 2;
    const int tiles_vm = ((B + 15) / 16) * ((F + 15) / 16);
    const int nblk_kl = tiles_vm, nblk_mse_tiles = ((B + 15) / 16) * ((S + 1 + 15) / 16);   // mse partials: one pair per dec.heads tile
    const int nblk_mse = fold_mse ? (B + 15) / 16 : nblk_mse_tiles;                        // (folded: one pair per 16-row tile)
    float* part_kl = ws.f(nblk_kl); float* part_mse = ws.f((size_t)2 * nblk_mse_tiles);
    // actor buffers are needed by the feature program variant that carries the policy forwards
    ActorBufs ab = alloc_actor(b, B, A, Ha);                                                 // policy on s' (critic step)
    ActorBufs ab_pi = alloc_actor(b, B, A, Ha);                                              // policy on s  (actor step)
    // ---- the forward + dX chains of a feature step as ONE launch of row-block programs (rowprog.hip) -------------------------------
    // Two workgroups per 16-row block: program E runs encoder -> sample / KL -> decoder -> decoder and encoder backward, program F runs
    // f forward, publishes its heads to E (the KL term needs both Gaussians), receives dKL/d(f heads) and runs f's backward beside E's
    // decoder passes.  `early`: two more programs run both policy forwards (what the first three launches of feat_bwd_h carry).
    const int nrb = (B + RP_ROWS - 1) / RP_ROWS;
    const int nblk_rp = nrb;
    float* part_kl_rp = ws.f((size_t)nblk_rp * 8); float* part_mse_rp = ws.f((size_t)2 * nblk_rp);       // (KL: one partial per workgroup, up to 8 members per row block)
    int* rp_flags = (int*)ws.alloc(sizeof(int) * 2 * nrb);
    if (!b.dry && rp_flags && b.ws.ok()) (void)hipMemset(rp_flags, 0, sizeof(int) * 2 * nrb);
    auto rp_feature = [&](RpAsm& A_, bool early) {
        const bool pair = !rl_off("rowprog_pair");
        auto Wp = [&](const char* n) { return ag->P(n); };
        const bool useT = ag->nsh[0] > 0;
        // forward layer `name`: from the transposed shadow when the agent keeps one (wide layers), else from W itself
        auto FW = [&](const RpBuf& x, int K, const std::string& name, const std::string& bias_name, int N, int act, const RpBuf* d, float* gout, int ldg) {
            if (useT && N >= 64 && ag->shadow_of.count(name + ".weight")) A_.fwdT(x, K, ag->PT(name + ".weight"), ag->P(bias_name + ".bias"), N, act, d, gout, ldg);
            else A_.fwd(x, K, ag->P(name + ".weight"), K, ag->P(bias_name + ".bias"), N, act, d, gout, ldg);
        };
        auto f_forward = [&](RpBuf& x, RpBuf& h1, RpBuf& h2) {
            x = A_.buf(SA); h1 = A_.buf(Hv); h2 = A_.buf(Hv);
            A_.load(s0.XF, SA, SA, x);
            FW(x, SA, "f.l1", "f.l1", Hv, ACT_RELU, &h1, gf.H1, Hv);
            FW(h1, Hv, "f.l2", "f.l2", Hv, ACT_RELU, &h2, gf.H2, Hv);
        };
        auto f_backward = [&](const RpBuf& g, const RpBuf* m2, const RpBuf* m1, const RpBuf& g2) {
            A_.load(GFH, 2 * F, 2 * F, g);
            A_.dx(g, 2 * F, Wp("f.mean_linear.weight"), Hv, Hv, ACT_RELU, m2, gf.H2, Hv, &g2, GH2f, Hv);
            A_.dx(g2, Hv, Wp("f.l2.weight"), Hv, Hv, ACT_RELU, m1, gf.H1, Hv, nullptr, GH1f, Hv);
        };
        // ---- program E (and, unpaired, the whole step) ----
        A_.begin();
        RpBuf r0b = A_.buf(std::max(KE, S + 1)), r1 = A_.buf(std::max(Hv, F)), r2 = A_.buf(std::max(Hv, F)), rhh = A_.buf(2 * F),
              rfh = A_.buf(std::max(2 * F, Hv)), r5 = A_.buf(std::max(F, Hv));
        if (!pair) {
            // f forward first, on the regions the encoder is about to use; its heads land where the KL op expects them
            RpBuf x = RpAsm::at(r0b, SA), h1 = RpAsm::at(r1, Hv), h2 = RpAsm::at(r2, Hv), fh = RpAsm::at(rfh, 2 * F);
            A_.load(s0.XF, SA, SA, x);
            FW(x, SA, "f.l1", "f.l1", Hv, ACT_RELU, &h1, gf.H1, Hv);
            FW(h1, Hv, "f.l2", "f.l2", Hv, ACT_RELU, &h2, gf.H2, Hv);
            FW(h2, Hv, "f.mean_linear", "f.mean_linear", 2 * F, ACT_NONE, &fh, gf.HH, 2 * F);
        }
        {
            RpBuf x = RpAsm::at(r0b, KE), h1 = RpAsm::at(r1, Hv), h2 = RpAsm::at(r2, Hv);
            A_.load(s0.XE, KE, KE, x);
            FW(x, KE, "encoder.l1", "encoder.l1", Hv, ACT_RELU, &h1, ge.H1, Hv);
            FW(h1, Hv, "encoder.l2", "encoder.l2", Hv, ACT_RELU, &h2, ge.H2, Hv);
            FW(h2, Hv, "encoder.mean_linear", "encoder.mean_linear", 2 * F, ACT_NONE, &rhh, ge.HH, 2 * F);
        }
        const RpBuf fh = RpAsm::at(rfh, 2 * F), z = RpAsm::at(r1, F), ez = RpAsm::at(r2, F);
        if (pair) { A_.wait(0); A_.load(gf.HH, 2 * F, 2 * F, fh); }
        {
            RpOp o = RpAsm::blank(RP_VAE_MID);
            o.src = rhh.off; o.lds = rhh.ld; o.src2 = fh.off; o.lds2 = fh.ld; o.N = F; o.dyn = 0; o.s0 = ag->inv_batch() / (float)F;
            o.dst = z.off; o.ldd = z.ld; o.wpad = z.w; o.dst2 = ez.off; o.ldd2 = ez.ld;
            o.gout = Z; o.ldg = F; o.gout2 = GFH; o.ldg2 = 2 * F; o.part = part_kl_rp; o.step = ag->adam_step + 0; o.flags = RPF_BUMP;
            A_.ops.push_back(o);
        }
        if (pair) A_.signal(1);
        // the f heads are dead: their region takes the decoder's hidden layer, then dz; z's region takes the encoder's dL/dh2
        RpBuf d1 = RpAsm::at(rfh, Hv), dh = RpAsm::at(r0b, S + 1), gd1 = RpAsm::at(r5, Hv), dz = RpAsm::at(rfh, F), g2 = RpAsm::at(r1, Hv);
        FW(z, F, "decoder.l1", "decoder.l1", Hv, ACT_RELU, &d1, D1, Hv);
        A_.fwd(d1, Hv, Wp("decoder.state_linear.weight"), Hv, Wp("decoder.state_linear.bias"), S + 1, ACT_NONE, &dh, nullptr, 0);
        {
            RpOp o = RpAsm::blank(RP_MSE);
            o.src = dh.off; o.lds = dh.ld; o.n0 = S; o.gin = s0.XE ? s0.XE + SA : nullptr; o.ldgin = KE; o.gin2 = s0.R;
            o.s0 = ag->inv_batch() / (float)S; o.s1 = ag->inv_batch(); o.gout = GDH; o.ldg = S + 1; o.part = part_mse_rp;
            A_.ops.push_back(o);
        }
        A_.dx(dh, S + 1, Wp("decoder.state_linear.weight"), Hv, Hv, ACT_RELU, &d1, nullptr, 0, &gd1, GD1, Hv);
        A_.dx(gd1, Hv, Wp("decoder.l1.weight"), F, F, ACT_NONE, nullptr, nullptr, 0, &dz, nullptr, 0);
        {
            RpOp o = RpAsm::blank(RP_REPARAM);
            o.src = dz.off; o.lds = dz.ld; o.src2 = ez.off; o.lds2 = ez.ld; o.dst = rhh.off; o.ldd = rhh.ld; o.N = F; o.gout = GEH; o.ldg = 2 * F;
            A_.ops.push_back(o);
        }
        A_.dx(rhh, 2 * F, Wp("encoder.mean_linear.weight"), Hv, Hv, ACT_RELU, nullptr, ge.H2, Hv, &g2, GH2e, Hv);
        A_.dx(g2, Hv, Wp("encoder.l2.weight"), Hv, Hv, ACT_RELU, nullptr, ge.H1, Hv, nullptr, GH1e, Hv);
        if (!pair) {
            RpBuf g = RpAsm::at(rfh, 2 * F), gg2 = RpAsm::at(r2, Hv);
            f_backward(g, nullptr, nullptr, gg2);
        }
        A_.end(nrb);
        if (pair) {
            A_.begin();
            RpBuf x, h1, h2;
            f_forward(x, h1, h2);
            FW(h2, Hv, "f.mean_linear", "f.mean_linear", 2 * F, ACT_NONE, nullptr, gf.HH, 2 * F);
            A_.signal(0);
            RpBuf g = A_.buf(2 * F), gg2 = A_.buf(Hv);
            A_.wait(1);
            f_backward(g, &h2, &h1, gg2);
            A_.end(nrb);
        }
        if (early) {
            for (int which = 0; which < 2; ++which) {
                const ActorBufs& abx = which == 0 ? ab : ab_pi;
                const float* X = which == 0 ? s0.XF2 : s0.XFpi;
                A_.begin();
                RpBuf x = A_.buf(S), a1 = A_.buf(Ha), a2 = A_.buf(Ha), ao = A_.buf(2 * A);
                A_.load(X, SA, S, x);
                A_.fwd(x, S, Wp("actor.trunk.0.weight"), S, Wp("actor.trunk.0.bias"), Ha, ACT_ELU, &a1, abx.A1, Ha);
                A_.fwd(a1, Ha, Wp("actor.trunk.2.weight"), Ha, Wp("actor.trunk.2.bias"), Ha, ACT_ELU, &a2, abx.A2, Ha);
                A_.fwd(a2, Ha, Wp("actor.trunk.4.weight"), Ha, Wp("actor.trunk.4.bias"), 2 * A, ACT_NONE, &ao, abx.AO, 2 * A);
                RpOp o = RpAsm::blank(RP_POLICY);
                o.src = ao.off; o.lds = ao.ld; o.n0 = A; o.dyn = which == 0 ? 1 : 2;
                o.gout = const_cast<float*>(X) ? const_cast<float*>(X) + S : nullptr; o.ldg = SA; o.gout2 = abx.logp;
                A_.ops.push_back(o);
                A_.end(nrb);
            }
        }
    };
    // OPT-IN (RLREP_ENABLE=rowprog): measured on MI355X at the headline dimensions the fused launch takes 91-95 us against 44 us (stages timed
    // alone) / ~57 us (in the dependent chain) for the nine launches it replaces -- one CU per 16-row block ingests every weight matrix
    // (256 KB per 256 x 256 layer at ~50-65 GB/s per CU) and runs fp32 MFMA at 41-53 cycles per instruction: 5-6 us per layer and row
    // block, i.e. a dependent launch.  DESIGN.md section 5.2 has the per-op timeline.

    // ---- cluster form (RLREP_ENABLE=rowprog=2): C workgroups per row block and chain, member m owns a column slice of every layer and the
    // members complete each other's vectors through tagged 8-byte granules in global memory (RP_XCHG; tools/exp/cluster_hop.hip: 1.9-2.4 us
    // per hop with 256 workgroups exchanging at once).  Masks come from the activations in global memory (each member wrote its own slice).
    int CS = 0;                                   // cluster size: 0 = not applicable
    for (int c : {8, 4, 2}) if (!CS && Hv % c == 0 && F % c == 0 && (long long)nrb * c * 2 <= 256 && 16 * (2 * F / c) <= RP_XSLOT && 16 * (Hv / c) <= RP_XSLOT) CS = c;
    unsigned long long* xbuf = (unsigned long long*)ws.alloc(rl_rowprog_cluster() && CS ? (size_t)nrb * 2 * RP_MAX_HOPS * CS * RP_XSLOT * 8 : 8);
    auto rp_feature_cluster = [&](RpAsm& A_) {
        const int wh = Hv / CS, wf = F / CS;
        auto Wp = [&](const std::string& n) { return ag->P(n); };
        auto last = [&]() -> RpOp& { return A_.ops.back(); };
        // forward slice of layer `name` (N_total outputs; this member: columns col_base + m*ws .. + ws) from the transposed shadow
        auto fwdS = [&](const RpBuf& x, int K, const std::string& name, const std::string& bias_name, int Ntot, int col_base, int wsl, int act,
                        const RpBuf& dfull, float* gout, int ldg) {
            RpBuf d = dfull; d.off += col_base; d.w = wsl;
            const float* WT = ag->PT(name + ".weight");
            const float* bias = Wp(bias_name + ".bias");
            A_.fwdT(x, K, WT ? WT + col_base : nullptr, bias ? bias + col_base : nullptr, wsl, act, &d, gout ? gout + col_base : nullptr, ldg);
            RpOp& o = last(); o.ldw = Ntot; o.wpad = wsl; o.m_w = wsl; o.m_b = wsl; o.m_dst = wsl; o.m_g = wsl;
        };
        // dX slice: columns m*ws .. of (G W) masked by the activation in global memory
        auto dxS = [&](const RpBuf& g, int K, const float* W, int ldw, int wsl, int act, const float* mask_g, int ldmask, const RpBuf* dfull, bool slice_dst,
                       float* gout, int ldg) {
            RpBuf d; if (dfull) { d = *dfull; d.w = wsl; }
            A_.dx(g, K, W, ldw, wsl, act, nullptr, mask_g, ldmask, dfull ? &d : nullptr, gout, ldg);
            RpOp& o = last(); o.wpad = wsl; o.m_w = wsl; o.m_g = wsl; o.m_gaux = wsl; o.m_dst = slice_dst ? 0 : wsl;
        };
        // ---------------- program E ----------------
        A_.begin();
        {
            RpBuf bx = A_.buf(std::max(KE, S + 1)), bA = A_.buf(2 * F > Hv ? 2 * F : Hv), bB = A_.buf(2 * F > Hv ? 2 * F : Hv), bC = A_.buf(std::max(F, Hv));
            RpBuf ezs = A_.buf(wf), dzs = A_.buf(wf);
            A_.load(s0.XE, KE, KE, bx);
            fwdS(bx, KE, "encoder.l1", "encoder.l1", Hv, 0, wh, ACT_RELU, bA, ge.H1, Hv);
            A_.xop(RP_XCHG, bA, 0, wh, 1, 0);
            fwdS(bA, Hv, "encoder.l2", "encoder.l2", Hv, 0, wh, ACT_RELU, bB, ge.H2, Hv);
            A_.xop(RP_XCHG, bB, 1, wh, 1, 0);
            fwdS(bB, Hv, "encoder.mean_linear", "encoder.mean_linear", 2 * F, 0, wf, ACT_NONE, bA, ge.HH, 2 * F);
            fwdS(bB, Hv, "encoder.mean_linear", "encoder.mean_linear", 2 * F, F, wf, ACT_NONE, bA, ge.HH, 2 * F);
            A_.xop(RP_GATHER, bB, 2, wf, 2, F, 2);                      // my slice of the f heads, from member m of the F cluster (its hop 2)
            {
                RpOp o = RpAsm::blank(RP_VAE_MID);
                o.src = bA.off; o.lds = bA.ld; o.src2 = bB.off; o.lds2 = bB.ld; o.N = wf; o.K = F; o.wpad = wf; o.dyn = 0; o.s0 = ag->inv_batch() / (float)F;
                o.dst = bC.off; o.ldd = bC.ld; o.dst2 = ezs.off; o.ldd2 = ezs.ld;
                o.gout = Z; o.ldg = F; o.gout2 = GFH; o.ldg2 = 2 * F; o.part = part_kl_rp; o.step = ag->adam_step + 0; o.flags = RPF_BUMP | RPF_FH_INPLACE;
                o.m_src = wf; o.m_s2 = wf; o.m_dst = wf; o.m_g = wf; o.m_g2 = wf; o.m_gin = wf;
                A_.ops.push_back(o);
            }
            A_.xop(RP_PUBLISH, bB, 7, wf, 2, F);                        // dKL/d(f heads) for the F cluster
            A_.xop(RP_XCHG, bC, 2, wf, 1, 0);                           // z
            fwdS(bC, F, "decoder.l1", "decoder.l1", Hv, 0, wh, ACT_RELU, bB, D1, Hv);
            A_.xop(RP_XCHG, bB, 3, wh, 1, 0);
            RpBuf dh = RpAsm::at(bx, S + 1);
            A_.fwd(bB, Hv, Wp("decoder.state_linear.weight"), Hv, Wp("decoder.state_linear.bias"), S + 1, ACT_NONE, &dh, nullptr, 0);   // every member, whole
            {
                RpOp o = RpAsm::blank(RP_MSE);
                o.src = dh.off; o.lds = dh.ld; o.n0 = S; o.gin = s0.XE ? s0.XE + SA : nullptr; o.ldgin = KE; o.gin2 = s0.R;
                o.s0 = ag->inv_batch() / (float)S; o.s1 = ag->inv_batch(); o.gout = GDH; o.ldg = S + 1; o.part = part_mse_rp;
                A_.ops.push_back(o);
            }
            dxS(dh, S + 1, Wp("decoder.state_linear.weight"), Hv, wh, ACT_RELU, D1, Hv, &bC, false, GD1, Hv);
            A_.xop(RP_XCHG, bC, 4, wh, 1, 0);
            dxS(bC, Hv, Wp("decoder.l1.weight"), F, wf, ACT_NONE, nullptr, 0, &dzs, true, nullptr, 0);
            {
                RpOp o = RpAsm::blank(RP_REPARAM);
                o.src = dzs.off; o.lds = dzs.ld; o.src2 = ezs.off; o.lds2 = ezs.ld; o.dst = bA.off; o.ldd = bA.ld; o.N = wf; o.K = F; o.gout = GEH; o.ldg = 2 * F;
                o.m_dst = wf; o.m_g = wf;
                A_.ops.push_back(o);
            }
            A_.xop(RP_XCHG, bA, 5, wf, 2, F);                           // dL/d(encoder heads), both halves
            dxS(bA, 2 * F, Wp("encoder.mean_linear.weight"), Hv, wh, ACT_RELU, ge.H2, Hv, &bB, false, GH2e, Hv);
            A_.xop(RP_XCHG, bB, 6, wh, 1, 0);
            dxS(bB, Hv, Wp("encoder.l2.weight"), Hv, wh, ACT_RELU, ge.H1, Hv, nullptr, false, GH1e, Hv);
        }
        A_.end(nrb, CS, 0);
        // ---------------- program F ----------------
        A_.begin();
        {
            RpBuf bx = A_.buf(SA), bA = A_.buf(Hv), bB = A_.buf(Hv), bH = A_.buf(2 * F);
            A_.load(s0.XF, SA, SA, bx);
            fwdS(bx, SA, "f.l1", "f.l1", Hv, 0, wh, ACT_RELU, bA, gf.H1, Hv);
            A_.xop(RP_XCHG, bA, 0, wh, 1, 0);
            fwdS(bA, Hv, "f.l2", "f.l2", Hv, 0, wh, ACT_RELU, bB, gf.H2, Hv);
            A_.xop(RP_XCHG, bB, 1, wh, 1, 0);
            fwdS(bB, Hv, "f.mean_linear", "f.mean_linear", 2 * F, 0, wf, ACT_NONE, bH, gf.HH, 2 * F);
            fwdS(bB, Hv, "f.mean_linear", "f.mean_linear", 2 * F, F, wf, ACT_NONE, bH, gf.HH, 2 * F);
            A_.xop(RP_PUBLISH, bH, 2, wf, 2, F);                        // my slice of the heads, for member m of the E cluster
            A_.xop(RP_GATHER, bH, 7, wf, 2, F, 1);                      // dKL/d(f heads): every E member's slice
            dxS(bH, 2 * F, Wp("f.mean_linear.weight"), Hv, wh, ACT_RELU, gf.H2, Hv, &bA, false, GH2f, Hv);
            A_.xop(RP_XCHG, bA, 3, wh, 1, 0);
            dxS(bA, Hv, Wp("f.l2.weight"), Hv, wh, ACT_RELU, gf.H1, Hv, nullptr, false, GH1f, Hv);
        }
        A_.end(nrb, CS, 1);
    };
    bool use_rp = rl_rowprog_enabled();
    const bool use_cluster = rl_rowprog_cluster() && CS > 0 && ag->nsh[0] > 0;
    {
        RpAsm probe; if (use_cluster) rp_feature_cluster(probe); else rp_feature(probe, true);
        if (probe.lds_bytes() > RP_LDS_DYN_MAX || probe.ops.size() > 4096) use_rp = false;
        // the paired programs wait for each other inside the launch: every workgroup of it must be resident at once (256 CUs, as many
        // workgroups per CU as their LDS allows, at most 2 of these 512-thread ones) -- otherwise waiters could hold the chip while their
        // partners are never scheduled
        const int per_cu = std::max(1, std::min(2, (int)((160u * 1024u) / std::max<size_t>(probe.lds_bytes(), 1))));
        if (probe.blocks > 256 * per_cu) use_rp = false;
        for (auto& pr : probe.progs) if (pr.op_end - pr.op_begin > 40) use_rp = false;
    }
    auto with_adam = [&](GemmTask t, bool on, float* tw, float* tb) {
        if (!on || !ag->a.grad_dev || !t.C) return t;
        const int64_t ow = t.C - ag->a.grad_dev, ob = t.out2 - ag->a.grad_dev;
        t.flags |= FLAG_ADAM;
        t.ad_p = ag->a.param_dev + ow; t.ad_m = ag->a.exp_avg_dev + ow; t.ad_v = ag->a.exp_avg_sq_dev + ow; t.ad_t = tw;
        t.ad_pb = ag->a.param_dev + ob; t.ad_mb = ag->a.exp_avg_dev + ob; t.ad_vb = ag->a.exp_avg_sq_dev + ob; t.ad_tb = tb;
        t.ad_grp = ag->adam_step + 0;
        return t;
    };
    // fuse_l1: the weight-gradient tasks of encoder.l1 / f.l1 run their optimizer (and f.l1's Polyak into f_target.l1) in the epilogue
    // (FLAG_ADAM): the variant whose optimizer launch carries the next step's first layers (rlrep_feature_chain_next)
    auto feature_program = [&](Program& p, bool early, bool fuse_l1 = false) {
        GemmTask te[3], tf[3];
        gauss_tasks(ag, false, "encoder", s0.XE, KE, KE, ge, te);
        gauss_tasks(ag, false, "f", s0.XF, SA, SA, gf, tf);
        if (use_rp) {
            RpAsm A_; if (use_cluster && !early) rp_feature_cluster(A_); else rp_feature(A_, early);
            RpLaunch L; memset(&L, 0, sizeof(L));
            L.ops = b.upload(A_.ops); L.flags = rp_flags; L.nprog = (int)A_.progs.size(); L.B = B; L.low_prio = 0;
            L.lds_floats = A_.peak; L.xbuf = xbuf; L.epoch = ag->rp_epoch; L.err = ag->xc_err;
            for (size_t q = 0; q < A_.progs.size(); ++q) L.prog[q] = A_.progs[q];
            const int total = A_.blocks;
            rlrep_agent* a = ag;
            p.stages.push_back({[=](hipStream_t st) {
                RpLaunch l2 = L; l2.dyn[0] = a->cur_eps; l2.dyn[1] = a->cur_eps3; l2.dyn[2] = a->cur_eps2;
                return rl_launch_rowprog(&l2, total, st);
            }, early ? "row programs: encoder | f | policy(s') | policy(s): forward + dX" : "row programs: encoder | f: forward + dX"});
        } else
        b.chain_begin(p);              // everything up to the weight gradients is row-local: ONE persistent launch (xchain.hip)
        if (use_rp) {
        } else if (early) {
            b.fwd_stage(p, {te[0], tf[0], actor_l(ag, 0, s0.XF2, SA, ab), actor_l(ag, 0, s0.XFpi, SA, ab_pi)}, "enc.l1 f.l1 actor.l1(s') actor.l1(s)");
            b.fwd_stage(p, {te[1], tf[1], actor_l(ag, 1, nullptr, 0, ab), actor_l(ag, 1, nullptr, 0, ab_pi)}, "enc.l2 f.l2 actor.l2 x2");
        } else {
            // the first layers ride in the second layers' launch when their transposed shadows exist (one launch less per feature step)
            const bool have_t = ag->shadow_of.count("encoder.l1.weight") && ag->shadow_of.count("f.l1.weight");
            if (!have_t || !b.fwd_stage12(p, {{te[0], te[1], ag->PT("encoder.l1.weight")}, {tf[0], tf[1], ag->PT("f.l1.weight")}}, "enc.l1+l2 f.l1+l2")) {
                b.fwd_stage(p, {te[0], tf[0]}, "enc.l1 f.l1");
                b.fwd_stage(p, {te[1], tf[1]}, "enc.l2 f.l2");
            }
        }
        if (!use_rp) {
        {
            HeadsVae hv; memset(&hv, 0, sizeof(hv));
            hv.Ae = ge.H2; hv.Af = gf.H2; hv.lda = Hv; hv.We = Pw("encoder.mean_linear.weight"); hv.be = Pw("encoder.mean_linear.bias");
            hv.Wf = Pw("f.mean_linear.weight"); hv.bf = Pw("f.mean_linear.bias");
            hv.Z = Z; hv.EZ = EZ; hv.GEH = GEH; hv.GFH = GFH; hv.partial = part_kl; hv.EH = nullptr; hv.FH = nullptr;       // (nothing downstream of vae_mid reads the heads themselves)
            hv.B = B; hv.F = F; hv.K = Hv; hv.tiles_c = rl_heads_vae_tiles_c(F); hv.scale = ag->inv_batch() / (float)F; hv.step = ag->adam_step + 0;
            b.heads_vae_stage(p, hv, "enc.heads f.heads + vae_mid");
        }
        if (early)                  // the two policy heads of the early variant ride with the next forward launch instead of the heads launch
            b.fwd_stage(p, {Builder::fwd(Z, F, B, F, Pw("decoder.l1.weight"), F, Pw("decoder.l1.bias"), Hv, D1, Hv, ACT_RELU),
                            policy_head_task(ag, ab, s0.XF2 + S, SA, FLAG_DYN_EPS3), policy_head_task(ag, ab_pi, s0.XFpi + S, SA, FLAG_DYN_EPS2)},
                        "dec.l1 actor.head x2 + policy");
        else
        b.fwd_stage(p, {Builder::fwd(Z, F, B, F, Pw("decoder.l1.weight"), F, Pw("decoder.l1.bias"), Hv, D1, Hv, ACT_RELU)}, "dec.l1");
        if (!fold_mse) {
            // decoder heads with the 0.5*mse loss fused into the epilogue: the launch writes d loss / d[s_hat | r_hat]
            // (GDH) directly and per-tile partial sums of the squared errors (vlsac_agent.py:137-140)
            GemmTask t = Builder::fwd(D1, Hv, B, Hv, Pw("decoder.state_linear.weight"), Hv, Pw("decoder.state_linear.bias"), S + 1, GDH, S + 1, ACT_NONE);
            rl_task_mse(t, S, s0.XE ? s0.XE + SA : nullptr, KE, s0.R, ag->inv_batch() / (float)S, ag->inv_batch(), part_mse);
            b.fwd_stage(p, {t}, "dec.heads + mse");
        }
        {
            GemmTask t = Builder::dx(GD1, Hv, B, Hv, Pw("decoder.l1.weight"), F, GEH, 2 * F, F, ACT_NONE, nullptr, 0);
            rl_task_reparam(t, EZ, F, F);
            // the K = 18 product dL/d(dec.l1 output) = d[s_hat|r_hat] W_heads rides in the dec.l1 dX launch (one launch less per feature step)
            if (fold_mse) {
                // ... and so does the heads' forward + mse (FLAG_PRE_MSE): every tile of the launch computes d[s_hat|r_hat] of its 16 rows itself
                rl_task_pre_mse(t, GDH, S + 1, Pw("decoder.state_linear.weight"), Hv, Pw("decoder.state_linear.bias"), S, D1, Hv, GD1, Hv,
                                s0.XE ? s0.XE + SA : nullptr, KE, s0.R, ag->inv_batch() / (float)S, ag->inv_batch(), part_mse);
                b.gemm_small(p, LD_ROW, LD_COL, {t}, "dec.heads + mse | dec.heads dx | dec.l1 dx -> (dmean, dlog_std)");
            } else
            b.dx_stage12(p, Builder::dx(GDH, S + 1, B, S + 1, Pw("decoder.state_linear.weight"), Hv, GD1, Hv, Hv, ACT_RELU, D1, Hv), t,
                         "dec.heads dx", "dec.l1 dx -> (dmean, dlog_std)");
        }
        b.dx_stage(p, {Builder::dx(GEH, 2 * F, B, 2 * F, Pw("encoder.mean_linear.weight"), Hv, GH2e, Hv, Hv, ACT_RELU, ge.H2, Hv),
                       Builder::dx(GFH, 2 * F, B, 2 * F, Pw("f.mean_linear.weight"), Hv, GH2f, Hv, Hv, ACT_RELU, gf.H2, Hv)}, "heads dx");
        b.dx_stage(p, {Builder::dx(GH2e, Hv, B, Hv, Pw("encoder.l2.weight"), Hv, GH1e, Hv, Hv, ACT_RELU, ge.H1, Hv),
                       Builder::dx(GH2f, Hv, B, Hv, Pw("f.l2.weight"), Hv, GH1f, Hv, Hv, ACT_RELU, gf.H1, Hv)}, "l2 dx");
        }
        b.chain_end();
        b.dw_stage(p, {Builder::dw(GDH, S + 1, S + 1, D1, Hv, Hv, B, Gw("decoder.state_linear.weight"), Hv, Gw("decoder.state_linear.bias")),
                       Builder::dw(GD1, Hv, Hv, Z, F, F, B, Gw("decoder.l1.weight"), F, Gw("decoder.l1.bias")),
                       Builder::dw(GEH, 2 * F, 2 * F, ge.H2, Hv, Hv, B, Gw("encoder.mean_linear.weight"), Hv, Gw("encoder.mean_linear.bias")),
                       Builder::dw(GFH, 2 * F, 2 * F, gf.H2, Hv, Hv, B, Gw("f.mean_linear.weight"), Hv, Gw("f.mean_linear.bias")),
                       Builder::dw(GH2e, Hv, Hv, ge.H1, Hv, Hv, B, Gw("encoder.l2.weight"), Hv, Gw("encoder.l2.bias")),
                       Builder::dw(GH2f, Hv, Hv, gf.H1, Hv, Hv, B, Gw("f.l2.weight"), Hv, Gw("f.l2.bias")),
                       with_adam(Builder::dw(GH1e, Hv, Hv, s0.XE, KE, KE, B, Gw("encoder.l1.weight"), KE, Gw("encoder.l1.bias")), fuse_l1, nullptr, nullptr),
                       with_adam(Builder::dw(GH1f, Hv, Hv, s0.XF, SA, SA, B, Gw("f.l1.weight"), SA, Gw("f.l1.bias")), fuse_l1,
                                 nft ? nullptr : Tw("f_target.l1.weight"), nft ? nullptr : Tw("f_target.l1.bias"))}, fuse_l1 ? "feature dW (+ adam l1)" : "feature dW");
    };
    feature_program(ag->feat_bwd, false);
    const bool can_hoist = policy_fusable(ag) && !rl_off("hoist");
    if (can_hoist && !rl_off("early_policy")) feature_program(ag->feat_bwd_h, true);
    {
        // apply: Adam over (encoder, decoder, f) + Polyak f -> f_target (vlsac_agent.py:152-154, 240-242)
        const std::vector<FinTask> feat_fins = {
            Builder::fin_sum(use_rp ? part_kl_rp : part_kl, use_rp ? nblk_rp * (use_cluster ? CS : 1) : nblk_kl, 1, 1.0f / ((float)B * F), ag->metrics + M_KL),
            Builder::fin_sum((use_rp ? part_mse_rp : part_mse) + 0, use_rp ? nblk_rp : nblk_mse, 2, 0.5f / ((float)B * S), ag->metrics + M_S_LOSS),
            Builder::fin_sum((use_rp ? part_mse_rp : part_mse) + 1, use_rp ? nblk_rp : nblk_mse, 2, 0.5f / (float)B, ag->metrics + M_R_LOSS),
            Builder::fin_combine(ag->metrics + M_R_LOSS, 1.f, ag->metrics + M_S_LOSS, 1.f, ag->metrics + M_FEAT_A),
            Builder::fin_combine(ag->metrics + M_FEAT_A, 1.f, ag->metrics + M_KL, 1.f, ag->metrics + M_FEAT_TOTAL),
            // the next row-program launch gets a fresh epoch for its exchange granules (harmless when none is used)
            Builder::fin_inc(ag->rp_epoch)};
        const LT& f0 = ag->L.get("f.l1.weight");
        const LT& flast = ag->L.get("f.log_std_linear.bias");
        const int64_t fn = flast.off + flast.rows - f0.off;
        if (nft) b.adam(ag->feat_apply, 0, ag->h.lr_feature, nullptr, 0, 0, 0.f, feat_fins, "adam feature");
        else b.adam(ag->feat_apply, 0, ag->h.lr_feature, Tw("f_target.l1.weight"), f0.off, fn, ag->h.feature_tau, feat_fins, "adam feature + polyak f");
        // chained form (rlrep_feature_chain_next): first layers' optimizer in the weight-gradient epilogues, the rest + the NEXT step's first layers in one launch
        if (!use_rp && !Builder::chain_enabled() && ag->h.world_size <= 1 && ag->nsh[0] == 0 && !rl_off("chain_next")) {
            feature_program(ag->feat_bwd_m, false, true);
            GemmTask te[3], tf[3];
            gauss_tasks(ag, false, "encoder", s0.XE, KE, KE, ge, te);
            gauss_tasks(ag, false, "f", s0.XF, SA, SA, gf, tf);
            const LT& ew = ag->L.get("encoder.l1.weight"); const LT& eb = ag->L.get("encoder.l1.bias");
            const LT& fw = ag->L.get("f.l1.weight"); const LT& fb = ag->L.get("f.l1.bias");
            const int64_t g0 = ag->L.group_off[0];
            b.adam_l1(ag->feat_apply_m, 0, ag->h.lr_feature, nft ? nullptr : Tw("f_target.l1.weight"), f0.off, nft ? 0 : fn, nft ? 0.f : ag->h.feature_tau, feat_fins,
                      ew.off - g0, eb.off + eb.rows - ew.off, fw.off - g0, fb.off + fb.rows - fw.off, te[0], tf[0],
                      "adam feature (- l1) + polyak f | next enc.l1 f.l1");
        }
    }

    // ---- critic / actor shared buffers ----
    GaussBufs gt{ws.f((size_t)B * Hv), ws.f((size_t)B * Hv), ws.f((size_t)B * 2 * F)};      // f_target(s, a)
    GaussBufs gn{ws.f((size_t)B * Hv), ws.f((size_t)B * Hv), ws.f((size_t)B * 2 * F)};      // f_target(s', a')
    GaussBufs gp{ws.f((size_t)B * Hv), ws.f((size_t)B * Hv), ws.f((size_t)B * 2 * F)};      // f_target(s, a_pi)
    float* HmT = ws.f((size_t)2 * B * H); float* HmC = ws.f((size_t)2 * B * H);
    float* U = ws.f((size_t)2 * B * N * H);
    float* Et = ws.f((size_t)2 * B * H); float* Ec = ws.f((size_t)2 * B * H);
    float* GE = ws.f((size_t)2 * B * H); float* GHm = ws.f((size_t)2 * B * H);
    float* dq = ws.f((size_t)2 * B);
    float* SIG = ws.f((size_t)B * F);
    float* GTH = ws.f((size_t)B * 2 * F); float* GT2 = ws.f((size_t)B * Hv); float* GT1 = ws.f((size_t)B * Hv);
    const int nblk = qhead_blocks(B);
    float* part_q = ws.f((size_t)4 * nblk); float* part_l = ws.f(nblk);
    const size_t BH = (size_t)B * H, BNH = (size_t)B * N * H;
    const float* noise = Tw("critic.noise");

    auto nc_task = [&](const float* HH, const float* W, const float* bias, float* Hm, float* Ubuf, const unsigned char* W3 = nullptr) {
        NcFwdTask t; memset(&t, 0, sizeof(t));
        t.mean = HH; t.lstd = HH ? HH + F : nullptr; t.ld_ml = 2 * F; t.noise = noise; t.W = W; t.W3 = W3; t.bias = bias; t.Hm = Hm; t.U = Ubuf;
        t.B = B; t.F = F; t.H = H; t.N = N;
        return t;
    };
    auto nc_stage = [&](Program& p, std::vector<NcFwdTask> tasks, const char* what) {
        // batch rows per workgroup = 4*g2: the largest tile that still gives every CU a workgroup (more
        // accumulators per wave amortise the LDS-table staging and the epilogue over more MFMAs)
        // measured on MI355X (B=256, F=H=256): 4 batch rows per workgroup (4 waves per SIMD) beats 8 and 16 rows
        // (39.8 / 41.6 / 52.2 us for the 4-head launch): one wave per SIMD cannot keep the f32 MFMA pipe busy
        // behind the VALU that builds its operands.
        // (the bf16x3 engine, when the shapes allow it, takes 8 rows: rl_nc_fwd_plan)
        int g2 = 1, engine = 0, cols = 128;
        rl_nc_fwd_plan(tasks.data(), (int)tasks.size(), &engine, &g2, &cols);
        NcFwdBatch nb; memset(&nb, 0, sizeof(nb));
        nb.ntasks = (int)tasks.size(); nb.engine = engine; nb.cols = cols; nb.nt_u = rl_opt("nc_u_nt") ? 1 : 0;
        const int total = rl_nc_fwd_number_tiles(tasks.data(), (int)tasks.size(), g2, cols);
        for (size_t q = 0; q < tasks.size(); ++q) nb.t[q] = tasks[q];
        // the form of the fp32 forward is decided here, once (RLREP_ENABLE is not read on a launch path); the K-chunked one runs under a name of its own
        const int chunked = (engine == 0 && rl_nc_fwd_chunked(F, g2)) ? 1 : 0;
        if (chunked) { ag->stage_names.push_back(std::string(what) + " [K-chunked]"); what = ag->stage_names.back().c_str(); }
        p.stages.push_back({[=](hipStream_t st) { return rl_launch_nc_fwd(&nb, total, g2, chunked, st); }, what});
        {   // per head: [B*N, F] x [F, H]; reads mean / log_std / W, writes the noise-row mean (and U where the head keeps it)
            double by = 0.0;
            for (auto& t : tasks) by += 4.0 * (2.0 * (double)B * F + (double)F * H + (double)B * H + (t.U ? (double)B * N * H : 0.0));
            Builder::tag(p, RLREP_ENGINE_NOISE_CRITIC, (double)tasks.size() * 2.0 * (double)B * N * F * H, by);
        }
    };

    // ---- critic step (vlsac_agent.py:201-237) ----
    // hoist = true builds the variant that also carries the forward half of the FOLLOWING actor step (policy on s,
    // f_target on (s, a_pi)): those GEMMs read nothing the critic update writes, and as extra tasks of launches that
    // exist anyway they take six launches (~5 us each at B = 256) off the critical path of train().
    const std::vector<FinTask> cfins = {
        Builder::fin_sum(part_q + 0, nblk, 4, 1.0f / (float)B, ag->metrics + M_Q1_LOSS), Builder::fin_sum(part_q + 1, nblk, 4, 1.0f / (float)B, ag->metrics + M_Q2_LOSS),
        Builder::fin_sum(part_q + 2, nblk, 4, 1.0f / (float)B, ag->metrics + M_Q1), Builder::fin_sum(part_q + 3, nblk, 4, 1.0f / (float)B, ag->metrics + M_Q2)};
    // split-K slabs of the noise critic's weight gradient (bf16x3 form): ONE set for every variant of the critic program (no two of them are
    // ever in flight together), summed by the critic group's optimizer launch when there is no all-reduce between the two (AdamTask::Slab)
    const int ncdw_splits = rl_nc_dw_splits(B, F, H, 2);
    float* const ncdw_slab = ws.f((size_t)2 * ncdw_splits * H * F);
    float* const ncdw_bslab = ws.f((size_t)2 * ncdw_splits * H);
    const bool ncdw_in_adam = rl_nc_dw_engine() == 1 && ag->h.world_size <= 1 && ((H * F) & 3) == 0 && (H & 3) == 0 && ncdw_splits <= 16 && !rl_off("fold_ncdw");
    if (ncdw_in_adam) {
        const LT& w1 = ag->L.get("critic.l1.weight"); const LT& b1 = ag->L.get("critic.l1.bias");
        AdamTask::Slab sw; memset(&sw, 0, sizeof(sw));
        sw.off = w1.off - ag->L.group_off[1]; sw.n = 2ll * H * F; sw.per = (long long)H * F; sw.slab = ncdw_slab; sw.splits = ncdw_splits;
        AdamTask::Slab sb = sw;
        sb.off = b1.off - ag->L.group_off[1]; sb.n = 2ll * H; sb.per = H; sb.slab = ncdw_bslab;
        b.group_slabs[1] = {sw, sb};
    }
    auto critic_program = [&](Program& p, int hoist) {      // 0: plain, 1: carries the actor step's forward half, 2: both policies ran already
        GemmTask tt[3], tn[3], tp[3];
        gauss_tasks(ag, !nft, fnet, s0.XF, SA, SA, gt, tt);
        gauss_tasks(ag, !nft, fnet, s0.XF2, SA, SA, gn, tn);
        gauss_tasks(ag, !nft, fnet, s0.XFpi, SA, SA, gp, tp);
        if (hoist == 2) {
            b.fwd_stage(p, {tt[0], tn[0], tp[0]}, "ft.l1(s,a) ft.l1(s',a') ft.l1(s,a_pi)");
            b.fwd_stage(p, {tt[1], tn[1], tp[1]}, "ft.l2 x3");
            b.fwd_stage(p, {tt[2], tn[2], tp[2]}, "ft.heads x3");
        } else if (hoist == 1) {
            b.fwd_stage(p, {actor_l(ag, 0, s0.XF2, SA, ab), actor_l(ag, 0, s0.XFpi, SA, ab_pi), tt[0]}, "actor.l1(s') actor.l1(s) ft.l1(s,a)");
            b.fwd_stage(p, {actor_l(ag, 1, nullptr, 0, ab), actor_l(ag, 1, nullptr, 0, ab_pi), tt[1]}, "actor.l2 x2 ft.l2");
            b.fwd_stage(p, {policy_head_task(ag, ab, s0.XF2 + S, SA, FLAG_DYN_EPS), policy_head_task(ag, ab_pi, s0.XFpi + S, SA, FLAG_DYN_EPS2), tt[2]},
                        "actor.head x2 ft.heads + policy");
            b.fwd_stage(p, {tn[0], tp[0]}, "ft.l1(s',a') ft.l1(s,a_pi)");
            b.fwd_stage(p, {tn[1], tp[1]}, "ft.l2 x2");
            b.fwd_stage(p, {tn[2], tp[2]}, "ft.heads x2");
        } else {
            b.fwd_stage(p, {actor_l(ag, 0, s0.XF2, SA, ab), tt[0]}, "actor.l1(s') ft.l1(s,a)");
            b.fwd_stage(p, {actor_l(ag, 1, nullptr, 0, ab), tt[1]}, "actor.l2 ft.l2");
            actor_head_stage(b, p, ag, ab, s0.XF2 + S, SA, {tt[2]}, "actor.head ft.heads + policy");
            b.fwd_stage(p, {tn[0]}, "ft.l1(s',a')");
            b.fwd_stage(p, {tn[1]}, "ft.l2");
            b.fwd_stage(p, {tn[2]}, "ft.heads");
        }
        {
            NcFwdTask live1 = nc_task(gt.HH, Pw("critic.l1.weight"), Pw("critic.l1.bias"), HmC, U, ag->W3("critic.l1.weight"));
            live1.sigma_out = SIG;
            nc_stage(p, {nc_task(gn.HH, Tw("critic_target.l1.weight"), Tw("critic_target.l1.bias"), HmT, nullptr, ag->W3("critic_target.l1.weight")),
                         nc_task(gn.HH, Tw("critic_target.l4.weight"), Tw("critic_target.l4.bias"), HmT + BH, nullptr, ag->W3("critic_target.l4.weight")),
                         live1,
                         nc_task(gt.HH, Pw("critic.l4.weight"), Pw("critic.l4.bias"), HmC + BH, U + BNH, ag->W3("critic.l4.weight"))}, "noise critic l1/l4 (target+live)");
        }
        b.fwd_stage(p, {Builder::fwd(HmT, H, B, H, Tw("critic_target.l2.weight"), H, Tw("critic_target.l2.bias"), H, Et, H, ACT_ELU),
                        Builder::fwd(HmT + BH, H, B, H, Tw("critic_target.l5.weight"), H, Tw("critic_target.l5.bias"), H, Et + BH, H, ACT_ELU),
                        Builder::fwd(HmC, H, B, H, Pw("critic.l2.weight"), H, Pw("critic.l2.bias"), H, Ec, H, ACT_ELU),
                        Builder::fwd(HmC + BH, H, B, H, Pw("critic.l5.weight"), H, Pw("critic.l5.bias"), H, Ec + BH, H, ACT_ELU)}, "critic l2/l5");
        QHeadCritic q; memset(&q, 0, sizeof(q));
        q.Et[0] = Et; q.Et[1] = Et + BH; q.Ec[0] = Ec; q.Ec[1] = Ec + BH;
        // quirk Q2: BOTH heads end in l3 (l6 is dead)
        q.wt[0] = q.wt[1] = Tw("critic_target.l3.weight"); q.bt[0] = q.bt[1] = Tw("critic_target.l3.bias");
        q.wc[0] = q.wc[1] = Pw("critic.l3.weight"); q.bc[0] = q.bc[1] = Pw("critic.l3.bias");
        q.logp = ab.logp; q.R = s0.Rn; q.D = s0.D; q.alpha_state = ag->a.alpha_state_dev; q.gamma = ag->h.discount;      // (Rn: s0.R unless rlrep_set_critic_nstep)
        q.inv_batch = ag->inv_batch(); q.dq = dq; q.GE[0] = GE; q.GE[1] = GE + BH; q.partial = part_q;
        q.B = B; q.H = H; q.nblk = nblk; q.train = 1; q.step = ag->adam_step + 1;
        p.stages.push_back({[=](hipStream_t st) { return critic_head_launch(ag, q, st); }, "qhead critic"});
        b.dx_stage(p, {Builder::dx(GE, H, B, H, Pw("critic.l2.weight"), H, GHm, H, H, ACT_NONE, nullptr, 0),
                       Builder::dx(GE + BH, H, B, H, Pw("critic.l5.weight"), H, GHm + BH, H, H, ACT_NONE, nullptr, 0)}, "critic l2/l5 dx");
        b.dw_stage(p, {Builder::dw(dq, 1, 1, Ec, H, H, 2 * B, Gw("critic.l3.weight"), H, Gw("critic.l3.bias")),     // shared l3: heads stacked
                       Builder::dw(GE, H, H, HmC, H, H, B, Gw("critic.l2.weight"), H, Gw("critic.l2.bias")),
                       Builder::dw(GE + BH, H, H, HmC + BH, H, H, B, Gw("critic.l5.weight"), H, Gw("critic.l5.bias"))}, "critic dW l3 l2 l5");
        {
            NcDwBatch nb; memset(&nb, 0, sizeof(nb));
            nb.ntasks = 2;
            nb.lean = b.low_prio ? 1 : 0;     // deferred chain (fp32 kernel only): leave registers for the feature chain's launches
            auto ncdw = [&](int q, float* Ubuf, float* GH, float* gW, float* gb) {
                NcDwTask& t = nb.t[q];
                t.U = Ubuf; t.GH = GH; t.ldgh = H; t.mean = gt.HH; t.sigma = SIG; t.ld_ml = 2 * F;
                t.noise = noise; t.gW = gW; t.gb = gb; t.B = B; t.F = F; t.H = H; t.N = N;
            };
            ncdw(0, U, GHm, Gw("critic.l1.weight"), Gw("critic.l1.bias"));
            ncdw(1, U + BNH, GHm + BH, Gw("critic.l4.weight"), Gw("critic.l4.bias"));
            // bf16x3 split-K form: 64 x 64 tiles x splits, partial tiles in workspace slabs (reserved in the dry pass as well)
            nb.splits = ncdw_splits; nb.slab = ncdw_slab; nb.bslab = ncdw_bslab;
            nb.engine = rl_nc_dw_engine();
            nb.fin_in_adam = ncdw_in_adam ? 1 : 0;
            nb.rows = rl_off("nc_dw_rows") ? 0 : 1;       // (read here, where the program is built: never on a launch path)
            const int total = rl_nc_dw_number_tiles(&nb);
            p.stages.push_back({[=](hipStream_t st) { return rl_launch_nc_dw(&nb, total, st); }, "noise critic dW l1/l4"});
            Builder::tag(p, RLREP_ENGINE_NOISE_CRITIC, 2.0 * 2.0 * (double)B * N * F * H, 2.0 * 4.0 * ((double)B * N * H + (double)B * H + 2.0 * (double)B * F + (double)F * H));
        }
    };
    critic_program(ag->critic_bwd, 0);
    if (can_hoist) critic_program(ag->critic_bwd_h, 1);
    if (!ag->feat_bwd_h.stages.empty()) critic_program(ag->critic_bwd_h2, 2);
    b.adam(ag->critic_apply, 1, ag->h.lr_critic, nullptr, 0, 0, 0.f, cfins, "adam critic");
    critic_apply_folded(b, ag, "critic_target.l1.weight", cfins);

    // ---- actor + temperature step (vlsac_agent.py:165-198) ----
    auto actor_program = [&](Program& p, int& resume) {
        GemmTask tt[3];
        gauss_tasks(ag, !nft, fnet, s0.XFpi, SA, SA, gp, tt);
        b.fwd_stage(p, {actor_l(ag, 0, s0.XFpi, SA, ab_pi)}, "actor.l1(s)");
        b.fwd_stage(p, {actor_l(ag, 1, nullptr, 0, ab_pi)}, "actor.l2");
        actor_head_stage(b, p, ag, ab_pi, s0.XFpi + S, SA, {}, "actor.head + policy");
        b.fwd_stage(p, {tt[0]}, "ft.l1(s,a_pi)");
        b.fwd_stage(p, {tt[1]}, "ft.l2");
        b.fwd_stage(p, {tt[2]}, "ft.heads");
        resume = (int)p.stages.size();                // everything above is what critic_bwd_h already did
        nc_stage(p, {nc_task(gp.HH, Pw("critic.l1.weight"), Pw("critic.l1.bias"), HmC, U, ag->W3("critic.l1.weight")),
                     nc_task(gp.HH, Pw("critic.l4.weight"), Pw("critic.l4.bias"), HmC + BH, U + BNH, ag->W3("critic.l4.weight"))}, "noise critic l1/l4");
        b.fwd_stage(p, {Builder::fwd(HmC, H, B, H, Pw("critic.l2.weight"), H, Pw("critic.l2.bias"), H, Ec, H, ACT_ELU),
                        Builder::fwd(HmC + BH, H, B, H, Pw("critic.l5.weight"), H, Pw("critic.l5.bias"), H, Ec + BH, H, ACT_ELU)}, "critic l2/l5");
        QHeadActor q; memset(&q, 0, sizeof(q));
        q.Ec[0] = Ec; q.Ec[1] = Ec + BH; q.wc[0] = q.wc[1] = Pw("critic.l3.weight"); q.bc[0] = q.bc[1] = Pw("critic.l3.bias");
        q.logp = ab_pi.logp; q.alpha_state = ag->a.alpha_state_dev; q.inv_batch = ag->inv_batch(); q.target_entropy = ag->h.target_entropy;
        q.GE[0] = GE; q.GE[1] = GE + BH; q.partial_loss = part_l; q.partial_c = ag->Gtail();
        q.B = B; q.H = H; q.nblk = nblk; q.step = ag->adam_step + 2;
        p.stages.push_back({[=](hipStream_t st) { return rl_launch_qhead_actor(&q, st); }, "qhead actor"});
        b.dx_stage(p, {Builder::dx(GE, H, B, H, Pw("critic.l2.weight"), H, GHm, H, H, ACT_NONE, nullptr, 0),
                       Builder::dx(GE + BH, H, B, H, Pw("critic.l5.weight"), H, GHm + BH, H, H, ACT_NONE, nullptr, 0)}, "critic l2/l5 dx");
        {
            NcDxTask t; memset(&t, 0, sizeof(t));
            t.GH[0] = GHm; t.GH[1] = GHm + BH; t.ldgh = H; t.U[0] = U; t.U[1] = U + BNH;
            t.W[0] = Pw("critic.l1.weight"); t.W[1] = Pw("critic.l4.weight"); t.noise = noise;
            t.lstd = gp.HH ? gp.HH + F : nullptr; t.ld_l = 2 * F; t.G = GTH; t.ldg = 2 * F;
            t.B = B; t.F = F; t.H = H; t.N = N; t.nheads = 2;
            rl_nc_dx_number_tiles(&t);
            p.stages.push_back({[=](hipStream_t st) { return rl_launch_nc_dx(&t, st); }, "noise critic dX -> (dmean, dlog_std)"});
            Builder::tag(p, RLREP_ENGINE_NOISE_CRITIC, 2.0 * 2.0 * (double)B * N * F * H, 4.0 * (2.0 * ((double)B * N * H + (double)B * H + (double)F * H) + 3.0 * (double)B * F));
        }
        b.dx_stage(p, {Builder::dx(GTH, 2 * F, B, 2 * F, FT("mean_linear.weight"), Hv, GT2, Hv, Hv, ACT_RELU, gp.H2, Hv)}, "ft.heads dx");
        b.dx_stage(p, {Builder::dx(GT2, Hv, B, Hv, FT("l2.weight"), Hv, GT1, Hv, Hv, ACT_RELU, gp.H1, Hv)}, "ft.l2 dx");
        actor_backward(b, p, ag, ab_pi, s0.XFpi, SA, s0.XFpi + S, SA, Builder::dx(GT1, Hv, B, Hv, FT("l1.weight") ? FT("l1.weight") + S : nullptr, SA, ab_pi.dA, A, A, ACT_NONE, nullptr, 0));
    };
    actor_program(ag->actor_bwd, ag->actor_resume);
    actor_apply_program(b, ag, part_l, nblk);
    update_target_program(ag, "critic.l1.weight", "critic_target.l1.weight");

    // ---- deferred variants: the same critic / actor programs against a snapshot set (see rlrep_agent::dset) ----
    for (int set = 0; set < rlrep_agent::NSETS; ++set) {
        const LT& f0 = ag->L.get(fnet + ".l1.weight");
        const LT& fl = ag->L.get(fnet + ".log_std_linear.bias");
        float* fbase = nft ? ag->a.param_dev : ag->a.target_dev;          // the snapshot is of whichever copy the two steps read
        const Slot keep = defer_begin(b, ag, set, nft ? "f." : "f_target.", nft ? "f.l1.weight" : "f_target.l1.weight", fbase ? fbase + f0.off : nullptr,
                                      fl.off + fl.rows - f0.off);
        {
            // the same block as the feature group's optimizer launch produces it (rlrep_defer_arm): the live f's range of the group, or the
            // range its Polyak writes into f_target (both start at f.l1.weight's offset in the group)
            rlrep_agent::DeferSet& D = ag->dset[set];
            const LT& p0 = ag->L.get("f.l1.weight");
            D.block_off = p0.off - ag->L.group_off[0]; D.block_n = fl.off + fl.rows - f0.off; D.block_which = nft ? 0 : 1;
            // (with N > 1 ranks too: the optimizer launch that writes the snapshot is the one that has summed the ranks' gradients)
            if (rl_off("fold_snapshot")) D.block_which = -1;
        }
        critic_program(ag->dset[set].critic_bwd, can_hoist ? 1 : 0);
        actor_program(ag->dset[set].actor_bwd, ag->dset[set].actor_resume);
        if (!can_hoist) ag->dset[set].actor_resume = 0;
        defer_end(b, ag, set, keep, "critic_target.l1.weight", cfins);
    }
}

Slot defer_begin(Builder& b, rlrep_agent* ag, int set, const char* prefix, const char* first, const float* block_src, int64_t block_n) {
    Workspace& ws = b.ws;
    const int B = ag->B, S = ag->d.state_dim, A = ag->d.action_dim, SA = S + A;
    Slot& s0 = ag->slot[0];
    rlrep_agent::DeferSet& D = ag->dset[set];
    Slot d; d.XE = nullptr; d.XF = ws.f((size_t)B * SA); d.XF2 = ws.f((size_t)B * SA); d.XFpi = ws.f((size_t)B * SA); d.R = ws.f(B); d.D = ws.f(B);
    const bool own_rn = s0.Rn != s0.R && ag->cn_block;                  // n-step critic targets: the heads' reward array is snapshotted too
    d.Rn = own_rn ? ag->cn_block + (1 + set) * ag->cn_stride : d.R;
    D.slot = d;
    D.block = block_n > 0 ? ws.f((size_t)block_n) : nullptr;
    D.eps = ws.f((size_t)2 * B * A); D.steps = (int*)ws.alloc(sizeof(int) * 4);
    CopySegs& cs = D.segs; memset(&cs, 0, sizeof(cs));
    long long end = 0; int n = 0;
    auto seg = [&](const float* src, float* dst, long long cnt) { cs.src[n] = src; cs.dst[n] = dst; end += cnt; cs.end[n] = end; ++n; };
    seg(s0.XF, d.XF, (long long)B * SA); seg(s0.XF2, d.XF2, (long long)B * SA); seg(s0.XFpi, d.XFpi, (long long)B * SA);
    seg(s0.R, d.R, B); seg(s0.D, d.D, B);
    if (own_rn) seg(s0.Rn, d.Rn, B);                                    // (9 of COPY_MAX_SEGS = 10 segments at the most)
    if (block_n > 0) seg(block_src, D.block, block_n);
    seg(nullptr, D.eps, (long long)B * A);                             // critic-step policy noise (patched per call)
    seg(nullptr, D.eps ? D.eps + (size_t)B * A : nullptr, (long long)B * A);   // actor-step policy noise
    cs.n = n; cs.isrc = ag->steps; cs.idst = D.steps;
    const Slot keep = s0;
    s0.XF = d.XF; s0.XF2 = d.XF2; s0.XFpi = d.XFpi; s0.R = d.R; s0.D = d.D; s0.Rn = d.Rn;
    ag->ov_base = b.dry ? nullptr : D.block; ag->ov_prefix = prefix; ag->ov_first = first;      // the dry pass only sizes the workspace
    ag->dcur = set;
    b.low_prio = true;
    return keep;
}
void defer_end(Builder& b, rlrep_agent* ag, int set, const Slot& keep, const std::string& critic_target_first, std::vector<FinTask> cfins) {
    ag->ov_base = nullptr;
    ag->slot[0] = keep;
    b.low_prio = false;
    critic_apply_folded(b, ag, critic_target_first, cfins, &ag->dset[set].critic_apply, ag->dset[set].steps);
    ag->dset[set].valid = false;
}
