// Seed groups (rlrep_group_create): R agents of identical shape whose blocks lie at a constant byte stride in ONE allocation.  The step
// programs are built once, against member 0; a launch issued while a group is active runs every live member at once -- grid y is a slot of
// the live table (RL_GRP_MEMBER below; slot r is member r while nobody is retired) -- and rebases EVERY pointer it dereferences by r * stride (the replay ring by r * ring_stride, the ring's size word by r).
// The grid's x dimension, the tile decomposition and every summation order are a standalone agent's: member r computes bit for bit
// what SACAgent(seed = s_r) computes.  No member reads another member's words.
//
// The group forms are SEPARATE kernels (`*_grp_kernel`) around the same device bodies: the kernels the single agents launch are untouched.
// The large bodies (`*_body.h`) are #included into both kernels rather than called: moved into a forceinline function, the gemm_lds
// kernels' instruction schedules changed.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "kparams.h"

#define RLREP_GROUP_MAX_MEMBERS 64

// host: the group of the library call in progress (null outside one); set by the group entry points for the duration of the call
struct RlGrp {
    int members;
    long long stride;                   // bytes between two members' blocks (multiple of 256)
    long long ring_stride;              // bytes between two members' replay rings (train prologue only)
    const unsigned long long* seeds;    // [members] Philox seeds (device), train prologue only
    const MemberHyper* hyp;             // member 0's by-value hyper-parameters (kparams.h); member r's lie r * stride further
    const int* live;                    // the live table (device): n_live, then slot_member[members] -- see RL_GRP_MEMBER
    int grid_y;                         // grid y of the group launches: members (RLREP_ENABLE=grp_compact: the live members at the last rlrep_group_set_live)
};
// what a launcher without a group form returns while a group is active (the stage fails with this code: no member is left behind silently)
#define RL_GRP_UNSUPPORTED 77

#define RL_UNPAREN(...) __VA_ARGS__

// Retired members (rlrep_group_set_live).  One device table per group, an allocation of its own: int n_live, then int slot_member[members], the
// live members in ascending order.  Grid y stays `members` (captured graphs are kept); every group kernel form begins with RL_GRP_MEMBER(m, live):
// slot = blockIdx.y, a slot at or behind n_live returns, otherwise m = slot_member[slot].  Both reads are wave-uniform (scalar loads) and the
// return comes before any LDS use, barrier, ticket or counter access.  A member's blocks all leave or all stay, so the per-member protocols
// (split-K tickets, "last block finalises", the prologue's ticket) stay sound, and a retired member's block is neither read nor written.
struct LiveTab { int n_live; int slot_member[RLREP_GROUP_MAX_MEMBERS]; };
#define RL_GRP_MEMBER(m, live) \
    if ((int)blockIdx.y >= (live)[0]) return; \
    const int m = (live)[1 + blockIdx.y]

// rlrep_group_clone_members (group_clone.hip): what one clone launch copies from member src's block to member dst's, both by value in the
// kernel arguments.  A segment is [off, off + bytes) from the member block's base, both multiples of 4.  Segment rec_seg holds the device
// records and moves word by word: of its words [rec_w0, rec_w0 + rec_nw) -- the optimizer records, rec_words words each -- words 1..5 of every
// record (lr, beta1, beta2, eps, tau) stay the destination's.
#define RL_CLONE_MAX_SEGS 8
struct CloneSeg { long long off, bytes; };
struct CloneTab {
    char* base;                         // member 0's block (rlrep_agent::grp_lo)
    long long stride;                   // bytes between two members' blocks
    int nseg, rec_seg, rec_w0, rec_nw, rec_words, pad_;
    CloneSeg seg[RL_CLONE_MAX_SEGS];
};
struct ClonePairs { int src[RLREP_GROUP_MAX_MEMBERS], dst[RLREP_GROUP_MAX_MEMBERS]; };

#ifdef __HIPCC__
template <class T> __device__ __forceinline__ void rl_rb(T*& p, long long d) { if (p) p = (T*)((uintptr_t)p + (uintptr_t)d); }
// p moved by d bytes in a group form (GRP), p itself in the single-agent kernel: for bodies that read a pointer from a record left in the
// kernel-argument segment, at the place they load it (no local copy of the record: no scratch)
template <bool GRP, class T> __device__ __forceinline__ T* rl_mv(T* p, long long d) {
    if constexpr (GRP) return (T*)((uintptr_t)p + (uintptr_t)d);
    else { (void)d; return p; }
}
__device__ __forceinline__ void rl_rebase(GemmTask& t, long long d) {
    rl_rb(t.A, d); rl_rb(t.B, d); rl_rb(t.C, d); rl_rb(t.bias, d); rl_rb(t.aux, d); rl_rb(t.r1u, d); rl_rb(t.r1v, d);
    rl_rb(t.gidx, d); rl_rb(t.out2, d);
#pragma unroll
    for (int q = 0; q < 5; ++q) rl_rb(t.sp[q], d);
    rl_rb(t.aux2, d); rl_rb(t.aux3, d);
    rl_rb(t.ad_p, d); rl_rb(t.ad_m, d); rl_rb(t.ad_v, d); rl_rb(t.ad_t, d);
    rl_rb(t.ad_pb, d); rl_rb(t.ad_mb, d); rl_rb(t.ad_vb, d); rl_rb(t.ad_tb, d); rl_rb(t.ad_grp, d);
    rl_rb(t.x0, d); rl_rb(t.x1, d); rl_rb(t.x2, d); rl_rb(t.y0, d); rl_rb(t.y1, d); rl_rb(t.dptr, d);
    rl_rb(t.tgs, d); rl_rb(t.tgr, d); rl_rb(t.mse_part, d); rl_rb(t.slab, d); rl_rb(t.bslab, d);
}
__device__ __forceinline__ void rl_rebase(FinTask& f, long long d) {
    rl_rb(f.partials, d); rl_rb(f.out, d); rl_rb(f.out2, d); rl_rb(f.in_a, d); rl_rb(f.in_b, d); rl_rb(f.alpha_state, d);
}
// ring_d: the replay ring's own stride (a gather from the ring); the slot buffers and the index stream live in the member's block
__device__ __forceinline__ void rl_rebase(SlotFill& s, long long d, long long ring_d) {
    rl_rb(s.ring, ring_d); rl_rb(s.idx, d);
    rl_rb(s.s, d); rl_rb(s.a, d); rl_rb(s.r, d); rl_rb(s.s2, d); rl_rb(s.d, d);
    rl_rb(s.XE, d); rl_rb(s.XF, d); rl_rb(s.XF2, d); rl_rb(s.XFpi, d); rl_rb(s.R, d); rl_rb(s.D, d);
}
__device__ __forceinline__ void rl_rebase(AdamTask& t, long long d) {
    rl_rb(t.p, d); rl_rb(t.g, d); rl_rb(t.m, d); rl_rb(t.v, d); rl_rb(t.grp, d); rl_rb(t.target, d); rl_rb(t.pol_steps, d);
#pragma unroll
    for (int q = 0; q < 8; ++q) rl_rb(t.slabs[q].slab, d);
    rl_rb(t.sync_steps, d);
}
__device__ __forceinline__ void rl_rebase(QHeadCritic& p, long long d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        rl_rb(p.Et[h], d); rl_rb(p.Ec[h], d); rl_rb(p.wt[h], d); rl_rb(p.bt[h], d); rl_rb(p.wc[h], d); rl_rb(p.bc[h], d); rl_rb(p.GE[h], d);
    }
    rl_rb(p.logp, d); rl_rb(p.R, d); rl_rb(p.D, d); rl_rb(p.alpha_state, d); rl_rb(p.dq, d); rl_rb(p.partial, d); rl_rb(p.step, d);
}
__device__ __forceinline__ void rl_rebase(InfoNce& p, long long d) {
    rl_rb(p.S, d); rl_rb(p.rhat, d); rl_rb(p.r, d); rl_rb(p.drhat, d); rl_rb(p.partial, d); rl_rb(p.step, d);
    rl_rb(p.Z, d); rl_rb(p.theta_w, d); rl_rb(p.theta_b, d); rl_rb(p.ZM, d);
}
__device__ __forceinline__ void rl_rebase(QHeadActor& p, long long d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) { rl_rb(p.Ec[h], d); rl_rb(p.wc[h], d); rl_rb(p.bc[h], d); rl_rb(p.GE[h], d); }
    rl_rb(p.logp, d); rl_rb(p.alpha_state, d); rl_rb(p.partial_loss, d); rl_rb(p.partial_c, d); rl_rb(p.step, d);
}
#endif
