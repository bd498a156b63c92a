// Shared device/host definitions for librlrep_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// diagnostic switches (engine.hip): a token listed in RLREP_DISABLE / the value of a token of RLREP_ENABLE ("1" when listed bare; nullptr: not
// listed), as parsed at the last library entry (rlrep_layout / rlrep_agent_create / rlrep_gemm*: rl_switches_read) -- never read on a launch path
bool rl_off(const char* token);
const char* rl_opt(const char* token);

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define RL_WAVE 64

// ------------------------------------------------------------------------------------------------
// activation / epilogue codes
// ------------------------------------------------------------------------------------------------
enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_ELU = 2, ACT_SIN = 3, ACT_TANH = 4 };

// operand loaders of the tile GEMM (see gemm16.hip)
enum Load : int {
    LD_ROW = 0,     // element(i, kk) = P[(base+i)*ld + kk]           (inner index contiguous)
    LD_COL = 1      // element(i, kk) = P[kk*ld + base+i]              (inner index is the row)
};

// epilogues
enum Epi : int {
    EPI_FWD = 0,        // C = act(acc + bias[c]); ACT_SIN also stores the pre-activation to out2
    EPI_DX = 1,         // C (=|+=) acc * act'(aux[r,c])
    EPI_DX_REPARAM = 2, // vlsac: C[r,c] += acc ; C[r,c+F] += acc * aux3[r,c]  (aux3 = eps*exp(l)*clamp-mask)
    EPI_DW = 3,         // C = acc (weight gradient), bias gradient = column sums of operand A
    EPI_FWD_MSE = 4,    // vlsac decoder heads: C <- d(0.5 mse)/d(pred) vs targets x0 (cols < n0) / x1 (col n0); partial sums -> y0
    EPI_FWD_POLICY = 5, // actor head (2A <= 16): C <- raw [mu|rho]; y0 <- tanh(mu + eps*sigma); y1 <- log pi   (agent/sac/actor.py:76-91)
    EPI_DX_POLICYBWD = 6, // acc = dL/da: y0 <- dL/d[mu|rho]; no C store
    EPI_DWA = 7          // COMPILE-TIME kind only (tasks carry EPI_DW): weight-gradient launch some of whose tasks run the optimizer (FLAG_ADAM)
};

#define FLAG_ACCUM 1       // C += value instead of C = value
#define FLAG_BIASGRAD 2    // EPI_DW: also emit the bias gradient (only by column-tile 0)
#define FLAG_DYN_EPS 4     // x2 is the per-call noise pointer (patched into the kernel arguments at launch)
#define FLAG_DYN_EPS2 8    // x2 is the noise pointer of the policy forward that rides along (rlrep_prefetch_policy)
#define FLAG_DYN_EPS3 16   // x2 is the critic step's policy noise while that policy rides in the last feature step
// gemm_lds.hip: operand / output not eligible for 16-byte accesses (row stride, inner length or pointer not a multiple of 4
// floats, e.g. the K = 119 first layers of spedersac): that side falls back to clamped 4-byte accesses
#define FLAG_SCALAR_A 32
#define FLAG_SCALAR_B 64
#define FLAG_SCALAR_C 128
// gemm16.hip: the A operand is not read from memory but is the output of a fused SHORT product that precedes this one in the chain,
//   A[i][k] = ( sum_{j < K1} X[i][j] * Wt[j][k] ) * relu'(M[i][k]),   K1 <= 32,  Wt k-major ([K1][K]: lanes read consecutive k),
// recomputed by every tile for its 16 rows (x0 = X, ldx0; x1 = Wt, ldx1; n0 = K1; x2 = M, ldaux2 its row stride; y0 = where column
// tile 0 stores A for the weight-gradient pass, ldout2 its row stride).  vlsac: dL/d(dec.l1 output) = (dL/d[s_hat|r_hat] [B,18]) W_heads
// rides in the dec.l1 dX launch instead of being a launch of its own.
#define FLAG_PRE 256
// ... or, FORWARD form (FLAG_PRE | FLAG_PRE_FWD): the A operand is the previous layer's activation itself,
//   A[i][k] = relu( sum_{j < K1} X[i][j] * Wt[j][k] + b1[k] ),   K1 <= 48,  Wt = the TRANSPOSED first-layer weight [K1][K] (a shadow kept by the
// optimizer launch: rows of W1 itself would be 92-/160-byte-strided 4-byte reads), x2 = b1 (ldaux2 = 0).  vlsac: encoder.l1 / f.l1 ride in
// the encoder.l2 / f.l2 launch.
#define FLAG_PRE_FWD 512
// dX form only: the fused short product's mask is ELU'(M) = (M > 0 ? 1 : M + 1) instead of ReLU'(M) -- the actor head's dX (K1 = 2A) riding in
// the dX launch of the actor's second layer (agent/sac/actor.py:31-45 backward)
#define FLAG_PRE_ELU 1024
// dX form of the fused short product (FLAG_PRE), vlsac decoder only: the short product's ROW operand X [R, K1] is not read from memory either -- it is
// the gradient of the decoder's 0.5*mse losses, computed here from the layer's own saved activation M:
//   X = dmse( M Wt^T + bias ; targets ),   Wt = the heads' weight [K1, K] (the short product's own matrix), M [R, K] (= x2),
// i.e. the `dec.heads + mse` launch (EPI_FWD_MSE) rides in the launch that consumes it: every tile recomputes the K1 <= 32 head outputs of its 16 rows
// (MFMA, inner dimension split over the waves, fixed-order LDS reduction), column tile 0 files X (x0 / ldx0: the weight-gradient pass reads it) and the
// per-row-tile squared-error partials (mse_part: [2 * row tile], [.. + 1]).  Targets: tgs [R, n0] (row stride ldtgs) for columns < n0, tgr [R] for column n0;
// gradient scales s0 / s1.  One dependent launch less per feature step (vlsac_agent.py:137-145).
#define FLAG_PRE_MSE 4096
// EPI_DW only: the optimizer runs in this task's epilogue (Adam on the tile's own weights and, column tile 0, bias; Polyak into the target
// copy where ad_t / ad_tb are set) -- the FIRST layers of the vlsac feature nets, whose updated weights the next feature step's first launch
// needs, so that the rest of the group's optimizer work can share a launch with that first layer.  GemmTask::ad_*.
#define FLAG_FIN_IN_ADAM 8192  // split-K task of the LDS-tiled engine whose partial slabs are summed by its group's optimizer launch (AdamTask::Slab): no finishing blocks
#define FLAG_FIN_INLINE 16384  // split-K task of the 64-wide bf16x3 tile whose LAST split workgroup of every tile sums the slabs and runs the epilogue itself (gemm_x3s_kernel): no finishing launch
#define FLAG_ADAM 2048

struct GroupCfg;
struct GemmTask {
    // ---- hot block: read by every tile in ONE scalar-load burst (first 112 bytes) -------------------
    const float* A;      // operand A (output rows)
    const float* B;      // operand B (output cols)
    float* C;
    const float* bias;   // EPI_FWD: bias[Cn];  EPI_DW: unused
    const float* aux;    // EPI_DX: saved activation (or pre-activation for sin);  LD_NCG: GH
    const float* r1u;    // EPI_DX: optional rank-1 term added to acc: r1u[r] * r1v[c]
    const float* r1v;
    int lda, ldb, ldc, ldaux;
    int R, Cn, K;        // output R x Cn, inner length K
    int tiles_c, tile_base;
    int epi, act, flags;
    const int* gidx;     // row gather (gemm16 forward launches riding in an optimizer launch): operand-A row i is A[gidx[i] * lda + k] (null: row i)
    float scale;         // multiplies acc before the epilogue (1.0 default)
    int n0;              // fused loss / policy epilogues: column split (S or A)
    float* out2;         // EPI_FWD+ACT_SIN: pre-activation; EPI_DW: bias gradient
    int ldout2;
    int ntiles;
    // ---- the epilogue's operand SLOTS, precomputed on the host (rl_gemm16_plan) ---------------------------
    // The epilogue kind only selects up to five slot descriptors -- base, row stride, column stride (1, or 0 if bit q of scs0 is set),
    // offset, column window [slo, shi) -- and the kernel's operand loads are generic.  Deriving them in the kernel cost every tile a
    // ladder of scalar branches with a dependent scalar-load round trip per case (x0, ldx0, aux3, F ...: ~1 800 cycles between
    // "workgroup starts" and "first operand load issued"); as part of the record they arrive with the hot block in one burst.
    // spx2: bit q set = slot q's base is x2, which a launch whose table lives in device memory patches per call (FLAG_DYN_EPS*).
    const float* sp[5]; int srs[5], sof[5], slo[5], shi[5]; int scs0, spx2;
    // ---- cold block: only the epilogue that needs a field reads it ---------------------------------
    const float* aux2;   // LD_NCX: log-std
    const float* aux3;   // EPI_DX_REPARAM: eps*exp(l)*mask;  LD_NCX: mean
    int ldaux2, ldaux3;
    int ncN;             // noise rows (20) for LD_NCG/LD_NCX
    int F;               // EPI_DX_REPARAM: column offset of the log-std half
    // EPI_DW + FLAG_ADAM: Adam on the tile's own weights (and bias), plus Polyak into the target copy.  Bases of tensors laid out like C / out2.
    float* ad_p; float* ad_m; float* ad_v; float* ad_t;          // weight: param, exp_avg, exp_avg_sq, target (or null)
    float* ad_pb; float* ad_mb; float* ad_vb; float* ad_tb;      // bias
    const GroupCfg* ad_grp;
    // generic operands of the fused loss / policy epilogues
    const float* x0; const float* x1; const float* x2; float* y0; float* y1; const double* dptr;
    int ldx0, ldx1; float s0, s1;
    const float* tgs; const float* tgr; float* mse_part; int ldtgs, pad_mse;      // FLAG_PRE_MSE
    // gemm_lds.hip only: split-K plan (splits > 1: partial tiles go to slab [splits][R][Cn], bias partials to
    // bslab [splits][R]; the finishing launch adds them in split order) -- zero for gemm16 launches
    int splits, kchunk, fin_base;
    float* slab; float* bslab;
};

// host side: fill the slots of a finished task record (every launcher of the 16-row tile engine calls it on its copy of the record)
static inline void rl_gemm16_plan(GemmTask& t) {
    for (int q = 0; q < 5; ++q) { t.sp[q] = nullptr; t.srs[q] = 0; t.sof[q] = 0; t.slo[q] = 0; t.shi[q] = t.Cn; }
    t.scs0 = 0; t.spx2 = 0;
    switch (t.epi) {
    case EPI_FWD: t.sp[0] = t.bias; break;
    case EPI_DX:
        if (t.act != ACT_NONE) { t.sp[0] = t.aux; t.srs[0] = t.ldaux; }
        if (t.flags & FLAG_ACCUM) { t.sp[1] = t.C; t.srs[1] = t.ldc; }
        if (t.r1u) { t.sp[2] = t.r1u; t.srs[2] = 1; t.scs0 |= 4; t.sp[3] = t.r1v; }
        break;
    case EPI_FWD_MSE:
        t.sp[0] = t.bias;
        t.sp[1] = t.x0; t.srs[1] = t.ldx0; t.shi[1] = t.n0;
        t.sp[2] = t.x1; t.srs[2] = 1; t.scs0 |= 4; t.slo[2] = t.n0;
        break;
    case EPI_FWD_POLICY:
        t.sp[0] = t.bias;
        t.sp[1] = t.x2; t.srs[1] = t.n0; t.shi[1] = t.n0; t.spx2 = 2;
        break;
    case EPI_DX_POLICYBWD:
        t.sp[0] = t.x0; t.srs[0] = 2 * t.n0; t.sof[0] = t.n0;
        t.sp[1] = t.x2; t.srs[1] = t.n0; t.spx2 = 2;
        t.sp[2] = t.x1; t.srs[2] = t.ldx1;
        break;
    case EPI_DX_REPARAM:
        t.sp[0] = t.aux3; t.srs[0] = t.ldaux3;
        t.sp[1] = t.C; t.srs[1] = t.ldc;
        t.sp[2] = t.C; t.srs[2] = t.ldc; t.sof[2] = t.F;
        break;
    default:   // EPI_DW
        if (t.flags & FLAG_ACCUM) { t.sp[1] = t.C; t.srs[1] = t.ldc; }
        if ((t.flags & FLAG_ADAM) && t.ad_p) {      // optimizer in the epilogue: the tile of the parameter, its Adam moments (and its Polyak target)
            t.sp[0] = t.ad_p; t.sp[2] = t.ad_m; t.sp[3] = t.ad_v; t.sp[4] = t.ad_t;
            t.srs[0] = t.srs[2] = t.srs[3] = t.srs[4] = t.ldc;
        }
    }
}

#define GEMM_MAX_TASKS 8
// passed by value (kernarg segment).
// tb / tcs: first tile and column tiles of each task, copied next to the header by the launcher so that a workgroup finds its task and its
// tile coordinates from ONE burst of scalar loads (then the task record with a second one), instead of a round trip per dependent field
// total: tiles of the launch
struct GemmBatch { int ntasks; int low_prio; int total; int tb[GEMM_MAX_TASKS], tcs[GEMM_MAX_TASKS]; int xcd_runs; GemmTask t[GEMM_MAX_TASKS]; };    // low_prio: launch of a chain with slack (deferred critic / actor)

// ------------------------------------------------------------------------------------------------
// elementwise task (Adam / Polyak)
// ------------------------------------------------------------------------------------------------
// Transposed shadow copy of a weight matrix (rowprog.hip reads W^T so that a lane's 16-byte B fragment and its neighbours' are
// contiguous): tensor at float offset `off` (n = rows * cols) of an arena, shadow [cols][rows] at sp; st = shadow of its Polyak target.
//
// kind 1 (noisecritic.hip): the bf16x3 images of a weight matrix [rows = H][cols = F], F % 32 == 0, in the order the noise critic's B
// fragments are read: [F / 32 steps][3 images hi, mid, lo][H rows][4 groups of 8 consecutive k][8 bf16] -- 64 bytes per (step, image, row).
// sp / st then point at those byte images (3 * rows * cols * 2 bytes each).  `src`, when set, is the tensor itself (the refresh launch of a
// table whose entries live in different arenas: live and target critic); otherwise base + off as for kind 0.
struct ShadowEnt { long long off, n; int rows, cols; float* sp; float* st; const float* src; int kind, pad; };

struct AdamTask {
    float* p; const float* g; float* m; float* v;
    long long n;
    float lr, beta1, beta2, eps;
    const GroupCfg* grp;        // group state (step already bumped for this step)
    // optional Polyak of a sub-range [pol_off, pol_off+pol_n) of p into target
    float* target; long long pol_off, pol_n; float tau;
    const int* pol_steps; int pol_period;     // if pol_steps != nullptr: Polyak only when *pol_steps % pol_period == 0
    const ShadowEnt* sh; int nsh;             // transposed shadows of this group's weight matrices, kept current by this launch (or null)
    // Gradients that arrive as split-K PARTIALS (the vlsac noise critic's dW on bf16x3: noisecritic.hip nc_dw_x3_kernel): for elements
    // [off, off + n) of the group the gradient is the sum, in split order, of slab[(q * splits + sp) * per + r] (q = l / per, r = l % per,
    // l = element - off) -- the finishing launch those partials used to need rides here, and the sum is filed in the gradient arena too.
    // per % 4 == 0, off % 4 == 0, 16-byte aligned slabs (the builder only folds then).  nslab = 0: plain gradients.
    // cols > 0: ONE matrix of rows of `cols` elements whose slab rows are padded to `ldpad` floats (the LDS-tiled engine's split-K slabs of a
    // [512, 119] gradient: ldpad = 120), consecutive splits `sstride` floats apart: element l sits at slab[sp * sstride + (l / cols) * ldpad + l % cols].
    struct Slab { long long off, n, per, sstride; const float* slab; int splits, cols, ldpad, pad; } slabs[8];
    int nslab;
    // ranges of the group that this launch leaves alone (their optimizer ran in the weight-gradient epilogues: FLAG_ADAM); multiples of 4 floats
    int nskip; long long skip_off[2], skip_n[2];
    // train() counter block {counter, -, counter as the NEXT train prologue will read it}: the optimizer launches that follow a prologue in ITS launch
    // chain (the feature group's; every group's for an agent without one) bring word 2 up to word 0 (elementwise.hip train_prologue_kernel)
    int* sync_steps;
};

struct PolyakTask {
    const float* src; float* dst; long long n; float tau;
    const int* steps; int period;     // if steps != nullptr: only when *steps % period == 0
};

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float clamp_lstd(float x) { return fminf(fmaxf(x, -20.f), 2.f); }
__device__ __forceinline__ float lstd_mask(float x) { return (x >= -20.f && x <= 2.f) ? 1.f : 0.f; }

__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : expm1f(x); }
// ELU through the hardware exp2 (v_exp_f32): |error| <= ~1.5e-7 absolute on (-inf, 0] against expm1f's 1 ulp relative -- the
// difference only exists where elu(x) ~ x and is far below the 1e-4 parity bar.  For the noise critic's 5120 x 256 ELUs per
// head (expm1f is ~35 VALU instructions and every wave of the launch runs them at the same time, after its MFMAs).
__device__ __forceinline__ float elu_fast(float x) { return x > 0.f ? x : __builtin_amdgcn_exp2f(x * 1.4426950408889634f) - 1.0f; }
// derivative of ELU expressed through its OUTPUT y (in-place ELU in the reference, utils/util.py:89-91)
__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.f ? 1.f : y + 1.f; }

__device__ __forceinline__ float softplus_f(float u) {   // torch F.softplus, beta=1, threshold=20
    return u > 20.f ? u : log1pf(expf(u));
}

// one Adam update (torch/optim/adam.py::_single_tensor_adam order) + optional Polyak of the new value
struct AdamScal { float nss, bc2s, w1, w2, b2, eps, tau, omt; };
__device__ __forceinline__ AdamScal adam_scalars(float lr, float b1, float b2, float eps, float tau, int step) {
    AdamScal a;
    const double st = (double)step;
    const double bc1 = 1.0 - pow((double)b1, st), bc2 = 1.0 - pow((double)b2, st);
    a.nss = (float)(-((double)lr / bc1));
    a.bc2s = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - (double)b1);
    a.w2 = (float)(1.0 - (double)b2);
    a.b2 = b2; a.eps = eps; a.tau = tau; a.omt = (float)(1.0 - (double)tau);
    return a;
}
__device__ __forceinline__ void adam_elem(const AdamScal& a, float g, float* p, float* m, float* v, float* target) {
    // every operation PINNED (explicit fma / mul / add / div / sqrt, round to nearest): this function is inlined into the optimizer launch
    // and into weight-gradient epilogues (FLAG_ADAM), and the two must agree bit for bit whatever the compiler would contract where
    float mm = *m, vv = *v, pv = *p;
    mm = __fmaf_rn(a.w1, __fsub_rn(g, mm), mm);
    vv = __fmul_rn(vv, a.b2);
    vv = __fmaf_rn(__fmul_rn(a.w2, g), g, vv);
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(vv), a.bc2s), a.eps);
    pv = __fmaf_rn(a.nss, __fdiv_rn(mm, denom), pv);
    *m = mm; *v = vv; *p = pv;
    if (target) *target = __fmaf_rn(a.tau, pv, __fmul_rn(a.omt, *target));
}

// Per-optimizer-group device state: hyper-parameters (written once at create), the Adam step counter and the
// bias-correction scalars of the CURRENT step.  The loss kernel of a step program bumps it (one thread) so that the
// optimizer epilogues only read eight floats.
// b1p / b2p = beta^step in double precision, advanced by ONE multiplication per step: the two double-precision pow() calls this
// replaced ran in a single thread of a launch on the critical chain (heads_vae / qhead: its block 0 ended ~1 us after the others).
// They are trusted only while (pstep, pb1, pb2) say they belong to the current (step, beta1, beta2) -- a caller that rewrites the record
// (checkpoint restore, a test that zeroes the step) falls back to pow() once.
struct GroupCfg { int step; float lr, b1, b2, eps, tau; AdamScal sc; int pstep; float pb1, pb2; int pad_; double b1p, b2p; };
__device__ __forceinline__ void bump_group(GroupCfg* g) {
    const int step = g->step + 1;
    const float b1 = g->b1, b2 = g->b2;
    double p1, p2;
    if (g->pstep == step - 1 && g->pb1 == b1 && g->pb2 == b2 && step > 1) { p1 = g->b1p * (double)b1; p2 = g->b2p * (double)b2; }
    else { p1 = pow((double)b1, (double)step); p2 = pow((double)b2, (double)step); }
    g->step = step; g->pstep = step; g->pb1 = b1; g->pb2 = b2; g->b1p = p1; g->b2p = p2;
    AdamScal a;
    const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
    a.nss = (float)(-((double)g->lr / bc1));
    a.bc2s = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - (double)b1);
    a.w2 = (float)(1.0 - (double)b2);
    a.b2 = b2; a.eps = g->eps; a.tau = g->tau; a.omt = (float)(1.0 - (double)g->tau);
    g->sc = a;
}

// block-wide sum for 256-thread blocks; result valid in thread 0
__device__ __forceinline__ float block_sum_256(float v, float* sh /* >= 4 floats */) {
    v = wave_sum(v);
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return r;
}
