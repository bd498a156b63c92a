// Elementwise, reduction and optimizer kernels of the update path (gfx950).
// All of them are HBM/L2-latency bound at batch 256: one pass, coalesced, wave-shuffle reductions,
// deterministic per-block partial sums (no float atomics) that the optimizer launch finalises.
#include "common.h"
#include "kparams.h"
#include "heads_vae_tile.h"      // (also: RL_CONST_AS)
#include "x3.h"
#include "group.h"
#include "launchers.h"

// ------------------------------------------------------------------------------------------------
// minibatch slot fill: replay-ring gather (idx) or five separate arrays (reference Batch fields)
// reference: utils/buffer.py:39-48 (sample), utils/util.py:10-11 (unpack_batch)
// ------------------------------------------------------------------------------------------------
struct IdxGen { int on; unsigned long long seed, off; uint32_t stream_id; int hi; };
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1);
__device__ __forceinline__ int philox_index(const IdxGen& g, int e) {       // element e of a kind-1 PhiloxFill stream
    const long long q = e >> 2;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)g.off, (uint32_t)(g.off >> 32) ^ g.stream_id};
    philox4x32_10(c, (uint32_t)g.seed, (uint32_t)(g.seed >> 32));
    const uint32_t v = (e & 3) == 0 ? c[0] : (e & 3) == 1 ? c[1] : (e & 3) == 2 ? c[2] : c[3];
    return (int)(((unsigned long long)v * (unsigned long long)g.hi) >> 32);
}
// blocks [0, nblocks) of a launch cooperate on one slot fill
__device__ __forceinline__ void fill_slot_body(const SlotFill& p, const IdxGen& gen, int block, int nblocks) {
    const int row_w = 2 * p.S + p.A + 2;
    const long long total = (long long)p.B * row_w;
    for (long long e = (long long)block * 256 + threadIdx.x; e < total; e += (long long)nblocks * 256) {
        const int b = (int)(e / row_w), c = (int)(e - (long long)b * row_w);
        float v;
        if (p.ring) {
            const int src = gen.on ? philox_index(gen, b) : p.idx[b];
            v = p.ring[(size_t)src * row_w + c];
        } else {
            if (c < p.S) v = p.s[(size_t)b * p.S + c];
            else if (c < p.S + p.A) v = p.a[(size_t)b * p.A + (c - p.S)];
            else if (c < 2 * p.S + p.A) v = p.s2[(size_t)b * p.S + (c - p.S - p.A)];
            else if (c == 2 * p.S + p.A) v = p.r[b];
            else v = p.d[b];
        }
        const int SA = p.S + p.A;
        if (c < p.S) {
            p.XE[(size_t)b * (SA + p.S) + c] = v;
            p.XF[(size_t)b * SA + c] = v;
            p.XFpi[(size_t)b * SA + c] = v;
        } else if (c < SA) {
            p.XE[(size_t)b * (SA + p.S) + c] = v;
            p.XF[(size_t)b * SA + c] = v;
        } else if (c < SA + p.S) {
            p.XE[(size_t)b * (SA + p.S) + c] = v;
            p.XF2[(size_t)b * SA + (c - SA)] = v;
        } else if (c == SA + p.S) {
            p.R[b] = v;
        } else {
            p.D[b] = v;
        }
    }
}
__global__ __launch_bounds__(256) void fill_slot_kernel(SlotFill p) {
    IdxGen none; none.on = 0;
    fill_slot_body(p, none, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011): counter-based, replayable under hipGraph (counter from device)
// ------------------------------------------------------------------------------------------------
#include "philox.h"

__device__ __forceinline__ void philox_fill_body(const PhiloxFill& p, int block, int nblocks) {
    const unsigned long long step = p.step_dev ? (unsigned long long)(*p.step_dev + p.step_add) : 0ull;
    const unsigned long long off = p.offset + step;
    const int hi = p.hi_dev ? *p.hi_dev : p.hi;
    const long long nq = (p.n + 3) / 4;
    for (long long q = (long long)block * 256 + threadIdx.x; q < nq; q += (long long)nblocks * 256) {
        uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32) ^ p.stream_id};
        philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
        float out[4];
        if (p.kind == 0) {          // standard normal * std, Box-Muller on two pairs
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
                const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
                const float rad = sqrtf(-2.0f * logf(u1));
                float sn, cs;
                sincosf(6.283185307179586f * u2, &sn, &cs);
                out[2 * h] = rad * cs * p.std;
                out[2 * h + 1] = rad * sn * p.std;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long long e = q * 4 + s;
            if (e >= p.n) break;
            if (p.kind == 0) p.dst_f[e] = out[s];
            else p.dst_i[e] = (int)(((unsigned long long)c[s] * (unsigned long long)hi) >> 32);   // uniform in [0,hi)
        }
    }
}
__global__ __launch_bounds__(256) void philox_fill_kernel(PhiloxFill p) { philox_fill_body(p, blockIdx.x, gridDim.x); }
// the bare bijection on caller-given (counter, key) pairs: known-answer tests only (rlrep_philox_raw)
__global__ __launch_bounds__(256) void philox_raw_kernel(const uint32_t* __restrict__ ck, uint32_t* __restrict__ out, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    uint32_t c[4] = {ck[6 * e], ck[6 * e + 1], ck[6 * e + 2], ck[6 * e + 3]};
    philox4x32_10(c, ck[6 * e + 4], ck[6 * e + 5]);
#pragma unroll
    for (int s = 0; s < 4; ++s) out[4 * e + s] = c[s];
}

// ------------------------------------------------------------------------------------------------
// transposed weight shadows (ShadowEnt): block t of a shadow launch transposes one 32 x 32 tile through LDS
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int shadow_tiles(const ShadowEnt& e) { return ((e.rows + 31) / 32) * ((e.cols + 31) / 32); }
__device__ __forceinline__ void shadow_tile_body(const ShadowEnt* __restrict__ sh, int nsh, const float* __restrict__ base, int tile, bool target) {
    __shared__ float tl[32][33];
    int ei = 0, t0 = 0;
    for (int q = 0; q < nsh; ++q) { const int nt = shadow_tiles(sh[q]); if (tile < t0 + nt) { ei = q; break; } t0 += nt; if (q == nsh - 1) return; }
    const ShadowEnt e = sh[ei];
    float* dst = target ? e.st : e.sp;
    if (!dst) return;
    const int tc = (e.cols + 31) / 32, local = tile - t0;
    const int r0 = (local / tc) * 32, c0 = (local % tc) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 256 threads: 8 rows per pass
    const float* src = e.src ? e.src : base + e.off;
    if (e.kind == 1) {
        // bf16x3 images: the tile is one 32-deep step of 32 rows; thread = (row, four consecutive k) -> 8 bytes of each image
        const int r = r0 + (threadIdx.x >> 3), k4 = threadIdx.x & 7;
        if (r < e.rows) x3_shadow_store(reinterpret_cast<unsigned char*>(dst), e.rows, r, c0 + 4 * k4, *reinterpret_cast<const f32x4*>(src + (size_t)r * e.cols + c0 + 4 * k4));
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        tl[ty + 8 * k][tx] = (r < e.rows && c < e.cols) ? src[(size_t)r * e.cols + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (r < e.rows && c < e.cols) dst[(size_t)c * e.rows + r] = tl[tx][ty + 8 * k];
    }
}
__global__ __launch_bounds__(256) void shadow_kernel(const ShadowEnt* __restrict__ sh, int nsh, const float* __restrict__ base, int target) {
    shadow_tile_body(sh, nsh, base, blockIdx.x, target != 0);
}
extern "C" int rl_launch_shadow(const ShadowEnt* sh_dev, int nsh, int ntiles, const float* base, int target, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    if (ntiles <= 0 || nsh <= 0) return 0;
    hipLaunchKernelGGL(shadow_kernel, dim3(ntiles), dim3(256), 0, st, sh_dev, nsh, base, target);
    return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void train_prologue_kernel(TrainPrologue p) {
#include "train_prologue_body.h"
}
// group form: member m = blockIdx.y draws from its own seed, gathers from its own ring (bounded by its own size word) and counts its own steps
__global__ __launch_bounds__(256) void train_prologue_kernel_grp(TrainPrologue p0, long long mstride, long long rstride, const unsigned long long* __restrict__ seeds,
                                                                 const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    const long long dm = (long long)m * mstride;
    TrainPrologue p = p0;
    rl_rb(p.idx.dst_i, dm); rl_rb(p.idx.step_dev, dm); p.idx.seed = seeds[m];
    if (p.idx.hi_dev) p.idx.hi_dev += m;
    rl_rb(p.eps.dst_f, dm); rl_rb(p.eps.step_dev, dm); p.eps.seed = seeds[m];
    if (p.eps.hi_dev) p.eps.hi_dev += m;
    rl_rebase(p.fill, dm, (long long)m * rstride);
    rl_rb(p.counter, dm); rl_rb(p.ticket, dm);
#include "train_prologue_body.h"
}

// ------------------------------------------------------------------------------------------------
// tanh-squashed Gaussian policy head  (agent/sac/actor.py:76-91, 16-60)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void policy_fwd_kernel(PolicyFwd p) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    const float* o = p.O + (size_t)b * 2 * p.A;
    float lp = 0.f;
    for (int j = 0; j < p.A; ++j) {
        const float mu = o[j];
        const float t = tanhf(o[p.A + j]);
        const float l = -5.f + 3.5f * (t + 1.f);
        const float sg = expf(l);
        const float e = p.eps ? p.eps[(size_t)b * p.A + j] : 0.f;
        const float x = mu + e * sg;
        const float y = tanhf(x);
        p.act[(size_t)b * p.ld_act + j] = p.clamp ? fminf(fmaxf(y, p.lo), p.hi) : y;
        lp += -0.5f * e * e - l - 0.91893853320467274f - 2.f * (0.69314718055994531f - x - softplus_f(-2.f * x));
    }
    if (p.logp) p.logp[b] = lp;
}

// SACAgent.select_action (sac_agent.py:89-96) for ONE observation in ONE launch: the three actor layers as wave-cooperative dot products (a wave
// per output row, 4-byte loads along the row, fixed-order lane reduction), the tanh-Gaussian head, the Philox draw of fill_normal(seed, offset)
// for its A elements.  obs / act may be pinned HOST buffers (mapped): no copy launch on either side -- main.py's loop pays one launch and one
// stream synchronisation per environment step instead of nine dependent operations (tools/exp/host_loop.py).
__global__ __launch_bounds__(1024) void select_action_kernel(SelectAct p) {
#include "select_action_body.h"
}
// group form: member m = blockIdx.y acts on observation m with its own actor and its own Philox seed, writes action m
__global__ __launch_bounds__(1024) void select_action_kernel_grp(SelectAct p0, long long mstride, const unsigned long long* __restrict__ seeds, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    const long long dm = (long long)m * mstride;
    SelectAct p = p0;
    p.obs += (long long)m * p.S; p.act += (long long)m * p.A;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
#include "select_action_body.h"
}
// SACAgent.select_actions: E = gridDim.x observations in ONE launch, one observation row per workgroup -- workgroup e acts on obs + e * S, writes
// act + e * A and draws at offset + (e << 20), i.e. at call counter c + e when the caller passes c << 20: E successive select_action calls in
// row order (the device environments' convention, group_env.h).  The body is select_action_kernel's: row e is bit for bit that kernel's
// action for the same observation at that offset, in the same summation order and with the same latency.
__global__ __launch_bounds__(1024) void select_action_kernel_n(SelectAct p0) {
    const long long e = blockIdx.x;
    SelectAct p = p0;
    p.obs += e * p.S; p.act += e * p.A;
    p.offset += (unsigned long long)e << 20;
#include "select_action_body.h"
}
// group form: workgroup (e, slot) is row e of member m -- observation and action row m * E + e, the member's actor and seed
__global__ __launch_bounds__(1024) void select_action_kernel_grp_n(SelectAct p0, long long mstride, const unsigned long long* __restrict__ seeds, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    const long long dm = (long long)m * mstride;
    const long long row = (long long)m * gridDim.x + blockIdx.x;
    SelectAct p = p0;
    p.obs += row * p.S; p.act += row * p.A;
    p.offset += (unsigned long long)blockIdx.x << 20;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
#include "select_action_body.h"
}

// gradient of the actor loss w.r.t. the trunk output [mu | rho]; h = dL/d(action) from the critic path
__global__ __launch_bounds__(256) void policy_bwd_kernel(PolicyBwd p) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    const float g = (float)exp(p.alpha_state[0]) * p.inv_batch;      // dL/dlogpi = alpha / B
    const float* o = p.O + (size_t)b * 2 * p.A;
    for (int j = 0; j < p.A; ++j) {
        const float t = tanhf(o[p.A + j]);
        const float l = -5.f + 3.5f * (t + 1.f);
        const float sg = expf(l);
        const float e = p.eps[(size_t)b * p.A + j];
        const float y = p.act[(size_t)b * p.ld_act + j];
        const float h = p.dA[(size_t)b * p.ld_dA + j] * (1.f - y * y);
        const float dmu = g * 2.f * y + h;
        const float dl = g * (-1.f + 2.f * y * e * sg) + h * e * sg;
        p.G[(size_t)b * 2 * p.A + j] = dmu;
        p.G[(size_t)b * 2 * p.A + p.A + j] = dl * 3.5f * (1.f - t * t);
    }
}

// ------------------------------------------------------------------------------------------------
// vlsac ELBO pieces (agent/vlsac/vlsac_agent.py:135-150)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vae_mid_kernel(VaeMid p) {
    __builtin_amdgcn_s_setprio(3);      // small launch on a latency-critical chain (see gemm16_kernel)
    __shared__ float sh[4];
    const int F = p.F;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    float k = 0.f;
    if (e < (long long)p.B * F) {
        const int b = (int)(e / F), j = (int)(e - (long long)b * F);
        const float m1 = p.EH[(size_t)b * 2 * F + j], l1r = p.EH[(size_t)b * 2 * F + F + j];
        const float m2 = p.FH[(size_t)b * 2 * F + j], l2r = p.FH[(size_t)b * 2 * F + F + j];
        const float l1 = clamp_lstd(l1r), l2 = clamp_lstd(l2r);
        const float es = p.eps[(size_t)b * F + j] * expf(l1);
        p.Z[(size_t)b * F + j] = m1 + es;
        p.EZ[(size_t)b * F + j] = es * lstd_mask(l1r);        // dz/dlog_std (clamp gradient folded in)
        const float v1 = expf(2.f * l1), iv2 = expf(-2.f * l2), d = m1 - m2;
        k = l2 - l1 + 0.5f * (v1 + d * d) * iv2 - 0.5f;
        const float sc = p.scale;                       // 1 / (B_global * F)
        const float dm1 = d * iv2 * sc;
        p.GEH[(size_t)b * 2 * F + j] = dm1;
        p.GEH[(size_t)b * 2 * F + F + j] = (v1 * iv2 - 1.f) * sc * lstd_mask(l1r);
        p.GFH[(size_t)b * 2 * F + j] = -dm1;
        p.GFH[(size_t)b * 2 * F + F + j] = (1.f - (v1 + d * d) * iv2) * sc * lstd_mask(l2r);
    }
    const float s = block_sum_256(k, sh);
    if (threadIdx.x == 0) {
        p.partial[blockIdx.x] = s;
        if (blockIdx.x == 0 && p.step) bump_group(p.step);    // Adam step counter of the feature group
    }
}

// The two Gaussian heads (encoder, f) and vae_mid in ONE launch: one 16 x 16 tile per workgroup (heads_vae_tile.h).  One dependent launch
// less per feature step than the heads launch + vae_mid_kernel.
__global__ __launch_bounds__(256) void heads_vae_kernel(HeadsVae p) {
    __builtin_amdgcn_s_setprio(3);      // small launch on a latency-critical chain (see gemm16_kernel)
    __shared__ float red[4][4][256];    // [wave][net * 2 + part][16 x 16]
    __shared__ float sh[4];
    const int tr = blockIdx.x / p.tiles_c, tc = blockIdx.x - tr * p.tiles_c;
    heads_vae_tile<false>(p, tr, tc, p.eps, red, sh);
}

__global__ __launch_bounds__(256) void vae_mse_kernel(VaeMse p) {
    __shared__ float sh[4];
    const int W = p.S + 1;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    float es = 0.f, er = 0.f;
    if (e < (long long)p.B * W) {
        const int b = (int)(e / W), c = (int)(e - (long long)b * W);
        const float pred = p.DH[(size_t)b * W + c];
        if (c < p.S) {
            const float d = pred - p.s2[(size_t)b * p.ld_s2 + c];
            es = d * d;
            p.GDH[(size_t)b * W + c] = d * p.scale_s;   // 1/(B_global*S)
        } else {
            const float d = pred - p.r[b];
            er = d * d;
            p.GDH[(size_t)b * W + c] = d * p.scale_r;   // 1/B_global
        }
    }
    const float a = block_sum_256(es, sh);
    const float c2 = block_sum_256(er, sh);
    if (threadIdx.x == 0) { p.partial[2 * blockIdx.x] = a; p.partial[2 * blockIdx.x + 1] = c2; }
}

// ------------------------------------------------------------------------------------------------
// Q heads: last H->1 linear on an ELU activation, TD target, critic / actor losses
// (sac_agent.py:112-123,141-159; vlsac_agent.py:207-226,169-180)
// one wave per batch row
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float row_dot(const float* __restrict__ e, const float* __restrict__ w, int H, int lane) {
    float s = 0.f;
    for (int k = lane; k < H; k += 64) s = fmaf(e[k], w[k], s);
    return wave_sum(s);
}

__global__ __launch_bounds__(256) void qhead_critic_kernel(QHeadCritic p) {
#include "qhead_critic_body.h"
}
// hyp: member 0's MemberHyper (kparams.h) -- the member's discount comes from its record, not from member 0's p0.gamma
__global__ __launch_bounds__(256) void qhead_critic_kernel_grp(QHeadCritic p0, long long mstride, const MemberHyper* __restrict__ hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    QHeadCritic p = p0;
    rl_rebase(p, (long long)member * mstride);
    p.gamma = rl_mv<true>(hyp, (long long)member * mstride)->gamma;
#include "qhead_critic_body.h"
}

__global__ __launch_bounds__(256) void qhead_actor_kernel(QHeadActor p) {
#include "qhead_actor_body.h"
}
__global__ __launch_bounds__(256) void qhead_actor_kernel_grp(QHeadActor p0, long long mstride, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    QHeadActor p = p0;
    rl_rebase(p, (long long)member * mstride);
#include "qhead_actor_body.h"
}

// ------------------------------------------------------------------------------------------------
// fused multi-tensor Adam (+ Polyak of a sub-range) + metric finalisation + temperature update
// torch/optim/adam.py::_single_tensor_adam operation order; SURVEY Appendix A.11/A.12
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void copy_segs_body(const CopySegs& p, int blk, int nblk) {
    const long long total = p.end[p.n - 1];
    for (long long e = (long long)blk * 256 + threadIdx.x; e < total; e += (long long)nblk * 256) {
        int q = 0;
#pragma unroll
        for (int k = 0; k < COPY_MAX_SEGS - 1; ++k) if (k < p.n - 1 && e >= p.end[k]) q = k + 1;
        const long long base = q ? p.end[q - 1] : 0;
        p.dst[q][e - base] = p.src[q][e - base];
    }
    if (blk == 0 && threadIdx.x == 0 && p.isrc) *p.idst = *p.isrc;
}
// The ONE optimizer task of the launch travels twice: as the by-value record `t` and -- its four arena pointers, the group record, the Polyak
// target, the element count and the block count -- as 14 leading scalar arguments that the hardware PRELOADS into SGPRs at wave launch
// (build.sh compiles this file with -mllvm -amdgpu-kernarg-preload-count=14): an optimizer block issues its four 16-byte loads and the load of the
// group's scalars with its first instructions, instead of after three dependent round trips (task table -> record -> group record).
// hdr = adam_blocks | vec_ok << 30 (vec_ok: every arena pointer 16-byte aligned and the Polyak sub-range on multiples of four floats).
// (the body of an optimizer block; `bid` = block index within the optimizer part of the launch)
// DP (compile time): the data-parallel instantiation (dp_pull.h).  A run-time switch would put the prefetched loads of p / g / m / v into
// control-flow diamonds (hipcc drains vmcnt at their merges): the single-GPU launch must not pay for code it never runs (measured: 5.4 -> 11.7 us).
// the target-update period of the Polyak gate: the record's in the single-agent kernels, the member's MemberHyper in a group form
template <bool GRP> __device__ __forceinline__ int pol_period_of(const AdamTask& t, const MemberHyper* hyp, long long mdelta) {
    if constexpr (GRP) return rl_mv<GRP>(hyp, mdelta)->pol_period;
    else { (void)hyp; (void)mdelta; return t.pol_period; }
}
template <int DP, bool GRP = false>
__device__ __forceinline__ void adam_elems(const int bid, float* __restrict__ ap, const float* __restrict__ agr, float* __restrict__ am, float* __restrict__ av,
                                           const GroupCfg* __restrict__ agrp, float* __restrict__ atarget, int an, int hdr, const AdamTask& t, const AdamSnap& snap, const DpPull& dp,
                                           long long mdelta = 0, const MemberHyper* hyp = nullptr);
template <int DP, bool GRP = false>
__device__ __forceinline__ void adam_block(const int bid, float* __restrict__ ap, const float* __restrict__ agr, float* __restrict__ am, float* __restrict__ av,
                                           const GroupCfg* __restrict__ agrp, float* __restrict__ atarget, int an, int hdr, const AdamTask& t,
                                           const FinTask* __restrict__ fin, int nfin, const SlotFill& sf, int fill_blocks, const SlotFill& sf2, int fill2_blocks,
                                           const AdamSnap& snap, int snap_blocks, const DpPull& dp, long long mdelta = 0, const MemberHyper* hyp = nullptr) {
    const int adam_blocks = hdr & 0x3fffffff;
    // Data parallel (DP != 0, dp_pull.h): the optimizer blocks and the trailing block wait for the peers' gradients, read every rank's arena in
    // rank order where they used to read one gradient (DP == 1), or sum their rank's shard first and read the sums from the shards' owners (DP == 2),
    // and the last of them to finish runs the DONE handshake.  A block that saw a wait time out applies NOTHING.  The riders below take no part.
    constexpr bool dpon = DP != 0;
    if (bid > adam_blocks + fill_blocks + fill2_blocks) {       // the small segments of a folded snapshot (AdamSnap)
        copy_segs_body(snap.segs, bid - adam_blocks - fill_blocks - fill2_blocks - 1, snap_blocks);
        return;
    }
    if (bid > adam_blocks + fill_blocks) {       // rlrep_prefetch_batch_slot(1): spedersac's second minibatch rides here too
        IdxGen none; none.on = 0;
        fill_slot_body(sf2, none, bid - adam_blocks - fill_blocks - 1, fill2_blocks);
        return;
    }
    if (bid > adam_blocks) {
        // rlrep_prefetch_batch: the gather of the NEXT minibatch rides here (the step that owned the slot has finished
        // reading it: its weight-gradient launch precedes this one)
        IdxGen none; none.on = 0;
        fill_slot_body(sf, none, bid - adam_blocks - 1, fill_blocks);
        return;
    }
    if (bid == adam_blocks) {
        // trailing block: finalises the step's metrics / temperature
        unsigned dpe = 0; bool good = true;
        if constexpr (dpon) dpe = dp_begin(dp, false, true, &good);
        if (threadIdx.x == 64 && t.sync_steps) rl_mv<GRP>(t.sync_steps, mdelta)[2] = rl_mv<GRP>(t.sync_steps, mdelta)[0];          // (beside the metric tasks, not in their serial chain)
        if (threadIdx.x < 64 && good) finalize_tasks<GRP>(fin, nfin, threadIdx.x, dpon ? &dp : nullptr, mdelta, hyp);
        if constexpr (dpon) dp_end(dp, dpe, true);
        return;
    }
    unsigned dpe = 0; bool good = true;
    if constexpr (dpon) dpe = dp_begin(dp, bid == 0, true, &good);
    if constexpr (DP == 2) good = dp_reduce_scatter(dp, dpe, bid, (long long)(agr - dp.base[dp.rank]), (long long)an >> 2, good) && good;
    if (good) adam_elems<DP, GRP>(bid, ap, agr, am, av, agrp, atarget, an, hdr, t, snap, dp, mdelta, hyp);
    if constexpr (dpon) dp_end(dp, dpe, true);
}

// the elements of one optimizer block (thread-level early exits inside: the caller brackets it with the data-parallel handshake)
// GRP (a seed group's launch, group.h): `t` is member 0's record as it lies in the kernel-argument segment; the pointers read from it are moved by
// mdelta where they are dereferenced (a rebased local copy of the record put slabs[] in scratch memory: its index is known at run time only)
template <int DP, bool GRP>
__device__ __forceinline__ void adam_elems(const int bid, float* __restrict__ ap, const float* __restrict__ agr, float* __restrict__ am, float* __restrict__ av,
                                           const GroupCfg* __restrict__ agrp, float* __restrict__ atarget, int an, int hdr, const AdamTask& t, const AdamSnap& snap, const DpPull& dp,
                                           long long mdelta, const MemberHyper* hyp) {
    constexpr bool dpon = DP != 0;
    // (the arena pointers and the group record are preloaded arguments: these loads go out before the record `t` has arrived)
    const long long i = ((long long)bid * 256 + threadIdx.x) * 4;
    if (i >= an) return;
    const AdamScal sc = agrp->sc;
    const bool vec = (i + 4 <= an) && ((hdr >> 30) & 1);
    f32x4 g = {0.f, 0.f, 0.f, 0.f}, p4 = g, m4 = g, v4 = g;
    if (vec) {
        if constexpr (!dpon) g = *reinterpret_cast<const f32x4*>(agr + i);
        p4 = *reinterpret_cast<f32x4*>(ap + i); m4 = *reinterpret_cast<f32x4*>(am + i); v4 = *reinterpret_cast<f32x4*>(av + i);
    }
    asm volatile("" ::: "memory");      // (pin: the loads above stay ahead of the reads of the record below)
    long long goff = 0;                                                        // the group slice inside the shared arena (same layout on every rank)
    if constexpr (dpon) {
        goff = (long long)(agr - dp.base[dp.rank]);
        if constexpr (DP == 2) { if (vec) g = dp_gather4(dp, goff, i >> 2); }        // (the launcher takes the two-shot form only for slices wholly on the 16-byte path)
        else if (vec) g = dp_sum4(dp, goff + i);
    }
    const int ti = 0;
    // ranges whose optimizer ran in the weight-gradient epilogues (FLAG_ADAM): nothing to do here
    if (t.nskip > 0 && i >= t.skip_off[0] && i < t.skip_off[0] + t.skip_n[0]) return;
    if (t.nskip > 1 && i >= t.skip_off[1] && i < t.skip_off[1] + t.skip_n[1]) return;
    const bool pol_on = atarget && (!t.pol_steps || ((*rl_mv<GRP>(t.pol_steps, mdelta)) % pol_period_of<GRP>(t, hyp, mdelta)) == 0);
    if (vec && t.nslab) {
        // split-K partial gradients finished here (AdamTask::Slab): all partials in flight together, summed in split order (the order of
        // the finishing launch this replaces: bit-identical), the sum filed in the gradient arena for whoever reads gradients
        int qs = -1;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < t.nslab && i >= t.slabs[q].off && i < t.slabs[q].off + t.slabs[q].n) qs = q;
        if (qs >= 0) {
            const AdamTask::Slab& sl = t.slabs[qs];
            const long long l = i - sl.off;
            const int splits = sl.splits;
            if (sl.cols == 0 || sl.cols == sl.ldpad) {
                const long long task = l / sl.per, r = l - task * sl.per;
                const long long ss = sl.cols ? sl.sstride : sl.per;
                const float* s0 = rl_mv<GRP>(sl.slab, mdelta) + (size_t)task * splits * sl.per + r;
                f32x4 part[16];
#pragma unroll
                for (int sp = 0; sp < 16; ++sp) part[sp] = *reinterpret_cast<const f32x4*>(s0 + (size_t)min(sp, splits - 1) * ss);
                g = part[0];
#pragma unroll
                for (int sp = 1; sp < 16; ++sp) if (sp < splits) g += part[sp];
            } else {
                // padded slab rows (cols % 4 != 0): the four elements may sit on two rows -- element-wise, same split order
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const long long ll = l + s, row = ll / sl.cols, col = ll - row * sl.cols;
                    const float* s0 = rl_mv<GRP>(sl.slab, mdelta) + (size_t)row * sl.ldpad + col;
                    float a = s0[0];
                    for (int sp = 1; sp < splits; ++sp) a += s0[(size_t)sp * sl.sstride];
                    g[s] = a;
                }
            }
            *reinterpret_cast<f32x4*>(const_cast<float*>(agr) + i) = g;
        }
    }
    if (vec) {
        const bool pol = pol_on && i >= t.pol_off && i < t.pol_off + t.pol_n;
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
        if (pol) t4 = *reinterpret_cast<f32x4*>(atarget + (i - t.pol_off));
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float pp = p4[s], mm = m4[s], vv = v4[s], tt = t4[s];
            adam_elem(sc, g[s], &pp, &mm, &vv, pol ? &tt : nullptr);
            p4[s] = pp; m4[s] = mm; v4[s] = vv; t4[s] = tt;
        }
        *reinterpret_cast<f32x4*>(ap + i) = p4; *reinterpret_cast<f32x4*>(am + i) = m4; *reinterpret_cast<f32x4*>(av + i) = v4;
        if (pol) *reinterpret_cast<f32x4*>(atarget + (i - t.pol_off)) = t4;
        if (snap.on && ti == 0 && i >= snap.off && i < snap.off + snap.n) {        // folded snapshot: the new values, as the deferred chain will read them
            const f32x4 sv = snap.which == 0 ? p4 : (pol ? t4 : *reinterpret_cast<const f32x4*>(atarget + (i - t.pol_off)));
            if (i + 4 <= snap.off + snap.n && !(snap.off & 3) && !(((uintptr_t)snap.block) & 15)) *reinterpret_cast<f32x4*>(snap.block + (i - snap.off)) = sv;
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (i + q < snap.off + snap.n) snap.block[i + q - snap.off] = sv[q];      // (a range that does not end on a multiple of four)
            }
        }
        if (t.sh) {
            // keep the transposed shadows of the weight matrices current (4 scattered 4-byte stores; tensors start on multiples of 4 floats,
            // so the four elements belong to one tensor or to alignment padding)
            for (int q = 0; q < t.nsh; ++q) {
                const ShadowEnt e = t.sh[q];
                if (i < e.off || i >= e.off + e.n) continue;
                if (e.kind == 1) {
                    // (cols % 32 == 0 and the tensor starts on a multiple of 4 floats: the four elements are four consecutive k of one row)
                    const long long l = i - e.off;
                    const int r = (int)(l / e.cols), c = (int)(l - (long long)r * e.cols);
                    x3_shadow_store(reinterpret_cast<unsigned char*>(e.sp), e.rows, r, c, p4);
                    if (pol && e.st) x3_shadow_store(reinterpret_cast<unsigned char*>(e.st), e.rows, r, c, t4);
                    break;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const long long l = i + s - e.off;
                    if (l >= e.n) break;
                    const int r = (int)(l / e.cols), c = (int)(l - (long long)r * e.cols);
                    e.sp[(size_t)c * e.rows + r] = p4[s];
                    if (pol && e.st) e.st[(size_t)c * e.rows + r] = t4[s];
                }
                break;
            }
        }
    } else {
        for (int s = 0; s < 4 && i + s < an; ++s) {
            const long long e = i + s;
            float* tp = (pol_on && e >= t.pol_off && e < t.pol_off + t.pol_n) ? atarget + (e - t.pol_off) : nullptr;
            float ge;
            if constexpr (dpon) ge = dp_sum1(dp, goff + e); else ge = agr[e];
            adam_elem(sc, ge, ap + e, am + e, av + e, tp);
            if (snap.on && ti == 0 && e >= snap.off && e < snap.off + snap.n) snap.block[e - snap.off] = snap.which == 0 ? ap[e] : atarget[e - t.pol_off];
            for (int q = 0; t.sh && q < t.nsh; ++q) {
                const ShadowEnt se = t.sh[q];
                if (e < se.off || e >= se.off + se.n) continue;
                const long long l = e - se.off;
                const int r = (int)(l / se.cols), c = (int)(l - (long long)r * se.cols);
                if (se.kind == 1) {         // (unreachable for the shapes that get such a shadow: their arrays take the 16-byte path above)
                    x3_shadow_store1(reinterpret_cast<unsigned char*>(se.sp), se.rows, r, c, ap[e]);
                    if (tp && se.st) x3_shadow_store1(reinterpret_cast<unsigned char*>(se.st), se.rows, r, c, *tp);
                    break;
                }
                se.sp[(size_t)c * se.rows + r] = ap[e];
                if (tp && se.st) se.st[(size_t)c * se.rows + r] = *tp;
                break;
            }
        }
    }
}

// Two kernels: the single-GPU one carries no DpPull in its kernel-argument segment (440 bytes it never reads: VERDICT r05 item 6) and is byte for
// byte the kernel of round 4; the data-parallel one (one-shot / two-shot) takes the record by value -- its first instructions need it.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ ap, const float* __restrict__ agr, float* __restrict__ am, float* __restrict__ av,
                                                   const GroupCfg* __restrict__ agrp, float* __restrict__ atarget, int an, int hdr, AdamTask t,
                                                   const FinTask* __restrict__ fin, int nfin, SlotFill sf, int fill_blocks, SlotFill sf2, int fill2_blocks, AdamSnap snap, int snap_blocks) {
    __builtin_amdgcn_s_setprio(3);      // small launch on a latency-critical chain (see gemm16_kernel)
    const DpPull nodp = DpPull();
    adam_block<0>(blockIdx.x, ap, agr, am, av, agrp, atarget, an, hdr, t, fin, nfin, sf, fill_blocks, sf2, fill2_blocks, snap, snap_blocks, nodp);
}
// group form (group.h): member = blockIdx.y; the arenas, the riders and the metric finishers' pointers move to the member's block, and so do the
// pointers adam_block / adam_elems read from the record `t`, where they read them (the record itself stays in the kernel-argument segment).  No
// folded snapshot (the launcher refuses one: a group has no deferred chain); `snap` only fills the argument list.  hyp: member 0's MemberHyper
// (kparams.h) -- the Polyak gate's period and the temperature optimizer's lr / learn gate come from the member's record, not from `t` / `fin`.
__global__ __launch_bounds__(256) void adam_kernel_grp(float* ap, const float* agr, float* am, float* av, const GroupCfg* agrp, float* atarget, int an, int hdr, AdamTask t,
                                                       const FinTask* __restrict__ fin, int nfin, SlotFill sf, int fill_blocks, SlotFill sf2, int fill2_blocks, AdamSnap snap, int snap_blocks,
                                                       long long mstride, long long rstride, const MemberHyper* hyp, const int* __restrict__ live) {
    RL_GRP_MEMBER(member, live);
    __builtin_amdgcn_s_setprio(3);
    const long long dm = (long long)member * mstride, dr = (long long)member * rstride;
    rl_rb(ap, dm); rl_rb(agr, dm); rl_rb(am, dm); rl_rb(av, dm); rl_rb(agrp, dm); rl_rb(atarget, dm);
    SlotFill s1 = sf, s2 = sf2; rl_rebase(s1, dm, dr); rl_rebase(s2, dm, dr);
    const DpPull nodp = DpPull();
    adam_block<0, true>(blockIdx.x, ap, agr, am, av, agrp, atarget, an, hdr, t, fin, nfin, s1, fill_blocks, s2, fill2_blocks, snap, snap_blocks, nodp, dm, hyp);
}
template <int DP>
__global__ __launch_bounds__(256) void adam_dp_kernel(float* __restrict__ ap, const float* __restrict__ agr, float* __restrict__ am, float* __restrict__ av,
                                                      const GroupCfg* __restrict__ agrp, float* __restrict__ atarget, int an, int hdr, AdamTask t,
                                                      const FinTask* __restrict__ fin, int nfin, SlotFill sf, int fill_blocks, SlotFill sf2, int fill2_blocks, AdamSnap snap, int snap_blocks, DpPull dp) {
    __builtin_amdgcn_s_setprio(3);
    adam_block<DP>(blockIdx.x, ap, agr, am, av, agrp, atarget, an, hdr, t, fin, nfin, sf, fill_blocks, sf2, fill2_blocks, snap, snap_blocks, dp);
}

// The optimizer launch of feature step k AND the first launch of feature step k + 1: blocks [0, gtiles) are 16 x 16 tiles of the
// next step's first layers (encoder.l1 / f.l1: their weights were already updated in step k's weight-gradient epilogues, FLAG_ADAM, and
// their input rows come straight from the replay ring through the index pool -- the minibatch slot itself is being gathered by the fill
// blocks of this very launch); the blocks behind them are an ordinary optimizer launch that skips those two layers (AdamTask::skip_*).
// The two parts share nothing: one dependent launch less per feature step.
__global__ __launch_bounds__(256) void adam_l1_kernel(float* __restrict__ ap, const float* __restrict__ agr, float* __restrict__ am, float* __restrict__ av,
                                                      const GroupCfg* __restrict__ agrp, float* __restrict__ atarget, int an, int hdr, int gtiles, int tb1, int tcs0, int tcs1,
                                                      AdamTask t, const FinTask* __restrict__ fin, int nfin, SlotFill sf, int fill_blocks, GemmTask g0, GemmTask g1) {
    __shared__ float red[4][1][4][64];
    __shared__ float bsum[4][16];
    __builtin_amdgcn_s_setprio(3);
    const int bid = blockIdx.x;
    if (bid < gtiles) {
        const bool second = bid >= tb1;
        const GemmTask& gt = second ? g1 : g0;
        const int local = second ? bid - tb1 : bid, tiles_c = second ? tcs1 : tcs0;
        const int tr = local / tiles_c, tc = local - tr * tiles_c;
#ifdef RL_TIMING
        gemm16_tile<LD_ROW, LD_ROW, 1, false, false, false, false, GemmTask, EPI_FWD, ACT_RELU, true>(gt, tr, tc, red, bsum, nullptr, nullptr);
#else
        gemm16_tile<LD_ROW, LD_ROW, 1, false, false, false, false, GemmTask, EPI_FWD, ACT_RELU, true>(gt, tr, tc, red, bsum, nullptr);
#endif
        return;
    }
    SlotFill none2 = SlotFill(); AdamSnap nosnap = AdamSnap(); DpPull nodp = DpPull();
    adam_block<0>(bid - gtiles, ap, agr, am, av, agrp, atarget, an, hdr, t, fin, nfin, sf, fill_blocks, none2, 0, nosnap, 0, nodp);
}

__global__ __launch_bounds__(256) void polyak_kernel(PolyakTask t) {
    if (t.steps && ((*t.steps) % t.period) != 0) return;
    const float omt = (float)(1.0 - (double)t.tau);
    if ((t.n & 3) == 0 && (((uintptr_t)t.src | (uintptr_t)t.dst) & 15) == 0) {
        for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < t.n; i += (long long)gridDim.x * 1024) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(t.src + i);
            f32x4 b = *reinterpret_cast<f32x4*>(t.dst + i);
#pragma unroll
            for (int s = 0; s < 4; ++s) b[s] = t.tau * a[s] + omt * b[s];
            *reinterpret_cast<f32x4*>(t.dst + i) = b;
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < t.n; i += (long long)gridDim.x * 256)
        t.dst[i] = t.tau * t.src[i] + omt * t.dst[i];
}

__global__ void counter_inc_kernel(int* c, int mirror) { if (threadIdx.x == 0 && blockIdx.x == 0) { const int v = *c + 1; *c = v; if (mirror) c[mirror] = v; } }

// c[mirror] = c[0] (the train() counter's copy that the next train prologue reads: rlrep_train_prologue's catch-up launch)
__global__ void counter_sync_kernel(int* c, int mirror) { if (threadIdx.x == 0 && blockIdx.x == 0) c[mirror] = c[0]; }

__global__ __launch_bounds__(256) void copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

// segments laid end to end: element e of the concatenation belongs to the first segment whose end > e
__global__ __launch_bounds__(256) void copy_segs_kernel(CopySegs p) {
    __builtin_amdgcn_s_setprio(3);      // small launch on a latency-critical chain (see gemm16_kernel)
    copy_segs_body(p, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static inline int grid_for(long long n, int per_block, int cap) {
    long long g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

extern "C" int rl_launch_fill_slot(const SlotFill* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    const long long total = (long long)p->B * (2 * p->S + p->A + 2);
    hipLaunchKernelGGL(fill_slot_kernel, dim3(grid_for(total, 256, 2048)), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_philox(const PhiloxFill* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(philox_fill_kernel, dim3(grid_for((p->n + 3) / 4, 256, 2048)), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_philox_raw(const uint32_t* ck, uint32_t* out, long long n, hipStream_t st) {
    hipLaunchKernelGGL(philox_raw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ck, out, n);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_policy_fwd(const PolicyFwd* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(policy_fwd_kernel, dim3((p->B + 255) / 256), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
// ReplayBuffer.add's staged rows into the device ring, wrap-around included, and the new fill level into the device scalar the index generator
// reads: ONE launch that reads the pinned staging rows in place (it replaces an SDMA copy per ring segment plus a fill launch for the scalar --
// three stream operations in front of every train() graph of main.py's loop)
__global__ __launch_bounds__(256) void replay_add_kernel(float* __restrict__ ring, long long capacity, int row, long long ptr, const float* __restrict__ rows,
                                                         long long nrows, int* size_dev, int new_size) {
    const long long n = nrows * row;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long r = e / row, c = e - r * row;
        long long dst = ptr + r; if (dst >= capacity) dst -= capacity;
        ring[dst * row + c] = rows[e];
    }
    if (size_dev && blockIdx.x == 0 && threadIdx.x == 0) *size_dev = new_size;
}
// group form: member m = blockIdx.y copies its own nrows staged rows (rows + m * rows_stride) into its own ring (ring + m * ring_stride floats)
// and writes its own fill level (size_dev[m])
__global__ __launch_bounds__(256) void replay_add_kernel_grp(float* __restrict__ ring, long long ring_stride, long long capacity, int row, long long ptr,
                                                             const float* __restrict__ rows, long long rows_stride, long long nrows, int* size_dev, int new_size) {
    const int m = blockIdx.y;
    ring += (long long)m * ring_stride; rows += (long long)m * rows_stride;
    const long long n = nrows * row;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long r = e / row, c = e - r * row;
        long long dst = ptr + r; if (dst >= capacity) dst -= capacity;
        ring[dst * row + c] = rows[e];
    }
    if (size_dev && blockIdx.x == 0 && threadIdx.x == 0) size_dev[m] = new_size;
}
// ReplayBuffer.add_device: n transitions that already live on the device as five arrays (states, actions, next states, rewards, dones; each with
// its row stride) packed into ring rows [s, a, s', r, d] from row `start` on, wrapping at `capacity`, and the new fill level into the size word
// as replay_add_kernel writes it: ONE launch, ordinary per-lane loads and stores.
__device__ __forceinline__ void replay_add_cols_body(const ReplayCols& p, float* __restrict__ ring, long long plane) {
    const long long total = p.n * p.row;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long r = e / p.row; const int c = (int)(e - r * p.row);
        const long long src = plane + r;
        float v;
        if (c < p.S) v = p.s[src * p.ld_s + c];
        else if (c < p.S + p.A) v = p.a[src * p.ld_a + (c - p.S)];
        else if (c < 2 * p.S + p.A) v = p.s2[src * p.ld_s2 + (c - p.S - p.A)];
        else if (c == 2 * p.S + p.A) v = p.r[src];
        else v = p.d[src];
        long long dst = p.start + r; if (dst >= p.capacity) dst -= p.capacity;
        ring[dst * p.row + c] = v;
    }
}
__global__ __launch_bounds__(256) void replay_add_cols_kernel(ReplayCols p) {
    replay_add_cols_body(p, p.ring, 0);
    if (p.size_dev && blockIdx.x == 0 && threadIdx.x == 0) *p.size_dev = p.new_size;
}
// group form: member m = blockIdx.y packs plane m of the five arrays (rows m * n ..) into its own ring and writes its own fill level; like
// replay_add_kernel_grp it does not look at the live table
__global__ __launch_bounds__(256) void replay_add_cols_kernel_grp(ReplayCols p) {
    const int m = blockIdx.y;
    replay_add_cols_body(p, p.ring + (long long)m * p.ring_stride, (long long)m * p.n);
    if (p.size_dev && blockIdx.x == 0 && threadIdx.x == 0) p.size_dev[m] = p.new_size;
}
// counter-reading form (rlrep_replay_add_cols_ctl, capturable): the first row and the fill level come from the loop record (kparams.h
// RL_CTL_*) as the act launch of the same iteration left them; the row packing is replay_add_cols_body.  Every workgroup reads START; ONE
// thread publishes SIZE to the size word and advances the words this launch never reads: ITER, T, and CALLS unless the iteration was a warm-up one.
__global__ __launch_bounds__(256) void replay_add_cols_kernel_ctl(ReplayCols p0, long long* __restrict__ ctl) {
    ReplayCols p = p0;
    const long long st = ctl[RL_CTL_START];
    p.start = (st < 0 || st >= p.capacity) ? 0 : st;                       // (a cursor written by the host: never leave the ring)
    replay_add_cols_body(p, p.ring, 0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (p.size_dev) *p.size_dev = (int)min(max(ctl[RL_CTL_SIZE], 0ll), p.capacity);
        ctl[RL_CTL_ITER] += 1;
        ctl[RL_CTL_T] += p.n;
        if (!ctl[RL_CTL_WARM]) ctl[RL_CTL_CALLS] += p.n;
    }
}
// group form of the counter-reading kernel (rlrep_group_replay_add_cols_ctl; kparams.h "the loop record of a GROUP"): workgroup (x, slot)
// packs plane m of the five arrays (rows m * n ..) into member m's ring from ITS start row (row m of the record) and thread 0 of workgroup
// (0, slot) publishes ITS fill level; the one of slot 0 advances the group's ITER, T and CALLS once.  Unlike replay_add_cols_kernel_grp it
// honours the live table: the ring, the fill level and the cursor of a retired member stand still.
__global__ __launch_bounds__(256) void replay_add_cols_kernel_ctl_grp(ReplayCols p0, long long* __restrict__ ctl, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    ReplayCols p = p0;
    const long long* cm = ctl + (long long)m * RL_LOOP_CTL_WORDS;
    const long long st = cm[RL_CTL_START];
    p.start = (st < 0 || st >= p.capacity) ? 0 : st;                       // (a cursor written by the host: never leave the ring)
    replay_add_cols_body(p, p.ring + (long long)m * p.ring_stride, (long long)m * p.n);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (p.size_dev) p.size_dev[m] = (int)min(max(cm[RL_CTL_SIZE], 0ll), p.capacity);
        if (blockIdx.y == 0) {
            ctl[RL_CTL_ITER] += 1;
            ctl[RL_CTL_T] += p.n;
            if (!ctl[RL_CTL_WARM]) ctl[RL_CTL_CALLS] += p.n;
        }
    }
}
extern "C" int rl_launch_replay_add_cols_ctl(const ReplayCols* p, long long* ctl, hipStream_t st) {
    const long long total = p->n * p->row;
    const int blocks = (int)std::min<long long>(1024, std::max<long long>(1, (total + 255) / 256));
    hipLaunchKernelGGL(replay_add_cols_kernel_ctl, dim3(blocks), dim3(256), 0, st, *p, ctl);
    return (int)hipGetLastError();
}
// the group's (the caller holds the group active: grid y and the live table are its)
extern "C" int rl_launch_replay_add_cols_ctl_grp(const ReplayCols* p, long long* ctl, hipStream_t st) {
    const RlGrp* gr = rl_grp_active();
    if (!gr || !gr->live) return RL_GRP_UNSUPPORTED;
    const long long total = p->n * p->row;
    const int blocks = (int)std::min<long long>(1024, std::max<long long>(1, (total + 255) / 256));
    hipLaunchKernelGGL(replay_add_cols_kernel_ctl_grp, dim3(blocks, gr->grid_y), dim3(256), 0, st, *p, ctl, gr->live);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_replay_add_cols(const ReplayCols* p, int members, hipStream_t st) {
    const long long total = p->n * p->row;
    const int blocks = (int)std::min<long long>(1024, std::max<long long>(1, (total + 255) / 256));
    if (members > 0)
        hipLaunchKernelGGL(replay_add_cols_kernel_grp, dim3(blocks, members), dim3(256), 0, st, *p);
    else
        hipLaunchKernelGGL(replay_add_cols_kernel, dim3(blocks), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_replay_add_grp(float* ring, long long ring_stride, int members, long long capacity, int row, long long ptr, const float* rows,
                                        long long rows_stride, long long nrows, int* size_dev, int new_size, hipStream_t st) {
    const long long n = nrows * row;
    const int blocks = (int)std::min<long long>(256, std::max<long long>(1, (n + 255) / 256));
    hipLaunchKernelGGL(replay_add_kernel_grp, dim3(blocks, members), dim3(256), 0, st, ring, ring_stride, capacity, row, ptr, rows, rows_stride, nrows, size_dev, new_size);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_replay_add(float* ring, long long capacity, int row, long long ptr, const float* rows, long long nrows, int* size_dev, int new_size, hipStream_t st) {
    const long long n = nrows * row;
    const int blocks = (int)std::min<long long>(256, std::max<long long>(1, (n + 255) / 256));
    hipLaunchKernelGGL(replay_add_kernel, dim3(blocks), dim3(256), 0, st, ring, capacity, row, ptr, rows, nrows, size_dev, new_size);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_select_action(const SelectAct* p, hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)p->S + 2 * (size_t)p->Ha + 2 * (size_t)p->A);
    if (lds > 60 * 1024) return -7;
    if (const RlGrp* gr = rl_grp_active()) {
        if (!gr->seeds) return RL_GRP_UNSUPPORTED;
        hipLaunchKernelGGL(select_action_kernel_grp, dim3(1, gr->grid_y), dim3(1024), lds, st, *p, gr->stride, gr->seeds, gr->live);
    } else
        hipLaunchKernelGGL(select_action_kernel, dim3(1), dim3(1024), lds, st, *p);
    return (int)hipGetLastError();
}
// `rows` observations (per member while a group is active) in one launch: grid x = rows.  The LDS rule and the -7 refusal are the one-row launcher's.
extern "C" int rl_launch_select_action_n(const SelectAct* p, int rows, hipStream_t st) {
    const size_t lds = sizeof(float) * ((size_t)p->S + 2 * (size_t)p->Ha + 2 * (size_t)p->A);
    if (lds > 60 * 1024) return -7;
    if (const RlGrp* gr = rl_grp_active()) {
        if (!gr->seeds) return RL_GRP_UNSUPPORTED;
        hipLaunchKernelGGL(select_action_kernel_grp_n, dim3(rows, gr->grid_y), dim3(1024), lds, st, *p, gr->stride, gr->seeds, gr->live);
    } else
        hipLaunchKernelGGL(select_action_kernel_n, dim3(rows), dim3(1024), lds, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_policy_bwd(const PolicyBwd* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(policy_bwd_kernel, dim3((p->B + 255) / 256), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_heads_vae(const HeadsVae* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    const int tiles = ((p->B + 15) / 16) * p->tiles_c;
    hipLaunchKernelGGL(heads_vae_kernel, dim3(tiles), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_vae_mid(const VaeMid* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(vae_mid_kernel, dim3(p->nblk), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_vae_mse(const VaeMse* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(vae_mse_kernel, dim3(p->nblk), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_qhead_critic(const QHeadCritic* p, hipStream_t st) {
    if (const RlGrp* gr = rl_grp_active()) hipLaunchKernelGGL(qhead_critic_kernel_grp, dim3(p->nblk, gr->grid_y), dim3(256), 0, st, *p, gr->stride, gr->hyp, gr->live);
    else hipLaunchKernelGGL(qhead_critic_kernel, dim3(p->nblk), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_qhead_actor(const QHeadActor* p, hipStream_t st) {
    if (const RlGrp* gr = rl_grp_active()) hipLaunchKernelGGL(qhead_actor_kernel_grp, dim3(p->nblk, gr->grid_y), dim3(256), 0, st, *p, gr->stride, gr->live);
    else hipLaunchKernelGGL(qhead_actor_kernel, dim3(p->nblk), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_adam(const AdamTask* task, int adam_blocks, const FinTask* fin, int nfin, const SlotFill* sf, const SlotFill* sf2, const AdamSnap* snap, const DpPull* dp, hipStream_t st) {
    SlotFill none = SlotFill();
    AdamSnap nosnap = AdamSnap();
    DpPull dpv = DpPull();
    const RlGrp* gr = rl_grp_active();
    if (gr && ((dp && dp->world > 1) || (task && task->sh) || (snap && snap->on))) return RL_GRP_UNSUPPORTED;
    if (dp && dp->world > 1) {
        if (!task || adam_blocks <= 0 || task->nslab || task->nskip) return -9;     // (split-K folds and epilogue optimizers are single-rank forms: the gradient must be complete in the arena)
        dpv = *dp; dpv.nblocks = adam_blocks + 1;                                  // the optimizer blocks and the trailing block take a ticket
    }
    AdamTask t = AdamTask();
    if (task && adam_blocks > 0) t = *task; else adam_blocks = 0;
    if (t.n >= (1ll << 31) || adam_blocks >= (1 << 30)) return -5;
    const int fb = sf ? grid_for((long long)sf->B * (2 * sf->S + sf->A + 2), 256, 2048) : 0;
    const int fb2 = sf2 ? grid_for((long long)sf2->B * (2 * sf2->S + sf2->A + 2), 256, 2048) : 0;
    const int sb = (snap && snap->on && snap->segs.n > 0) ? grid_for(snap->segs.end[snap->segs.n - 1], 256, 256) : 0;
    const bool vec_ok = ((t.pol_off & 3) == 0) && ((t.pol_n & 3) == 0) &&
                        (((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v) | ((uintptr_t)t.target)) & 15) == 0);
    if (t.nslab > 0 && (!vec_ok || (t.n & 3))) return -6;          // (the builder folds split-K partials in only for groups on the 16-byte path)
    for (int q = 0; q < t.nslab; ++q) if (t.slabs[q].splits < 1 || t.slabs[q].splits > 16) return -6;
    const int hdr = adam_blocks | (vec_ok ? (1 << 30) : 0);
    const dim3 grid(adam_blocks + 1 + fb + fb2 + sb);
    if (dpv.world > 1) {
        // two-shot (dp_pull.h) where the attachment asked for it and the whole slice is on the 16-byte path: shard = ceil(n / 4 / world) elements,
        // summed by the first ceil(shard / 256) blocks of every rank's launch
        bool two = dpv.mode == 2 && vec_ok && (t.n & 3) == 0 && dpv.red[dpv.rank] != nullptr;
        if (two) {
            dpv.shard4 = ((t.n >> 2) + dpv.world - 1) / dpv.world;
            dpv.nblocks_a = (int)((dpv.shard4 + 255) / 256);
            if (dpv.nblocks_a < 1 || dpv.nblocks_a > adam_blocks) two = false;
        }
        if (two)
            hipLaunchKernelGGL(adam_dp_kernel<2>, grid, dim3(256), 0, st, t.p, t.g, t.m, t.v, t.grp, t.target, (int)t.n, hdr, t,
                               fin, nfin, sf ? *sf : none, fb, sf2 ? *sf2 : none, fb2, snap ? *snap : nosnap, sb, dpv);
        else {
            dpv.mode = 1;
            hipLaunchKernelGGL(adam_dp_kernel<1>, grid, dim3(256), 0, st, t.p, t.g, t.m, t.v, t.grp, t.target, (int)t.n, hdr, t,
                               fin, nfin, sf ? *sf : none, fb, sf2 ? *sf2 : none, fb2, snap ? *snap : nosnap, sb, dpv);
        }
    } else if (gr)
        hipLaunchKernelGGL(adam_kernel_grp, dim3(grid.x, gr->grid_y), dim3(256), 0, st, t.p, t.g, t.m, t.v, t.grp, t.target, (int)t.n, hdr, t,
                           fin, nfin, sf ? *sf : none, fb, sf2 ? *sf2 : none, fb2, snap ? *snap : nosnap, sb, gr->stride, gr->ring_stride, gr->hyp, gr->live);
    else
        hipLaunchKernelGGL(adam_kernel, grid, dim3(256), 0, st, t.p, t.g, t.m, t.v, t.grp, t.target, (int)t.n, hdr, t,
                           fin, nfin, sf ? *sf : none, fb, sf2 ? *sf2 : none, fb2, snap ? *snap : nosnap, sb);
    return (int)hipGetLastError();
}
// occupancy of the data-parallel optimizer kernels (blocks of 256 threads per CU): what rl_agent_attach_dp checks the co-residency bound against
extern "C" int rl_adam_dp_occupancy(int* one_shot, int* two_shot) {
    int a = 0, b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, adam_dp_kernel<1>, 256, 0) != hipSuccess) return -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, adam_dp_kernel<2>, 256, 0) != hipSuccess) return -1;
    if (one_shot) *one_shot = a;
    if (two_shot) *two_shot = b;
    return 0;
}
// optimizer launch of one group + the two first-layer tasks of the NEXT feature step as leading tiles (adam_l1_kernel); sf: the gather of that
// step's minibatch (must be armed: the tiles read the same ring rows through sf->idx)
extern "C" int rl_launch_adam_l1(const AdamTask* task, int adam_blocks, const FinTask* fin, int nfin, const SlotFill* sf, const GemmTask* g0, const GemmTask* g1, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    if (!task || adam_blocks <= 0 || !sf || !sf->ring || !sf->idx || !g0 || !g1) return -7;
    AdamTask t = *task;
    if (t.n >= (1ll << 31) || adam_blocks >= (1 << 30)) return -5;
    const int fb = grid_for((long long)sf->B * (2 * sf->S + sf->A + 2), 256, 2048);
    const bool vec_ok = ((t.pol_off & 3) == 0) && ((t.pol_n & 3) == 0) &&
                        (((((uintptr_t)t.p) | ((uintptr_t)t.g) | ((uintptr_t)t.m) | ((uintptr_t)t.v) | ((uintptr_t)t.target)) & 15) == 0);
    if (!vec_ok || (t.n & 3) || t.nslab) return -6;            // (skip ranges are honoured on the 16-byte path)
    GemmTask a = *g0, b = *g1;
    const int row_w = 2 * sf->S + sf->A + 2;
    for (GemmTask* q : {&a, &b}) {
        if (q->epi != EPI_FWD || q->act != ACT_RELU || q->K > row_w || q->R != sf->B) return -7;
        q->A = sf->ring; q->lda = row_w; q->gidx = sf->idx;
        q->tiles_c = (q->Cn + 15) / 16; q->ntiles = ((q->R + 15) / 16) * q->tiles_c;
        rl_gemm16_plan(*q);
    }
    a.tile_base = 0; b.tile_base = a.ntiles;
    const int gtiles = a.ntiles + b.ntiles;
    const int hdr = adam_blocks | (1 << 30);
    hipLaunchKernelGGL(adam_l1_kernel, dim3(gtiles + adam_blocks + 1 + fb), dim3(256), 0, st, t.p, t.g, t.m, t.v, t.grp, t.target, (int)t.n, hdr, gtiles, b.tile_base,
                       a.tiles_c, b.tiles_c, t, fin, nfin, *sf, fb, a, b);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_train_prologue(TrainPrologue* p, hipStream_t st) {
    p->nb_idx = grid_for((p->idx.n + 3) / 4, 256, 2048);
    p->nb_eps = grid_for((p->eps.n + 3) / 4, 256, 2048);
    p->nb_fill = grid_for((long long)p->fill.B * (2 * p->fill.S + p->fill.A + 2), 256, 2048);
    if (const RlGrp* gr = rl_grp_active()) {
        if (p->nsh || p->nb_tr || !gr->seeds) return RL_GRP_UNSUPPORTED;          // (shadow refresh: no sac form carries one)
        hipLaunchKernelGGL(train_prologue_kernel_grp, dim3(p->nb_idx + p->nb_eps + p->nb_fill, gr->grid_y), dim3(256), 0, st, *p, gr->stride, gr->ring_stride, gr->seeds, gr->live);
    } else
        hipLaunchKernelGGL(train_prologue_kernel, dim3(p->nb_idx + p->nb_eps + p->nb_fill + p->nb_tr), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_polyak(const PolyakTask* t, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(polyak_kernel, dim3(grid_for(t->n, 1024, 1024)), dim3(256), 0, st, *t);
    return (int)hipGetLastError();
}
// mirror > 0: c[mirror] follows c[0] (the train() counter's copy for the next train prologue)
extern "C" int rl_launch_counter_inc(int* c, int mirror, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(counter_inc_kernel, dim3(1), dim3(64), 0, st, c, mirror);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_counter_sync(int* c, int mirror, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(counter_sync_kernel, dim3(1), dim3(64), 0, st, c, mirror);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_copy_segs(const CopySegs* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    if (p->n <= 0) return 0;
    hipLaunchKernelGGL(copy_segs_kernel, dim3(grid_for(p->end[p->n - 1], 1024, 1024)), dim3(256), 0, st, *p);
    return (int)hipGetLastError();
}
extern "C" int rl_launch_copy(const float* src, float* dst, long long n, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    hipLaunchKernelGGL(copy_kernel, dim3(grid_for(n, 1024, 1024)), dim3(256), 0, st, src, dst, n);
    return (int)hipGetLastError();
}
