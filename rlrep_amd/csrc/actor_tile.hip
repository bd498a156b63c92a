// SACAgent.act_device: the three actor layers and the tanh-Gaussian head for N device-resident observation rows in ONE launch.  A 256-thread
// workgroup takes 16 rows through actor.trunk.{0,2,4}: the 16-row activation tiles stay in LDS between the layers, the weights stream from
// global memory / L2 as the B operand of v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate), and every weight a workgroup fetches serves 16 rows
// (select_action_kernel_n fetches all of them for one).
//
// Operand maps (gemm16_tile.h): A: lane l holds X[i = l & 15][k = l >> 4]; B: lane l holds W[j = l & 15][k = l >> 4]; D: col = l & 15,
// row = 4 (l >> 4) + reg.  As there, a lane takes FOUR CONSECUTIVE inner indices kk = k0 + 4 (l >> 4) .. + 3 of a 16-wide inner block and feeds
// them to four successive MFMAs (A and B agree on the permutation): one ds_read_b128 and one 16-byte global load per operand and block.
//
// Row independence: output element (row, col) is ONE accumulator chain -- inner blocks of 16 ascending, four MFMAs each, every MFMA adding the
// four products k = k0 + s + {0, 4, 8, 12} -- and the chain is the same for every row position i, every tile and every grid size; the inner
// dimension is never split over waves (the four waves split a layer's 16-wide output column tiles).  A row's action therefore depends on its
// observation, the weights and its draw alone.
//
// LDS row pitch LD (floats): ds_read_b128 serves a wave in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32,
// and a 256-byte bank row holds sixteen 16-byte slots.  Lane (i, kq) reads slot (i * LD / 4 + kq) mod 16.  A group holds eight rows i with kq
// and the other eight with kq + 1 -- {0-3, 12-15} and {4-11} -- so an odd LD / 4 (the usual "+ 4 floats" pad) cannot work: i * LD / 4 would
// permute the 16 slots and the shifted half would have to avoid the unshifted one.  With LD / 4 = 2 (mod 16) both halves map onto the EVEN slots
// ({0-3, 12-15} -> 0 2 4 6 8 10 12 14, {4-11} -> 8 10 12 14 0 2 4 6), and the half that carries kq + 1 lands on the odd ones: 16 lanes, 16 slots,
// no conflict in any group.  So LD is the smallest value = 8 (mod 64) that holds max(S, Ha) rounded up to 16 (264 floats at Ha = 256).  The
// epilogue's ds_write_b32 (rows 4 kq + reg, 32 banks) is two-way on that pitch: 4 stores per 16 MFMAs, left alone.
#include <algorithm>
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "group.h"
#include "group_env.h"
#include "launchers.h"

// one layer for the 16 rows in `in` (LDS, pitch LD, zero-filled to a multiple of 16 columns): out[i][c] = act(sum_k in[i][k] W[c][k] + bias[c]).
// Wave w takes column tiles w, w + 4, ... NF at a time, sharing the A fragments; NU = 4 inner blocks (64 indices) have all their loads issued
// before an MFMA consumes one.  (NU = 8 at NF = 4 and NU = 16 at NF = 1 -- two and one exposed round trips per 256-wide layer instead of four --
// were measured SLOWER, 37.7 against 35.5 us at N = 256 and 251 against 202 us at N = 65 536: 256 + 24 registers leave one workgroup per CU.
// docs/history/act_device.md.)  Loads are branch-free: addresses clamped into the matrix,
// the B fragment zeroed behind K with a select.
// PAD: columns N .. next multiple of 16 of `out` are written as zeros (the next layer's inner padding).
template <int NF, int NU, bool VEC>
__device__ __forceinline__ void at_layer_t(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int LD, int K, int N,
                                           float* out, int ldo, bool elu, bool pad, int lane, int w) {
    const int i = lane & 15, kq = lane >> 4;
    const int ntiles = (N + 15) >> 4, K16 = (K + 15) & ~15;
    for (int tg = w; tg < ntiles; tg += 4 * NF) {
        f32x4 acc[NF];
        const float* wrow[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            wrow[f] = W + (size_t)min(16 * (tg + 4 * f) + i, N - 1) * K;
        }
        for (int k0 = 0; k0 < K16; k0 += 16 * NU) {
            f32x4 a[NU];
            float b[NU][NF][4];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int kk = k0 + 16 * u + 4 * kq;
                a[u] = *reinterpret_cast<const f32x4*>(in + i * LD + min(kk, K16 - 4));
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    if (VEC) {                       // K % 4 == 0 and 16-byte aligned rows: the four indices are valid together
                        const f32x4 x = *reinterpret_cast<const f32x4*>(wrow[f] + min(kk, K - 4));
                        b[u][f][0] = x[0]; b[u][f][1] = x[1]; b[u][f][2] = x[2]; b[u][f][3] = x[3];
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) b[u][f][s] = wrow[f][min(kk + s, K - 1)];
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int kk = k0 + 16 * u + 4 * kq;
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int s = 0; s < 4; ++s) b[u][f][s] = kk + s < K ? b[u][f][s] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < NU; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int f = 0; f < NF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], b[u][f][s], acc[f], 0, 0, 0);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int t = tg + 4 * f, c = 16 * t + i;
            const float bv = bias[min(c, N - 1)];
            if (t < ntiles && (c < N || pad)) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[f][r] + bv;
                    out[(4 * kq + r) * ldo + c] = c < N ? (elu ? elu_f(v) : v) : 0.f;
                }
            }
        }
    }
}
__device__ __forceinline__ void at_layer(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int LD, int K, int N,
                                         float* out, int ldo, bool elu, bool pad, int lane, int w) {
    const bool vec = (K & 3) == 0 && ((uintptr_t)W & 15) == 0;        // wave-uniform
    if (N > 64) {
        if (vec) at_layer_t<4, 4, true>(W, bias, in, LD, K, N, out, ldo, elu, pad, lane, w);
        else at_layer_t<4, 4, false>(W, bias, in, LD, K, N, out, ldo, elu, pad, lane, w);
    } else {
        if (vec) at_layer_t<1, 4, true>(W, bias, in, LD, K, N, out, ldo, elu, pad, lane, w);
        else at_layer_t<1, 4, false>(W, bias, in, LD, K, N, out, ldo, elu, pad, lane, w);
    }
}

__global__ __launch_bounds__(256) void actor_tile_kernel(ActTile p) {
    const int r0 = blockIdx.x * 16;
#include "actor_tile_body.h"
}
// group form: workgroup (x, slot) is row tile x of member m -- the member's actor and seed, its plane of `rows` observation / action rows
__global__ __launch_bounds__(256) void actor_tile_kernel_grp(ActTile p0, long long mstride, const unsigned long long* __restrict__ seeds, const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    const long long dm = (long long)m * mstride;
    ActTile p = p0;
    p.obs += (long long)m * p.rows * p.ld_obs; p.act += (long long)m * p.rows * p.ld_act;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
    const int r0 = blockIdx.x * 16;
#include "actor_tile_body.h"
}

// lo + (hi - lo) * u of the exploration mix, one rounding per operation (tests/sim_loop_reference.py restates it in NumPy): hipcc contracts
// a * b + c, and __fmul_rn / __fadd_rn do not stop it (docs/history/nstep.md), so each helper switches contraction off for its own operation
__device__ __forceinline__ float mix_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float mix_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float mix_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
// counter-reading form (rlrep_act_device_ctl, capturable: nothing that changes between two replays rides by value): the call counter, the step
// counter and the iteration come from the loop record (kparams.h RL_CTL_*).  The tile and the head are actor_tile_body.h as actor_tile_kernel
// compiles it, at explore = 1 and offset (calls + 1) << 20 -- the bytes of rlrep_act_device(explore = 1) at that counter.  Behind it the
// exploration mix of env_step_body.h for A components: row e takes clamp(lo + (hi - lo) u_j) in every component j during warm-up
// (T < start_timesteps) or if its pick word is below eps_greedy; the thread that stored element (row, j) in the body is the one that
// overwrites it.  Philox blocks (key = the agent's seed): counter {iter lo, iter hi, e, RL_STREAM_SIM + q}.  Every workgroup reads CALLS, T
// and ITER; ONE thread moves the cursor words, which this launch never reads.
__global__ __launch_bounds__(256) void actor_tile_kernel_ctl(ActTile p0, ActCtl k) {
    const unsigned long long calls = (unsigned long long)k.ctl[RL_CTL_CALLS];
    const long long tg = k.ctl[RL_CTL_T];
    const unsigned long long it = (unsigned long long)k.ctl[RL_CTL_ITER];
    ActTile p = p0;
    p.explore = 1; p.offset = (calls + 1ull) << 20;
    const int r0 = blockIdx.x * 16;
    {
#include "actor_tile_body.h"
    }
#include "actor_tile_mix.h"
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        long long ptr = k.ctl[RL_CTL_NEXT];
        if (ptr < 0 || ptr >= k.capacity) ptr = 0;                      // (a cursor written by the host: never leave the ring)
        const long long nxt = ptr + p.rows;                             // (the launcher holds rows <= capacity)
        k.ctl[RL_CTL_START] = ptr;
        k.ctl[RL_CTL_NEXT] = nxt < k.capacity ? nxt : nxt - k.capacity;
        k.ctl[RL_CTL_SIZE] = min(max(k.ctl[RL_CTL_SIZE], 0ll) + p.rows, k.capacity);
        k.ctl[RL_CTL_WARM] = warm ? 1 : 0;
    }
}
// group form of the counter-reading kernel (rlrep_group_act_device_ctl; kparams.h "the loop record of a GROUP"): actor_tile_kernel_grp's
// rebasing -- the member's actor, its plane of `rows` observation / action rows, its seed as the key of the head's draw and of the mix --
// around actor_tile_kernel_ctl's body.  CALLS, T and ITER are the group's (row 0 of the record); thread 0 of workgroup (0, slot) moves member
// m's own cursor words (row m), with the single form's clamps, and the one of slot 0 -- the first live member, there whenever anything runs --
// writes the group's WARM.  No workgroup of this launch reads any of the words written.
__global__ __launch_bounds__(256) void actor_tile_kernel_ctl_grp(ActTile p0, ActCtl k, long long mstride, const unsigned long long* __restrict__ seeds,
                                                                 const int* __restrict__ live) {
    RL_GRP_MEMBER(m, live);
    const unsigned long long calls = (unsigned long long)k.ctl[RL_CTL_CALLS];
    const long long tg = k.ctl[RL_CTL_T];
    const unsigned long long it = (unsigned long long)k.ctl[RL_CTL_ITER];
    const long long dm = (long long)m * mstride;
    ActTile p = p0;
    p.obs += (long long)m * p.rows * p.ld_obs; p.act += (long long)m * p.rows * p.ld_act;
    rl_rb(p.W1, dm); rl_rb(p.b1, dm); rl_rb(p.W2, dm); rl_rb(p.b2, dm); rl_rb(p.W3, dm); rl_rb(p.b3, dm);
    p.seed = seeds[m];
    p.explore = 1; p.offset = (calls + 1ull) << 20;
    const int r0 = blockIdx.x * 16;
    {
#include "actor_tile_body.h"
    }
#include "actor_tile_mix.h"
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        long long* cm = k.ctl + (long long)m * RL_LOOP_CTL_WORDS;
        long long ptr = cm[RL_CTL_NEXT];
        if (ptr < 0 || ptr >= k.capacity) ptr = 0;                      // (a cursor written by the host: never leave the ring)
        const long long nxt = ptr + p.rows;                             // (the launcher holds rows <= capacity)
        cm[RL_CTL_START] = ptr;
        cm[RL_CTL_NEXT] = nxt < k.capacity ? nxt : nxt - k.capacity;
        cm[RL_CTL_SIZE] = min(max(cm[RL_CTL_SIZE], 0ll) + p.rows, k.capacity);
        if (blockIdx.y == 0) k.ctl[RL_CTL_WARM] = warm ? 1 : 0;
    }
}

// LDS row pitch of the activation tiles (see the head of this file)
static int at_pitch(int S, int Ha) {
    const int d16 = (std::max(S, Ha) + 15) & ~15;
    return ((d16 - 8 + 63) / 64) * 64 + 8;
}
extern "C" long long rl_actor_tile_lds_bytes(int S, int Ha, int A) {
    return (long long)sizeof(float) * (2LL * 16 * at_pitch(S, Ha) + 16LL * 2 * A);
}
// -7: the shape needs more LDS than a workgroup may have (RL_ACT_TILE_LDS_MAX); the callers refuse it by name before they come here
extern "C" int rl_launch_actor_tile(const ActTile* p0, hipStream_t st) {
    const long long lds = rl_actor_tile_lds_bytes(p0->S, p0->Ha, p0->A);
    if (lds > RL_ACT_TILE_LDS_MAX) return -7;
    ActTile p = *p0;
    p.LD = at_pitch(p.S, p.Ha);
    const RlGrp* gr = rl_grp_active();
    if (gr && !gr->seeds) return RL_GRP_UNSUPPORTED;
    if (lds > 48 * 1024) {                             // above the default dynamic limit (host-side call, no device work)
        const hipError_t e = gr ? hipFuncSetAttribute(reinterpret_cast<const void*>(actor_tile_kernel_grp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
                                : hipFuncSetAttribute(reinterpret_cast<const void*>(actor_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const unsigned gx = (unsigned)((p.rows + 15) / 16);
    if (gr)
        hipLaunchKernelGGL(actor_tile_kernel_grp, dim3(gx, gr->grid_y), dim3(256), (size_t)lds, st, p, gr->stride, gr->seeds, gr->live);
    else
        hipLaunchKernelGGL(actor_tile_kernel, dim3(gx), dim3(256), (size_t)lds, st, p);
    return (int)hipGetLastError();
}
// the counter-reading form: one agent (the callers refuse a group's handle), same grid, same LDS
extern "C" int rl_launch_actor_tile_ctl(const ActTile* p0, const ActCtl* k, hipStream_t st) {
    const long long lds = rl_actor_tile_lds_bytes(p0->S, p0->Ha, p0->A);
    if (lds > RL_ACT_TILE_LDS_MAX) return -7;
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    ActTile p = *p0;
    p.LD = at_pitch(p.S, p.Ha);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(actor_tile_kernel_ctl), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(actor_tile_kernel_ctl, dim3((unsigned)((p.rows + 15) / 16)), dim3(256), (size_t)lds, st, p, *k);
    return (int)hipGetLastError();
}
// the counter-reading form of a group (the callers refuse everything but a group's handle): grid (ceil(rows / 16), grid_y), same LDS
extern "C" int rl_launch_actor_tile_ctl_grp(const ActTile* p0, const ActCtl* k, hipStream_t st) {
    const long long lds = rl_actor_tile_lds_bytes(p0->S, p0->Ha, p0->A);
    if (lds > RL_ACT_TILE_LDS_MAX) return -7;
    const RlGrp* gr = rl_grp_active();
    if (!gr || !gr->seeds || !gr->live) return RL_GRP_UNSUPPORTED;
    ActTile p = *p0;
    p.LD = at_pitch(p.S, p.Ha);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(actor_tile_kernel_ctl_grp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(actor_tile_kernel_ctl_grp, dim3((unsigned)((p.rows + 15) / 16), gr->grid_y), dim3(256), (size_t)lds, st, p, *k, gr->stride, gr->seeds, gr->live);
    return (int)hipGetLastError();
}
