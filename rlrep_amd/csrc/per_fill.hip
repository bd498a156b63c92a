// Prioritized replay of the critic's minibatch for vlsac / ctrlsac / spedersac / diffsrsac: the stratified sampler of per.hip
// and the slot gather of elementwise.hip as ONE launch.  The two bodies are restated here, not shared through a header: per_sample_kernel
// and fill_slot_kernel keep the code objects every other train() runs.
//
// Workgroup 0 is the sampler: per_sample_kernel's body, operation for operation -- all B draws, the batch minimum, idx[B] and w[B].
// Workgroups 1 .. G gather: workgroup g owns the `rows` consecutive samples from (g - 1) rows on (rows <= PSF_ROWS), repeats THEIR descents
// (one per thread, a single pass), keeps their indices in LDS and copies their ring rows into the slot arrays as fill_slot_body lays them
// out.  A draw is a function of (j, the tree, the Philox word) alone and the tree is read-only inside the launch, so the gatherers reach the indices
// workgroup 0 writes without any hand-off between workgroups -- the per-XCD L2s are not coherent inside a launch, a hand-off would need a
// release / acquire pair per workgroup.  A gatherer needs neither the weights nor the batch minimum, so only workgroup 0 runs all B descents:
// every draw is descended twice in the launch, whatever the grid.  LDS holds PSF_ROWS indices, whatever B is.
#include "common.h"
#include "kparams.h"
#include "philox.h"
#include "launchers.h"

#define PSF_THREADS 256
#define PSF_ROWS 256            // most samples per gathering workgroup: one descent per thread
#define PSF_ELEMS 4             // elements a thread of a gathering workgroup copies, about (the launcher's choice of `rows`)

// draw j of the stratified sampler (per_sample_kernel's loop body): the leaf it lands on and that leaf's value
__device__ __forceinline__ int psf_descend(const PerSample& p, int j, unsigned long long off, float total, float seg, float& val) {
    const long long q = j >> 2;
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const uint32_t word = (j & 3) == 0 ? c[0] : (j & 3) == 1 ? c[1] : (j & 3) == 2 ? c[2] : c[3];
    const float u = __fmul_rn(__fadd_rn((float)(word >> 8), 0.5f), 1.0f / 16777216.0f);
    float m = __fmul_rn(__fadd_rn((float)j, u), seg);
    // one aligned 8-byte load per level (both children); never into a zero-mass subtree: left needs m < l (so l > 0) or r == 0
    long long n = 1; val = total;
    while (n < p.P) {
        const float2 lr = *reinterpret_cast<const float2*>(p.tree + 2 * n);
        if (lr.y == 0.f || m < lr.x) { n = 2 * n; val = lr.x; }
        else { m = __fsub_rn(m, lr.x); n = 2 * n + 1; val = lr.y; }
    }
    return (int)(n - p.P);
}

__device__ __forceinline__ float psf_block_min(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}

__global__ __launch_bounds__(PSF_THREADS) void per_sample_fill_kernel(PerSampleFill pf) {
    const PerSample& p = pf.s;
    __shared__ float sh[4];
    __shared__ int rows[PSF_ROWS];
    // (the device step counter, read as per_sample_kernel reads it)
    const unsigned long long off = p.offset + (p.step_dev ? (unsigned long long)(unsigned)*p.step_dev : 0ull);
    const float total = p.tree[1], seg = __fdiv_rn(total, (float)p.B);
    if (blockIdx.x == 0) {
        // ---- the sampler: idx[B] and w[B] ----
        const float beta = p.scal[2];
        float pmin = __builtin_inff();
        if (!p.given) {
            for (int j = threadIdx.x; j < p.B; j += PSF_THREADS) {
                float val;
                p.idx[j] = psf_descend(p, j, off, total, seg, val);
                p.w[j] = val;                      // (the leaf, until the batch minimum is known)
                pmin = fminf(pmin, val);
            }
        } else {
            for (int j = threadIdx.x; j < p.B; j += PSF_THREADS) {
                const long long ix = p.idx[j];
                const float val = (ix >= 0 && ix < p.P) ? p.tree[p.P + ix] : 0.f;       // (the caller checks given indices; never read outside the tree)
                p.w[j] = val;
                pmin = fminf(pmin, val);
            }
        }
        pmin = psf_block_min(pmin, sh);
        for (int j = threadIdx.x; j < p.B; j += PSF_THREADS) {       // (each thread reads back what it wrote itself)
            const float pj = p.w[j];
            p.w[j] = (pj == pmin || beta == 0.f) ? 1.0f : powf(__fdiv_rn(pmin, pj), beta);
        }
        return;
    }
    // ---- a gatherer: samples [lo, lo + n) ----
    const SlotFill& f = pf.f;
    const int lo = (blockIdx.x - 1) * pf.rows, n = p.B - lo < pf.rows ? p.B - lo : pf.rows;
    if ((int)threadIdx.x < n) {
        float val;
        long long ix = p.given ? (long long)p.idx[lo + threadIdx.x] : (long long)psf_descend(p, lo + threadIdx.x, off, total, seg, val);
        // a drawn leaf carries mass, so its row is one the ring holds; a given index is the caller's to check.  Whatever it is, nothing is
        // read outside the ring
        ix = ix < 0 ? 0 : ix >= pf.capacity ? pf.capacity - 1 : ix;
        rows[threadIdx.x] = (int)ix;
    }
    __syncthreads();
    const int row_w = 2 * f.S + f.A + 2, SA = f.S + f.A;
    const int count = n * row_w;                    // (about PSF_ELEMS * 256 elements, or one row)
    // PSF_ELEMS loads at a time into registers, then their stores: written as one loop, every load waits for the stores in front of it (the
    // slot arrays might alias the ring, for all the compiler knows), and a thread's elements cost a memory latency EACH
    for (int base = 0; base < count; base += PSF_ELEMS * PSF_THREADS) {
        float v[PSF_ELEMS]; int kk[PSF_ELEMS], cc[PSF_ELEMS];
#pragma unroll
        for (int u = 0; u < PSF_ELEMS; ++u) {
            const int e = base + u * PSF_THREADS + threadIdx.x;
            kk[u] = e / row_w; cc[u] = e - kk[u] * row_w;
            v[u] = e < count ? f.ring[(size_t)rows[kk[u]] * row_w + cc[u]] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PSF_ELEMS; ++u) {
            if (base + u * PSF_THREADS + (int)threadIdx.x >= count) continue;
            const int c = cc[u], b = lo + kk[u];
            if (c < f.S) {
                f.XE[(size_t)b * (SA + f.S) + c] = v[u];
                f.XF[(size_t)b * SA + c] = v[u];
                f.XFpi[(size_t)b * SA + c] = v[u];
            } else if (c < SA) {
                f.XE[(size_t)b * (SA + f.S) + c] = v[u];
                f.XF[(size_t)b * SA + c] = v[u];
            } else if (c < SA + f.S) {
                f.XE[(size_t)b * (SA + f.S) + c] = v[u];
                f.XF2[(size_t)b * SA + (c - SA)] = v[u];
            } else if (c == SA + f.S) {
                f.R[b] = v[u];
            } else {
                f.D[b] = v[u];
            }
        }
    }
}

// Grid: rl_launch_fill_slot gives every element of the B rows a thread of its own (up to 2048 workgroups).  Here a gathering workgroup first
// pays a descent of log2 P dependent loads (20 for 10^6 rows) in as many lanes as it owns samples, so it takes WHOLE rows -- a row cut in two
// would be descended once more -- and enough of them that a thread then copies about PSF_ELEMS = 4 elements, loaded together: the copy adds
// about one more memory latency to the ~20 of the descent, while the number of descents in the launch stays 2 B whatever the grid.
// rows = clamp(4 * 256 / row width, 1, 256): 24 rows at (S, A) = (17, 6) -- 1 + 11 workgroups at B = 256 -- and 1 row at (376, 17),
// 1 + 256 workgroups.  Measured (profiles/per_critic.txt, its last section): with 8 elements a thread, copied one after the other, the
// launch lost to per_sample + fill_slot at (17, 6) B = 256 (9.5 against 7.5 us); this form wins in all eight cases measured.
extern "C" int rl_launch_per_sample_fill(PerSampleFill* p, hipStream_t st) {
    if (rl_grp_active()) return RL_GRP_UNSUPPORTED;
    const int row_w = 2 * p->f.S + p->f.A + 2;
    int rows = PSF_ELEMS * PSF_THREADS / row_w;
    rows = rows < 1 ? 1 : rows > PSF_ROWS ? PSF_ROWS : rows;
    p->rows = rows;
    hipLaunchKernelGGL(per_sample_fill_kernel, dim3(1 + (p->s.B + rows - 1) / rows), dim3(PSF_THREADS), 0, st, *p);
    return (int)hipGetLastError();
}
