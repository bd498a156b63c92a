// Population-based training on a seed group (include/rlrep.h rlrep_group_clone_members): member dst becomes a copy of member src, in ONE
// launch for every pair.  Members lie at a constant byte stride in one allocation (group.h), so a clone is a strided device copy of the
// words a standalone agent's load(snapshot) restores: the parameter, target, exp_avg and exp_avg_sq arenas, the fp64 alpha_state and the
// batch-independent device records (train() counter block, the four optimizer records, the metric slots) -- but for words 1..5 of every
// optimizer record (lr, beta1, beta2, eps, tau), which stay the destination's (rlrep_group_set_member_hyper owns them).  DESIGN.md 6b lists
// every word that survives from one train() to the next and on which side of the copy it falls.
//
// Shape: grid (x, npairs), pair = blockIdx.y, 256 threads.  The segment table and the pair table ride BY VALUE in the kernel arguments and are
// read in place with wave-uniform indices (scalar loads; no local copy, no scratch).  A segment's 16-byte-aligned body moves as 16-byte vectors,
// four independent loads in flight per lane before their stores (a pure copy: HBM-bound for a ctrlsac F = 2048 member, launch-bound for a sac
// one); what lies in front of and behind the body moves as 32-bit words.  Source and destination differ by a multiple of the member stride
// (a multiple of 256 bytes), so both sides of every access share their alignment.
// The launcher (engine.hip) excludes what would make pairs depend on each other -- a member that is both a source and a destination, a
// destination named twice, src == dst -- and checks every segment against the member block before it launches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "group.h"
#include "launchers.h"

__global__ __launch_bounds__(256) void group_clone_kernel(CloneTab tab, ClonePairs pairs) {
    const int pair = blockIdx.y;
    const long long delta_s = (long long)pairs.src[pair] * tab.stride, delta_d = (long long)pairs.dst[pair] * tab.stride;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nthr = (long long)gridDim.x * 256;
    for (int s = 0; s < tab.nseg; ++s) {
        const long long off = tab.seg[s].off, bytes = tab.seg[s].bytes;          // (multiples of 4: the launcher checked)
        const char* src = tab.base + delta_s + off;
        char* dst = tab.base + delta_d + off;
        if (s == tab.rec_seg) {
            // the device records, word by word: words 1..5 of each optimizer record are the destination's own and stay
            const int nw = (int)(bytes >> 2);
            for (int w = (int)tid; w < nw; w += (int)nthr) {
                const int q = w - tab.rec_w0;
                const bool keep = q >= 0 && q < tab.rec_nw && (q % tab.rec_words) >= 1 && (q % tab.rec_words) <= 5;
                if (!keep) ((unsigned*)dst)[w] = ((const unsigned*)src)[w];
            }
            continue;
        }
        const long long head = std::min<long long>(bytes, (16 - ((uintptr_t)src & 15)) & 15);      // bytes in front of the aligned body
        const long long nvec = (bytes - head) >> 4, tail0 = head + (nvec << 4);
        const uint4* sv = (const uint4*)(src + head);
        uint4* dv = (uint4*)(dst + head);
        long long i = tid;
        for (; i + 3 * nthr < nvec; i += 4 * nthr) {
            const uint4 a = sv[i], b = sv[i + nthr], c = sv[i + 2 * nthr], d = sv[i + 3 * nthr];
            dv[i] = a; dv[i + nthr] = b; dv[i + 2 * nthr] = c; dv[i + 3 * nthr] = d;
        }
        for (; i < nvec; i += nthr) dv[i] = sv[i];
        const long long nedge = (head + (bytes - tail0)) >> 2, nhead = head >> 2;       // words outside the body
        for (long long w = tid; w < nedge; w += nthr) {
            const long long o = w < nhead ? (w << 2) : tail0 + ((w - nhead) << 2);
            *(unsigned*)(dst + o) = *(const unsigned*)(src + o);
        }
    }
}

// rlrep_group_set_live: the group's live table (group.h LiveTab) rewritten from the kernel arguments, one word per lane -- stream-ordered like
// any launch, so a captured train() graph obeys it from its next replay and the host keeps no staging buffer alive.
__global__ __launch_bounds__(128) void group_live_kernel(int* __restrict__ table, LiveTab tab, int members) {
    const int w = threadIdx.x;
    if (w == 0) table[0] = tab.n_live;
    else if (w <= members) table[w] = tab.slot_member[w - 1];
}
extern "C" int rl_launch_group_live(int* table_dev, const LiveTab* tab, int members, hipStream_t st) {
    if (members < 1 || members > RLREP_GROUP_MAX_MEMBERS) return -7;
    hipLaunchKernelGGL(group_live_kernel, dim3(1), dim3(128), 0, st, table_dev, *tab, members);
    return (int)hipGetLastError();
}

extern "C" int rl_launch_group_clone(const CloneTab* tab, const ClonePairs* pairs, int npairs, hipStream_t st) {
    long long longest = 0;
    for (int s = 0; s < tab->nseg; ++s) longest = std::max(longest, tab->seg[s].bytes);
    // one 16-byte vector per lane and unrolled pass where the segment is large enough, and no more workgroups than keep the chip's 256 CUs
    // eight deep over all pairs
    const long long want = (longest / 16 + 4 * 256 - 1) / (4 * 256);
    const int blocks = (int)std::min<long long>(std::max<long long>(1, 2048 / npairs), std::max<long long>(1, want));
    hipLaunchKernelGGL(group_clone_kernel, dim3(blocks, npairs), dim3(256), 0, st, *tab, *pairs);
    return (int)hipGetLastError();
}
