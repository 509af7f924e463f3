// gfx950 (CDNA4 / MI355X): the index-hopping matrix, a post-pass behind an exact-match launch (qd_hop_enable).
//
// Only when enabled, and only for a dual plan.  The pairs whose final routing code is 0xFFFF are listed (the rescue's list when a
// rescue ran, else the unknown tally's, else a compaction of its own: quade_mismatch.hip mm_compact), then one kernel runs on the
// launch's stream:
//   hop_count : one lane per listed pair.  Index read 1's slice and index read 2's slice are folded each into its own canonical
//               words starting at byte 0 (mm_load, qd_fold8; the parts are not merged) and looked up, exactly, in the sheet's
//               distinct index-1 values and distinct index-2 values: two read-only open-addressing tables in global memory (they
//               are a few hundred KiB at most and stay in L2; nothing is staged in LDS), a 64-bit tag per entry and a compare with
//               the part's full key words behind a tag hit, so that equal tags of different parts never give a false match.  The
//               pair's cell is a * (n2 + 1) + b, a = n1 / b = n2 for "no part".  Equal cells are combined first in the wave and
//               then in the workgroup's LDS hash of cell -> count (quade_tally.h: tally_combine, tally_lds_flush), so a hot cell
//               -- (n1, n2) takes all of PhiX -- costs one global atomic per workgroup and not one per pair.  A pair with a read
//               that ends inside its index window (uk_key's test: a zero byte inside the slice) adds 1 to `short`, summed over
//               the wave and added once per workgroup.
// The matrix is updated with atomics only and nothing else is written: launches on different streams need no order among
// themselves.  Plain C++ and vector memory operations throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "quade_hop.h"
#include "quade_kernels.h"
#include "quade_rowkey.h"
#include "quade_tally.h"

namespace {

// part k of pair r, case folded, from byte 0 of w; false: the read ends inside its index window (the row is zero padded there)
template <int KW>
__device__ __forceinline__ bool hop_key(const HopParams& p, int k, int64_t r, u64 (&w)[KW]) {
    const u64 L = 0x0101010101010101ull, H = 0x8080808080808080ull;
    const int iw = p.idx_w[k];
    mm_load<KW>(p.seq[k] + r * p.seq_stride[k] + p.idx_off[k], iw, w);
    bool full = true;
#pragma unroll
    for (int q = 0; q < KW; ++q) {
        const int left = iw - 8 * q;  // bytes of this word inside the slice; the others read as 0xFF
        const u64 keep = left >= 8 ? 0 : (left <= 0 ? ~0ull : ~0ull << (8 * left));
        const u64 x = w[q] | keep;
        full = full && (((x - L) & ~x & H) == 0);
        w[q] = qd_fold8(w[q]);
    }
    return full;
}

// the ordinal of the part whose key words equal w, or `none`
template <int KW>
__device__ __forceinline__ uint32_t hop_find(const HopPart& t, const u64 (&w)[KW], uint32_t none) {
    u64 k4[QD_KEY_WORDS] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < KW; ++q) k4[q] = w[q];
    const u64 tag = qd_hop_tag(k4);
    uint32_t s = qd_uk_home(tag, t.lg);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {  // (at most half of the entries are taken: an empty one ends the walk)
        const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(&t.slots[s]);  // tag, then ordinal
        if (e.x == 0) return none;
        if (e.x == tag) {
            const uint32_t ord = (uint32_t)e.y;
            const u64* kw = t.keys + (size_t)ord * QD_KEY_WORDS;
            bool same = true;
#pragma unroll
            for (int q = 0; q < KW; ++q) same = same && kw[q] == w[q];
            if (same) return ord;
        }
        s = (s + 1) & t.mask;
    }
    return none;
}

template <int KW>
__global__ __launch_bounds__(UK_BLOCK) void hop_count(const HopParams p) {
    __shared__ uint32_t lslot[UK_LDS];
    __shared__ uint32_t lcnt[UK_LDS];
    __shared__ uint32_t short_wg;
    tally_lds_init(lslot, lcnt);
    if (threadIdx.x == 0) short_wg = 0;
    __syncthreads();
    const uint32_t nm = p.miss[0];
    const int lane = threadIdx.x & 63;
    uint32_t n_short = 0;
    // the trip count is the same for every lane of the workgroup: the wave-level combining below needs whole waves
    for (u64 base = (u64)blockIdx.x * UK_BLOCK; base < nm; base += (u64)gridDim.x * UK_BLOCK) {
        const u64 i = base + threadIdx.x;
        bool pend = false;
        uint32_t cell = 0;
        if (i < nm) {
            const int64_t r = p.miss[4 + (size_t)i];
            if (r < p.n && p.codes[r] == QD_CODE_UNDET) {  // (a stale entry: rescued since it was listed)
                u64 w1[KW], w2[KW];
                const bool f1 = hop_key<KW>(p, 0, r, w1);
                const bool f2 = hop_key<KW>(p, 1, r, w2);
                if (f1 && f2) {
                    const uint32_t a = hop_find<KW>(p.part[0], w1, p.n1);
                    const uint32_t b = hop_find<KW>(p.part[1], w2, p.n2);
                    cell = a * (p.n2 + 1) + b;
                    pend = true;
                } else {
                    ++n_short;
                }
            }
        }
        tally_combine(lslot, lcnt, p.table, pend, cell, lane);
    }
    n_short = uk_wave_sum(n_short);
    if (lane == 0 && n_short) atomicAdd(&short_wg, n_short);
    __syncthreads();
    tally_lds_flush(lslot, lcnt, p.table);
    if (threadIdx.x == 0 && short_wg)
        atomicAdd(reinterpret_cast<unsigned long long*>(&p.table[(size_t)(p.n1 + 1) * (p.n2 + 1)]), (unsigned long long)short_wg);
}

}  // namespace

hipError_t qd_launch_hop(const HopParams& p, int cus, hipStream_t st) {
    if (p.n <= 0) return hipSuccess;
    const int64_t nb = (p.n + UK_BLOCK - 1) / UK_BLOCK;
    const unsigned grid = (unsigned)std::min<int64_t>(nb, (int64_t)cus * 8);
    // a part is at most K - 1 bytes: two words up to K = 16 (as quade_unknown.hip), four beyond
    if (p.K <= 16) hipLaunchKernelGGL(hop_count<2>, dim3(grid), dim3(UK_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(hop_count<4>, dim3(grid), dim3(UK_BLOCK), 0, st, p);
    return hipGetLastError();
}
