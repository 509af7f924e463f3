// gfx950 (CDNA4 / MI355X): tally of the unknown barcodes, the second post-pass behind an exact-match launch (qd_unknown_enable).
//
// Only when enabled.  The pairs whose final routing code is 0xFFFF are listed (the rescue's list when a rescue ran, else the same
// compaction, quade_mismatch.hip mm_compact), then two kernels run on the launch's stream:
//   uk_claim : one lane per listed pair.  It rebuilds the pair's canonical key (as mm_rescue does: both index reads' slices,
//              case folded, fused), takes a non-zero 64-bit tag of it and walks a bounded linear probe sequence over the tag
//              words of the table with a 64-bit compare-and-swap (0 = empty).  The lane whose swap installed the tag writes the
//              key words with plain vector stores.  Every lane leaves the slot it found -- or "none", "short", "skip" -- in the
//              stream's scratch list.
//   uk_count : a launch of its own, so that uk_claim's key stores are visible to every XCD at the kernel boundary: no flag, no
//              spinning lane.  Each lane compares its key with the entry's key words; equal: the entry's count goes up, unequal
//              (two keys of one tag) or no slot: `dropped` goes up.  Equal slots are combined first in the wave (two rounds of
//              leader election: a hot key is most of a wave) and then in an LDS hash of slot -> count that lives as long as the
//              workgroup, so a hot key costs one global atomic per workgroup and not one per pair; the four totals are summed
//              per workgroup as well.
// Launches on different streams are ordered by the caller (an event behind uk_count that the next launch's stream waits for
// before its uk_claim): otherwise a uk_count could compare against an entry whose tag another batch's uk_claim has installed
// but whose key words are not written yet.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "quade_kernels.h"
#include "quade_rowkey.h"
#include "quade_tally.h"
#include "quade_unknown.h"

namespace {

// (the block size, the claim, the wave and LDS combining: quade_tally.h, shared with quade_dup.hip)
constexpr int UK_GATHER_ITERS = 8;

// canonical key of pair r; false: a read ends inside its index window (the row is zero padded there)
template <int KW>
__device__ __forceinline__ bool uk_key(const UnknownParams& p, int64_t r, u64 (&w)[KW]) {
    const u64 L = 0x0101010101010101ull, H = 0x8080808080808080ull;
#pragma unroll
    for (int q = 0; q < KW; ++q) w[q] = 0;
    bool full = true;
    int at = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (k >= p.n_streams) break;
        const int iw = p.idx_w[k];
        u64 v[KW];
        mm_load<KW>(p.seq[k] + r * p.seq_stride[k] + p.idx_off[k], iw, v);
#pragma unroll
        for (int q = 0; q < KW; ++q) {
            const int left = iw - 8 * q;  // bytes of this word inside the slice; the others read as 0xFF
            const u64 keep = left >= 8 ? 0 : (left <= 0 ? ~0ull : ~0ull << (8 * left));
            const u64 x = v[q] | keep;
            full = full && (((x - L) & ~x & H) == 0);
            v[q] = qd_fold8(v[q]);
        }
        mm_or_shifted<KW>(w, v, at);
        at += iw;
    }
    return full;
}

template <int KW>
__global__ __launch_bounds__(UK_BLOCK) void uk_claim(const UnknownParams p) {
    __shared__ uint32_t installs_wg;
    if (threadIdx.x == 0) installs_wg = 0;
    __syncthreads();
    const uint32_t nm = p.miss[0];
    const UnknownTable& t = p.t;
    uint32_t installs = 0;
    for (u64 i = (u64)blockIdx.x * UK_BLOCK + threadIdx.x; i < nm; i += (u64)gridDim.x * UK_BLOCK) {  // 64-bit: nm may be near 2^32
        const int64_t r = p.miss[4 + (size_t)i];
        uint32_t res = QD_UK_SKIP;
        if (r < p.n && p.codes[r] == QD_CODE_UNDET) {
            u64 w[KW];
            if (!uk_key<KW>(p, r, w)) {
                res = QD_UK_ISSHORT;
            } else {
                u64 k4[QD_KEY_WORDS] = {0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < KW; ++q) k4[q] = w[q];
                const u64 tag = qd_uk_trim(qd_uk_tag(k4), t.tag_mask);
                res = tally_claim(t, k4, tag, installs);
            }
        }
        p.where[i] = res;
    }
    tally_installs(t, installs, &installs_wg);
}

template <int KW>
__global__ __launch_bounds__(UK_BLOCK) void uk_count(const UnknownParams p) {
    __shared__ uint32_t lslot[UK_LDS];
    __shared__ uint32_t lcnt[UK_LDS];
    __shared__ uint32_t tot[3];  // tallied, short, dropped of this workgroup
    tally_lds_init(lslot, lcnt);
    if (threadIdx.x < 3) tot[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t nm = p.miss[0];
    const UnknownTable& t = p.t;
    const int lane = threadIdx.x & 63;
    uint32_t n_tal = 0, n_short = 0, n_drop = 0;
    // the trip count is the same for every lane of the workgroup: the wave-level combining below needs whole waves
    for (u64 base = (u64)blockIdx.x * UK_BLOCK; base < nm; base += (u64)gridDim.x * UK_BLOCK) {
        const u64 i = base + threadIdx.x;
        const uint32_t res = i < nm ? p.where[i] : QD_UK_SKIP;
        bool pend = false;
        if (res == QD_UK_ISSHORT) {
            ++n_short;
        } else if (res == QD_UK_NONE) {
            ++n_drop;
        } else if (res != QD_UK_SKIP) {
            u64 w[KW];
            (void)uk_key<KW>(p, (int64_t)p.miss[4 + (size_t)i], w);
            const u64* e = t.keys + (size_t)res * QD_KEY_WORDS;
            bool same = true;
#pragma unroll
            for (int q = 0; q < KW; ++q) same = same && e[q] == w[q];
            if (same) {
                pend = true;
                ++n_tal;
            } else {
                ++n_drop;  // another key holds this tag's entry
            }
        }
        tally_combine(lslot, lcnt, t.counts, pend, res, lane);
    }
    n_tal = uk_wave_sum(n_tal);
    n_short = uk_wave_sum(n_short);
    n_drop = uk_wave_sum(n_drop);
    if (lane == 0) {
        if (n_tal) atomicAdd(&tot[0], n_tal);
        if (n_short) atomicAdd(&tot[1], n_short);
        if (n_drop) atomicAdd(&tot[2], n_drop);
    }
    __syncthreads();
    tally_lds_flush(lslot, lcnt, t.counts);
    if (threadIdx.x < 3 && tot[threadIdx.x])  // QD_UK_TALLIED, _SHORT, _DROPPED = 0, 1, 2
        atomicAdd(reinterpret_cast<unsigned long long*>(&t.totals[threadIdx.x]), (unsigned long long)tot[threadIdx.x]);
}

// read-out: a workgroup takes UK_GATHER_ITERS x 256 consecutive slots and reserves room for its occupied ones with one atomic
__global__ __launch_bounds__(UK_BLOCK) void uk_gather(const UnknownTable t, u64* out_keys, u64* out_counts, uint32_t* out_n, uint32_t cap) {
    __shared__ uint32_t wsum[UK_BLOCK / 64];
    __shared__ uint32_t bbase;
    const size_t s0 = (size_t)blockIdx.x * UK_BLOCK * UK_GATHER_ITERS + threadIdx.x;
    const size_t slots = (size_t)t.mask + 1;
    uint32_t bits = 0;
#pragma unroll
    for (int it = 0; it < UK_GATHER_ITERS; ++it) {
        const size_t s = s0 + (size_t)it * UK_BLOCK;
        if (s < slots && t.tags[s] != 0) bits |= 1u << it;
    }
    const uint32_t c = __popc(bits);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < UK_BLOCK / 64; ++w) total += wsum[w];
        bbase = total ? atomicAdd(out_n, total) : 0;
    }
    __syncthreads();
    size_t at = (size_t)bbase + inc - c;
    for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
    for (int it = 0; it < UK_GATHER_ITERS; ++it) {
        if (!(bits & (1u << it))) continue;
        const size_t s = s0 + (size_t)it * UK_BLOCK;
        if (at < cap) {
            const ulonglong2* kp = reinterpret_cast<const ulonglong2*>(t.keys + s * QD_KEY_WORDS);
            ulonglong2* op = reinterpret_cast<ulonglong2*>(out_keys + at * QD_KEY_WORDS);
            op[0] = kp[0];
            op[1] = kp[1];
            out_counts[at] = t.counts[s];
        }
        ++at;
    }
}

}  // namespace

hipError_t qd_launch_unknown(const UnknownParams& p, int cus, hipEvent_t before_claim, hipStream_t st) {
    if (p.n <= 0) return hipSuccess;
    hipError_t e;
    if (before_claim && (e = hipStreamWaitEvent(st, before_claim, 0)) != hipSuccess) return e;
    const int64_t nb = (p.n + UK_BLOCK - 1) / UK_BLOCK;
    const unsigned grid = (unsigned)std::min<int64_t>(nb, (int64_t)cus * 8);
    if (p.K <= 16) hipLaunchKernelGGL(uk_claim<2>, dim3(grid), dim3(UK_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(uk_claim<4>, dim3(grid), dim3(UK_BLOCK), 0, st, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.K <= 16) hipLaunchKernelGGL(uk_count<2>, dim3(grid), dim3(UK_BLOCK), 0, st, p);
    else hipLaunchKernelGGL(uk_count<4>, dim3(grid), dim3(UK_BLOCK), 0, st, p);
    return hipGetLastError();
}

hipError_t qd_launch_unknown_gather(const UnknownTable& t, uint64_t* out_keys, uint64_t* out_counts, uint32_t* out_n, uint32_t cap,
                                    hipStream_t st) {
    hipError_t e = hipMemsetAsync(out_n, 0, 4, st);
    if (e != hipSuccess) return e;
    const size_t slots = (size_t)t.mask + 1, per_block = (size_t)UK_BLOCK * UK_GATHER_ITERS;
    hipLaunchKernelGGL(uk_gather, dim3((unsigned)((slots + per_block - 1) / per_block)), dim3(UK_BLOCK), 0, st, t, out_keys, out_counts,
                       out_n, cap);
    return hipGetLastError();
}
