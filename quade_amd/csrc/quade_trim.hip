// gfx950 (CDNA4 / MI355X): 3' quality and adapter trimming of a batch's insert reads (qd_trim_set) while their text sits in HBM.
// A trim is a new seq_len: the kernel writes trimmed copies of the scan's record tables and counts what it cut.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a read; blockIdx.y says R1 or R2.  The quality and the
// sequence line are staged in the row's slab of LDS, the sequence with its case folded.
//   quality trim  : lane i takes the i-th stretch of ceil(L / 16) bytes from the 3' end.  The stretch sums are scanned over the
//                   row (DPP row_shr); every lane then walks its stretch again from the true running sum, notes where it turns
//                   negative and its strict maximum; the first negative lane ends the walk and the largest maximum of the lanes
//                   up to it -- the one nearest the 3' end among equals -- is the cut.
//   adapter search: lane i tries positions i, i + 16, ...: four bases per step, an unaligned word of the slab made of two
//                   aligned ones (v_alignbyte) against the adapter's packed words from the kernel arguments, the bytes that
//                   differ counted in the word; a candidate ends when its budget is spent.  The row minimum of the accepted
//                   positions is the leftmost; the search ends with the first round that accepts one.
// A line of more than 21 words does not fit its slab: the same two algorithms then read bytes from global memory.
// Lanes 0 .. 7 of every row keep one counter each in a register (quade_row.h's flush_row_counters).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "quade_row.h"
#include "quade_trim.h"

namespace {

constexpr uint32_t TR_BLOCK = 256;
constexpr uint32_t TR_GROUPS = TR_BLOCK / ROW;      // reads per step of a workgroup
constexpr uint32_t TR_WG_READS = 1024;              // reads per workgroup
static_assert(TR_WG_READS % TR_GROUPS == 0, "whole steps");

// Quality trim of q[0 .. L) with cutoff C > 0 (the caller's row holds one read): the length kept, in every lane.  SUM: wide enough
// for L * 255.
template <typename SUM, typename PTR>
__device__ __forceinline__ uint32_t quality_trim(PTR q, uint32_t L, uint32_t C, uint32_t sub) {
    const uint32_t T = (L + ROW - 1) / ROW;  // lane i: [L - (i + 1) T, L - i T), walked downwards
    const uint32_t hi = L > sub * T ? L - sub * T : 0, lo = hi > T ? hi - T : 0;
    auto step = [&](uint32_t i) {
        const uint32_t b = q[i];
        return (SUM)C - (SUM)(b > 33 ? b - 33 : 0);
    };
    SUM sum = 0;
    for (uint32_t i = hi; i-- > lo;) sum += step(i);
    SUM run = row_sum_below(sum);  // what the walk has summed when it enters this lane's stretch
    SUM best = 0;
    uint32_t pos = 0;
    bool neg = false;
    for (uint32_t i = hi; i-- > lo;) {
        run += step(i);
        if (run < 0) {
            neg = true;
            break;
        }
        if (run > best) {
            best = run;
            pos = i;
        }
    }
    const uint32_t first_neg = row_min(neg ? sub : ROW);  // the walk ends in this lane; the lanes behind it saw nothing real
    if (sub > first_neg) best = 0;
    const SUM top = row_max(best);
    // equal maxima: the strict '>' keeps the first the walk met, which is the one in the lowest lane = at the largest position
    const uint32_t stop = row_max(best == top ? pos : 0u);
    return top > 0 ? stop : L;
}

// Adapter search over the staged, case-folded sequence: slab holds the line from byte s on; -> La in every lane
__device__ __forceinline__ uint32_t adapter_staged(const uint32_t* slab, uint32_t s, uint32_t Lq, const uint32_t* ad, uint32_t A,
                                                   uint32_t min_overlap, uint32_t pct, uint32_t sub) {
    if (Lq < min_overlap) return Lq;
    const uint32_t n_p = Lq - min_overlap + 1;  // positions with an overlap of at least min_overlap (min_overlap <= A)
    for (uint32_t p0 = 0; p0 < n_p; p0 += ROW) {
        const uint32_t p = p0 + sub;
        uint32_t hit = 0xFFFFFFFFu;
        if (p < n_p) {
            const uint32_t ov = min(A, Lq - p), budget = ov * pct / 100u;
            const uint32_t at = s + p, sh = at & 3u;
            const uint32_t* w = slab + (at >> 2);
            uint32_t low = w[0], mm = 0;
            for (uint32_t k = 0; 4 * k < ov; ++k) {
                const uint32_t high = w[k + 1];
                uint32_t x = __builtin_amdgcn_alignbyte(high, low, sh) ^ ad[k];
                low = high;
                const uint32_t rem = ov - 4 * k;
                if (rem < 4) x &= (1u << (8 * rem)) - 1u;
                mm += differing_bytes(x);
                if (mm > budget) break;
            }
            if (mm <= budget) hit = p;
        }
        hit = row_min(hit);
        if (hit != 0xFFFFFFFFu) return hit;
    }
    return Lq;
}

// ... over the bytes in global memory (a line longer than its slab): the same answers
__device__ __forceinline__ uint32_t adapter_bytes(const uint8_t* seq, uint32_t Lq, const uint32_t* ad, uint32_t A, uint32_t min_overlap,
                                                  uint32_t pct, uint32_t sub) {
    if (Lq < min_overlap) return Lq;
    const uint32_t n_p = Lq - min_overlap + 1;
    for (uint32_t p0 = 0; p0 < n_p; p0 += ROW) {
        const uint32_t p = p0 + sub;
        uint32_t hit = 0xFFFFFFFFu;
        if (p0 <= 0xFFFFFFFFu - sub && p < n_p) {
            const uint32_t ov = min(A, Lq - p), budget = ov * pct / 100u;
            uint32_t mm = 0;
            for (uint32_t i = 0; i < ov; ++i) {
                const uint32_t b = seq[(size_t)p + i] & 0xDFu, c = (ad[i >> 2] >> (8 * (i & 3u))) & 0xFFu;
                mm += b != c;
                if (mm > budget) break;
            }
            if (mm <= budget) hit = p;
        }
        hit = row_min(hit);
        if (hit != 0xFFFFFFFFu) return hit;
        if (p0 > 0xFFFFFFFFu - ROW) break;
    }
    return Lq;
}

__global__ __launch_bounds__(TR_BLOCK) void trim_reads(qd_trim_dev P, qd_trim_args a, uint32_t n) {
    __shared__ uint4 slab[TR_GROUPS][2][SLAB_WORDS];  // per row: the quality line, the folded sequence line
    __shared__ unsigned long long part[QD_TRIM_COUNTERS];
    const uint32_t r = blockIdx.y;
    if (threadIdx.x < QD_TRIM_COUNTERS) part[threadIdx.x] = 0;
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint8_t* text = a.text[r];
    const qd_rec* recs = a.recs[r];
    qd_rec* out = a.out[r];
    const uint32_t* ad = P.adapter[r];
    const uint32_t A = P.adapter_len[r], C = P.cutoff;
    uint4* sq = slab[group][0];
    uint4* ss = slab[group][1];
    uint64_t acc = 0;  // counter `sub` of this row's reads
    const uint32_t first = blockIdx.x * TR_WG_READS, last = min(n, first + TR_WG_READS);
    for (uint32_t j0 = first; j0 < last; j0 += TR_GROUPS) {  // (the same trips for every wave: a barrier inside)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        qd_rec rec{};
        if (valid) rec = recs[j];
        const uint32_t L = rec.seq_len;
        const Line ql = make_line(text, rec.qual, L), sl = make_line(text, rec.seq, L);
        const bool staged = ql.n_words <= FAST_WORDS && sl.n_words <= FAST_WORDS;
        __syncthreads();  // the row's earlier read is done with the slab
        if (staged) {
            if (C) stage_line<false>(sq, ql, sub);
            if (A) stage_line<true>(ss, sl, sub);
        }
        __syncthreads();
        uint32_t Lq = L, La;
        if (staged) {
            if (C) Lq = quality_trim<int32_t>(reinterpret_cast<const uint8_t*>(sq) + ql.s, L, C, sub);
            La = A ? adapter_staged(reinterpret_cast<const uint32_t*>(ss), sl.s, Lq, ad, A, P.min_overlap, P.mismatch_pct, sub) : Lq;
        } else {
            if (C) Lq = quality_trim<int64_t>(text + rec.qual, L, C, sub);
            La = A ? adapter_bytes(text + rec.seq, Lq, ad, A, P.min_overlap, P.mismatch_pct, sub) : Lq;
        }
        const uint32_t Lout = max(La, min(P.min_length, L));
        if (valid) {
            if (sub == 0) {
                rec.seq_len = Lout;
                out[j] = rec;
            }
            const uint32_t v[QD_TRIM_COUNTERS] = {1u, L, Lout, Lq < L, L - Lq, La < Lq, Lq - La, Lout > La};
#pragma unroll
            for (uint32_t i = 0; i < QD_TRIM_COUNTERS; ++i)
                if (sub == i) acc += v[i];
        }
    }
    flush_row_counters<QD_TRIM_COUNTERS>(acc, sub, part, reinterpret_cast<unsigned long long*>(a.table) + r * QD_TRIM_COUNTERS);
}

}  // namespace

hipError_t qd_trim_launch(const qd_trim_dev& P, const qd_trim_args& a, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || P.adapter_len[0] > QD_TRIM_MAX_ADAPTER || P.adapter_len[1] > QD_TRIM_MAX_ADAPTER || !P.min_overlap)
        return hipErrorInvalidValue;
    const uint32_t grid = (n + TR_WG_READS - 1) / TR_WG_READS;
    hipLaunchKernelGGL(trim_reads, dim3(grid, 2), dim3(TR_BLOCK), 0, st, P, a, n);
    return hipGetLastError();
}
