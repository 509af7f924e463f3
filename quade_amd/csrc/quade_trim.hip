// gfx950 (CDNA4 / MI355X): 3' quality and adapter trimming of a batch's insert reads (qd_trim_set) while their text sits in HBM.
// A trim is a new seq_len: the kernel writes trimmed copies of the scan's record tables and counts what it cut.
//
// Shape: 16 lanes (one DPP row) share a read; blockIdx.y says R1 or R2.  The quality and the sequence line are read as 16-byte
// aligned words, one or two per lane, into a slab of LDS that belongs to the row (the sequence with its case folded), so that
// every lane reaches any offset of the line.
//   quality trim  : lane i takes the i-th stretch of ceil(L / 16) bytes from the 3' end.  The stretch sums are scanned over the
//                   row (DPP row_shr); every lane then walks its stretch again from the true running sum, notes where it turns
//                   negative and its strict maximum; the first negative lane ends the walk and the largest maximum of the lanes
//                   up to it -- the one nearest the 3' end among equals -- is the cut.
//   adapter search: lane i tries positions i, i + 16, ...: four bases per step, an unaligned word of the slab made of two
//                   aligned ones (v_alignbyte) against the adapter's packed words from the kernel arguments, the bytes that
//                   differ counted in the word; a candidate ends when its budget is spent.  The row minimum of the accepted
//                   positions is the leftmost; the search ends with the first round that accepts one.
// A line of more than 21 words does not fit its slab: the same two algorithms then read bytes from global memory.
// Lanes 0 .. 7 of every row keep one counter each in a register; a workgroup adds them in LDS and flushes eight 64-bit atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "quade_trim.h"

namespace {

constexpr uint32_t TR_BLOCK = 256;
constexpr uint32_t TR_GROUP = 16;                   // lanes per read: one DPP row
constexpr uint32_t TR_GROUPS = TR_BLOCK / TR_GROUP; // reads per step of a workgroup
constexpr uint32_t TR_WG_READS = 1024;              // reads per workgroup
constexpr uint32_t TR_FAST_WORDS = 21;              // 16-byte words of a staged line: 321 bases at any alignment, 336 at the best
constexpr uint32_t TR_SLAB_WORDS = TR_FAST_WORDS + 1;  // the compare looks one dword ahead
static_assert(TR_WG_READS % TR_GROUPS == 0 && QD_TRIM_COUNTERS <= TR_GROUP, "one lane per counter");
static_assert(TR_FAST_WORDS <= 2 * TR_GROUP, "two words per lane stage a line");
// the running sum of a staged line stays in 32 bits
static_assert((uint64_t)TR_FAST_WORDS * 16 * 255 < 0x7FFFFFFFull, "a staged line's quality sum can overflow");

// the value of another lane of the row (DPP), 32 or 64 bits wide
template <int CTRL, bool BOUND>
__device__ __forceinline__ int32_t dpp(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, BOUND);
}
template <int CTRL, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, BOUND);
}
template <int CTRL, bool BOUND>
__device__ __forceinline__ int64_t dpp(int64_t v) {
    const uint32_t lo = dpp<CTRL, BOUND>((uint32_t)v), hi = dpp<CTRL, BOUND>((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// over the 16 lanes of a row, the result in every lane: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
template <typename T, typename F>
__device__ __forceinline__ T row_all(T v, F f) {
    v = f(v, dpp<0xB1, false>(v));
    v = f(v, dpp<0x4E, false>(v));
    v = f(v, dpp<0x141, false>(v));
    v = f(v, dpp<0x140, false>(v));
    return v;
}
template <typename T>
__device__ __forceinline__ T row_min(T v) {
    return row_all(v, [](T a, T b) { return a < b ? a : b; });
}
template <typename T>
__device__ __forceinline__ T row_max(T v) {
    return row_all(v, [](T a, T b) { return a > b ? a : b; });
}
// sum of the lanes below this one in the row (row_shr 1, 2, 4, 8; lanes shifted in from outside the row are zero)
template <typename T>
__device__ __forceinline__ T row_sum_below(T v) {
    T s = v;
    s += dpp<0x111, true>(s);
    s += dpp<0x112, true>(s);
    s += dpp<0x114, true>(s);
    s += dpp<0x118, true>(s);
    return s - v;
}

// one line of a record as aligned 16-byte words: bytes [s, s + len) of the words from w0 on
struct Line {
    const uint4* w0;
    uint32_t s;
    uint32_t n_words;
};
__device__ __forceinline__ Line make_line(const uint8_t* text, uint32_t start, uint32_t len) {
    const uint8_t* p = text + start;
    Line L;
    L.s = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    L.w0 = reinterpret_cast<const uint4*>(p - L.s);
    L.n_words = len ? (uint32_t)(((uint64_t)L.s + len + 15) >> 4) : 0;  // every word holds at least one byte of the line
    return L;
}

// Quality trim of q[0 .. L) with cutoff C > 0 (the caller's row holds one read): the length kept, in every lane.  SUM: wide enough
// for L * 255.
template <typename SUM, typename PTR>
__device__ __forceinline__ uint32_t quality_trim(PTR q, uint32_t L, uint32_t C, uint32_t sub) {
    const uint32_t T = (L + TR_GROUP - 1) / TR_GROUP;  // lane i: [L - (i + 1) T, L - i T), walked downwards
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
    const uint32_t first_neg = row_min(neg ? sub : TR_GROUP);  // the walk ends in this lane; the lanes behind it saw nothing real
    if (sub > first_neg) best = 0;
    const SUM top = row_max(best);
    // equal maxima: the strict '>' keeps the first the walk met, which is the one in the lowest lane = at the largest position
    const uint32_t stop = row_max(best == top ? pos : 0u);
    return top > 0 ? stop : L;
}

__device__ __forceinline__ uint32_t differing_bytes(uint32_t x) {
    return (uint32_t)__popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}

// Adapter search over the staged, case-folded sequence: slab holds the line from byte s on; -> La in every lane
__device__ __forceinline__ uint32_t adapter_staged(const uint32_t* slab, uint32_t s, uint32_t Lq, const uint32_t* ad, uint32_t A,
                                                   uint32_t min_overlap, uint32_t pct, uint32_t sub) {
    if (Lq < min_overlap) return Lq;
    const uint32_t n_p = Lq - min_overlap + 1;  // positions with an overlap of at least min_overlap (min_overlap <= A)
    for (uint32_t p0 = 0; p0 < n_p; p0 += TR_GROUP) {
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
    for (uint32_t p0 = 0; p0 < n_p; p0 += TR_GROUP) {
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
        if (p0 > 0xFFFFFFFFu - TR_GROUP) break;
    }
    return Lq;
}

__global__ __launch_bounds__(TR_BLOCK) void trim_reads(qd_trim_dev P, qd_trim_args a, uint32_t n) {
    __shared__ uint4 slab[TR_GROUPS][2][TR_SLAB_WORDS];  // per row: the quality line, the folded sequence line
    __shared__ unsigned long long part[QD_TRIM_COUNTERS];
    const uint32_t r = blockIdx.y;
    if (threadIdx.x < QD_TRIM_COUNTERS) part[threadIdx.x] = 0;
    const uint32_t sub = threadIdx.x & (TR_GROUP - 1), group = threadIdx.x / TR_GROUP;
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
        const bool staged = ql.n_words <= TR_FAST_WORDS && sl.n_words <= TR_FAST_WORDS;
        __syncthreads();  // the row's earlier read is done with the slab
        if (staged) {
            for (uint32_t k = sub; k < ql.n_words && C; k += TR_GROUP) sq[k] = ql.w0[k];
            for (uint32_t k = sub; k < sl.n_words && A; k += TR_GROUP) {
                uint4 v = sl.w0[k];
                v.x &= 0xDFDFDFDFu;  // upper case for the letters; no other byte becomes A, C, G or T
                v.y &= 0xDFDFDFDFu;
                v.z &= 0xDFDFDFDFu;
                v.w &= 0xDFDFDFDFu;
                ss[k] = v;
            }
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
    __syncthreads();
    if (sub < QD_TRIM_COUNTERS && acc) atomicAdd(&part[sub], (unsigned long long)acc);
    __syncthreads();
    if (threadIdx.x < QD_TRIM_COUNTERS && part[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long*>(a.table) + r * QD_TRIM_COUNTERS + threadIdx.x, part[threadIdx.x]);
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
