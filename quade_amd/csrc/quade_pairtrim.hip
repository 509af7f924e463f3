// gfx950 (CDNA4 / MI355X): paired-end overlap trimming of a batch's insert reads with insert sizes (qd_pairtrim_set) while their
// text sits in HBM.  quade_pairtrim.h states the definition; a cut is a new seq_len, written into copies of the record tables.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a pair.  Both sequence lines are staged in the row's slab of
// LDS:
//   R1  : case folded (b & 0xDF), so a byte that is no letter of ACGT equals none of them and has bit 5 clear;
//   R2  : reverse-complemented -- source word k becomes word n_words - 1 - k with its bytes reversed, which puts RC2[x] at byte
//         t + x of the slab, t = 16 * n_words - (s + L2) -- and every byte that is no letter of ACGT becomes one with bit 5 set,
//         which a folded byte of R1 never equals.
// With d = L2 - I, candidate I is then a straight compare of R1[i] against RC2[i + d] over the overlap: four bases per step, two
// unaligned words each made of two aligned ones (v_alignbyte), the bytes that differ counted in the word; a candidate ends when
// its budget is spent.  Lane i of a round tries the i-th candidate of 16: first I >= M ascending, ending with the first round that
// accepts one (row minimum), then I < M descending (row maximum).
// A line of more than 21 words does not fit its slab: the pair then takes the same search over bytes in global memory.
// Lanes 0 .. 14 of every row keep one counter each in a register (quade_row.h's flush_row_counters); the insert sizes are a
// histogram in LDS of the workgroup's own, flushed behind them with 64-bit atomics for what is not zero.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_pairtrim.h"

namespace {

constexpr uint32_t PT_BLOCK = 256;
constexpr uint32_t PT_GROUPS = PT_BLOCK / ROW;      // pairs per step of a workgroup
constexpr uint32_t PT_WG_PAIRS = 1024;              // pairs per workgroup: a 32-bit partial cannot overflow
constexpr uint32_t PT_SCALARS = QD_PT_HIST;         // the 15 counters in front of the histogram
static_assert(PT_WG_PAIRS % PT_GROUPS == 0, "whole steps");

// four bytes of R2, in place: the complement of a letter of ACGT (either case) in upper case, a byte with bit 5 set for any other
__device__ __forceinline__ uint32_t complement4(uint32_t w) {
    w &= 0xDFDFDFDFu;
    const uint32_t at = bytes_eq(w, 'A') | bytes_eq(w, 'T'), cg = bytes_eq(w, 'C') | bytes_eq(w, 'G');
    return (w ^ (at & 0x15151515u) ^ (cg & 0x04040404u)) | (~(at | cg) & 0x20202020u);  // 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04
}
__device__ __forceinline__ uint32_t complement1(uint32_t b) {  // one byte, for the byte path: the same mapping
    b &= 0xDFu;
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : 0x20u;
}

// ov(I) = min(L1, I) - max(0, I - L2) = min(I, L1, L2, L1 + L2 - I) for 1 <= I <= L1 + L2
template <typename T>
__device__ __forceinline__ T overlap_of(T I, T L1, T L2) {
    return min(min(I, L1 + L2 - I), min(L1, L2));
}

struct Budget {
    uint32_t min_overlap, max_mismatches, pct;
    template <typename T>
    __device__ __forceinline__ uint32_t of(T ov) const {
        return (uint32_t)min((T)max_mismatches, (T)(ov * pct / 100u));
    }
};

// candidate I over the staged lines: a = R1 folded from byte s1 of its slab, b = RC2 from byte t of its slab
struct StagedAccept {
    const uint32_t *a, *b;
    uint32_t s1, t, L1, L2;
    Budget B;
    __device__ __forceinline__ bool operator()(uint32_t I) const {
        const uint32_t ov = overlap_of(I, L1, L2);
        if (ov < B.min_overlap) return false;
        const uint32_t budget = B.of(ov);
        const uint32_t pa = s1 + (I > L2 ? I - L2 : 0u), pb = t + (L2 > I ? L2 - I : 0u);
        const uint32_t sha = pa & 3u, shb = pb & 3u;
        const uint32_t *wa = a + (pa >> 2), *wb = b + (pb >> 2);
        uint32_t la = wa[0], lb = wb[0], mm = 0;
        for (uint32_t k = 0; 4 * k < ov; ++k) {
            // one dword ahead: at the line's end this can be a dword of the slab (at most dword 4 * n_words <= 84 of its 88) that
            // this pair never wrote; v_alignbyte shifts it out when sh == 0 and the tail mask below removes what is left of it
            const uint32_t ha = wa[k + 1], hb = wb[k + 1];
            uint32_t x = __builtin_amdgcn_alignbyte(ha, la, sha) ^ __builtin_amdgcn_alignbyte(hb, lb, shb);
            la = ha;
            lb = hb;
            const uint32_t rem = ov - 4 * k;
            if (rem < 4) x &= (1u << (8 * rem)) - 1u;
            mm += differing_bytes(x);
            if (mm > budget) return false;
        }
        return true;
    }
};

// ... over the bytes in global memory (a line longer than its slab): the same answers
struct BytesAccept {
    const uint8_t *s1, *s2;
    uint64_t L1, L2;
    Budget B;
    __device__ __forceinline__ bool operator()(uint64_t I) const {
        const uint64_t ov = overlap_of(I, L1, L2);
        if (ov < B.min_overlap) return false;
        const uint32_t budget = B.of(ov);
        const uint64_t i0 = I > L2 ? I - L2 : 0;  // i0 + ov = min(L1, I): j = I - 1 - i stays in [0, L2)
        uint32_t mm = 0;
        for (uint64_t k = 0; k < ov; ++k) {
            const uint64_t i = i0 + k;
            mm += (uint32_t)(s1[i] & 0xDFu) != complement1(s2[I - 1 - i]);
            if (mm > budget) return false;
        }
        return true;
    }
};

// I* of the pair in every lane of its row, 0 = none.  T: wide enough for L1 + L2 + 16.
template <typename T, typename ACCEPT>
__device__ __forceinline__ T find_insert(const ACCEPT& accept, T L1, T L2, T min_overlap, uint32_t sub) {
    if (min(L1, L2) < min_overlap) return 0;  // ov(I) <= min(L1, L2)
    const T M = max(L1, L2), hi = L1 + L2 - min_overlap;  // I >= M: ov = L1 + L2 - I, so I <= hi; hi >= M here
    for (T I0 = M; I0 <= hi; I0 += ROW) {
        const T I = I0 + sub;
        T hit = ~(T)0;
        if (I <= hi && accept(I)) hit = I;
        hit = row_min(hit);
        if (hit != ~(T)0) return hit;
    }
    // I < M: ov <= I, so I >= min_overlap (>= 1)
    for (T top = M; top > min_overlap; top = top > ROW ? top - ROW : 0) {  // this round: I = top - 1 - sub
        T hit = 0;
        if (top > sub && top - 1 - sub >= min_overlap && accept(top - 1 - sub)) hit = top - 1 - sub;
        hit = row_max(hit);
        if (hit) return hit;
    }
    return 0;
}

__global__ __launch_bounds__(PT_BLOCK) void pairtrim(qd_pairtrim_dev P, qd_pairtrim_args a, uint32_t n) {
    __shared__ uint4 slab[PT_GROUPS][2][SLAB_WORDS];  // per row: R1 folded, R2 reverse-complemented
    __shared__ uint32_t hist[QD_PT_BINS];
    __shared__ unsigned long long part[PT_SCALARS];
    for (uint32_t i = threadIdx.x; i < QD_PT_BINS; i += PT_BLOCK) hist[i] = 0;
    if (threadIdx.x < PT_SCALARS) part[threadIdx.x] = 0;
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    uint4* sa = slab[group][0];
    uint4* sb = slab[group][1];
    const Budget B{P.min_overlap, P.max_mismatches, P.mismatch_pct};
    uint64_t acc = 0;  // counter `sub` of this row's pairs
    const uint32_t first = blockIdx.x * PT_WG_PAIRS, last = min(n, first + PT_WG_PAIRS);
    for (uint32_t j0 = first; j0 < last; j0 += PT_GROUPS) {  // (the same trips for every wave: a barrier inside)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        qd_rec rec[2] = {};
        if (valid) {
            rec[0] = a.recs[0][j];
            rec[1] = a.recs[1][j];
        }
        const uint32_t L[2] = {rec[0].seq_len, rec[1].seq_len};
        const Line l1 = make_line(a.text[0], rec[0].seq, L[0]), l2 = make_line(a.text[1], rec[1].seq, L[1]);
        const bool staged = l1.n_words <= FAST_WORDS && l2.n_words <= FAST_WORDS;
        const bool search = min(L[0], L[1]) >= P.min_overlap;  // otherwise no candidate has overlap enough: nothing is read
        __syncthreads();  // the row's earlier pair is done with the slab (and, the first time, the partials are zero)
        if (staged && search) {
            stage_line<true>(sa, l1, sub);
            for (uint32_t k = sub; k < l2.n_words; k += ROW) {
                const uint4 v = l2.w0[k];
                uint4 o;
                o.x = __builtin_bswap32(complement4(v.w));
                o.y = __builtin_bswap32(complement4(v.z));
                o.z = __builtin_bswap32(complement4(v.y));
                o.w = __builtin_bswap32(complement4(v.x));
                sb[l2.n_words - 1 - k] = o;
            }
        }
        __syncthreads();
        uint64_t I = 0;  // I*, 0 = none
        if (search) {
            if (staged) {
                const StagedAccept acc_s{reinterpret_cast<const uint32_t*>(sa), reinterpret_cast<const uint32_t*>(sb), l1.s,
                                         16u * l2.n_words - (l2.s + L[1]), L[0], L[1], B};
                I = find_insert<uint32_t>(acc_s, L[0], L[1], P.min_overlap, sub);
            } else {
                const BytesAccept acc_b{a.text[0] + rec[0].seq, a.text[1] + rec[1].seq, L[0], L[1], B};
                I = find_insert<uint64_t>(acc_b, (uint64_t)L[0], (uint64_t)L[1], (uint64_t)P.min_overlap, sub);
            }
        }
        const uint32_t M = max(L[0], L[1]);
        const bool cut = I && I < M;
        if (valid) {
            uint32_t Lp[2], Lout[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                Lp[r] = cut ? (uint32_t)min((uint64_t)L[r], I) : L[r];
                Lout[r] = max(Lp[r], min(P.min_length, L[r]));
            }
            if (sub < 2) {
                qd_rec o = sub ? rec[1] : rec[0];
                o.seq_len = Lout[sub];
                a.out[sub][j] = o;
            }
            if (sub == 0 && I) atomicAdd(&hist[I < QD_PT_BINS - 1 ? (uint32_t)I : QD_PT_BINS - 1], 1u);
            if (sub == 0 && a.insert) a.insert[j] = I;  // the hand-over to the overlap base correction: 0 = none
            uint32_t add = 0;  // this lane's counter of the pair
            auto put = [&](uint32_t i, uint32_t x) {
                if (sub == i) add = x;
            };
#pragma unroll
            for (uint32_t r = 0; r < 2; ++r) {
                put(r * QD_PT_COUNTERS + QD_PT_READS, 1u);
                put(r * QD_PT_COUNTERS + QD_PT_BASES_IN, L[r]);
                put(r * QD_PT_COUNTERS + QD_PT_BASES_OUT, Lout[r]);
                put(r * QD_PT_COUNTERS + QD_PT_CUT_READS, Lp[r] < L[r]);
                put(r * QD_PT_COUNTERS + QD_PT_CUT_BASES, L[r] - Lp[r]);
                put(r * QD_PT_COUNTERS + QD_PT_FLOORED, Lout[r] > Lp[r]);
            }
            put(QD_PT_PAIRS, 1u);
            put(QD_PT_OVERLAPPED, I != 0);
            put(QD_PT_SHORT, cut);
            acc += add;
        }
    }
    unsigned long long* table = reinterpret_cast<unsigned long long*>(a.table);
    flush_row_counters<PT_SCALARS>(acc, sub, part, table);
    for (uint32_t i = threadIdx.x; i < QD_PT_BINS; i += PT_BLOCK)
        if (hist[i]) atomicAdd(table + QD_PT_HIST + i, (unsigned long long)hist[i]);
}

}  // namespace

hipError_t qd_pairtrim_launch(const qd_pairtrim_dev& P, const qd_pairtrim_args& a, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || !P.min_overlap || P.mismatch_pct > 100) return hipErrorInvalidValue;
    const uint32_t grid = (n + PT_WG_PAIRS - 1) / PT_WG_PAIRS;
    hipLaunchKernelGGL(pairtrim, dim3(grid), dim3(PT_BLOCK), 0, st, P, a, n);
    return hipGetLastError();
}
