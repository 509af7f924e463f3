// gfx950 (CDNA4 / MI355X): overlap base correction of a batch's read pairs (qd_paircorrect_set) while their text sits in HBM.
// quade_paircorrect.h states the rule; a correction is a base and its quality byte written over the doubtful call, in place.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a pair, whose insert length I* the overlap stage has stored.
// Staged path (both sequence lines fit their slabs): R1 is staged case folded and R2 reverse-complemented exactly as
// quade_pairtrim.hip stages them -- RC2[x] at byte t + x of its slab, t = 16 * n_words - (s + L2), every byte that is no letter of
// ACGT with bit 5 set -- so that candidate I* is a straight compare of R1[i] against RC2[i + L2 - I*].  Where pairtrim's lanes walk a
// candidate each, the row here shares the one: the overlap's dwords (four bases, two unaligned words each made of two aligned ones,
// v_alignbyte) are dealt across the lanes, dword m to lane m mod 16.  Only a lane that finds a differing dword goes to bytes.  The
// two slab bytes of a position say everything about its bases -- the folded R1 byte is valid iff it is a letter, the RC2 byte iff bit 5
// is clear, and then it IS comp(u(s2[j])), the base case 2 writes -- so the lane loads the two quality bytes from global memory,
// decides, and stores.  Quality lines are not staged: at most a handful of positions per pair need them.
// Byte path (a line of more than 21 words): the lanes stride over the positions in global memory and give the same answers.
// Stores are single bytes, each by the one lane that owns the position (quade_paircorrect.h says why nothing wider will do).
// Lanes 0 .. 9 of every row keep one counter each in a register (quade_row.h's flush_row_counters).  LDS: pairtrim's slabs without its
// histogram, 11 KB a workgroup -- the 32 waves of a CU, not the LDS, bound the occupancy.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_paircorrect.h"

namespace {

constexpr uint32_t PC_BLOCK = 256;
constexpr uint32_t PC_GROUPS = PC_BLOCK / ROW;  // pairs per step of a workgroup
constexpr uint32_t PC_WG_PAIRS = 1024;          // pairs per workgroup
static_assert(PC_WG_PAIRS % PC_GROUPS == 0, "whole steps");

// four bytes of R2, in place: the complement of a letter of ACGT (either case) in upper case, a byte with bit 5 set for any other
// (quade_pairtrim.hip's staging)
__device__ __forceinline__ uint32_t complement4(uint32_t w) {
    w &= 0xDFDFDFDFu;
    const uint32_t at = bytes_eq(w, 'A') | bytes_eq(w, 'T'), cg = bytes_eq(w, 'C') | bytes_eq(w, 'G');
    return (w ^ (at & 0x15151515u) ^ (cg & 0x04040404u)) | (~(at | cg) & 0x20202020u);  // 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04
}
__device__ __forceinline__ uint32_t complement1(uint32_t b) {  // one byte: the same mapping
    b &= 0xDFu;
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : 0x20u;
}

// this lane's share of a pair: bases written into R1 and into R2, positions left unresolved
struct Tally {
    uint32_t r1 = 0, r2 = 0, unresolved = 0;
};

// One mismatching position.  a: u(s1[i]); rc: s2[j] complemented as staged (bit 5 clear: valid, and rc == comp(u(s2[j]))).
__device__ __forceinline__ void decide(const qd_paircorrect_dev& P, uint32_t a, uint32_t rc, uint8_t* s1, uint8_t* q1, uint8_t* s2,
                                       uint8_t* q2, Tally& t) {
    const uint32_t qa = *q1, qb = *q2;  // phred(c) >= G iff c >= 33 + G, phred(c) <= B iff c <= 33 + B: the bytes unsigned
    const uint32_t ca = complement1(a);
    if (ca != 0x20u && qa >= P.good_byte && qb <= P.bad_byte) {  // R1 is trusted: R2 is corrected
        *s2 = (uint8_t)ca;
        *q2 = (uint8_t)qa;
        ++t.r2;
    } else if (!(rc & 0x20u) && qb >= P.good_byte && qa <= P.bad_byte) {  // R2 is trusted: R1 is corrected
        *s1 = (uint8_t)rc;
        *q1 = (uint8_t)qb;
        ++t.r1;
    } else {
        ++t.unresolved;
    }
}

__global__ __launch_bounds__(PC_BLOCK) void paircorrect(qd_paircorrect_dev P, qd_paircorrect_args a, uint32_t n) {
    __shared__ uint4 slab[PC_GROUPS][2][SLAB_WORDS];  // per row: R1 folded, R2 reverse-complemented
    __shared__ unsigned long long part[QD_PC_VALUES];
    if (threadIdx.x < QD_PC_VALUES) part[threadIdx.x] = 0;
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    uint4* sa = slab[group][0];
    uint4* sb = slab[group][1];
    uint64_t acc = 0;  // counter `sub` of this row's pairs
    const uint32_t first = blockIdx.x * PC_WG_PAIRS, last = min(n, first + PC_WG_PAIRS);
    for (uint32_t j0 = first; j0 < last; j0 += PC_GROUPS) {  // (the same trips for every wave: a barrier inside)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        qd_rec rec[2] = {};
        uint64_t I = 0;  // I*, 0 = none
        if (valid) {
            rec[0] = a.recs[0][j];
            rec[1] = a.recs[1][j];
            I = a.insert[j];
        }
        const uint64_t L1 = rec[0].seq_len, L2 = rec[1].seq_len;
        if (I > L1 + L2) I = 0;  // (no such candidate: no positions)
        const uint64_t i0 = I > L2 ? I - L2 : 0;             // the first position of R1 ...
        const uint64_t ov = (I < L1 ? I : L1) - i0;          // ... and how many: min(L1, I) - max(0, I - L2)
        const Line l1 = make_line(a.text[0], rec[0].seq, rec[0].seq_len), l2 = make_line(a.text[1], rec[1].seq, rec[1].seq_len);
        const bool staged = l1.n_words <= FAST_WORDS && l2.n_words <= FAST_WORDS;
        uint8_t* const s1 = a.text[0] + rec[0].seq;
        uint8_t* const q1 = a.text[0] + rec[0].qual;
        uint8_t* const s2 = a.text[1] + rec[1].seq;
        uint8_t* const q2 = a.text[1] + rec[1].qual;
        __syncthreads();  // the row's earlier pair is done with the slab (and, the first time, the partials are zero)
        if (staged && ov) {
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
        Tally t;
        if (ov && staged) {  // (lines of at most 336 bytes: 32 bits do)
            const uint32_t ov32 = (uint32_t)ov, at1 = (uint32_t)i0, I32 = (uint32_t)I, L2s = rec[1].seq_len;
            const uint32_t pa = l1.s + at1, pb = 16u * l2.n_words - (l2.s + L2s) + (L2s > I32 ? L2s - I32 : 0u);
            const uint32_t sha = pa & 3u, shb = pb & 3u;
            const uint32_t *wa = reinterpret_cast<const uint32_t*>(sa) + (pa >> 2), *wb = reinterpret_cast<const uint32_t*>(sb) + (pb >> 2);
            for (uint32_t m = sub; 4 * m < ov32; m += ROW) {
                // one dword ahead: at the line's end this can be a dword of the slab (at most dword 4 * n_words <= 84 of its 88) that
                // this pair never wrote; v_alignbyte shifts it out when sh == 0 and the tail mask below removes what is left of it
                const uint32_t xa = __builtin_amdgcn_alignbyte(wa[m + 1], wa[m], sha), xb = __builtin_amdgcn_alignbyte(wb[m + 1], wb[m], shb);
                uint32_t x = xa ^ xb;
                const uint32_t rem = ov32 - 4 * m;
                if (rem < 4) x &= (1u << (8 * rem)) - 1u;
                if (!x) continue;
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b) {
                    if (!((x >> (8 * b)) & 0xFFu)) continue;
                    const uint32_t i = at1 + 4 * m + b, jj = I32 - 1 - i;  // i < min(L1, I*), 0 <= jj < L2
                    decide(P, (xa >> (8 * b)) & 0xFFu, (xb >> (8 * b)) & 0xFFu, s1 + i, q1 + i, s2 + jj, q2 + jj, t);
                }
            }
        } else if (ov) {
            for (uint64_t k = sub; k < ov; k += ROW) {
                const uint64_t i = i0 + k, jj = I - 1 - i;  // i < min(L1, I*), 0 <= jj < L2
                const uint32_t u1 = s1[i] & 0xDFu, rc = complement1(s2[jj]);
                if (u1 != rc) decide(P, u1, rc, s1 + i, q1 + i, s2 + jj, q2 + jj, t);
            }
        }
        // the pair's sums in every lane of its row (every lane of the wave takes part)
        const uint64_t c1 = row_sum((uint64_t)t.r1), c2 = row_sum((uint64_t)t.r2), un = row_sum((uint64_t)t.unresolved);
        if (valid) {
            uint64_t add = 0;  // this lane's counter of the pair
            auto put = [&](uint32_t i, uint64_t x) {
                if (sub == i) add = x;
            };
            put(QD_PC_R1_READS, c1 != 0);
            put(QD_PC_R1_BASES, c1);
            put(QD_PC_R2_READS, c2 != 0);
            put(QD_PC_R2_BASES, c2);
            put(QD_PC_PAIRS, 1u);
            put(QD_PC_OVERLAPPED, I != 0);
            put(QD_PC_OVERLAP_BASES, ov);
            put(QD_PC_MISMATCHES, c1 + c2 + un);
            put(QD_PC_UNRESOLVED, un);
            put(QD_PC_CORRECTED_PAIRS, (c1 | c2) != 0);
            acc += add;
        }
    }
    flush_row_counters<QD_PC_VALUES>(acc, sub, part, reinterpret_cast<unsigned long long*>(a.table));
}

}  // namespace

hipError_t qd_paircorrect_launch(const qd_paircorrect_dev& P, const qd_paircorrect_args& a, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || P.good_byte < 34 || P.good_byte > 126 || P.bad_byte < 33 || P.bad_byte >= P.good_byte || !a.insert)
        return hipErrorInvalidValue;
    const uint32_t grid = (n + PC_WG_PAIRS - 1) / PC_WG_PAIRS;
    hipLaunchKernelGGL(paircorrect, dim3(grid), dim3(PC_BLOCK), 0, st, P, a, n);
    return hipGetLastError();
}
