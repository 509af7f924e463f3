// gfx950 (CDNA4 / MI355X): read filtering of the insert reads (qd_filter_set), one pass over the sequence and quality lines of a
// batch's insert reads while their text sits in HBM: a reason byte per pair and eight counters per destination.
//
// Shape (quade_row.h's counting stage; quade_qstats.hip reads the same four lines): 16 lanes (one DPP row) share a pair.  Each of
// the pair's four lines is read one aligned word per lane, head and tail masked: 256 bytes per step, so a 2 x 150 bp pair costs
// four loads per lane, all in flight together.  The bytes are counted four at a time in 32-bit words (SWAR compares, popcount,
// v_sad_u8 for the byte sum).  Particular to this stage is the neighbour compare: every folded word against itself shifted by one byte
// (v_alignbyte); the byte beyond a lane's 16 comes from the next lane (DPP row_shl:1), the byte beyond a 256-byte step from the
// next step's first word, and the positions are masked to [0, L - 1), so that neither the newline behind the line nor the byte in
// front of it ever counts.  The sums go over the row with DPP, every lane of the row then applies the rule, lane 0 stores the
// reason and lanes 0 .. 7 hold the pair's 8 values, one each, for quade_row.h's DestTable: LDS partials for a small S, merged
// global atomics for a large one.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_filter.h"

namespace {

constexpr uint32_t FL_BLOCK = 256;
constexpr uint32_t FL_GROUPS = FL_BLOCK / ROW;       // pairs per step of a workgroup
constexpr uint32_t FL_WG_PAIRS = 2048;               // pairs per workgroup
constexpr uint32_t FL_LDS_MAX_LEN = 2047;            // longer reads bypass the 32-bit partials
// the largest 32-bit partial is a destination's bases_in when it receives every pair of the workgroup
static_assert((uint64_t)FL_WG_PAIRS * 2 * FL_LDS_MAX_LEN <= 0xFFFFFFFFull, "a workgroup's LDS partials can overflow");
static_assert(QD_FL_LDS_MAX_DEST * QD_FL_VALUES * 4 <= 65536, "the LDS partials exceed 64 KiB");
static_assert(FL_WG_PAIRS % FL_GROUPS == 0, "whole steps");

struct ReadSums {  // one lane's share of a read
    uint32_t ge, nn, diff;
    uint64_t qsum;
};
// bytes outside the line are zero: neither 'N' nor a quality >= 33
__device__ __forceinline__ void add_seq(uint4 v, ReadSums& a) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t y = (w[i] | 0x20202020u) ^ 0x6E6E6E6Eu;  // zero bytes: 'N' and 'n' only
        a.nn += __popc(~bytes_nz(y) & 0x80808080u);
    }
}
// word k of a sequence line as loaded (not masked) and the dword behind it: the positions of [s, e - 1) whose byte and the byte
// behind it differ once bit 5 is folded away.  (Word n_words - 2 lies inside [s, e - 1) whole: only the edge words need the mask.)
__device__ __forceinline__ void add_diff(const Line& L, uint32_t k, uint4 v, uint32_t next, ReadSums& a) {
    v = fold_case(v);
    const uint32_t f[5] = {v.x, v.y, v.z, v.w, next & 0xDFDFDFDFu};
    const bool edge = edge_word(L, k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t m = bytes_nz(f[i] ^ __builtin_amdgcn_alignbyte(f[i + 1], f[i], 1u));
        if (edge) m &= byte_mask(L.s, (int64_t)L.e - 1, (int64_t)k * 16 + 4 * i);
        a.diff += __popc(m);
    }
}
__device__ __forceinline__ void add_qual(uint4 v, uint32_t t, ReadSums& a) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t sum = 0, c33 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t g33 = bytes_ge(w[i], 33);
        a.ge += __popc(bytes_ge(w[i], t));
        c33 += __popc(g33);
        sum = __builtin_amdgcn_sad_u8(w[i] & ((g33 >> 7) * 0xFFu), 0u, sum);  // sum of the bytes >= 33
    }
    a.qsum += sum - 33u * c33;
}
// one 256-byte step of a sequence line: lane sub holds word k0 + sub (zeros beyond the line); every lane of the row is here
__device__ __forceinline__ void seq_step(const Line& L, uint32_t k0, uint32_t sub, uint4 v, ReadSums& a) {
    const uint32_t k = k0 + sub;
    uint32_t next = from_next_lane(v.x);
    if (sub == ROW - 1 && k + 1 < L.n_words) next = L.w0[k + 1].x;  // the next step's first word
    add_seq(mask_word(L, k, v), a);
    add_diff(L, k, v, next, a);
}

// the rule: 0 or the first rule that a read of the pair fails
__device__ __forceinline__ uint32_t reason_of(const qd_filter_dev& P, const uint32_t len[2], const uint32_t nn[2], const uint32_t unq[2],
                                              const uint64_t qsum[2], const uint32_t diff[2]) {
    uint32_t why = 0;
#pragma unroll
    for (int r = 1; r >= 0; --r)
        if (P.min_complexity_pct >= 0 && (uint64_t)diff[r] * 100u < (uint64_t)P.min_complexity_pct * (len[r] ? len[r] - 1u : 0u)) why = QD_FL_LOW_COMPLEXITY;
#pragma unroll
    for (int r = 1; r >= 0; --r)
        if (P.min_mean_quality >= 0 && qsum[r] < (uint64_t)P.min_mean_quality * len[r]) why = QD_FL_LOW_MEAN_QUALITY;
#pragma unroll
    for (int r = 1; r >= 0; --r)
        if (P.max_unqualified_pct >= 0 && (uint64_t)unq[r] * 100u > (uint64_t)P.max_unqualified_pct * len[r]) why = QD_FL_LOW_QUALITY;
#pragma unroll
    for (int r = 1; r >= 0; --r)
        if (P.max_n >= 0 && nn[r] > (uint32_t)P.max_n) why = QD_FL_TOO_MANY_N;
#pragma unroll
    for (int r = 1; r >= 0; --r)
        if (P.min_length >= 0 && len[r] < (uint32_t)P.min_length) why = QD_FL_TOO_SHORT;
    return why;
}

template <bool LDS>
__global__ __launch_bounds__(FL_BLOCK) void filter_pairs(qd_filter_dev P, qd_filter_args a, uint32_t n_samples, uint32_t n) {
    extern __shared__ uint32_t part[];  // LDS path: [n_dest][QD_FL_VALUES]
    const uint32_t n_dest = 2 * n_samples + 1;
    const DestTable<LDS, QD_FL_VALUES, FL_BLOCK> table{part, reinterpret_cast<unsigned long long*>(a.table), n_dest * QD_FL_VALUES};
    table.init();
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint32_t first = blockIdx.x * FL_WG_PAIRS, last = min(n, first + FL_WG_PAIRS);
    const uint32_t qual_byte = (uint32_t)P.qual_byte;
    for (uint32_t j0 = first; j0 < last; j0 += FL_GROUPS) {  // (the same trips for every wave: the DPP sums need whole rows)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        uint32_t d = 0xFFFFFFFFu, len[2] = {0, 0};
        Line line[4];  // R1 sequence, R1 quality, R2 sequence, R2 quality
        uint4 w[4];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t seq = 0, qual = 0;
            if (valid) {
                const qd_rec* rec = a.recs[r] + j;
                seq = rec->seq;
                qual = rec->qual;
                len[r] = rec->seq_len;
            }
            line[2 * r] = make_line(a.text[r], seq, len[r]);
            line[2 * r + 1] = make_line(a.text[r], qual, len[r]);
        }
        if (valid) {
            const uint32_t c = a.codes[j];
            d = c == QD_CODE_UNDETERMINED ? 2 * n_samples : min(c, 2 * n_samples);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = sub < line[q].n_words ? line[q].w0[sub] : make_uint4(0, 0, 0, 0);  // four loads in flight
        ReadSums s[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const Line& sl = line[2 * r];
            const Line& ql = line[2 * r + 1];
            s[r] = ReadSums{0, 0, 0, 0};
            seq_step(sl, 0, sub, w[2 * r], s[r]);  // (a lane beyond the line holds zeros)
            add_qual(mask_word(ql, sub, w[2 * r + 1]), qual_byte, s[r]);
            // reads longer than 241 .. 256 bases: the trip count is the row's, so that row_shl finds every lane of the row
            for (uint32_t k0 = ROW; k0 < sl.n_words; k0 += ROW) {
                const uint32_t k = k0 + sub;
                seq_step(sl, k0, sub, k < sl.n_words ? sl.w0[k] : make_uint4(0, 0, 0, 0), s[r]);
            }
            for (uint32_t k = sub + ROW; k < ql.n_words; k += ROW) add_qual(mask_word(ql, k, ql.w0[k]), qual_byte, s[r]);
        }
        uint32_t nn[2], unq[2], diff[2];
        uint64_t qsum[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            nn[r] = row_sum(s[r].nn);
            unq[r] = len[r] - row_sum(s[r].ge);
            diff[r] = row_sum(s[r].diff);
            // a lane's quality sum can pass 32 bits (a read of hundreds of MB): 28 low bits and the rest apart
            qsum[r] = (uint64_t)row_sum((uint32_t)s[r].qsum & 0x0FFFFFFFu) + ((uint64_t)row_sum((uint32_t)(s[r].qsum >> 28)) << 28);
        }
        const uint32_t why = reason_of(P, len, nn, unq, qsum, diff);
        if (valid && sub == 0) a.reason[j] = (uint8_t)why;
        // the pair's 8 values, value i in lane i of the row
        const uint64_t bases = (uint64_t)len[0] + len[1];
        uint64_t v = 0;
        if (sub == QD_FL_PAIRS) v = 1;
        else if (sub <= QD_FL_LOW_COMPLEXITY) v = why == sub ? 1 : 0;
        else if (sub == QD_FL_BASES_IN) v = bases;
        else if (sub == QD_FL_BASES_DROPPED) v = why ? bases : 0;
        const bool mine = valid && sub < QD_FL_VALUES;
        if (!mine) v = 0;
        table.add(d, sub, v, mine, len[0] <= FL_LDS_MAX_LEN && len[1] <= FL_LDS_MAX_LEN);
    }
    table.flush();
}

}  // namespace

hipError_t qd_filter_launch(const qd_filter_dev& P, const qd_filter_args& a, uint32_t n_samples, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || n_samples > QD_MAX_SAMPLES) return hipErrorInvalidValue;
    const uint32_t grid = (n + FL_WG_PAIRS - 1) / FL_WG_PAIRS;
    if (qd_filter_path(n_samples) == QD_FL_PATH_LDS)
        hipLaunchKernelGGL(filter_pairs<true>, dim3(grid), dim3(FL_BLOCK), qd_filter_values(n_samples) * 4, st, P, a, n_samples, n);
    else
        hipLaunchKernelGGL(filter_pairs<false>, dim3(grid), dim3(FL_BLOCK), 0, st, P, a, n_samples, n);
    return hipGetLastError();
}
