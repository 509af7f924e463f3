// gfx950 (CDNA4 / MI355X): yield and quality counters per destination (qd_qstats_enable), one pass over the sequence and
// quality lines of a batch's insert reads while their text sits in HBM.
//
// Shape (quade_row.h's counting stage): 16 lanes (one DPP row) share a pair.  Each of the pair's four lines (R1 / R2 sequence
// and quality) is read one aligned word per lane, head and tail masked: 256 bytes per step, so a 2 x 150 bp pair costs four
// loads per lane, all in flight together.  The bytes are counted four at a time in 32-bit words (SWAR compares, popcount,
// v_sad_u8 for the byte sum), summed over the row with DPP, and lanes 0 .. 11 then hold the pair's 12 values, one each, for
// quade_row.h's DestTable: LDS partials for a small S, merged global atomics for a large one.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_qstats.h"

namespace {

constexpr uint32_t QS_BLOCK = 256;
constexpr uint32_t QS_GROUPS = QS_BLOCK / ROW;      // pairs per step of a workgroup
constexpr uint32_t QS_WG_PAIRS = 2048;              // pairs per workgroup
constexpr uint32_t QS_LDS_MAX_LEN = 2047;           // longer reads bypass the 32-bit partials
constexpr uint32_t QS_MAX_Q = 255 - 33;
// the largest 32-bit partial is a destination's qual_sum when it receives every pair of the workgroup
static_assert((uint64_t)QS_WG_PAIRS * QS_MAX_Q * QS_LDS_MAX_LEN <= 0xFFFFFFFFull, "a workgroup's LDS partials can overflow");
static_assert(QD_QS_LDS_MAX_DEST * QD_QS_VALUES * 4 <= 65536, "the LDS partials exceed 64 KiB");
static_assert(QS_WG_PAIRS % QS_GROUPS == 0, "whole steps");

struct ReadSums {  // one lane's share of a read
    uint32_t q20, q30, nn;
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
__device__ __forceinline__ void add_qual(uint4 v, ReadSums& a) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t sum = 0, c33 = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t g33 = bytes_ge(w[i], 33);
        a.q20 += __popc(bytes_ge(w[i], 33 + 20));
        a.q30 += __popc(bytes_ge(w[i], 33 + 30));
        c33 += __popc(g33);
        sum = __builtin_amdgcn_sad_u8(w[i] & ((g33 >> 7) * 0xFFu), 0u, sum);  // sum of the bytes >= 33
    }
    a.qsum += sum - 33u * c33;
}

template <bool LDS>
__global__ __launch_bounds__(QS_BLOCK) void qstats(qd_qstats_args a, uint32_t n_samples, uint32_t n) {
    extern __shared__ uint32_t part[];  // LDS path: [n_dest][QD_QS_VALUES]
    const uint32_t n_dest = 2 * n_samples + 1;
    const DestTable<LDS, QD_QS_VALUES, QS_BLOCK> table{part, reinterpret_cast<unsigned long long*>(a.table), n_dest * QD_QS_VALUES};
    table.init();
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint32_t first = blockIdx.x * QS_WG_PAIRS, last = min(n, first + QS_WG_PAIRS);
    for (uint32_t j0 = first; j0 < last; j0 += QS_GROUPS) {  // (the same trips for every wave: the DPP sums need whole waves)
        const uint32_t j = j0 + group;
        const bool valid = j < last && !(a.drop && a.drop[j]);
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
            s[r] = ReadSums{0, 0, 0, 0};
            add_seq(mask_word(line[2 * r], sub, w[2 * r]), s[r]);  // (a lane beyond the line holds zeros)
            add_qual(mask_word(line[2 * r + 1], sub, w[2 * r + 1]), s[r]);
            for (uint32_t k = sub + ROW; k < line[2 * r].n_words; k += ROW)  // reads longer than 241 .. 256 bases
                add_seq(mask_word(line[2 * r], k, line[2 * r].w0[k]), s[r]);
            for (uint32_t k = sub + ROW; k < line[2 * r + 1].n_words; k += ROW)
                add_qual(mask_word(line[2 * r + 1], k, line[2 * r + 1].w0[k]), s[r]);
        }
        // the pair's 12 values, value i in lane i of the row
        uint64_t v = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t q20 = row_sum(s[r].q20), q30 = row_sum(s[r].q30), nn = row_sum(s[r].nn);
            // a lane's quality sum can pass 32 bits (a read of hundreds of MB): 28 low bits and the rest apart
            const uint64_t qsum = (uint64_t)row_sum((uint32_t)s[r].qsum & 0x0FFFFFFFu) + ((uint64_t)row_sum((uint32_t)(s[r].qsum >> 28)) << 28);
            const uint32_t i = sub - (uint32_t)r * QD_QS_COUNTERS;
            if (i == QD_QS_RECORDS) v = valid ? 1 : 0;
            if (i == QD_QS_BASES) v = len[r];
            if (i == QD_QS_QUAL_SUM) v = qsum;
            if (i == QD_QS_Q20) v = q20;
            if (i == QD_QS_Q30) v = q30;
            if (i == QD_QS_N) v = nn;
        }
        table.add(d, sub, v, valid && sub < QD_QS_VALUES, len[0] <= QS_LDS_MAX_LEN && len[1] <= QS_LDS_MAX_LEN);
    }
    table.flush();
}

}  // namespace

hipError_t qd_qstats_launch(const qd_qstats_args& a, uint32_t n_samples, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || n_samples > QD_MAX_SAMPLES) return hipErrorInvalidValue;
    const uint32_t grid = (n + QS_WG_PAIRS - 1) / QS_WG_PAIRS;
    if (qd_qstats_path(n_samples) == QD_QS_PATH_LDS)
        hipLaunchKernelGGL(qstats<true>, dim3(grid), dim3(QS_BLOCK), qd_qstats_values(n_samples) * 4, st, a, n_samples, n);
    else
        hipLaunchKernelGGL(qstats<false>, dim3(grid), dim3(QS_BLOCK), 0, st, a, n_samples, n);
    return hipGetLastError();
}
