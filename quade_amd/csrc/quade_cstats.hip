// gfx950 (CDNA4 / MI355X): per-cycle quality and base content and the per-read distributions (qd_cstats_enable), one pass
// over the sequence and quality lines of a batch's insert reads while their text sits in HBM.  The definition of every
// counter: quade_cstats.h.
//
// Shape (quade_row.h's counting stage; quade_qstats.hip reads the same four lines): 16 lanes (one DPP row) share a pair.  Each of
// the pair's four lines is read one aligned word per lane, head and tail masked (a masked byte is zero: no letter,
// ph = 0, so it adds nothing); the first word of all four lines is in flight together.  A lane walks the 16 bytes of its
// word: byte i of word k of a line that starts s bytes into its first word is cycle c = 16 k + i - s.
//
// Accumulation (this stage's own, see quade_row.h): a workgroup keeps 32-bit partials in LDS and flushes the non-zero words once, with 64-bit global atomics:
//   cycles c < QD_CS_LDS_CYCLES   [g][r][counter][c & 15][c >> 4]   (see below)
//   every per-read histogram bin  [g][r][len 1025 | meanq 94 | gc 101]
// so a read within the LDS range costs no global atomic at all, and the one length of a run is an LDS word.  Cycles from
// QD_CS_LDS_CYCLES to QD_CS_CYCLES - 1 add to the 64-bit table directly; later ones count in the per-read values only.
//
// LDS layout.  In step i the 16 lanes of a row add to cycles 16 k + i - s for k = lane: a stride of 16 words.  With
// [counter][cycle] that is banks 16 k mod 32 -- two banks, an 8-way conflict (LDS atomics take the 32-bank rule of the
// writes, groups = the wave's two 32-lane halves).  Stored by column instead, word (c & 15) * (QD_CS_LDS_CYCLES / 16) +
// (c >> 4) of a counter, the row's lanes fall on 16 consecutive words whatever the counter (every counter's array starts
// at a multiple of 32 words): no conflict inside a row; the two rows of a half can meet, which is 2-way at most.
//
// 90 720 bytes of LDS: more than 64 KiB, so the kernel opts in (dynamic LDS) and one workgroup of 1 024 lanes lives on a
// CU: 16 waves per CU, 4 per SIMD.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_cstats.h"

namespace {

constexpr uint32_t CS_BLOCK = 1024;
constexpr uint32_t CS_GROUPS = CS_BLOCK / ROW;       // pairs per step of a workgroup
constexpr uint32_t CS_WG_PAIRS = 4096;               // pairs per workgroup
constexpr uint32_t CS_MAX_Q = 255 - 33;
constexpr uint32_t CS_COLS = QD_CS_LDS_CYCLES / 16;  // words per (c & 15) column
constexpr uint32_t CS_HIST = QD_CS_LEN_BINS + QD_CS_MEANQ_BINS + QD_CS_GC_BINS;  // per (g, r)
constexpr uint32_t CS_CYC_WORDS = QD_CS_GROUPS * 2 * QD_CS_COUNTERS * QD_CS_LDS_CYCLES;
constexpr uint32_t CS_LDS_WORDS = CS_CYC_WORDS + QD_CS_GROUPS * 2 * CS_HIST;
// the largest 32-bit partial is a cycle's qual_sum when every pair of the workgroup falls into one group (one add per read
// and cycle, whatever the read's length); a histogram bin holds a workgroup's pairs at most
static_assert((uint64_t)CS_WG_PAIRS * CS_MAX_Q <= 0xFFFFFFFFull, "a workgroup's LDS partials can overflow");
static_assert(CS_LDS_WORDS * 4 <= 160 * 1024, "the LDS partials exceed a CU's LDS");
static_assert(CS_WG_PAIRS % CS_GROUPS == 0 && QD_CS_LDS_CYCLES % 32 == 0, "whole steps; counter arrays start at bank 0");

// where the counters of one (g, r) live
struct Sink {
    uint32_t* lds;                // [QD_CS_COUNTERS][QD_CS_LDS_CYCLES], by column
    unsigned long long* table;    // cycle[QD_CS_CYCLES][QD_CS_COUNTERS]
};
__device__ __forceinline__ void add_cycle(const Sink& k, uint32_t counter, uint32_t c, uint32_t v) {
    if (c < QD_CS_LDS_CYCLES) atomicAdd(&k.lds[counter * QD_CS_LDS_CYCLES + (c & 15u) * CS_COLS + (c >> 4)], v);
    else if (c < QD_CS_CYCLES) atomicAdd(&k.table[(size_t)c * QD_CS_COUNTERS + counter], (unsigned long long)v);
}

// the letters by (u >> 1) & 7 of u = s & 0xDF: A 0, C 1, T 2, G 3, N 7; the byte each slot expects (0xFF: none, u has bit 5
// clear) and the counter it feeds
constexpr uint64_t CS_LETTER = 0x4EFFFFFF47544341ull;
constexpr uint32_t CS_COUNTER = 0x40002310u;

// the 16 bytes of a masked sequence word whose byte 0 is cycle c0 (mod 2^32; a byte before the line is zero and adds nothing)
__device__ __forceinline__ void add_seq(uint4 v, uint32_t c0, const Sink& k, uint32_t& gc) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t u = (w[i >> 2] >> (8 * (i & 3))) & 0xDFu, h = (u >> 1) & 7u;
        if ((uint32_t)(CS_LETTER >> (8 * h) & 0xFFu) == u) {
            const uint32_t counter = (CS_COUNTER >> (4 * h)) & 7u;
            gc += (counter == QD_CS_C || counter == QD_CS_G) ? 1u : 0u;
            add_cycle(k, counter, c0 + i, 1u);
        }
    }
}
__device__ __forceinline__ void add_qual(uint4 v, uint32_t c0, const Sink& k, uint64_t& qsum) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t q = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        if (q > 33u) {
            const uint32_t ph = q - 33u;
            sum += ph;
            add_cycle(k, QD_CS_QUAL_SUM, c0 + i, ph);
            if (ph >= 20u) add_cycle(k, QD_CS_Q20, c0 + i, 1u);
            if (ph >= 30u) add_cycle(k, QD_CS_Q30, c0 + i, 1u);
        }
    }
    qsum += sum;
}

__global__ __launch_bounds__(CS_BLOCK) void cstats(qd_cstats_args a, uint32_t n) {
    extern __shared__ uint32_t part[];  // cycles [g][r][counter][column][row], then histograms [g][r][len | meanq | gc]
    for (uint32_t i = threadIdx.x; i < CS_LDS_WORDS; i += CS_BLOCK) part[i] = 0;
    __syncthreads();
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint32_t first = blockIdx.x * CS_WG_PAIRS, last = min(n, first + CS_WG_PAIRS);
    for (uint32_t j0 = first; j0 < last; j0 += CS_GROUPS) {  // (the same trips for every wave: the DPP sums need whole waves)
        const uint32_t j = j0 + group;
        const bool valid = j < last && !(a.drop && a.drop[j]);
        uint32_t g = 0, len[2] = {0, 0};
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
            g = c == QD_CODE_UNDETERMINED ? 2u : (c & 1u);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = sub < line[q].n_words ? line[q].w0[sub] : make_uint4(0, 0, 0, 0);  // four loads in flight
#pragma unroll
        for (uint32_t r = 0; r < 2; ++r) {
            const uint32_t gr = g * 2 + r;
            Sink k;
            k.lds = part + gr * (QD_CS_COUNTERS * QD_CS_LDS_CYCLES);
            k.table = reinterpret_cast<unsigned long long*>(a.table) + (size_t)gr * QD_CS_GR_VALUES;
            const Line& ls = line[2 * r];
            const Line& lq = line[2 * r + 1];
            uint32_t gc = 0;
            uint64_t qsum = 0;
            if (sub < ls.n_words) add_seq(mask_word(ls, sub, w[2 * r]), 16 * sub - ls.s, k, gc);
            if (sub < lq.n_words) add_qual(mask_word(lq, sub, w[2 * r + 1]), 16 * sub - lq.s, k, qsum);
            for (uint32_t i = sub + ROW; i < ls.n_words; i += ROW)  // reads longer than 241 .. 256 bases
                add_seq(mask_word(ls, i, ls.w0[i]), 16 * i - ls.s, k, gc);
            for (uint32_t i = sub + ROW; i < lq.n_words; i += ROW)
                add_qual(mask_word(lq, i, lq.w0[i]), 16 * i - lq.s, k, qsum);
            // the read's own values, in every lane of the row
            gc = row_sum(gc);
            // a lane's quality sum can pass 32 bits (a read of hundreds of MB): 28 low bits and the rest apart
            const uint64_t qs = (uint64_t)row_sum((uint32_t)qsum & 0x0FFFFFFFu) + ((uint64_t)row_sum((uint32_t)(qsum >> 28)) << 28);
            const uint32_t L = len[r];
            uint32_t* hist = part + CS_CYC_WORDS + gr * CS_HIST;
            if (valid) {  // one LDS add per bin, three lanes
                if (sub == 0) atomicAdd(&hist[min(L, (uint32_t)QD_CS_LEN_BINS - 1)], 1u);
                if (sub == 1 && L) atomicAdd(&hist[QD_CS_LEN_BINS + (uint32_t)min((uint64_t)QD_CS_MEANQ_BINS - 1, qs / L)], 1u);
                if (sub == 2 && L) atomicAdd(&hist[QD_CS_LEN_BINS + QD_CS_MEANQ_BINS + (uint32_t)(100ull * gc / L)], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* table = reinterpret_cast<unsigned long long*>(a.table);
    for (uint32_t i = threadIdx.x; i < CS_LDS_WORDS; i += CS_BLOCK) {
        const uint32_t v = part[i];
        if (!v) continue;
        size_t at;
        if (i < CS_CYC_WORDS) {
            const uint32_t gr = i / (QD_CS_COUNTERS * QD_CS_LDS_CYCLES), rest = i % (QD_CS_COUNTERS * QD_CS_LDS_CYCLES);
            const uint32_t counter = rest / QD_CS_LDS_CYCLES, t = rest % QD_CS_LDS_CYCLES;
            const uint32_t c = (t % CS_COLS) * 16 + t / CS_COLS;
            at = (size_t)gr * QD_CS_GR_VALUES + (size_t)c * QD_CS_COUNTERS + counter;
        } else {
            const uint32_t h = i - CS_CYC_WORDS;
            at = (size_t)(h / CS_HIST) * QD_CS_GR_VALUES + (size_t)QD_CS_CYCLES * QD_CS_COUNTERS + h % CS_HIST;
        }
        atomicAdd(table + at, (unsigned long long)v);
    }
}

}  // namespace

hipError_t qd_cstats_launch(const qd_cstats_args& a, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu) return hipErrorInvalidValue;
    constexpr size_t lds = (size_t)CS_LDS_WORDS * 4;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cstats), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const uint32_t grid = (n + CS_WG_PAIRS - 1) / CS_WG_PAIRS;
    hipLaunchKernelGGL(cstats, dim3(grid), dim3(CS_BLOCK), lds, st, a, n);
    return hipGetLastError();
}
