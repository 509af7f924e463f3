// gfx950 (CDNA4 / MI355X): adapter content of a batch's insert reads as the scan left them (qd_adapters_set) while their text
// sits in HBM: for up to 16 probes of 12 bases the first position at which each starts in R1 and in R2.  quade_adapters.h states
// the rule and the table.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a read; blockIdx.y says R1 or R2.
//   staging : the sequence line is taken as aligned 16-byte words, one or two per lane, head and tail masked to the line, and packed
//             on the way into the row's slab as quade_screen.hip packs it: per word 16 two-bit codes (the first base in the top
//             bits) and 16 validity bits, side by side in one 64-bit slab word.
//   search  : lane i takes the starts p = i (mod 16), so that the row reads the same two slab words in a step.  The 12 bases from p
//             on are the top 24 bits of two code words shifted left by the offset of p in its word; the validity bits shifted alike
//             say whether all twelve are ACGT (else the word is one no probe has).  The word is compared with the 16 probe words,
//             which sit in scalar registers; a start that equals a probe lowers found[a] of its row in LDS (ds_min_u32).  Hits are
//             rare in a good library and one or two a read in an adapter-dimer run: the common trip is 16 compares and one branch.
//   a line of more than 21 words does not fit its slab: lane i then takes the i-th stretch of starts and rolls the word and the run
//             of valid bases over the bytes in global memory.
//   counting: lane a of the row holds first(a), the row minimum is first(any).  A workgroup keeps 32-bit partials in LDS -- the bins
//             below AD_LDS_BINS of every column's histogram, and the destination rows when the sheet has at most QD_AD_LDS_MAX_DEST
//             destinations -- and flushes the non-zero words once with 64-bit global atomics, so neither a dimer run (every read in
//             one bin) nor the reads column serialises on one global word.  Later bins add to the 64-bit table directly, and so do
//             the destination rows of a larger sheet.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_adapters.h"

namespace {

constexpr uint32_t AD_BLOCK = 512;
constexpr uint32_t AD_GROUPS = AD_BLOCK / ROW;        // reads per step of a workgroup
constexpr uint32_t AD_WG_READS = 2048;                // reads per workgroup
constexpr uint32_t AD_WORDS = SLAB_WORDS;             // packed words of a staged line: a start's 12 bases reach one word ahead
constexpr uint32_t AD_LDS_BINS = 352;                 // histogram bins with an LDS partial: every start of a staged line
constexpr uint32_t AD_NONE = 0xFFFFFFFFu;
constexpr uint32_t AD_WORD_MASK = (1u << (2 * QD_AD_K)) - 1u;
static_assert(AD_WG_READS % AD_GROUPS == 0, "whole steps");
static_assert(AD_WORDS <= 2 * ROW, "two words per lane stage a line");
static_assert(FAST_WORDS * 16 <= AD_LDS_BINS && AD_LDS_BINS < QD_AD_BINS, "a staged line's starts have LDS bins");
static_assert(QD_AD_PROBES == ROW, "lane a of the row holds first(a)");
constexpr uint32_t AD_NO_WORD = 0x80000000u;         // what a start with a byte that is no base compares as
static_assert((QD_AD_NO_PROBE & ~AD_WORD_MASK) != 0 && (AD_NO_WORD & ~AD_WORD_MASK) != 0 && AD_NO_WORD != QD_AD_NO_PROBE,
              "the word of an unused slot and the word of a start without 12 bases equal no probe's word, nor each other");
// per workgroup: histogram partials, the rows' slabs and found words, then (dynamic) the destination partials
static_assert(QD_AD_COLUMNS * AD_LDS_BINS * 4 + AD_GROUPS * AD_WORDS * 8 + AD_GROUPS * ROW * 4 + QD_AD_LDS_MAX_DEST * QD_AD_DEST_COLUMNS * 4 <= 64 * 1024,
              "the LDS of a workgroup exceeds 64 KiB");

// a start whose 12 bases are word w: found[a] of the probe it equals goes down to p (no two probes are equal)
__device__ __forceinline__ void note(const qd_adapters_dev& P, uint32_t w, uint32_t p, uint32_t* found) {
    bool hit = false;
#pragma unroll
    for (uint32_t a = 0; a < QD_AD_PROBES; ++a) hit = hit || w == P.word[a];
    if (hit) {
#pragma unroll
        for (uint32_t a = 0; a < QD_AD_PROBES; ++a)
            if (w == P.word[a]) atomicMin(&found[a], p);
    }
}

// the row packs the line into its slab: (codes << 32) | validity bits for every word k < AD_WORDS, zeros beyond the line
__device__ __forceinline__ void stage_packed(uint2* slab, const Line& L, uint32_t sub) {
    for (uint32_t k = sub; k < AD_WORDS; k += ROW) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < L.n_words) v = mask_word(L, k, L.w0[k]);
        slab[k] = make_uint2((base_codes4(v.x) << 24) | (base_codes4(v.y) << 16) | (base_codes4(v.z) << 8) | base_codes4(v.w),
                             (base_valid4(v.x) << 12) | (base_valid4(v.y) << 8) | (base_valid4(v.z) << 4) | base_valid4(v.w));
    }
}

// a staged line of L bases whose first base sits at offset s of word 0: this lane's starts
__device__ __forceinline__ void search_staged(const uint2* slab, uint32_t s, uint32_t L, const qd_adapters_dev& P, uint32_t* found, uint32_t sub) {
    if (L < QD_AD_K) return;
    const uint32_t npos = L - QD_AD_K + 1;
    for (uint32_t p = sub; p < npos; p += ROW) {
        const uint32_t q = p + s, k0 = q >> 4, o = q & 15u;
        const uint2 lo = slab[k0], hi = slab[k0 + 1];  // k0 + 1 <= FAST_WORDS < AD_WORDS
        const uint32_t vbits = (lo.y << 16) | hi.y;    // 32 bases from word k0 on, the first in bit 31
        const uint64_t codes = ((uint64_t)lo.x << 32) | hi.x;
        uint32_t w = (uint32_t)((codes << (2 * o)) >> (64 - 2 * QD_AD_K));
        if (((vbits << o) >> (32 - QD_AD_K)) != (1u << QD_AD_K) - 1u) w = AD_NO_WORD;  // a byte that is no base
        note(P, w, p, found);
    }
}

// the same over bytes in global memory, for a line that does not fit the slab: the lanes split the starts into 16 contiguous
// stretches and roll the word over the bytes of their stretch
__device__ __forceinline__ void search_bytes(const uint8_t* s, uint32_t L, const qd_adapters_dev& P, uint32_t* found, uint32_t sub) {
    if (L < QD_AD_K) return;
    const uint32_t npos = L - QD_AD_K + 1, per = (npos + ROW - 1) / ROW;
    const uint32_t p0 = min(sub * per, npos), p1 = min(p0 + per, npos);
    if (p0 >= p1) return;
    uint32_t w = 0, run = 0;  // run: valid bases in a row up to and including this one
    for (uint32_t i = p0; i < p1 + QD_AD_K - 1; ++i) {  // i <= npos + 10 = L - 1
        const uint32_t u = s[i] & 0xDFu;
        run = (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? run + 1 : 0;
        w = ((w << 2) | ((u >> 1) & 3u)) & AD_WORD_MASK;
        if (i + 1 >= p0 + QD_AD_K && run >= QD_AD_K) note(P, w, i + 1 - QD_AD_K, found);
    }
}

template <bool LDS_DEST>
__global__ __launch_bounds__(AD_BLOCK) void adapter_scan(qd_adapters_dev P, qd_adapters_args a, uint32_t n_samples, uint32_t n) {
    __shared__ uint32_t hist_part[QD_AD_COLUMNS * AD_LDS_BINS];  // [column][bin]
    __shared__ uint2 slab[AD_GROUPS][AD_WORDS];
    __shared__ uint32_t found_all[AD_GROUPS][ROW];
    extern __shared__ uint32_t dest_part[];  // LDS_DEST: [n_dest][QD_AD_DEST_COLUMNS]
    const uint32_t r = blockIdx.y, n_dest = 2 * n_samples + 1;
    for (uint32_t i = threadIdx.x; i < QD_AD_COLUMNS * AD_LDS_BINS; i += AD_BLOCK) hist_part[i] = 0;
    if (LDS_DEST)
        for (uint32_t i = threadIdx.x; i < n_dest * QD_AD_DEST_COLUMNS; i += AD_BLOCK) dest_part[i] = 0;
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint8_t* text = a.text[r];
    const qd_rec* recs = a.recs[r];
    unsigned long long* const table = reinterpret_cast<unsigned long long*>(a.table);
    unsigned long long* const hist = table + (size_t)r * QD_AD_COLUMNS * QD_AD_BINS;                           // [column][bin]
    unsigned long long* const dest = table + QD_AD_HIST_VALUES + (size_t)r * QD_AD_DEST_COLUMNS;                // row d at d * QD_AD_DEST_VALUES
    uint32_t* const found = found_all[group];
    const uint32_t first = blockIdx.x * AD_WG_READS, last = min(n, first + AD_WG_READS);
    for (uint32_t j0 = first; j0 < last; j0 += AD_GROUPS) {  // (the same trips for every wave: barriers inside)
        const uint32_t j = j0 + group;
        const bool valid = j < last;
        uint32_t seq = 0, L = 0, d = 0;
        if (valid) {
            const qd_rec* rec = recs + j;
            seq = rec->seq;
            L = rec->seq_len;
            const uint32_t c = a.codes[j];
            d = c == QD_CODE_UNDETERMINED ? 2 * n_samples : min(c, 2 * n_samples);
        }
        const Line line = make_line(text, seq, L);
        const bool staged = line.n_words <= FAST_WORDS;
        __syncthreads();  // the row's earlier read is done with the slab (and the partials are zero)
        if (staged) stage_packed(slab[group], line, sub);
        found[sub] = AD_NONE;
        __syncthreads();
        if (staged) search_staged(slab[group], line.s, L, P, found, sub);
        else search_bytes(text + seq, L, P, found, sub);
        __syncthreads();
        const uint32_t mine = found[sub];       // first(sub), AD_NONE: none
        const uint32_t any = row_min(mine);
        if (valid) {
            // column `sub`, and in lane 0 the reads and column any besides
            if (mine != AD_NONE) {
                const uint32_t bin = min(mine, QD_AD_BINS - 1);
                if (bin < AD_LDS_BINS) atomicAdd(&hist_part[sub * AD_LDS_BINS + bin], 1u);
                else atomicAdd(&hist[(size_t)sub * QD_AD_BINS + bin], 1ull);
                if (LDS_DEST) atomicAdd(&dest_part[d * QD_AD_DEST_COLUMNS + 1 + sub], 1u);
                else atomicAdd(&dest[(size_t)d * QD_AD_DEST_VALUES + 1 + sub], 1ull);
            }
            if (sub == 0) {
                if (LDS_DEST) atomicAdd(&dest_part[d * QD_AD_DEST_COLUMNS], 1u);
                else atomicAdd(&dest[(size_t)d * QD_AD_DEST_VALUES], 1ull);
                if (any != AD_NONE) {
                    const uint32_t bin = min(any, QD_AD_BINS - 1);
                    if (bin < AD_LDS_BINS) atomicAdd(&hist_part[QD_AD_PROBES * AD_LDS_BINS + bin], 1u);
                    else atomicAdd(&hist[(size_t)QD_AD_PROBES * QD_AD_BINS + bin], 1ull);
                    if (LDS_DEST) atomicAdd(&dest_part[d * QD_AD_DEST_COLUMNS + 1 + QD_AD_PROBES], 1u);
                    else atomicAdd(&dest[(size_t)d * QD_AD_DEST_VALUES + 1 + QD_AD_PROBES], 1ull);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < QD_AD_COLUMNS * AD_LDS_BINS; i += AD_BLOCK) {
        const uint32_t v = hist_part[i];
        if (v) atomicAdd(&hist[(size_t)(i / AD_LDS_BINS) * QD_AD_BINS + i % AD_LDS_BINS], (unsigned long long)v);
    }
    if (LDS_DEST)
        for (uint32_t i = threadIdx.x; i < n_dest * QD_AD_DEST_COLUMNS; i += AD_BLOCK) {
            const uint32_t v = dest_part[i];
            if (v) atomicAdd(&dest[(size_t)(i / QD_AD_DEST_COLUMNS) * QD_AD_DEST_VALUES + i % QD_AD_DEST_COLUMNS], (unsigned long long)v);
        }
}

}  // namespace

hipError_t qd_adapters_launch(const qd_adapters_dev& P, const qd_adapters_args& a, uint32_t n_samples, uint32_t n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || n_samples > QD_MAX_SAMPLES || !P.n_probes || P.n_probes > QD_AD_PROBES) return hipErrorInvalidValue;
    for (uint32_t i = 0; i < QD_AD_PROBES; ++i)
        if (i < P.n_probes ? (P.word[i] & ~AD_WORD_MASK) != 0 : P.word[i] != QD_AD_NO_PROBE) return hipErrorInvalidValue;
    const uint32_t grid = (n + AD_WG_READS - 1) / AD_WG_READS, n_dest = 2 * n_samples + 1;
    if (n_dest <= QD_AD_LDS_MAX_DEST)
        hipLaunchKernelGGL(adapter_scan<true>, dim3(grid, 2), dim3(AD_BLOCK), n_dest * QD_AD_DEST_COLUMNS * 4, st, P, a, n_samples, n);
    else
        hipLaunchKernelGGL(adapter_scan<false>, dim3(grid, 2), dim3(AD_BLOCK), 0, st, P, a, n_samples, n);
    return hipGetLastError();
}
