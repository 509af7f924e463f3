// gfx950 (CDNA4 / MI355X): the k-mer screen of a batch's insert reads against a reference (qd_screen_set) while their text sits in
// HBM: hits per read, a flag byte per pair and eight counters per destination.  quade_screen.h states the rule and the table.
//
// Shape (quade_row.h's searching stage): 16 lanes (one DPP row) share a pair; a workgroup of 1024 lanes holds 64 pairs per step and
// strides over the batch, so that the LDS path loads the reference's hash table once per workgroup.
//   staging : each of the pair's two sequence lines is taken as aligned 16-byte words, one or two per lane, head and tail masked to
//             the line, and packed on the way into the row's slab: per word 16 two-bit codes (the first base in the top bits) and
//             16 validity bits.  192 bytes of slab per line instead of 352 of text, and no byte is looked at twice.
//   hot loop: lane i takes the positions p = i (mod 16).  The k-mer's window is three consecutive code words of the slab: shifted
//             left by the offset of p in its word, the top 2 k bits are the forward word w; the bit pairs of w reversed (v_bfrev and
//             one swap of neighbours) and ^ 0xAAAA... are rc; the validity bits shifted alike say whether the k-mer exists.  The
//             canonical word min(w, rc) is looked up in an open-addressing table of 64-bit words, linear probing from
//             qd_screen_slot, until the word or the empty slot (all ones) is met; the table is at most half full.
//   LDS     : the table is the workgroup's dynamic LDS (128 KiB, copied from global memory before the first pair).
//   GLOBAL  : the table stays in global memory; the same probe.
// A line of more than 21 words does not fit its slab: every lane then takes a contiguous stretch of the positions and rolls w and
// rc over the bytes in global memory.  The pair's eight values go to the destination's row by DestTable's !LDS form: with the
// hash table in LDS the destination partials do not also fit.
#include <hip/hip_runtime.h>

#include "quade_row.h"
#include "quade_screen.h"

namespace {

constexpr uint32_t SC_BLOCK = 1024;
constexpr uint32_t SC_GROUPS = SC_BLOCK / ROW;  // pairs per step of a workgroup
constexpr uint32_t SC_WORDS = 24;               // packed words of a staged line: FAST_WORDS and the two a window reaches beyond them
constexpr uint32_t SC_LDS_TABLE_BYTES = 8u << QD_SC_LDS_SLOTS_LG;
static_assert(FAST_WORDS + 2 <= SC_WORDS && SC_WORDS <= 2 * ROW, "a window of three words stays inside the slab; two words per lane stage it");
static_assert(SC_GROUPS * 2 * 2 * SC_WORDS * 4 + SC_LDS_TABLE_BYTES <= 160 * 1024, "slabs and hash table exceed the CU's LDS");
static_assert(QD_SC_VALUES <= ROW, "one lane per value");

// the row packs the line (base_codes4 and base_valid4: quade_row.h) into its slab: codes[k] and valid[k] for every word k < SC_WORDS, zeros beyond the line
__device__ __forceinline__ void stage_packed(uint32_t* codes, uint32_t* valid, const Line& L, uint32_t sub) {
    for (uint32_t k = sub; k < SC_WORDS; k += ROW) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (k < L.n_words) v = mask_word(L, k, L.w0[k]);
        codes[k] = (base_codes4(v.x) << 24) | (base_codes4(v.y) << 16) | (base_codes4(v.z) << 8) | base_codes4(v.w);
        valid[k] = (base_valid4(v.x) << 12) | (base_valid4(v.y) << 8) | (base_valid4(v.z) << 4) | base_valid4(v.w);
    }
}

// the forward word's reverse complement: bit pairs reversed, moved down to 2 k bits, every code ^ 2
__device__ __forceinline__ uint64_t revcomp(uint64_t w, uint32_t k, uint64_t mask) {
    const uint64_t r = __brevll(w);
    const uint64_t pairs = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
    return (pairs >> (64 - 2 * k)) ^ (mask & 0xAAAAAAAAAAAAAAAAull);
}

// whether the canonical word is in the table (at most half full, so an empty slot ends every chain; the trip bound only keeps a
// damaged table from holding the lane)
__device__ __forceinline__ bool in_table(const uint64_t* tab, uint32_t slots_lg, uint64_t word) {
    const uint32_t mask = (1u << slots_lg) - 1u;
    uint32_t slot = qd_screen_slot(word, slots_lg);
    for (uint32_t i = 0; i <= mask; ++i) {
        const uint64_t v = tab[slot];
        if (v == word) return true;
        if (v == QD_SC_EMPTY) return false;
        slot = (slot + 1) & mask;
    }
    return false;
}

// a staged line of L bases whose first base sits at offset s of word 0: this lane's positions -> (k-mers that exist << 32) | hits
__device__ __forceinline__ uint64_t screen_staged(const uint32_t* codes, const uint32_t* valid, uint32_t s, uint32_t L, const qd_screen_dev& P,
                                                  const uint64_t* tab, uint32_t sub) {
    if (L < P.k) return 0;
    const uint32_t k = P.k, npos = L - k + 1;
    const uint64_t mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1ull;
    const uint32_t all = k == 32 ? 0xFFFFFFFFu : (1u << k) - 1u;
    uint64_t found = 0;
    for (uint32_t p = sub; p < npos; p += ROW) {
        const uint32_t q = p + s, k0 = q >> 4, o = q & 15u;
        const uint64_t vbits = ((uint64_t)valid[k0] << 32) | ((uint64_t)valid[k0 + 1] << 16) | valid[k0 + 2];  // 48 bases from word k0 on
        if (((uint32_t)((vbits << o) >> 16) >> (32 - k)) != all) continue;
        const uint64_t hi = ((uint64_t)codes[k0] << 32) | codes[k0 + 1];
        const uint64_t x = o ? (hi << (2 * o)) | ((uint64_t)codes[k0 + 2] >> (32 - 2 * o)) : hi;  // 32 bases from q on
        const uint64_t w = x >> (64 - 2 * k), rc = revcomp(w, k, mask);
        found += (1ull << 32) + (in_table(tab, P.slots_lg, w < rc ? w : rc) ? 1u : 0u);
    }
    return found;
}

// the same over bytes in global memory, for a line that does not fit the slab: the lanes split the positions into 16 contiguous
// stretches and roll the two words over the bytes of their stretch
__device__ __forceinline__ uint64_t screen_bytes(const uint8_t* s, uint32_t L, const qd_screen_dev& P, const uint64_t* tab, uint32_t sub) {
    if (L < P.k) return 0;
    const uint32_t k = P.k, npos = L - k + 1, per = (npos + ROW - 1) / ROW;
    const uint32_t p0 = min(sub * per, npos), p1 = min(p0 + per, npos);
    if (p0 >= p1) return 0;
    const uint64_t mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1ull;
    uint64_t w = 0, rc = 0, found = 0;
    uint32_t run = 0;  // valid bases in a row up to and including this one
    for (uint32_t i = p0; i < p1 + k - 1; ++i) {
        const uint32_t u = s[i] & 0xDFu, c = (u >> 1) & 3u;
        run = (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? run + 1 : 0;
        w = ((w << 2) | c) & mask;
        rc = (rc >> 2) | ((uint64_t)(c ^ 2u) << (2 * (k - 1)));
        if (i + 1 >= p0 + k && run >= k) found += (1ull << 32) + (in_table(tab, P.slots_lg, w < rc ? w : rc) ? 1u : 0u);
    }
    return found;
}

template <bool LDS>
__global__ __launch_bounds__(SC_BLOCK) void screen_pairs(qd_screen_dev P, qd_screen_args a, uint32_t n_samples, uint32_t n) {
    extern __shared__ uint4 lds_table[];                    // LDS path: the hash table, 1 << QD_SC_LDS_SLOTS_LG words
    __shared__ uint32_t slab[SC_GROUPS][2][2][SC_WORDS];    // per row and read: packed codes, validity bits
    if (LDS) {
        const uint4* src = reinterpret_cast<const uint4*>(a.slots);
        for (uint32_t i = threadIdx.x; i < SC_LDS_TABLE_BYTES / 16; i += SC_BLOCK) lds_table[i] = src[i];
        __syncthreads();
    }
    const uint64_t* tab = LDS ? reinterpret_cast<const uint64_t*>(lds_table) : a.slots;
    const DestTable<false, QD_SC_VALUES, SC_BLOCK> table{nullptr, reinterpret_cast<unsigned long long*>(a.table), 0};
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    for (uint32_t j0 = blockIdx.x * SC_GROUPS; j0 < n; j0 += gridDim.x * SC_GROUPS) {  // (the same trips for every wave: barriers inside)
        const uint32_t j = j0 + group;
        const bool valid = j < n;
        uint32_t skip = 0;
        if (valid && a.drop_in) skip = a.drop_in[j];
        const bool active = valid && !skip;
        uint32_t d = 0xFFFFFFFFu, len[2] = {0, 0}, seq[2] = {0, 0};
        if (active) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const qd_rec* rec = a.recs[r] + j;
                seq[r] = rec->seq;
                len[r] = rec->seq_len;
            }
            const uint32_t c = a.codes[j];
            d = c == QD_CODE_UNDETERMINED ? 2 * n_samples : min(c, 2 * n_samples);
        }
        Line line[2];
        bool staged[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            line[r] = make_line(a.text[r], seq[r], len[r]);
            staged[r] = line[r].n_words <= FAST_WORDS;
        }
        __syncthreads();  // the row's earlier pair is done with the slabs
#pragma unroll
        for (int r = 0; r < 2; ++r)
            if (staged[r]) stage_packed(slab[group][r][0], slab[group][r][1], line[r], sub);
        __syncthreads();
        uint32_t hits[2], kmers[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint64_t f = staged[r] ? screen_staged(slab[group][r][0], slab[group][r][1], line[r].s, len[r], P, tab, sub)
                                         : screen_bytes(a.text[r] + seq[r], len[r], P, tab, sub);
            const uint64_t t = row_sum(f);
            hits[r] = (uint32_t)t;
            kmers[r] = (uint32_t)(t >> 32);
        }
        const bool matched = active && hits[0] + hits[1] >= P.min_hits;
        if (valid && sub == 0) {
            if (a.hits) {
                a.hits[2 * (size_t)j] = hits[0];
                a.hits[2 * (size_t)j + 1] = hits[1];
            }
            if (a.flag) a.flag[j] = (uint8_t)(skip ? skip : matched && P.action == QD_SC_DROP ? QD_SC_DROPPED : 0u);
        }
        // the pair's 8 values, value i in lane i of the row
        const uint64_t bases = (uint64_t)len[0] + len[1];
        uint64_t v = 0;
        if (sub == QD_SC_PAIRS) v = 1;
        else if (sub == QD_SC_MATCHED) v = matched;
        else if (sub == QD_SC_R1_HIT) v = hits[0] > 0;
        else if (sub == QD_SC_R2_HIT) v = hits[1] > 0;
        else if (sub == QD_SC_KMERS) v = (uint64_t)kmers[0] + kmers[1];
        else if (sub == QD_SC_HIT_KMERS) v = (uint64_t)hits[0] + hits[1];
        else if (sub == QD_SC_BASES_IN) v = bases;
        else if (sub == QD_SC_BASES_MATCHED) v = matched ? bases : 0;
        const bool mine = active && sub < QD_SC_VALUES;
        if (!mine) v = 0;
        table.add(d, sub, v, mine, false);
    }
}

}  // namespace

hipError_t qd_screen_launch(const qd_screen_dev& P, const qd_screen_args& a, uint32_t n_samples, uint32_t n, int path, uint32_t cus,
                            hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || n_samples > QD_MAX_SAMPLES || P.k < QD_SC_MIN_K || P.k > QD_SC_MAX_K || P.slots_lg < QD_SC_MIN_SLOTS_LG ||
        P.slots_lg > 23 || !a.slots || (path == QD_SC_PATH_LDS && P.slots_lg != QD_SC_LDS_SLOTS_LG))
        return hipErrorInvalidValue;
    const uint32_t steps = (n + SC_GROUPS - 1) / SC_GROUPS;
    if (!cus) cus = 256;
    if (path == QD_SC_PATH_LDS) {  // one workgroup per CU: its LDS holds one table
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(screen_pairs<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)SC_LDS_TABLE_BYTES);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(screen_pairs<true>, dim3(min(steps, cus)), dim3(SC_BLOCK), SC_LDS_TABLE_BYTES, st, P, a, n_samples, n);
    } else {
        hipLaunchKernelGGL(screen_pairs<false>, dim3(min(steps, 2 * cus)), dim3(SC_BLOCK), 0, st, P, a, n_samples, n);
    }
    return hipGetLastError();
}
