// gfx950 (CDNA4 / MI355X): the duplication report's tally (qd_dup_set) -- the read-pair keys of a batch counted in a device-resident
// hash table while the batch's text sits in HBM.  quade_dup.h has the definition; three kernels per batch on one stream:
//   dup_keys  : one pass over the pairs, 16 lanes (one DPP row) per pair as in the other counting stages (quade_row.h), so that the
//               per-destination counters go through DestTable.  Only six lanes of a row load: the first 32 bases of a read lie in at
//               most three aligned 16-byte words, lanes 0 .. 2 take R1's and lanes 8 .. 10 R2's.  Each turns its 16 bytes into 16
//               2-bit codes and 16 "invalid" bits (SWAR), lane 0 / 8 collects the three words of its read over DPP, shifts the line's
//               offset out and masks to B bases; lane 0 then holds (w1, w2, d), classifies the pair, hashes the key and decides
//               whether it is in the sample.  The sampled pairs of a wave take their places in the workgroup's LDS list with one
//               LDS atomic; the workgroup reserves its room in the batch list with one global atomic and copies its keys out.
//   dup_claim : one lane per listed pair, quade_tally.h's claim (tag CAS at agent scope, the installing lane writes the key words
//               with plain vector stores); the slot found is left in the list's `where`.
//   dup_count : a launch of its own, so that the key stores are visible to every XCD at the kernel boundary.  Each lane compares its
//               key with the entry's; equal slots are combined in the wave and in the workgroup's LDS hash; a pair without an
//               entry, or whose tag belongs to another key, adds to its destination's not_tallied.
// The claim and the count are grid-stride loops bounded by the list's own length on the device: nothing is read back.
// Launches on different streams are ordered by the caller as the unknown tally's are (an event behind dup_count that the next
// launch's stream waits for before its dup_claim).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "quade_row.h"
#include "quade_tally.h"
#include "quade_dup.h"

namespace {

constexpr uint32_t DK_BLOCK = 256;
constexpr uint32_t DK_GROUPS = DK_BLOCK / ROW;  // pairs per step of a workgroup
constexpr uint32_t DK_WG_PAIRS = 512;           // pairs per workgroup: the stage is bound by latency, not by bytes -- more workgroups
constexpr uint32_t DK_WORDS = 3;                // aligned words that hold a read's first 32 bases at any offset
static_assert(QD_DUP_LDS_MAX_DEST * QD_DP_VALUES * 4 + DK_WG_PAIRS * QD_DUP_KEY_WORDS * 8 + 64 <= 65536, "the LDS partials and the workgroup's keys exceed 64 KiB");
static_assert(DK_WG_PAIRS % DK_GROUPS == 0, "whole steps");
static_assert(QD_DP_VALUES <= ROW / 2 && DK_WORDS <= ROW / 2, "a half row per read");
static_assert(QD_DUP_KEY_WORDS <= QD_KEY_WORDS, "a key fits an entry");

// the 2-bit codes of four bytes, byte i in bits 2 i .. 2 i + 1
__device__ __forceinline__ uint32_t codes4(uint32_t x) {
    const uint32_t t = (x >> 1) & 0x03030303u;
    return (t | (t >> 6) | (t >> 12) | (t >> 18)) & 0xFFu;
}
// bit i: byte i of x, case folded, is none of A, C, G, T
__device__ __forceinline__ uint32_t invalid4(uint32_t x) {
    const uint32_t u = x & 0xDFDFDFDFu;
    const uint32_t ok = bytes_eq(u, 'A') | bytes_eq(u, 'C') | bytes_eq(u, 'G') | bytes_eq(u, 'T');
    const uint32_t m = ~ok & 0x80808080u;
    return ((m >> 7) | (m >> 14) | (m >> 21) | (m >> 28)) & 0xFu;
}

// what a row needs of its pair before it can load text: fetched one step ahead, so that the record, code and reason loads of the
// next pair are in flight while this pair's words are
struct PairIn {
    bool valid;
    uint32_t d, len[2], seq;
};
__device__ __forceinline__ PairIn fetch_pair(const qd_dup_args& a, uint32_t j, uint32_t last, uint32_t r, uint32_t n_samples) {
    PairIn p{false, 0xFFFFFFFFu, {0, 0}, 0};
    if (j < last) {  // (the loads do not wait for the reason byte)
        const uint32_t why = a.drop ? a.drop[j] : 0u;
        const uint32_t l0 = a.recs[0][j].seq_len, l1 = a.recs[1][j].seq_len, seq = a.recs[r][j].seq, c = a.codes[j];
        if (!why) {
            p.valid = true;
            p.len[0] = l0;
            p.len[1] = l1;
            p.seq = seq;
            p.d = c == QD_CODE_UNDETERMINED ? 2 * n_samples : min(c, 2 * n_samples);
        }
    }
    return p;
}

template <bool LDS>
__global__ __launch_bounds__(DK_BLOCK) void dup_keys(qd_dup_args a, qd_dup_dev P, uint32_t n_samples, uint32_t n) {
    extern __shared__ uint32_t part[];  // LDS path: [n_dest][QD_DP_VALUES]
    __shared__ uint64_t lkeys[DK_WG_PAIRS * QD_DUP_KEY_WORDS];  // the workgroup's sampled keys, until its one reservation in the list
    __shared__ uint32_t lcount, lbase;
    if (threadIdx.x == 0) lcount = 0;
    __syncthreads();
    const uint32_t n_dest = 2 * n_samples + 1;
    const DestTable<LDS, QD_DP_VALUES, DK_BLOCK> table{part, reinterpret_cast<unsigned long long*>(a.table), n_dest * QD_DP_VALUES};
    table.init();
    const uint32_t sub = threadIdx.x & (ROW - 1), group = threadIdx.x / ROW;
    const uint32_t r = sub >> 3, k = sub & 7;  // this lane's read and word
    const int lane = threadIdx.x & 63;
    const uint32_t B = (uint32_t)P.bases;
    const uint64_t wmask = B >= 32 ? ~0ull : (1ull << (2 * B)) - 1, bmask = (1ull << B) - 1;
    const uint32_t first = blockIdx.x * DK_WG_PAIRS, last = min(n, first + DK_WG_PAIRS);
    PairIn next = fetch_pair(a, first + group, last, r, n_samples);
    for (uint32_t j0 = first; j0 < last; j0 += DK_GROUPS) {  // (the same trips for every wave: DPP and the ballots need whole waves)
        const PairIn cur = next;
        next = fetch_pair(a, j0 + DK_GROUPS + group, last, r, n_samples);
        const bool valid = cur.valid;
        const uint32_t d = cur.d, seq = cur.seq, len[2] = {cur.len[0], cur.len[1]};
        const Line line = make_line(a.text[r], seq, len[r]);
        uint4 w = make_uint4(0, 0, 0, 0);
        if (valid && k < DK_WORDS && k < line.n_words) w = line.w0[k];  // a whole aligned word that holds bytes of the line
        const uint32_t c0 = codes4(w.x) | (codes4(w.y) << 8) | (codes4(w.z) << 16) | (codes4(w.w) << 24);
        const uint32_t b0 = invalid4(w.x) | (invalid4(w.y) << 4) | (invalid4(w.z) << 8) | (invalid4(w.w) << 12);
        // lanes 0 and 8: the read's three words (row_shl 1 and 2), the line's offset shifted out, B bases kept.  When the read has
        // B bases or more every word that holds one of them was loaded; a shorter read makes the pair `short` whatever is here
        const uint32_t c1 = dpp<0x101, true>(c0), c2 = dpp<0x102, true>(c0);
        const uint32_t b1 = dpp<0x101, true>(b0), b2 = dpp<0x102, true>(b0);
        const uint32_t s = line.s;
        uint64_t key = ((uint64_t)c0 | ((uint64_t)c1 << 32)) >> (2 * s);
        if (s) key |= (uint64_t)c2 << (64 - 2 * s);
        key &= wmask;
        const uint32_t bad = (uint32_t)(((((uint64_t)b0) | ((uint64_t)b1 << 16) | ((uint64_t)b2 << 32)) >> s) & bmask);
        // lane 0: both reads (row_shl 8)
        const uint64_t key2 = dpp<0x108, true>(key);
        const uint32_t bad2 = dpp<0x108, true>(bad);
        const bool is_short = len[0] < B || len[1] < B;
        const bool with_n = !is_short && (bad | bad2) != 0;
        const uint64_t k4[QD_KEY_WORDS] = {key, key2, d, 0};
        const uint64_t h = qd_uk_tag(k4);
        const bool sampled = !is_short && !with_n && (P.sample_lg == 0 || (h >> (64 - P.sample_lg)) == 0);
        const uint32_t flags = (uint32_t)row_get((int32_t)((is_short ? 1u : 0u) | (with_n ? 2u : 0u) | (sampled ? 4u : 0u)), 0);
        // the wave's sampled pairs take their places among the workgroup's with one LDS atomic
        const bool listed = valid && sub == 0 && sampled;
        const uint64_t m = __ballot(listed);
        if (m) {
            const int leader = __ffsll((unsigned long long)m) - 1;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&lcount, (uint32_t)__popcll(m));
            base = (uint32_t)__shfl((int)base, leader, 64);
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            if (listed && at < DK_WG_PAIRS) {  // (every pair is listed once at most: at < DK_WG_PAIRS always)
                lkeys[at * QD_DUP_KEY_WORDS] = key;
                lkeys[at * QD_DUP_KEY_WORDS + 1] = key2;
                lkeys[at * QD_DUP_KEY_WORDS + 2] = d;
            }
        }
        // the pair's values, value i in lane i of the row
        uint64_t v = 0;
        if (sub == QD_DP_PAIRS) v = 1;
        if (sub == QD_DP_SHORT) v = flags & 1u;
        if (sub == QD_DP_WITH_N) v = (flags >> 1) & 1u;
        if (sub == QD_DP_SAMPLED) v = (flags >> 2) & 1u;
        if (!valid) v = 0;
        table.add(d, sub, v, valid && sub < QD_DP_VALUES, true);
    }
    // the workgroup's keys go to the batch list behind one global atomic, in whole coalesced words
    __syncthreads();
    const uint32_t mine = min(lcount, DK_WG_PAIRS);
    if (threadIdx.x == 0) lbase = mine ? atomicAdd(a.list_n, mine) : 0;
    __syncthreads();
    const uint64_t room = (uint64_t)n * QD_DUP_KEY_WORDS, at0 = (uint64_t)lbase * QD_DUP_KEY_WORDS;  // (the list holds n pairs: never reached)
    for (uint32_t i = threadIdx.x; i < mine * QD_DUP_KEY_WORDS; i += DK_BLOCK)
        if (at0 + i < room) a.list[at0 + i] = lkeys[i];
    table.flush();
}

__device__ __forceinline__ void load_key(const qd_dup_args& a, uint64_t i, uint64_t (&k4)[QD_KEY_WORDS]) {
    const uint64_t* e = a.list + (size_t)i * QD_DUP_KEY_WORDS;
    k4[0] = e[0];
    k4[1] = e[1];
    k4[2] = e[2];
    k4[3] = 0;
}

__global__ __launch_bounds__(UK_BLOCK) void dup_claim(const qd_dup_args a, uint32_t cap) {
    __shared__ uint32_t installs_wg;
    if (threadIdx.x == 0) installs_wg = 0;
    __syncthreads();
    const uint32_t nl = min(a.list_n[0], cap);
    const UnknownTable& t = a.t;
    uint32_t installs = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * UK_BLOCK + threadIdx.x; i < nl; i += (uint64_t)gridDim.x * UK_BLOCK) {
        uint64_t k4[QD_KEY_WORDS];
        load_key(a, i, k4);
        const uint64_t tag = qd_uk_trim(qd_uk_tag(k4), t.tag_mask);
        a.where[i] = tally_claim(t, k4, tag, installs);
    }
    tally_installs(t, installs, &installs_wg);
}

__global__ __launch_bounds__(UK_BLOCK) void dup_count(const qd_dup_args a, uint32_t cap) {
    __shared__ uint32_t lslot[UK_LDS];
    __shared__ uint32_t lcnt[UK_LDS];
    __shared__ uint32_t tallied_wg;
    tally_lds_init(lslot, lcnt);
    if (threadIdx.x == 0) tallied_wg = 0;
    __syncthreads();
    const uint32_t nl = min(a.list_n[0], cap);
    const UnknownTable& t = a.t;
    const int lane = threadIdx.x & 63;
    uint32_t n_tal = 0;
    // the trip count is the same for every lane of the workgroup: the wave-level combining needs whole waves
    for (uint64_t base = (uint64_t)blockIdx.x * UK_BLOCK; base < nl; base += (uint64_t)gridDim.x * UK_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        uint32_t res = QD_UK_SKIP;
        bool pend = false;
        if (i < nl) {
            res = a.where[i];
            uint64_t k4[QD_KEY_WORDS];
            load_key(a, i, k4);
            bool same = false;
            if (res != QD_UK_NONE) {
                const uint64_t* e = t.keys + (size_t)res * QD_KEY_WORDS;
                same = e[0] == k4[0] && e[1] == k4[1] && e[2] == k4[2];
            }
            if (same) {
                pend = true;
                ++n_tal;
            } else {  // no entry within the probe limit, or another key holds this tag's entry (rare: one atomic each)
                atomicAdd(reinterpret_cast<unsigned long long*>(a.table) + (size_t)k4[2] * QD_DP_VALUES + QD_DP_NOT_TALLIED, 1ull);
            }
        }
        tally_combine(lslot, lcnt, t.counts, pend, res, lane);
    }
    n_tal = uk_wave_sum(n_tal);
    if (lane == 0 && n_tal) atomicAdd(&tallied_wg, n_tal);
    __syncthreads();
    tally_lds_flush(lslot, lcnt, t.counts);
    if (threadIdx.x == 0 && tallied_wg)
        atomicAdd(reinterpret_cast<unsigned long long*>(&t.totals[QD_UK_TALLIED]), (unsigned long long)tallied_wg);
}

}  // namespace

hipError_t qd_dup_launch(const qd_dup_dev& P, const qd_dup_args& a, uint32_t n_samples, uint32_t n, int cus, hipEvent_t before_claim,
                         hipStream_t st) {
    if (!n) return hipSuccess;
    if (n > 0x7FFFFFFFu || n_samples > QD_MAX_SAMPLES || P.bases < 8 || P.bases > 32 || P.sample_lg < 0 || P.sample_lg > 10)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.list_n, 0, 4, st);
    if (e != hipSuccess) return e;
    const uint32_t grid = (n + DK_WG_PAIRS - 1) / DK_WG_PAIRS;
    if (qd_dup_path(n_samples) == QD_DUP_PATH_LDS)
        hipLaunchKernelGGL(dup_keys<true>, dim3(grid), dim3(DK_BLOCK), qd_dup_values(n_samples) * 4, st, a, P, n_samples, n);
    else
        hipLaunchKernelGGL(dup_keys<false>, dim3(grid), dim3(DK_BLOCK), 0, st, a, P, n_samples, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (before_claim && (e = hipStreamWaitEvent(st, before_claim, 0)) != hipSuccess) return e;
    // sized by the batch: twice the pairs the sample is expected to hold (the loops are grid-stride: any size is right)
    const int64_t expected = 2 * ((int64_t)n >> P.sample_lg) + UK_BLOCK;
    const unsigned tgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((expected + UK_BLOCK - 1) / UK_BLOCK, (int64_t)cus * 8));
    hipLaunchKernelGGL(dup_claim, dim3(tgrid), dim3(UK_BLOCK), 0, st, a, n);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(dup_count, dim3(tgrid), dim3(UK_BLOCK), 0, st, a, n);
    return hipGetLastError();
}
