// Device-only helpers of the stages that walk a batch's insert reads with 16 lanes (one DPP row) per read or pair:
// quade_trim.hip, quade_clip.hip, quade_pairtrim.hip, quade_posttrim.hip, quade_qstats.hip, quade_filter.hip, quade_cstats.hip,
// quade_screen.hip and quade_adapters.hip (which two pack the line to two bits a base on its way into the slab).
//
// The shared shape.  A record's line lies anywhere in the batch's text; a Line is the 16-byte aligned words that hold it, so that
// every load is a whole uint4 whatever the line's offset.  Two ways to take the words:
//   counting stages (qstats, filter, cstats): lane i of the row loads word i (256 bytes per step), the head and the tail word
//       are masked to the line (mask_word) and the bytes are counted four at a time in 32-bit words (the SWAR predicates below);
//   searching stages (trim, clip, pairtrim): the row copies the words, one or two per lane, into a slab of LDS of its own
//       (stage_line), after which every lane reaches any offset of the line; a line of more than FAST_WORDS words does not fit
//       and the stage falls back to bytes in global memory.
// Results go over the row with DPP (row_all and what is built on it), and into the stage's 64-bit table by one of two tails:
//   flush_row_counters: lane i of every row has summed counter i in a register; an LDS partial per counter, then one 64-bit
//       atomic per counter and workgroup (trim, clip, and pairtrim's scalars; pairtrim's histogram stays in its file);
//   DestTable: a table with a row of VALUES per destination, value i in lane i; 32-bit LDS partials per destination where they
//       fit, else the wave's four rows merged by destination and added globally (qstats, filter).
// cstats keeps its own tail: its partials are laid out by cycle column for the LDS banks, which no other stage shares.
//
// Everything here is __device__ __forceinline__ in an unnamed namespace, as the kernels' own helpers are.
#ifndef QUADE_ROW_H
#define QUADE_ROW_H

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

constexpr uint32_t ROW = 16;                      // lanes per read or pair: one DPP row
constexpr uint32_t FAST_WORDS = 21;               // 16-byte words of a staged line: 321 bases at any alignment, 336 at the best
constexpr uint32_t SLAB_WORDS = FAST_WORDS + 1;   // a word compare over the slab looks one dword ahead
static_assert(FAST_WORDS <= 2 * ROW, "two words per lane stage a line");
// the running sums of a staged line's bytes stay in 32 bits
static_assert((uint64_t)FAST_WORDS * 16 * 255 < 0x7FFFFFFFull, "a staged line's quality sum can overflow");

// ---- the row ---------------------------------------------------------------------------------------------------------------------
// the value of another lane of the row (DPP control CTRL; BOUND: a lane that CTRL takes from outside the row reads 0), 32 or 64
// bits wide, the low half first
template <int CTRL, bool BOUND>
__device__ __forceinline__ int32_t dpp(int32_t v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, BOUND);
}
template <int CTRL, bool BOUND>
__device__ __forceinline__ uint32_t dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, BOUND);
}
template <int CTRL, bool BOUND>
__device__ __forceinline__ uint64_t dpp(uint64_t v) {
    const uint32_t lo = dpp<CTRL, BOUND>((uint32_t)v), hi = dpp<CTRL, BOUND>((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
template <int CTRL, bool BOUND>
__device__ __forceinline__ int64_t dpp(int64_t v) {
    const uint32_t lo = dpp<CTRL, BOUND>((uint32_t)v), hi = dpp<CTRL, BOUND>((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// over the 16 lanes of a row, the result in every lane (every lane of the row is active): quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror
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
template <typename T>
__device__ __forceinline__ T row_sum(T v) {
    v += dpp<0xB1, false>(v);
    v += dpp<0x4E, false>(v);
    v += dpp<0x141, false>(v);
    v += dpp<0x140, false>(v);
    return v;
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
// the value lane `lane` (0 .. 15) of this row holds (ds_bpermute)
__device__ __forceinline__ int32_t row_get(int32_t v, uint32_t lane) { return __shfl(v, (int)lane, (int)ROW); }
__device__ __forceinline__ int64_t row_get(int64_t v, uint32_t lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)lane, (int)ROW);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), (int)lane, (int)ROW);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// the next lane's value (row_shl:1); lane 15 of the row gets 0
__device__ __forceinline__ uint32_t from_next_lane(uint32_t v) { return dpp<0x101, true>(v); }

// ---- bytes in 32-bit words (SWAR) ------------------------------------------------------------------------------------------------
// 0x80 in every byte of w that is >= t (bytes unsigned, 1 <= t <= 128)
__device__ __forceinline__ uint32_t bytes_ge(uint32_t w, uint32_t t) {
    return (((w & 0x7F7F7F7Fu) + (0x80u - t) * 0x01010101u) | w) & 0x80808080u;
}
// 0x80 in every byte of w that is not zero
__device__ __forceinline__ uint32_t bytes_nz(uint32_t w) {
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
// 0xFF in every byte of w that equals c
__device__ __forceinline__ uint32_t bytes_eq(uint32_t w, uint32_t c) {
    return ((~bytes_nz(w ^ (c * 0x01010101u)) & 0x80808080u) >> 7) * 0xFFu;
}
// how many bytes of x are not zero: x = a ^ b, the bytes in which a and b differ
__device__ __forceinline__ uint32_t differing_bytes(uint32_t x) { return (uint32_t)__popc(bytes_nz(x)); }
// upper case for the letters; no other byte becomes a letter of ACGT
__device__ __forceinline__ uint4 fold_case(uint4 v) {
    v.x &= 0xDFDFDFDFu;
    v.y &= 0xDFDFDFDFu;
    v.z &= 0xDFDFDFDFu;
    v.w &= 0xDFDFDFDFu;
    return v;
}
// Two bits a base (screen, adapters): the code of a base is (u >> 1) & 3 of u = b & 0xDF -- A 0, C 1, T 2, G 3.
// four bytes -> their four codes, the first byte's in bits 7 .. 6 (the products' bit fields do not meet: no carries)
__device__ __forceinline__ uint32_t base_codes4(uint32_t x) { return (((x >> 1) & 0x03030303u) * 0x40100401u) >> 24; }
// four bytes -> four bits, the first byte's in bit 3: 1 = A, C, G or T in either case
__device__ __forceinline__ uint32_t base_valid4(uint32_t x) {
    const uint32_t u = x & 0xDFDFDFDFu;
    const uint32_t m = (bytes_eq(u, 'A') | bytes_eq(u, 'C') | bytes_eq(u, 'G') | bytes_eq(u, 'T')) & 0x01010101u;
    return (m * 0x08040201u) >> 24;
}

// ---- the aligned line ------------------------------------------------------------------------------------------------------------
// one line of a record as aligned 16-byte words: bytes [s, e) of the words from w0 on
struct Line {
    const uint4* w0;
    uint32_t s;
    uint32_t n_words;
    uint64_t e;
};
__device__ __forceinline__ Line make_line(const uint8_t* text, uint32_t start, uint32_t len) {
    const uint8_t* p = text + start;
    Line L;
    L.s = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    L.w0 = reinterpret_cast<const uint4*>(p - L.s);
    L.e = (uint64_t)L.s + len;
    L.n_words = len ? (uint32_t)((L.e + 15) >> 4) : 0;  // every word holds at least one byte of the line
    return L;
}
// the bytes of [s, e) among the four at o .. o + 3
__device__ __forceinline__ uint32_t byte_mask(int64_t s, int64_t e, int64_t o) {
    const int64_t lo = s > o ? s - o : 0, hi = e - o < 4 ? e - o : 4;
    if (hi <= lo) return 0;
    const uint32_t upto = hi >= 4 ? 0xFFFFFFFFu : (1u << (8 * (uint32_t)hi)) - 1u;
    return upto & ~((1u << (8 * (uint32_t)lo)) - 1u);
}
// Whether word k can hold bytes outside the line: the first word, the last, and any "word" beyond the line (k >= n_words: a lane of
// the row that the line does not reach).  The callers give such a lane a zero word, so `k + 1 == n_words` would do for them; `>=`
// masks it to zero whatever it holds, and is the one form all three counting stages share.
__device__ __forceinline__ bool edge_word(const Line& L, uint32_t k) { return k == 0 || k + 1 >= L.n_words; }
// word k as loaded -> its bytes outside the line zero
__device__ __forceinline__ uint4 mask_word(const Line& L, uint32_t k, uint4 v) {
    if (edge_word(L, k)) {
        const int64_t o = (int64_t)k * 16;
        v.x &= byte_mask(L.s, (int64_t)L.e, o);
        v.y &= byte_mask(L.s, (int64_t)L.e, o + 4);
        v.z &= byte_mask(L.s, (int64_t)L.e, o + 8);
        v.w &= byte_mask(L.s, (int64_t)L.e, o + 12);
    }
    return v;
}
// the row copies the line's words into its slab, lane sub words sub and sub + 16 (the caller: n_words <= FAST_WORDS, a barrier
// before and behind); FOLD: with the case folded
template <bool FOLD>
__device__ __forceinline__ void stage_line(uint4* slab, const Line& L, uint32_t sub) {
    for (uint32_t k = sub; k < L.n_words; k += ROW) slab[k] = FOLD ? fold_case(L.w0[k]) : L.w0[k];
}

// ---- the tails -------------------------------------------------------------------------------------------------------------------
// Lane i < COUNTERS of every row holds in acc what its reads add to counter i: summed over the workgroup in part (LDS, zeroed by
// the kernel before its first barrier), then one 64-bit atomic per counter that is not zero.  Every lane of the workgroup calls it.
template <uint32_t COUNTERS>
__device__ __forceinline__ void flush_row_counters(uint64_t acc, uint32_t sub, unsigned long long* part, unsigned long long* table) {
    static_assert(COUNTERS <= ROW, "one lane per counter");
    __syncthreads();
    if (sub < COUNTERS && acc) atomicAdd(&part[sub], (unsigned long long)acc);
    __syncthreads();
    if (threadIdx.x < COUNTERS && part[threadIdx.x]) atomicAdd(table + threadIdx.x, part[threadIdx.x]);
}

// A table uint64[n_dest][VALUES] that rows add to, value i of a pair in lane i of its row.
//   LDS  : 32-bit partials of the whole table in the workgroup's LDS, flushed (non-zero entries, 64-bit global atomics) once.  A
//          few destinations receive most pairs: the hot words stay in LDS.
//   !LDS : the partials do not fit; contention is low.  The wave's four pairs are merged where their destinations are equal, then
//          contiguous 64-bit global atomics per distinct destination.
template <bool LDS, uint32_t VALUES, uint32_t BLOCK>
struct DestTable {
    static_assert(VALUES <= ROW, "one lane per value");
    uint32_t* part;  // [n_values], LDS only
    unsigned long long* table;
    uint32_t n_values;

    // every lane of the workgroup, before the first add
    __device__ __forceinline__ void init() const {
        if (LDS) {
            for (uint32_t i = threadIdx.x; i < n_values; i += BLOCK) part[i] = 0;
            __syncthreads();
        }
    }
    // every lane of the wave: v is value `sub` of the row's pair for destination d; mine: the pair is real and sub < VALUES;
    // fits32: the workgroup's sum of this pair's kind cannot pass 32 bits (else the value goes to the table directly)
    __device__ __forceinline__ void add(uint32_t d, uint32_t sub, uint64_t v, bool mine, bool fits32) const {
        if (LDS) {
            if (mine && v) {
                if (fits32) atomicAdd(&part[d * VALUES + sub], (uint32_t)v);
                else atomicAdd(table + (size_t)d * VALUES + sub, (unsigned long long)v);
            }
        } else {
            // the wave's four pairs: the first of each destination adds for the later ones
            bool leader = true;
            uint64_t total = v;
#pragma unroll
            for (uint32_t h = 0; h < 64 / ROW; ++h) {
                const uint32_t dh = __shfl(d, (int)(h * ROW), 64);
                const unsigned long long vh = __shfl((unsigned long long)v, (int)(h * ROW + sub), 64);
                const uint32_t me = (threadIdx.x & 63u) / ROW;
                if (dh == d && h < me) leader = false;
                if (dh == d && h > me) total += vh;
            }
            if (mine && leader && total) atomicAdd(table + (size_t)d * VALUES + sub, (unsigned long long)total);
        }
    }
    // every lane of the workgroup, behind the last add
    __device__ __forceinline__ void flush() const {
        if (LDS) {
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < n_values; i += BLOCK) {
                const uint32_t c = part[i];
                if (c) atomicAdd(table + i, (unsigned long long)c);
            }
        }
    }
};

}  // namespace

#endif
