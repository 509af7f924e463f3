// K-mer screen of the insert reads against a reference (opt-in, qd_screen_set): PhiX, a spike-in, a vector, a contaminant.
// Parameters as the kernel takes them, table layout, the hash table's shape and launch entry points (quade_screen.hip).  No
// reference counterpart: Quade 0.3.2 knows no reference sequence.
//
// Definition (include/quade_hip.h, tests/screen_model.py and the kernel state exactly this).  u(b) = b & 0xDF; a base is valid when
// u(b) is one of A, C, G, T; its code is c(b) = (u(b) >> 1) & 3 (A 0, C 1, T 2, G 3, the duplication key's code), the complement
// c ^ 2.  The k-mer at position p of s exists when s[p .. p + k) are all valid; forward word w = sum c(s[p + i]) << 2 (k - 1 - i),
// reverse-complement word rc = sum (c(s[p + k - 1 - i]) ^ 2) << 2 (k - 1 - i), canonical word min(w, rc).  hits(read) = the
// positions p in [0, L - k] whose k-mer exists and whose canonical word is in the reference set R.  A pair is matched when
// hits(R1) + hits(R2) >= min_hits.
//
// The set R sits in an open-addressing table of 64-bit words, linear probing, a power of two of slots, at most half full.  The
// empty slot is all ones, which no canonical word equals: at k = 32 the all-ones forward word (poly-G) has rc 0x5555... (poly-C).
// Compares are exact: the hash function decides where a word is found, never whether.
//   LDS    : n_kmers <= QD_SCREEN_LDS_MAX_KMERS = 6144: 16384 slots = 128 KiB of the workgroup's LDS, copied from global memory
//            once per workgroup.  The cap is measured: the slots are fixed, so the table fills with the reference, and a wave waits
//            for the longest of its 64 probe chains -- at 8192 words (half full) a batch without hits took 8.2 ms, at PhiX's 5356
//            (a third) 4.4 ms, no more than the global path over a quarter-full table.  24 KiB of row slabs beside the table:
//            152 KiB of the CU's 160, one workgroup of 1024 lanes per CU (16 waves, 4 per SIMD).  The destination partials do not
//            also fit: DestTable's !LDS form.
//   GLOBAL : up to QD_SCREEN_MAX_KMERS = 2^22: the same probe over a table in global memory (at most 2^23 slots, 64 MiB).
//
// Table: uint64[(2 * S + 1)][QD_SC_VALUES], destination-major as qd_qstats (destination = routing code, 0xFFFF -> 2 * S).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_SC_PAIRS = 0,          // pairs seen
    QD_SC_MATCHED = 1,        // pairs with hits(R1) + hits(R2) >= min_hits
    QD_SC_R1_HIT = 2,         // pairs whose R1 has at least one hit
    QD_SC_R2_HIT = 3,         // ... whose R2 has
    QD_SC_KMERS = 4,          // k-mers that exist, over both reads
    QD_SC_HIT_KMERS = 5,      // ... whose canonical word is in R
    QD_SC_BASES_IN = 6,       // sum of L over both reads of every pair
    QD_SC_BASES_MATCHED = 7,  // ... of the matched pairs
    QD_SC_VALUES = 8,         // per destination
};

enum { QD_SC_PATH_LDS = 1, QD_SC_PATH_GLOBAL = 2 };
enum { QD_SC_REPORT = 0, QD_SC_DROP = 1 };

#define QD_SC_MIN_K 15
#define QD_SC_MAX_K 32
#define QD_SC_MAX_KMERS (1u << 22)
#define QD_SC_LDS_SLOTS_LG 14u                         // 16384 slots x 8 bytes = 128 KiB
#define QD_SC_LDS_MAX_KMERS (3u << (QD_SC_LDS_SLOTS_LG - 3))  // three eighths full at the most: 6144 (see below)
#define QD_SC_MIN_SLOTS_LG 4u
#define QD_SC_EMPTY 0xFFFFFFFFFFFFFFFFull
#define QD_SC_DROPPED 0x80u                            // the flag byte of a pair the screen drops

static inline size_t qd_screen_values(uint32_t n_samples) { return ((size_t)2 * n_samples + 1) * QD_SC_VALUES; }
static inline int qd_screen_path(uint64_t n_kmers) { return n_kmers <= QD_SC_LDS_MAX_KMERS ? QD_SC_PATH_LDS : QD_SC_PATH_GLOBAL; }
// log2 of the slots of a table for n_kmers words: the LDS path always fills its 128 KiB (the shorter the probe chains), the global
// path takes the first power of two that leaves the table at most half full
static inline uint32_t qd_screen_slots_lg(uint64_t n_kmers) {
    if (qd_screen_path(n_kmers) == QD_SC_PATH_LDS) return QD_SC_LDS_SLOTS_LG;
    uint32_t lg = QD_SC_LDS_SLOTS_LG + 1;
    while (((uint64_t)1 << lg) < 2 * n_kmers) ++lg;
    return lg;
}
// the first slot probed for a canonical word (Fibonacci hashing: the top slots_lg bits of the product); host and device
static inline __host__ __device__ uint32_t qd_screen_slot(uint64_t word, uint32_t slots_lg) {
    return (uint32_t)((word * 0x9E3779B97F4A7C15ull) >> (64 - slots_lg));
}

// the kernel's parameters (checked by qd_screen_set)
struct qd_screen_dev {
    uint32_t k;          // 15 .. 32
    uint32_t min_hits;   // 1 .. 65535
    uint32_t action;     // QD_SC_REPORT | QD_SC_DROP
    uint32_t slots_lg;   // the table has 1 << slots_lg slots
};

// Pairs [0, n): pair j is recs[r][j] in text[r] (r = 0: R1, 1: R2), routed by codes[j].  drop_in: nullptr or a byte per pair, a
// non-zero one = the pair is skipped and counted nowhere.  hits: nullptr or uint32[n][2].  flag: nullptr or a byte per pair that
// receives drop_in[j] when that is non-zero, else QD_SC_DROPPED when the pair is matched and the action is drop, else 0; it may be
// drop_in itself.  Adds to table.  slots: the hash table in global memory.  Device pointers, returns after the launch.  n < 2^31.
struct qd_screen_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    const uint16_t* codes;
    const uint8_t* drop_in;
    uint32_t* hits;
    uint8_t* flag;
    const uint64_t* slots;
    uint64_t* table;
};
hipError_t qd_screen_launch(const qd_screen_dev& P, const qd_screen_args& a, uint32_t n_samples, uint32_t n, int path, uint32_t cus,
                            hipStream_t st);

// The context's parameters, hash table and counters (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream,
// after asking qd_screen_active whether there is anything to do (off: no buffer, no launch); qd_screen_active returns 0 (off),
// 1 (action report: flag may be nullptr) or 2 (action drop: flag is the pipeline's drop buffer).
extern "C" int qd_screen_active(const qd_ctx* ctx);
extern "C" int qd_screen_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2,
                                uint32_t n, const uint16_t* codes, const uint8_t* drop_in, uint32_t* hits, uint8_t* flag, void* stream);
