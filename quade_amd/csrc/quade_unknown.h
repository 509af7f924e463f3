// Tally of the unknown barcodes (opt-in, qd_unknown_enable): table layout, parameter block, launch entry points.
// Internal to libquade_hip.so.  The tally is a post-pass behind the exact-match launch and the mismatch rescue: the pairs
// that stay undetermined are listed and their fused barcode keys counted in a device-resident hash table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_common.h"

#define QD_UK_MIN_LG 10
#define QD_UK_MAX_LG 28
#define QD_UK_PROBES 1024 /* probe limit: a table of 2^10 slots admits keys until it is full */
#define QD_UK_HEAD 64     /* bytes in front of the table: the four 64-bit totals */

// totals in the table's head
enum { QD_UK_TALLIED = 0, QD_UK_SHORT = 1, QD_UK_DROPPED = 2, QD_UK_DISTINCT = 3 };

// what uk_claim leaves per listed pair for uk_count (any other value: the pair's slot)
#define QD_UK_NONE 0xFFFFFFFFu  /* no slot within the probe limit */
#define QD_UK_ISSHORT 0xFFFFFFFEu /* the read ends inside its index window */
#define QD_UK_SKIP 0xFFFFFFFDu  /* not undetermined any more (rescued) */

// 64-bit tag of a canonical key (never 0 once qd_uk_trim has seen it)
QD_HD uint64_t qd_uk_tag(const uint64_t (&w)[QD_KEY_WORDS]) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (int q = 0; q < QD_KEY_WORDS; ++q) {
        h = (h ^ w[q]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}
// the low `bits` of the tag (test knob unknown_tag_bits), 0 avoided: 0 marks an empty slot
QD_HD uint64_t qd_uk_trim(uint64_t tag, uint64_t tag_mask) {
    tag &= tag_mask;
    return tag ? tag : 1;
}
// first slot of a tag's probe sequence: a function of the (trimmed) tag alone, so equal tags walk the same sequence
QD_HD uint32_t qd_uk_home(uint64_t tag, int lg) { return (uint32_t)((tag * 0x9E3779B97F4A7C15ull) >> (64 - lg)); }

// one device allocation: [QD_UK_HEAD bytes of totals][tags: slots x 8][counts: slots x 8][keys: slots x 32]
struct UnknownTable {
    uint64_t* totals;
    uint64_t* tags;    // 0 = empty
    uint64_t* counts;
    uint64_t* keys;    // [slots][QD_KEY_WORDS] canonical key words
    uint32_t mask;     // slots - 1
    int32_t lg;        // log2(slots)
    uint32_t probes;   // min(slots, QD_UK_PROBES)
    uint64_t tag_mask; // all ones but for the test knob
};

struct UnknownParams {
    const uint8_t* seq[2];
    const uint16_t* codes;
    const uint32_t* miss; // [0] = number of listed pairs, the list from [4] on
    uint32_t* where;      // per listed pair: its slot or QD_UK_NONE / _ISSHORT / _SKIP
    UnknownTable t;
    int64_t n;
    int32_t n_streams, K;
    int32_t idx_off[2], idx_w[2], seq_stride[2];
};

inline size_t qd_uk_bytes(int64_t slots) { return (size_t)QD_UK_HEAD + (size_t)slots * (8 + 8 + 8 * QD_KEY_WORDS); }
inline void qd_uk_carve(void* base, int64_t slots, UnknownTable& t) {
    uint8_t* b = static_cast<uint8_t*>(base);
    t.totals = reinterpret_cast<uint64_t*>(b);
    t.tags = reinterpret_cast<uint64_t*>(b + QD_UK_HEAD);
    t.counts = t.tags + slots;
    t.keys = t.counts + slots;
    t.mask = (uint32_t)(slots - 1);
    t.lg = 0;
    while (((int64_t)1 << t.lg) < slots) ++t.lg;
    t.probes = (uint32_t)(slots < QD_UK_PROBES ? slots : QD_UK_PROBES);
}

// Device: uk_claim then uk_count over the listed pairs of one batch, on st.  `before_claim` (may be NULL): an event the stream
// waits for between the listing and uk_claim (the previous launch's uk_count, whatever stream it ran on).
hipError_t qd_launch_unknown(const UnknownParams& p, int cus, hipEvent_t before_claim, hipStream_t st);

// Device: the occupied entries of the table packed into out_keys[i][QD_KEY_WORDS] / out_counts[i], i < cap, in any order;
// *out_n (zeroed first) counts all occupied entries.
hipError_t qd_launch_unknown_gather(const UnknownTable& t, uint64_t* out_keys, uint64_t* out_counts, uint32_t* out_n, uint32_t cap,
                                    hipStream_t st);
