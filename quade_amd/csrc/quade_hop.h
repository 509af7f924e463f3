// Index-hopping matrix (opt-in, qd_hop_enable): part lookup tables, parameter block, launch entry point.
// Internal to libquade_hip.so.  The matrix is a post-pass behind the exact-match launch, the mismatch rescue and the unknown tally:
// the pairs that stay undetermined are looked up part by part -- index read 1's slice among the sheet's distinct index-1 values,
// index read 2's among its distinct index-2 values -- and counted in a dense table of (n1 + 1) x (n2 + 1) cells.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "quade_common.h"
#include "quade_unknown.h"

#define QD_HOP_MAX_CELLS ((int64_t)1 << 24) /* (n1 + 1) * (n2 + 1) at most: 128 MiB of counters per context */
#define QD_HOP_MIN_SLOTS 16

// one entry of a part's open-addressing table (16 bytes: one load): the 64-bit tag of the part's canonical key (qd_uk_tag, never
// 0: 0 marks an empty entry) and the part's ordinal
struct HopSlot {
    uint64_t tag;
    uint32_t ord, pad;
};

// A part list on the device: a power-of-two number of slots (>= 2 * n, so a probe sequence always ends at an empty entry), the
// home slot of a tag is qd_uk_home(tag, lg); keys[ord][QD_KEY_WORDS] holds the part's canonical key words, which confirm a hit.
struct HopPart {
    const HopSlot* slots;
    const uint64_t* keys;
    uint32_t mask;
    int32_t lg;
};

struct HopParams {
    const uint8_t* seq[2];
    const uint16_t* codes;
    const uint32_t* miss;  // [0] = number of listed pairs, the list from [4] on
    HopPart part[2];
    uint64_t* table;       // [(n1 + 1) * (n2 + 1) + 1], row-major; the last value is `short`
    int64_t n;
    int32_t K;
    uint32_t n1, n2;
    int32_t idx_off[2], idx_w[2], seq_stride[2];
};

// tag of a part's canonical key (zero padded to QD_KEY_WORDS words), on the host and on the device
QD_HD uint64_t qd_hop_tag(const uint64_t (&k4)[QD_KEY_WORDS]) { return qd_uk_trim(qd_uk_tag(k4), ~0ull); }

inline int64_t qd_hop_slots(int64_t n) {
    int64_t m = QD_HOP_MIN_SLOTS;
    while (m < 2 * n) m <<= 1;
    return m;
}

// Host: the table of n parts whose canonical keys are keys[i][QD_KEY_WORDS] (distinct), qd_hop_slots(n) entries
inline void qd_hop_build(const std::vector<uint64_t>& keys, int64_t n, std::vector<HopSlot>& slots, uint32_t& mask, int32_t& lg) {
    const int64_t m = qd_hop_slots(n);
    slots.assign((size_t)m, HopSlot{0, 0, 0});
    mask = (uint32_t)(m - 1);
    lg = 0;
    while (((int64_t)1 << lg) < m) ++lg;
    for (int64_t i = 0; i < n; ++i) {
        uint64_t k4[QD_KEY_WORDS];
        for (int q = 0; q < QD_KEY_WORDS; ++q) k4[q] = keys[(size_t)i * QD_KEY_WORDS + q];
        const uint64_t tag = qd_hop_tag(k4);
        uint32_t s = qd_uk_home(tag, lg);
        while (slots[s].tag != 0) s = (s + 1) & mask;
        slots[s] = HopSlot{tag, (uint32_t)i, 0};
    }
}

// Device: one launch over the listed pairs of one batch, on st.  Adds to p.table with atomics only: launches on different streams
// need no order among themselves.
hipError_t qd_launch_hop(const HopParams& p, int cus, hipStream_t st);
