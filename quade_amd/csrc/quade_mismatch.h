// Mismatch-tolerant matching (opt-in, qd_set_mismatches): parameter block, host table builder, launch entry point.
// Internal to libquade_hip.so.  The rescue is a post-pass behind the exact-match launch: the pairs it left undetermined
// are listed, and each is assigned to the one K-long barcode within budget of it per part.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "quade_common.h"

#define QD_MM_MAX_SEG 3 /* segments of the pigeonhole part: budget + 1, budgets 0..2 */

// 64-bit tag of segment j of a canonical key, given as the key's words masked to the segment's bytes
QD_HD uint64_t qd_mm_seg_tag(const uint64_t (&s)[QD_KEY_WORDS], int j) {
    uint64_t h = 0x9E3779B97F4A7C15ull * (uint64_t)(j + 1);
    for (int q = 0; q < QD_KEY_WORDS; ++q) {
        h = (h ^ s[q]) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    return h ^ (h >> 29);
}

// 0x01 in every byte lane of x that is not zero
QD_HD uint64_t qd_nz_bytes(uint64_t x) {
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;
    return x & 0x0101010101010101ull;
}

// one bucket of the segment table: the candidates of one segment value are cand[start .. start + count)
struct QdMmBucket {
    uint32_t tag_lo, tag_hi, start, count;  // count == 0: empty
};

struct MismatchParams {
    const uint8_t* seq[2];
    const uint8_t* qual[2];
    uint16_t* codes;
    uint64_t* adjust;     // the context's 64-bit totals (signed moves, as demux_fixup)
    const uint32_t* miss; // [0] = number of listed pairs, the list from [4] on
    const uint64_t* bk32; // [S][4] canonical keys of every barcode
    const QdMmBucket* htab;
    const uint16_t* cand;
    int64_t n;
    int32_t n_streams, K;
    int32_t idx_off[2], idx_w[2], seq_stride[2], qual_stride[2];
    uint32_t thr, n_samples, hist_entries, hmask, ncand;
    int32_t m[2];                                 // budgets of the parts [0, w1) and [w1, K)
    int32_t nseg;                                 // 0: no usable pigeonhole part, every K-long barcode is a candidate
    uint64_t part[2][QD_KEY_WORDS];               // 0x01 in every byte lane of the part
    uint64_t segmask[QD_MM_MAX_SEG][QD_KEY_WORDS]; // 0xFF in every byte lane of segment j of the chosen part
};

// Host: the first colliding ordinal pair (i < j, lexicographic) of the K-long barcodes, or false.  Brute force over all pairs
// (SWAR per-part Hamming distances, rows dealt to up to 16 threads).
bool qd_mm_first_collision(int32_t S, const uint8_t* barcodes, const int32_t* offsets, int32_t K, int32_t w1, int32_t m1, int32_t m2,
                           int32_t* first, int32_t* second);

// Host: the pigeonhole tables for the K-long barcodes (fills p.m, p.part, p.segmask, p.nseg, p.ncand, p.hmask).
void qd_mm_build(int32_t S, const uint8_t* barcodes, const int32_t* offsets, int32_t K, int32_t w1, int32_t m1, int32_t m2,
                 MismatchParams& p, std::vector<QdMmBucket>& htab, std::vector<uint16_t>& cand);

// Device: the undetermined pairs of codes[0..n) listed in miss ([0] = count, zeroed first; the list from [4] on, n entries at most).
hipError_t qd_launch_compact(const uint16_t* codes, int64_t n, uint32_t* miss, hipStream_t st);

// Device: compaction of the undetermined pairs of codes[0..n) into miss (zeroed count first), then the rescue.
hipError_t qd_launch_mismatch(const MismatchParams& p, uint32_t* miss, int cus, hipStream_t st);
