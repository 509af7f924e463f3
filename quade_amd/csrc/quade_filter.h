// Read filtering of the insert reads (opt-in, qd_filter_set): parameters as the kernel takes them, table layout and launch entry
// points (quade_filter.hip).  No reference counterpart: Quade 0.3.2 writes every pair it assigns.
//
// Definition (include/quade_hip.h, tests/filter_model.py and the kernel state exactly this).  Per read as the trimming stages left
// it, of length L with sequence bytes s and quality bytes q (unsigned):
//   n_count = bytes 'N' or 'n'            unq  = the q[i] < 33 + qualified_quality
//   qsum    = sum of max(0, q[i] - 33)    diff = the i in [0, L - 1) with (s[i] & 0xDF) != (s[i + 1] & 0xDF)
// A pair is dropped for the first of these rules that either of its reads fails (rules that are off, -1, are skipped; 64-bit):
//   1 too_short         L < min_length
//   2 too_many_n        n_count > max_n
//   3 low_quality       unq * 100 > max_unqualified_pct * L
//   4 low_mean_quality  qsum < min_mean_quality * L
//   5 low_complexity    diff * 100 < min_complexity_pct * max(L - 1, 0)
// An empty read fails rule 1 only.  The stage writes one reason byte per pair (0 = kept) that the quality counters, the output
// lengths and the formatter honour: a dropped pair is in no output file.
//
// Table: uint64[(2 * S + 1)][QD_FL_VALUES], destination-major as qd_qstats (destination = routing code, 0xFFFF -> 2 * S).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_FL_PAIRS = 0,          // pairs seen
    QD_FL_TOO_SHORT = 1,      // pairs dropped by rule 1 .. 5: the reason byte is the index
    QD_FL_TOO_MANY_N = 2,
    QD_FL_LOW_QUALITY = 3,
    QD_FL_LOW_MEAN_QUALITY = 4,
    QD_FL_LOW_COMPLEXITY = 5,
    QD_FL_BASES_IN = 6,       // sum of L over both reads of every pair
    QD_FL_BASES_DROPPED = 7,  // ... of the dropped pairs
    QD_FL_VALUES = 8,         // per destination
};

// which accumulation a launch for n_samples takes
enum { QD_FL_PATH_LDS = 1, QD_FL_PATH_GLOBAL = 2 };
// 32-bit partials of a workgroup live in LDS while (2 * S + 1) * QD_FL_VALUES of them fit 64 KiB: 2048 destinations, S <= 1023
#define QD_FL_LDS_MAX_DEST 2048u

static inline size_t qd_filter_values(uint32_t n_samples) { return ((size_t)2 * n_samples + 1) * QD_FL_VALUES; }
static inline int qd_filter_path(uint32_t n_samples) { return 2 * n_samples + 1 <= QD_FL_LDS_MAX_DEST ? QD_FL_PATH_LDS : QD_FL_PATH_GLOBAL; }

// the kernel's parameters (checked by qd_filter_set); -1 = the rule is off
struct qd_filter_dev {
    int32_t min_length;
    int32_t max_n;
    int32_t max_unqualified_pct;
    int32_t qual_byte;  // 33 + qualified_quality: 34 .. 126
    int32_t min_mean_quality;
    int32_t min_complexity_pct;
};

// Pairs [0, n): pair j is recs[r][j] in text[r] (r = 0: R1, 1: R2), routed by codes[j]; reason[j] = 0 or the rule that dropped
// it; adds to table.  Device pointers, returns after the launch.  n < 2^31.
struct qd_filter_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    const uint16_t* codes;
    uint8_t* reason;
    uint64_t* table;
};
hipError_t qd_filter_launch(const qd_filter_dev& P, const qd_filter_args& a, uint32_t n_samples, uint32_t n, hipStream_t st);

// The context's parameters and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, after asking
// qd_filter_active whether there is anything to do (off: no buffer, no launch, no pair leaves).
extern "C" int qd_filter_active(const qd_ctx* ctx);
extern "C" int qd_filter_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2,
                                uint32_t n, const uint16_t* codes, uint8_t* reason, void* stream);
