// Yield and quality counters per destination (opt-in, qd_qstats_enable): table layout and launch entry points
// (quade_qstats.hip).  No reference counterpart: Quade 0.3.2 reports pair counts only.
//
// Table: uint64[(2 * S + 1)][2][QD_QS_COUNTERS], destination-major; destination = routing code, 0xFFFF -> 2 * S (as
// qd_text_dest_lens); [read R1 / R2][counter].  Every value is an exact integer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_QS_RECORDS = 0,  // pairs routed to the destination
    QD_QS_BASES = 1,    // sum of seq_len
    QD_QS_QUAL_SUM = 2, // sum of max(0, b - 33) over the quality bytes b (unsigned)
    QD_QS_Q20 = 3,      // quality bytes with b - 33 >= 20
    QD_QS_Q30 = 4,      // ... >= 30
    QD_QS_N = 5,        // sequence bytes 'N' or 'n'
    QD_QS_COUNTERS = 6,
    QD_QS_VALUES = 2 * QD_QS_COUNTERS,  // per destination
};

// which accumulation a launch for n_samples takes
enum { QD_QS_PATH_LDS = 1, QD_QS_PATH_GLOBAL = 2 };
// 32-bit partials of a workgroup live in LDS while (2 * S + 1) * QD_QS_VALUES of them fit 64 KiB (what a kernel gets
// without opting in to more, and two workgroups still share a CU): 1365 destinations, S <= 682
#define QD_QS_LDS_MAX_DEST 1365u

static inline size_t qd_qstats_values(uint32_t n_samples) { return ((size_t)2 * n_samples + 1) * QD_QS_VALUES; }
static inline int qd_qstats_path(uint32_t n_samples) { return 2 * n_samples + 1 <= QD_QS_LDS_MAX_DEST ? QD_QS_PATH_LDS : QD_QS_PATH_GLOBAL; }

// Pairs [0, n): pair j is recs[r][j] in text[r] (r = 0: R1, 1: R2), routed by codes[j]; adds to table.  Device pointers,
// returns after the launch.  n < 2^31.  drop != NULL: pair j is skipped where drop[j] != 0 (the read filter's reason bytes,
// quade_filter.h: the table counts the pairs that are written).
struct qd_qstats_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    const uint16_t* codes;
    const uint8_t* drop;  // optional
    uint64_t* table;
};
hipError_t qd_qstats_launch(const qd_qstats_args& a, uint32_t n_samples, uint32_t n, hipStream_t st);

// The context's table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream.  Nothing is launched
// and QD_OK returned when the table is off.
extern "C" int qd_qstats_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                     const uint16_t* codes, const uint8_t* drop, void* stream);
