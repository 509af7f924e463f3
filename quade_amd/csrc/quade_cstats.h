// Per-cycle quality and base content, and the distributions of read length, per-read mean quality and GC content (opt-in,
// qd_cstats_enable): table layout and launch entry points (quade_cstats.hip).  No reference counterpart.
//
// Definition (include/quade_hip.h states it in the same words):
//   group g   from the routing code: an even code is pass (0), an odd code is fail (1), 0xFFFF is Undetermined (2)
//   read r    0 / 1 for R1 / R2
//   bytes     sequence bytes s; quality bytes q unsigned, ph = max(0, q - 33), as in qd_qstats
//   per cycle c < QD_CS_CYCLES, every read with L > c adds to cycle[g][r][c][8]:
//     0 A  1 C  2 G  3 T  4 N   (s[c] & 0xDF) == the letter
//     5 qual_sum += ph[c]       6 q20  ph[c] >= 20       7 q30  ph[c] >= 30
//   per read: len[g][r][1025] bin min(L, 1024); for L > 0 meanq[g][r][94] bin min(93, sum(ph) / L) and gc[g][r][101] bin
//     100 * (G and C count, either case) / L, both over the whole read, integer division
// Table: uint64, group-major, then read; for each (g, r) cycle, len, meanq, gc = QD_CS_GR_VALUES values; QD_CS_VALUES in all,
// independent of S.  Every value is an exact integer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

// cycles whose 32-bit partials a workgroup keeps in LDS; later cycles (up to QD_CS_CYCLES) go to the 64-bit table directly
#define QD_CS_LDS_CYCLES 320u
static_assert(QD_CS_LDS_CYCLES % 16 == 0 && QD_CS_LDS_CYCLES <= QD_CS_CYCLES, "the LDS layout takes whole 16-cycle columns");
static_assert(QD_CS_GR_VALUES == QD_CS_CYCLES * QD_CS_COUNTERS + QD_CS_LEN_BINS + QD_CS_MEANQ_BINS + QD_CS_GC_BINS, "table layout");
static_assert(QD_CS_VALUES == QD_CS_GROUPS * 2 * QD_CS_GR_VALUES, "table layout");

// Pairs [0, n): pair j is recs[r][j] in text[r] (r = 0: R1, 1: R2), grouped by codes[j]; adds to table.  Device pointers,
// returns after the launch.  n < 2^31.  drop != NULL: pair j is skipped where drop[j] != 0 (the read filter's reason bytes).
struct qd_cstats_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    const uint16_t* codes;
    const uint8_t* drop;  // optional
    uint64_t* table;
};
hipError_t qd_cstats_launch(const qd_cstats_args& a, uint32_t n, hipStream_t st);

// The context's table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, directly behind
// qd_qstats_device.  Nothing is launched and QD_OK returned when the table is off.
extern "C" int qd_cstats_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                     const uint16_t* codes, const uint8_t* drop, void* stream);
