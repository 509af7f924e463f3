// Adapter content of the insert reads as the scan left them (opt-in, qd_adapters_set): where the first 12 bases of known adapters
// start in R1 and R2.  Probe words as the kernel takes them, table layout and launch entry points (quade_adapters.hip).  No
// reference counterpart: Quade 0.3.2 knows no adapter.
//
// Definition (include/quade_hip.h, tests/adapter_model.py and the kernel state exactly this).  A probe is QD_AD_K = 12 bases of
// ACGT; up to QD_AD_PROBES = 16 are in force, slot a = the a-th probe given.  u[i] = s[i] & 0xDF, L the sequence length:
// first(a) = the smallest p in [0, L - 12] with u[p .. p + 12) equal to probe a, else none; a byte that is not A, C, G or T after
// folding matches nothing.  first(any) = the minimum over the probes in force.
//
// A probe's word: the code of a base is (u >> 1) & 3 (A 0, C 1, T 2, G 3, the duplication key's and the screen's code), the word
// sum code(probe[i]) << 2 (11 - i), 24 bits; QD_AD_NO_PROBE in an unused slot equals no read's word.
//
// Table: uint64[QD_AD_HIST_VALUES + (2 * S + 1) * QD_AD_DEST_VALUES]:
//   hist[r][a][bin]   r = 0 / 1 for R1 / R2, a = 0 .. 15 the slots and 16 = any, bin = min(first(a), 1024): 2 x 17 x 1025
//   dest[d][r][c]     d = the routing code, 0xFFFF -> 2 * S (as qd_qstats); c = 0 the reads, c = 1 + a the reads with first(a)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

#define QD_AD_K 12u
#define QD_AD_PROBES 16u
#define QD_AD_COLUMNS (QD_AD_PROBES + 1u)       // the slots, then any
#define QD_AD_BINS 1025u                        // first(a) < 1024, then >= 1024
#define QD_AD_HIST_VALUES (2u * QD_AD_COLUMNS * QD_AD_BINS)  // 34 850
#define QD_AD_DEST_COLUMNS (QD_AD_COLUMNS + 1u) // reads, the slots, any
#define QD_AD_DEST_VALUES (2u * QD_AD_DEST_COLUMNS)  // per destination: 36
#define QD_AD_NO_PROBE 0xFFFFFFFFu
// destinations whose 32-bit partials a workgroup keeps in LDS; a larger sheet adds to the 64-bit table directly
#define QD_AD_LDS_MAX_DEST 227u

static inline size_t qd_adapters_values(uint32_t n_samples) {
    return (size_t)QD_AD_HIST_VALUES + ((size_t)2 * n_samples + 1) * QD_AD_DEST_VALUES;
}

// the probe words in slot order, QD_AD_NO_PROBE from n_probes on (qd_adapters_set makes them)
struct qd_adapters_dev {
    uint32_t word[QD_AD_PROBES];
    uint32_t n_probes;
};

// Reads [0, n) of R1 and of R2: read j of r is recs[r][j] in text[r], routed by codes[j]; adds to table.  Device pointers, returns
// after the launch.  n < 2^31.
struct qd_adapters_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    const uint16_t* codes;
    uint64_t* table;
};
hipError_t qd_adapters_launch(const qd_adapters_dev& P, const qd_adapters_args& a, uint32_t n_samples, uint32_t n, hipStream_t st);

// The context's probes and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, in front of the
// stages that rewrite the record tables, on the scan's tables and the final codes.  Nothing is launched and QD_OK returned when
// the stage is off (qd_adapters_active: 1 on, 0 off).
extern "C" int qd_adapters_active(const qd_ctx* ctx);
extern "C" int qd_adapters_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2,
                                  uint32_t n, const uint16_t* codes, void* stream);
