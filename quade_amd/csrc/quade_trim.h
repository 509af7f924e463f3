// 3' quality and adapter trimming of the insert reads (opt-in, qd_trim_set): parameters as the kernel takes them, counter layout
// and launch entry points (quade_trim.hip).  No reference counterpart: Quade 0.3.2 writes the insert reads as they came.
//
// A trim is a new seq_len per record: the stage writes trimmed copies of the two insert-read tables and everything behind it
// (quality counters, output lengths, formatter) reads sequence and quality through them.  The scan's own tables stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_TRIM_READS = 0,      // reads seen
    QD_TRIM_BASES_IN = 1,   // sum of L
    QD_TRIM_BASES_OUT = 2,  // sum of Lout
    QD_TRIM_Q_READS = 3,    // reads with Lq < L
    QD_TRIM_Q_BASES = 4,    // sum of L - Lq
    QD_TRIM_A_READS = 5,    // reads with La < Lq
    QD_TRIM_A_BASES = 6,    // sum of Lq - La
    QD_TRIM_FLOORED = 7,    // reads with Lout > La
    QD_TRIM_COUNTERS = 8,
    QD_TRIM_VALUES = 2 * QD_TRIM_COUNTERS,  // uint64[2][8]: R1, R2
};

#define QD_TRIM_MAX_ADAPTER 64

// the kernel's parameters: adapters upper case, packed little-endian four bases per word, zero padded
struct qd_trim_dev {
    uint32_t adapter[2][QD_TRIM_MAX_ADAPTER / 4];
    uint32_t adapter_len[2];  // 0 = none
    uint32_t cutoff;          // 0 = no quality trim
    uint32_t min_overlap;
    uint32_t mismatch_pct;
    uint32_t min_length;
};

// Reads [0, n) of R1 and R2: out[r][j] = recs[r][j] with seq_len = the length the read keeps; adds to table (uint64[2][8]).
// Device pointers, returns after the launch.  n < 2^31.
struct qd_trim_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    qd_rec* out[2];
    uint64_t* table;
};
hipError_t qd_trim_launch(const qd_trim_dev& P, const qd_trim_args& a, uint32_t n, hipStream_t st);

// The context's parameters and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, after asking
// qd_trim_active whether there is anything to do (off: no buffers, no launch, the scan's tables go on as they are).
extern "C" int qd_trim_active(const qd_ctx* ctx);
extern "C" int qd_trim_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                              qd_rec* out1, qd_rec* out2, void* stream);
