// Post-trimming of the insert reads (opt-in, qd_posttrim_set): trailing N, a poly-X tail and a crop to max_length, behind the
// clip, 3' trimming and overlap trimming stages and in front of the read filter.  Parameters as the kernel takes them, counter
// layout and launch entry points (quade_posttrim.hip).  No reference counterpart: Quade 0.3.2 writes the insert reads as they
// came.  include/quade_hip.h states the rule.
//
// A post-trim is a new seq_len per record: the stage writes copies of the two insert-read tables and everything behind it reads
// the lengths through them.  seq and qual never move, no pair is dropped, and the tables the stage received stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_POST_READS = 0,           // reads seen
    QD_POST_BASES_IN = 1,        // sum of L
    QD_POST_BASES_OUT = 2,       // sum of Lout
    QD_POST_N_READS = 3,         // reads with Ln < L
    QD_POST_N_BASES = 4,         // sum of L - Ln
    QD_POST_A_READS = 5,         // reads whose tail base is A, and 6 the sum of Ln - Lp over them; C, G and T follow in pairs
    QD_POST_A_BASES = 6,
    QD_POST_CROP_READS = 13,     // reads with Lm < Lp
    QD_POST_CROP_BASES = 14,     // sum of Lp - Lm
    QD_POST_FLOORED = 15,        // reads with Lout > Lm
    QD_POST_COUNTERS = 16,       // one DPP row
    QD_POST_TABLE = 2 * QD_POST_COUNTERS,  // uint64[2][16]: R1, R2
};

#define QD_POST_MIN_POLYX 6
#define QD_POST_MAX_POLYX 100

// the kernel's parameters
struct qd_posttrim_dev {
    uint32_t tail_n;         // 1 = cut trailing N
    uint32_t poly_x;         // P, 0 = no poly-X rule
    uint32_t max_length[2];  // M of R1, R2; 0 = no crop
    uint32_t min_length;
};

// Reads [0, n) of R1 and R2: out[r][j] = recs[r][j] with seq_len = the length the read keeps; adds to table (uint64[2][16]).  Only
// the sequence lines are read.  Device pointers, returns after the launch.  n < 2^31.
struct qd_posttrim_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    qd_rec* out[2];
    uint64_t* table;
};
hipError_t qd_posttrim_launch(const qd_posttrim_dev& P, const qd_posttrim_args& a, uint32_t n, hipStream_t st);

// The context's parameters and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, after asking
// qd_posttrim_active whether there is anything to do (off: no buffers, no launch, the tables of the stage in front go on).
extern "C" int qd_posttrim_active(const qd_ctx* ctx);
extern "C" int qd_posttrim_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                                  qd_rec* out1, qd_rec* out2, void* stream);
