// End clipping, sliding-window quality trimming and poly-G tail trimming of the insert reads (opt-in, qd_clip_set): parameters as
// the kernel takes them, counter layout and launch entry points (quade_clip.hip).  No reference counterpart: Quade 0.3.2 writes
// the insert reads as they came.  include/quade_hip.h states the rule.
//
// A clip is a new seq, qual and seq_len per record: the stage writes copies of the two insert-read tables, in front of the 3'
// trimming (quade_trim.h), and everything behind it reads sequence and quality through them.  The scan's own tables stay as
// they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_CLIP_READS = 0,        // reads seen
    QD_CLIP_BASES_IN = 1,     // sum of L
    QD_CLIP_BASES_OUT = 2,    // sum of Lout
    QD_CLIP_FRONT_READS = 3,  // reads with f > 0
    QD_CLIP_FRONT_BASES = 4,  // sum of f
    QD_CLIP_TAIL_READS = 5,   // reads with Lc < L - f
    QD_CLIP_TAIL_BASES = 6,   // sum of L - f - Lc
    QD_CLIP_WIN_READS = 7,    // reads with Lw < Lc
    QD_CLIP_WIN_BASES = 8,    // sum of Lc - Lw
    QD_CLIP_G_READS = 9,      // reads with Lg < Lw
    QD_CLIP_G_BASES = 10,     // sum of Lw - Lg
    QD_CLIP_FLOORED = 11,     // reads with Lout > Lg
    QD_CLIP_COUNTERS = 12,
    QD_CLIP_TABLE = 2 * QD_CLIP_COUNTERS,  // uint64[2][12]: R1, R2
};

#define QD_CLIP_MAX_WINDOW 100
#define QD_CLIP_MAX_POLYG 100

// the kernel's parameters
struct qd_clip_dev {
    uint32_t front[2], tail[2];  // bases cut from the 5' / 3' end of R1, R2
    uint32_t window;             // W, 0 = no window rule
    uint32_t window_sum;         // Q * W: a window whose Phred sum is below it fails
    uint32_t poly_g;             // P, 0 = no poly-G rule
    uint32_t min_length;
};

// Reads [0, n) of R1 and R2: out[r][j] = recs[r][j] with seq and qual moved by the front clip and seq_len = the length the read
// keeps; adds to table (uint64[2][12]).  Device pointers, returns after the launch.  n < 2^31.
struct qd_clip_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    qd_rec* out[2];
    uint64_t* table;
};
hipError_t qd_clip_launch(const qd_clip_dev& P, const qd_clip_args& a, uint32_t n, hipStream_t st);

// The context's parameters and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, after asking
// qd_clip_active whether there is anything to do (off: no buffers, no launch, the scan's tables go on as they are).
extern "C" int qd_clip_active(const qd_ctx* ctx);
extern "C" int qd_clip_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                              qd_rec* out1, qd_rec* out2, void* stream);
