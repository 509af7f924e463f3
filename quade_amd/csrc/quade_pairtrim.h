// Paired-end overlap trimming of the insert reads with insert sizes (opt-in, qd_pairtrim_set): parameters as the kernel takes them,
// table layout and launch entry points (quade_pairtrim.hip).  No reference counterpart: Quade 0.3.2 never looks at R1 and R2 of a
// pair together.
//
// Definition (include/quade_hip.h, tests/pairtrim_model.py and the kernel state exactly this).  Per pair, the two insert reads as
// the stage receives them: sequences s1, s2 of current lengths L1, L2 (only the first L bytes of each count).
//   fold      : u(b) = b & 0xDF; a base is valid only if u(b) is one of A C G T; comp maps A<->T and C<->G
//   candidate : an insert length I, 1 <= I <= L1 + L2, pairs position i of R1 with j = I - 1 - i of R2 for all i with 0 <= i < L1
//               and 0 <= j < L2: ov(I) = min(L1, I) - max(0, I - L2) positions.  A position matches iff u(s1[i]) is valid and
//               u(s2[j]) == comp(u(s1[i])); everything else (N in either read, N opposite N) is a mismatch.  I is accepted iff
//               ov(I) >= min_overlap and mismatches <= min(max_mismatches, ov(I) * max_mismatch_pct / 100) (rounded down)
//   insert I* : with M = max(L1, L2): the smallest accepted I >= M if there is one (the reads overlap or the insert spans them:
//               nothing is cut, and a tandem repeat that also matches at a shorter I causes no trim); otherwise the largest
//               accepted I < M; otherwise none
//   cut       : I* < M: Lp_r = min(L_r, I*); otherwise Lp_r = L_r
//   floor     : Lout_r = max(Lp_r, min(min_length, L_r)).  min_length is the 3' trimming's (qd_trim_set): that stage left
//               L_r >= min(min_length, L0_r) of the length L0_r it was given, so L_r < min_length only where L_r == L0_r, and
//               min(min_length, L_r) == min(min_length, L0_r) either way: the stage's input length serves as L_r
// A cut is a new seq_len per record: the stage writes copies of the two tables it is given and everything behind it reads sequence
// and quality through them.  The tables it is given stay as they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_PT_READS = 0,      // reads seen
    QD_PT_BASES_IN = 1,   // sum of L
    QD_PT_BASES_OUT = 2,  // sum of Lout
    QD_PT_CUT_READS = 3,  // reads with Lp < L
    QD_PT_CUT_BASES = 4,  // sum of L - Lp
    QD_PT_FLOORED = 5,    // reads with Lout > Lp
    QD_PT_COUNTERS = 6,   // per read: uint64[2][6] (R1, R2) at the table's start
    QD_PT_PAIRS = 2 * QD_PT_COUNTERS,  // then: pairs seen
    QD_PT_OVERLAPPED = QD_PT_PAIRS + 1,  // pairs with an I*
    QD_PT_SHORT = QD_PT_PAIRS + 2,       // pairs with I* < M
    QD_PT_HIST = QD_PT_PAIRS + 3,        // then the insert sizes: bin I* for I* < 1024, the last bin for I* >= 1024
    QD_PT_BINS = 1025,
    QD_PT_VALUES = QD_PT_HIST + QD_PT_BINS,  // 1040
};

// the kernel's parameters (checked by qd_pairtrim_set)
struct qd_pairtrim_dev {
    uint32_t min_overlap;     // >= 1
    uint32_t max_mismatches;
    uint32_t mismatch_pct;
    uint32_t min_length;
};

// Pairs [0, n): out[r][j] = recs[r][j] with seq_len = the length the read keeps; adds to table (uint64[1040]).
// Device pointers, returns after the launch.  n < 2^31.
// insert: nullptr (every caller value-initialises the struct), or n values: lane 0 of the pair's row stores its I*, 0 = none, for the
// overlap base correction behind this stage (quade_paircorrect.h).  64 bits wide: exact for every L1 + L2 the record tables can
// express (two 32-bit lengths).  Nothing else the kernel computes or writes depends on it.
struct qd_pairtrim_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    qd_rec* out[2];
    uint64_t* table;
    uint64_t* insert;
};
hipError_t qd_pairtrim_launch(const qd_pairtrim_dev& P, const qd_pairtrim_args& a, uint32_t n, hipStream_t st);

// The context's parameters and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, after asking
// qd_pairtrim_active whether there is anything to do (off: no buffers, no launch, the tables go on as they are).
extern "C" int qd_pairtrim_active(const qd_ctx* ctx);
extern "C" int qd_pairtrim_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2,
                                  uint32_t n, qd_rec* out1, qd_rec* out2, void* stream);
// the same launch, which also stores every pair's I* (0 = none) in inserts[0 .. n) when inserts is not nullptr
extern "C" int qd_pairtrim_device_inserts(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2,
                                          uint32_t n, qd_rec* out1, qd_rec* out2, uint64_t* inserts, void* stream);
