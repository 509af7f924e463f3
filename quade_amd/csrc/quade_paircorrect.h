// Overlap base correction of read pairs (opt-in, qd_paircorrect_set): parameters as the kernel takes them, table layout and launch
// entry points (quade_paircorrect.hip).  No reference counterpart: Quade 0.3.2 never looks at R1 and R2 of a pair together.  The
// first stage that writes into a window's text: every other stage expresses its result as a new start or length in a copy of the
// record tables.
//
// The rule (include/quade_hip.h, tests/paircorrect_model.py and the kernel state exactly this).  The stage runs directly behind the
// overlap trimming stage and in front of post-trimming, over every pair for which that stage found an insert length I* (I* >= M and
// I* < M alike), whatever its destination, the write flags and later filtering.  It uses the record tables the overlap stage
// RECEIVED: sequences s1, s2 and quality lines q1, q2 of lengths L1, L2, starting at the tables' seq / qual (a 5' clip is respected).
//   definitions : u(b) = b & 0xDF; valid(b) iff u(b) is one of A C G T; comp maps A<->T and C<->G; the phred of a quality byte c is
//                 (int)c - 33, so a byte below 33 is negative and therefore "bad" (as in quade_pairtrim.h)
//   positions   : i with max(0, I* - L2) <= i < min(L1, I*), with partner j = I* - 1 - i; every such i, j lies inside what the overlap
//                 stage keeps of both reads (<= Lp <= Lout)
//   mismatch    : a position mismatches iff not (valid(s1[i]) and u(s2[j]) == comp(u(s1[i]))): the overlap stage's definition exactly
//   at a mismatching position, with G = good_quality and B = bad_quality (B < G, so at most one of the first two cases holds):
//     1. if valid(s1[i]) and phred(q1[i]) >= G and phred(q2[j]) <= B: s2[j] = comp(u(s1[i])) and q2[j] = q1[i] -- R2 is corrected
//     2. else if valid(s2[j]) and phred(q2[j]) >= G and phred(q1[i]) <= B: s1[i] = comp(u(s2[j])) and q1[i] = q2[j] -- R1 is corrected
//     3. else nothing is written: the position is unresolved
//   The written base is upper case.  The doubtful byte may be anything (N, lower case, any other byte); the trusted one must be a letter.
//   properties  : nothing else in the text changes; no length changes and no pair is dropped; names, index reads and the :IDX[:MOL]
//                 tag never change; a position's outcome depends on its own four bytes only; applying the rule twice equals applying it
//                 once, because a corrected position matches afterwards
//
// Stores.  Every store is one byte, by the one lane that owns the position (plain C++ stores).  A wider read-modify-write store would
// lose another lane's correction in the same dword, or another row's correction in a neighbouring record that shares the 16-byte
// word.  make_line's aligned loads (quade_row.h) do read bytes of neighbouring lines, in this kernel and in every stage behind it;
// those bytes are masked or never compared, so a concurrent write to them is harmless.  Within a pair the positions i are distinct and
// so are their partners j: no byte has two writers, and the row reads its own lines into the slab before a barrier and writes behind it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"

enum {
    QD_PC_R1_READS = 0,    // R1 reads with at least one corrected base
    QD_PC_R1_BASES = 1,    // bases written into R1 (case 2)
    QD_PC_R2_READS = 2,    // R2 reads with at least one corrected base
    QD_PC_R2_BASES = 3,    // bases written into R2 (case 1)
    QD_PC_PAIRS = 4,       // pairs seen
    QD_PC_OVERLAPPED = 5,  // pairs with an I* (I* != 0)
    QD_PC_OVERLAP_BASES = 6,  // sum of ov(I*) = the positions looked at
    QD_PC_MISMATCHES = 7,  // mismatching positions: R1 bases + R2 bases + unresolved, by construction
    QD_PC_UNRESOLVED = 8,  // case 3
    QD_PC_CORRECTED_PAIRS = 9,  // pairs with at least one write
    QD_PC_VALUES = 10,
};

// the kernel's parameters (checked by qd_paircorrect_set): quality BYTES, 33 + phred
struct qd_paircorrect_dev {
    uint32_t good_byte;  // a trusted call has a quality byte >= this (34 .. 126)
    uint32_t bad_byte;   // a doubtful call has a quality byte <= this (33 .. good_byte - 1)
};

// Pairs [0, n): insert[j] is the pair's I* (0 = none; a value above L1 + L2 has no positions either).  Corrects text[0] / text[1]
// in place through recs (seq, qual, seq_len) and adds to table (uint64[10]).  Device pointers, returns after the launch.  n < 2^31.
struct qd_paircorrect_args {
    uint8_t* text[2];
    const qd_rec* recs[2];
    const uint64_t* insert;
    uint64_t* table;
};
hipError_t qd_paircorrect_launch(const qd_paircorrect_dev& P, const qd_paircorrect_args& a, uint32_t n, hipStream_t st);

// The context's parameters and table (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, directly behind
// qd_pairtrim_device_inserts, after asking qd_paircorrect_active whether there is anything to do (off: no buffers, no launch).
extern "C" int qd_paircorrect_active(const qd_ctx* ctx);
extern "C" int qd_paircorrect_device(qd_ctx* ctx, uint8_t* text1, const qd_rec* recs1, uint8_t* text2, const qd_rec* recs2,
                                     const uint64_t* inserts, uint32_t n, void* stream);
