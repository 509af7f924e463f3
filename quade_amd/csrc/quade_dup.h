// Duplication report (opt-in, qd_dup_set): the read-pair keys of a batch tallied in a device-resident table -- parameters as the
// kernels take them, table layouts and launch entry points (quade_dup.hip).  No reference counterpart: Quade 0.3.2 reports pair
// counts only.
//
// Definition (include/quade_hip.h, tests/dup_model.py and the kernels state exactly this).  Parameters: B = bases (8 .. 32),
// sample (a power of two, 1 .. 1024), slots (a power of two, 2^10 .. 2^28).  Per pair that carries no filter reason, with reads
// s1, s2 of current lengths L1, L2 and starts as the record tables in force give them (a front clip moves the start):
//   fold     u(b) = b & 0xDF; a base is valid when u(b) is one of A, C, G, T
//   code     c(b) = (u(b) >> 1) & 3: A 0, C 1, T 2, G 3
//   class    the first that applies: short (L1 < B or L2 < B), with_n (an invalid base among the first B of either read), keyed
//   key      (w1, w2, d): w_r = sum over i < B of c(s_r[i]) << (2 i) (no shift by 64 at B = 32); d = the destination as qd_qstats
//            numbers it (the routing code, 0xFFFF -> 2 S).  Equal sequences in two destinations are two keys
//   hash     h = qd_uk_tag({w1, w2, d, 0}) (quade_unknown.h)
//   sampled  sample == 1, or h >> (64 - log2 sample) == 0: key-space sampling, a sampled key keeps its exact multiplicity and
//            every context and rank samples the same keys
//   tally    sampled pairs are counted per key in a table of `slots` entries per context; slot tag qd_uk_trim(h, tag_mask), home
//            slot qd_uk_home, probe limit min(slots, 1024), all as in the unknown tally.  A pair that finds no entry within the
//            probe limit, or whose tag belongs to another key, is not_tallied
//
// Counters: uint64[(2 * S + 1)][QD_DUP_VALUES], destination-major as qd_qstats (QD_DP_VALUES here is the public QD_DUP_VALUES).
// Per destination sampled == tallied + not_tallied, tallied being the sum of the counts of the table's entries of that destination.
// Key table: an UnknownTable (quade_unknown.h) of four key words per slot: {w1, w2, d, 0}; its totals: QD_UK_TALLIED and
// QD_UK_DISTINCT (the other two stay 0: short and not_tallied are counted per destination).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quade_text.h"
#include "quade_unknown.h"

enum {
    QD_DP_PAIRS = 0,        // pairs seen (no filter reason)
    QD_DP_SHORT = 1,        // a read shorter than B
    QD_DP_WITH_N = 2,       // an invalid base among the first B of either read
    QD_DP_SAMPLED = 3,      // keyed pairs whose key is in the sample
    QD_DP_NOT_TALLIED = 4,  // sampled pairs the table did not admit
    QD_DP_VALUES = 5,       // per destination
};
#define QD_DUP_KEY_WORDS 3 /* (w1, w2, d) as listed and read out */

// which accumulation a launch for n_samples takes
enum { QD_DUP_PATH_LDS = 1, QD_DUP_PATH_GLOBAL = 2 };
// 32-bit partials of a workgroup live in LDS up to the read filter's bound: 2048 destinations (40 KiB of counters), S <= 1023
#define QD_DUP_LDS_MAX_DEST 2048u

static inline size_t qd_dup_values(uint32_t n_samples) { return ((size_t)2 * n_samples + 1) * QD_DP_VALUES; }
static inline int qd_dup_path(uint32_t n_samples) { return 2 * n_samples + 1 <= QD_DUP_LDS_MAX_DEST ? QD_DUP_PATH_LDS : QD_DUP_PATH_GLOBAL; }

// the kernels' parameters (checked by qd_dup_set)
struct qd_dup_dev {
    int32_t bases;      // B
    int32_t sample_lg;  // log2(sample)
};

// the batch list of a stream: [0] the number of listed pairs (the kernels' own counter, zeroed in front of dup_keys), then from
// byte QD_DUP_LIST_HEAD on the keys uint64[cap][3], then each listed pair's slot uint32[cap]
#define QD_DUP_LIST_HEAD 16
static inline size_t qd_dup_list_bytes(size_t cap) { return QD_DUP_LIST_HEAD + cap * (QD_DUP_KEY_WORDS * 8 + 4); }

// Pairs [0, n): pair j is recs[r][j] in text[r] (r = 0: R1, 1: R2), routed by codes[j]; drop != NULL: pair j is skipped where
// drop[j] != 0 (the read filter's reason bytes).  Device pointers.  n < 2^31, and the list has room for n pairs.
struct qd_dup_args {
    const uint8_t* text[2];
    const qd_rec* recs[2];
    const uint16_t* codes;
    const uint8_t* drop;  // optional
    uint64_t* table;      // the counters
    uint32_t* list_n;     // the batch list: its length ...
    uint64_t* list;       // ... its keys [n][3] ...
    uint32_t* where;      // ... and the slots the claim found [n]
    UnknownTable t;
};
// dup_keys, then dup_claim and dup_count over the list, on st.  `before_claim` (may be NULL): an event the stream waits for in
// front of dup_claim (the previous launch's dup_count, whatever stream it ran on).
hipError_t qd_dup_launch(const qd_dup_dev& P, const qd_dup_args& a, uint32_t n_samples, uint32_t n, int cus, hipEvent_t before_claim,
                         hipStream_t st);

// A stream that carried work of the context is idle and may be destroyed before the context waits again (the pipeline's compute
// stream at the end of qd_pipe_run): the context drops the events it recorded on it -- its "work up to here" marker and, where that
// stream ran last, the two tallies' ordering events.  An event must not be waited for once its stream is gone.
extern "C" int qd_stream_retired(qd_ctx* ctx, void* stream);

// The context's parameters and tables (quade_api.cpp): what qd_pipe_run calls once per batch on its compute stream, after asking
// qd_dup_active whether there is anything to do (off: no buffer, no launch).
extern "C" int qd_dup_active(const qd_ctx* ctx);
extern "C" int qd_dup_device(qd_ctx* ctx, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                             const uint16_t* codes, const uint8_t* drop, void* stream);
