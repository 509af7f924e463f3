/*
 * quade_hip.h -- C ABI of the MI355X (gfx950) demultiplexing library, libquade_hip.so.
 *
 * Drop-in boundary for the per-read hot path of a-slide/Quade 0.3.2.  The reference has no FFI:
 * its seam is one Python classmethod call per read pair.  Each entry point below names the
 * reference interface it replaces (file:line under /root/reference).  The library is
 * batch-granular: one call processes n read pairs whose index reads were packed into
 * fixed-stride rows (layout: qd_layout).
 *
 * Conventions
 *   - plain C types only; every function returns QD_OK (0) or a negative QD_ERR_* code;
 *     qd_last_error() gives the text.  No exceptions or callbacks cross the boundary.
 *   - a qd_ctx is bound to one HIP device and must be driven by one thread at a time;
 *     different contexts may be driven concurrently from different threads.
 *   - there is NO CPU fallback: qd_create() fails with QD_ERR_NO_DEVICE when no gfx950 device is
 *     usable.  The host-only helpers (qd_plan_layout, qd_pack_*, qd_fastq_*, qd_build_tags,
 *     qd_format_records, qd_version, qd_strerror) never touch the GPU.
 *
 * Routing code (uint16) written per pair -- src/Sample.py:65-91:
 *     0xFFFF            index matches no sample            (Sample.py:86-91, "Undetermined")
 *     2*ordinal         matched, min phred >= minimal_qual (Sample.py:70-75, "<name>_pass")
 *     2*ordinal + 1     matched, quality gate failed       (Sample.py:78-83, "<name>_fail")
 *   ordinal = position of the sample in SAMPLE_LIST, i.e. order of the [sampleN] sections
 *   (src/Quade.py:133, src/Sample.py:153).
 *
 * Counter vector (uint64[2*S+4]) -- src/Sample.py:32,62,71-72,79-80,88:
 *     [0] TOTAL  [1] PASS_QUAL  [2] FAIL_QUAL  [3] UNDETERMINED
 *     [4+2*i] sample i pass_qual   [5+2*i] sample i fail_qual
 */
#ifndef QUADE_HIP_H
#define QUADE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QD_ABI_VERSION 6

#define QD_OK 0
#define QD_ERR_INVALID (-1)     /* bad argument (NULL pointer, misaligned buffer, size out of range)   */
#define QD_ERR_NO_DEVICE (-2)   /* no usable HIP device / not gfx950 -- the library never falls back   */
#define QD_ERR_HIP (-3)         /* a HIP runtime call failed; text in qd_last_error()                   */
#define QD_ERR_STATE (-4)       /* call order: plan and barcodes must be set before demux/submit        */
#define QD_ERR_UNSUPPORTED (-5) /* plan outside the supported envelope (window > QD_MAX_WINDOW ...)     */
#define QD_ERR_BARCODE (-6)     /* barcode table rejected (duplicate index: src/Sample.py:140)          */
#define QD_ERR_FORMAT (-7)      /* malformed fastq text handed to a host helper                         */

#define QD_CODE_UNDETERMINED 0xFFFFu
#define QD_MAX_WINDOW 64   /* widest index-read window (idx U mol) kept per row, bytes                  */
#define QD_MAX_KEY 32      /* longest fused barcode the match kernels compare, bytes                    */
#define QD_MAX_SAMPLES 32767

typedef struct qd_ctx qd_ctx;

/* ---- plan: the parameters the hot path reads (src/Quade.py:96-116) -------------------------------
 * start values are 0-based (the conf's 1-based start minus 1, Quade.py:106), end values are the
 * conf's 1-based inclusive ends, so a slice is read[start:end] exactly as Quade.py:217-218,246-247.
 * Disabled parts are 0:0 (Quade.py:109-116).  min_qual is the phred threshold (Quade.py:96,
 * Sample.py:70), 0..40 (Quade.py:262). */
typedef struct qd_plan {
    int32_t dual;     /* [index] index2 (Quade.py:100): 1 = two index reads fused, 0 = one */
    int32_t min_qual; /* [quality] minimal_qual */
    int32_t idx1_start, idx1_end;
    int32_t idx2_start, idx2_end;
    int32_t mol1_start, mol1_end;
    int32_t mol2_start, mol2_end;
} qd_plan;

/* ---- row layout derived from a plan --------------------------------------------------------------
 * For index stream k (0 = index_R1, 1 = index_R2):
 *   seq row  : seq_stride[k] bytes = columns [seq_off[k], seq_off[k]+seq_width[k]) of the read's
 *              sequence line, as read (case preserved), zero-padded (0x00) to the stride and where
 *              the read is shorter than the window.
 *   qual row : qual_stride[k] bytes = quality characters (Phred+33 text, as read) of columns
 *              [qual_off[k], qual_off[k]+qual_width[k]) = the barcode slice only (Sample.py:70 takes
 *              the minimum over the fused barcode positions, nothing else), padded with 0xFF.
 *   len row  : optional uint8 per read = min(255, read length).  Omitted (NULL) when every read of
 *              the batch covers its whole window -- then the fast kernels run.
 * Outputs: codes = uint16 per pair; mol = mol_width bytes per pair (raw case, I1 part then I2 part
 * packed together, zero padded when reads are short) -- Quade.py:218.  A stride is its window's width
 * rounded up to an even number of bytes (minimum 2), so rows carry at most one byte of padding.     */
typedef struct qd_layout {
    int32_t n_streams;
    int32_t seq_off[2], seq_width[2], seq_stride[2];
    int32_t qual_off[2], qual_width[2], qual_stride[2];
    int32_t key_width; /* K = fused barcode slice width = sum of (idx_end-idx_start)            */
    int32_t mol_width; /* M = fused molecular slice width; 0 when both molecular flags are off  */
} qd_layout;

/* Host only.  Replaces nothing in the reference; states the packing contract. */
int qd_plan_layout(const qd_plan* plan, qd_layout* out);

/* ---- library ------------------------------------------------------------------------------------*/
int qd_version(void);
const char* qd_strerror(int code);
/* Text of the last error on this context (ctx == NULL: last error of qd_create on this thread). */
const char* qd_last_error(const qd_ctx* ctx);

/* ---- context --------------------------------------------------------------------------------------
 * qd_create replaces the implicit process-global state of src/Sample.py:32-44 (one run per
 * process) with an explicit context bound to HIP device `device_id`. */
int qd_device_count(int32_t* n_devices); /* gfx950 or not; QD_ERR_NO_DEVICE when the runtime finds none */
int qd_create(int device_id, qd_ctx** out);
int qd_destroy(qd_ctx* ctx);
/* name: >= 64 bytes.  Any output pointer may be NULL. */
int qd_device_info(const qd_ctx* ctx, char* name, int32_t name_cap, int32_t* compute_units,
                   int64_t* total_mem_bytes);

/* Replaces Sample.CLASS_INIT(min_qual=...) (src/Sample.py:48-54, called at src/Quade.py:125-129)
 * and the position fields of Quade.__init__ (src/Quade.py:99-116).  The write_* flags are not a
 * device concern: counters move regardless (Sample.py:71-91) and routing is decided by code.
 * Resets the mismatch budgets (qd_set_mismatches) to 0. */
int qd_set_plan(qd_ctx* ctx, const qd_plan* plan);
int qd_get_layout(const qd_ctx* ctx, qd_layout* out);

/* Replaces the registration side of Sample.__init__ (src/Sample.py:132-153, called at
 * src/Quade.py:137,139): n_samples upper-case barcodes in ordinal order, concatenated in
 * `barcodes`, barcode i = barcodes[offsets[i] .. offsets[i+1]).  Lengths may differ from the slice
 * width and from each other (the reference never checks, Sample.py:132-141); such a barcode can
 * only match reads whose clamped slice has exactly that length.  Duplicate -> QD_ERR_BARCODE.
 * Alphabet checks stay on the Python side (message text parity, Sample.py:141). Resets counters and the
 * mismatch budgets (qd_set_mismatches). */
int qd_set_barcodes(qd_ctx* ctx, int32_t n_samples, const uint8_t* barcodes, const int32_t* offsets);

/* ---- device-resident hot path ---------------------------------------------------------------------
 * Replaces, for n_pairs reads at once: index/molecular extraction and fusion (src/Quade.py:217-218,
 * 246-247) + Sample.FINDER (src/Sample.py:56-91).  All pointers are DEVICE pointers, 16-byte
 * aligned, laid out as qd_layout says.  seq[1]/qual[1]/len[1] are ignored for a single-index plan.
 * codes_dev: n_pairs uint16.  mol_dev: n_pairs*mol_width bytes, may be NULL when mol_width == 0.
 * `stream` is a hipStream_t: NULL is HIP's null (default) stream, ordered with the caller's other
 * default-stream work; QD_STREAM_CONTEXT is the context's own non-blocking stream.  Asynchronous:
 * returns after the launch.  Counters accumulate in the context.  The library never synchronises the
 * whole device: rows written by work on ANOTHER stream must be complete (or ordered by the caller)
 * before the launch on `stream` reads them. */
#define QD_STREAM_CONTEXT ((void*)(intptr_t)-1)
typedef struct qd_rows {
    const uint8_t* seq[2];
    const uint8_t* qual[2];
    const uint8_t* len[2]; /* NULL: every read covers its window */
} qd_rows;
int qd_demux_device(qd_ctx* ctx, int64_t n_pairs, const qd_rows* rows, uint16_t* codes_dev,
                    uint8_t* mol_dev, void* stream);

/* Ragged batch: some reads are shorter than their window (Python slice clamping of a short index
 * read, src/Quade.py:217-218), and the caller knows which.  rows->len must be given;
 * short_idx_dev[0..n_short) = the pair indices (device memory, unique, any order) at which ANY stream's
 * read is shorter than seq_off+seq_width of that stream.  When the plan is eligible for the fast
 * kernels, the whole batch runs on them and only the listed pairs are redone with the length-aware
 * byte-granular path (results and counters are those of running every pair that way); otherwise, or
 * when more than half of the pairs are listed, the generic kernel takes the batch. */
int qd_demux_device_ragged(qd_ctx* ctx, int64_t n_pairs, const qd_rows* rows, uint16_t* codes_dev, uint8_t* mol_dev,
                           int64_t n_short, const uint32_t* short_idx_dev, void* stream);

/* Which kernel qd_demux_device would launch for a batch: 1 = fast (LDS table, vector rows),
 * 2 = generic.  Informational (tests, bench). */
int qd_kernel_kind(const qd_ctx* ctx, int has_len);

/* Tuning / test knobs (no reference counterpart).  Names:
 *   "fast_workgroups_per_cu"  0 = automatic (default), 1..4096 = fixed
 *   "fast_block"              0 = automatic (default), 256 / 512 / 1024 threads per workgroup
 *   "mol_strips"              1 = stage molecular bytes through LDS for 16-byte stores (default), 0 = off
 *   "force_generic"           1 = always launch the generic kernel
 *   "kernel"                  0 = automatic (default), 1 = fast (when the plan is eligible), 2 = generic
 *   "fold_pairs"              the device counts into 32-bit per-workgroup rows that are folded into 64-bit totals
 *                             before this many pairs have been launched since the last fold (default and
 *                             maximum 2^32 - 1; tests lower it)
 *   "unknown_tag_bits"        (tests only: the unknown-barcode tally keeps the low b bits of a key's 64-bit tag, 1..64,
 *                             default 64, so that tag collisions can be produced at will; set it before the first
 *                             tallied launch or right after qd_reset_counts)
 *   "dup_tag_bits"            (tests only: the same knob for the duplication tally's table, qd_dup_set) */
int qd_set_option(qd_ctx* ctx, const char* name, int64_t value);

/* ---- mismatch-tolerant matching (opt-in; no reference counterpart: Quade 0.3.2 matches exactly) ---------
 * Budgets m1 (index read 1's part of the fused barcode, bytes [0, w1) with w1 = idx1_end - idx1_start) and m2
 * (index read 2's part, [w1, K)), each 0..2.  A pair whose exact lookup fails and whose fused slice is K bytes
 * long is assigned to the barcode of length K with ham(key[0:w1], bc[0:w1]) <= m1 and ham(key[w1:K], bc[w1:K])
 * <= m2 (bytes compared after the case fold: N is an ordinary symbol).  Exact hits, short slices and barcodes
 * of another length behave as with budgets 0.  The quality gate, the codes and the counter layout are
 * unchanged: a rescued pair counts as its sample's pass or fail.  The rescue is a post-pass of every launch
 * (qd_demux_device, _ragged, qd_submit, qd_submit_ragged) on the launch's stream; with budgets 0 none runs.
 *
 * Collision rule: barcodes A and B of length K collide when d1 <= 2*m1 and d2 <= 2*m2 (per-part Hamming
 * distances), i.e. exactly when some pair is within budget of both.  Host only, never touches the GPU:
 * returns QD_OK (*first = *second = -1) or QD_ERR_BARCODE with the first colliding ordinal pair (first <
 * second, lexicographic); QD_ERR_INVALID on bad arguments.  Brute force over all pairs (SWAR, up to 16
 * threads): DESIGN.md 4.8 gives its time at S = QD_MAX_SAMPLES. */
int qd_check_mismatch_collisions(int32_t n_samples, const uint8_t* barcodes, const int32_t* offsets, int32_t key_width,
                                 int32_t w1, int32_t m1, int32_t m2, int32_t* first, int32_t* second);
/* Sets the budgets of this context.  Needs qd_set_plan and qd_set_barcodes first (QD_ERR_STATE); m1, m2 in
 * 0..2 and m2 == 0 for a single-index plan (QD_ERR_INVALID); runs the collision check on the registered
 * barcodes (QD_ERR_BARCODE, qd_last_error names the two ordinals) and builds the device tables.  Waits for
 * the context's outstanding work.  qd_set_plan and qd_set_barcodes reset both budgets to 0. */
int qd_set_mismatches(qd_ctx* ctx, int32_t m1, int32_t m2);

/* ---- top unknown barcodes (opt-in; no reference counterpart: Quade 0.3.2 only writes the Undetermined files) ------
 * A device-resident table of `slots` entries counts the fused barcode keys of the pairs whose FINAL routing code is
 * 0xFFFF (after the exact kernels, the ragged fix-up and the mismatch rescue).  The key is the pair's fused slice of
 * key_width bytes after the case fold, index read 1's part then index read 2's -- the key the lookup uses; N and
 * any other byte are ordinary symbols.  A pair with a read that ends inside its index window is not tallied by
 * sequence: it adds 1 to `short`.  A key the table cannot admit (no free entry within the probe limit of 1024, or
 * another key with the same 64-bit tag holds the entry) adds 1 to `dropped`.  For all work launched since the tally
 * was enabled or emptied: sum(counts) + short + dropped == qd_get_counts()[3].  Every entry's count is exact; a key
 * that is not in the table has at most `dropped` occurrences.  The tally is a post-pass of every launch
 * (qd_demux_device, _ragged, qd_submit, qd_submit_ragged, qd_pipe_run) on the launch's stream; launches on different
 * streams are ordered among themselves (the tally kernels only).  Disabled, nothing is launched or allocated.
 *
 * qd_unknown_enable: slots == 0 turns the tally off and frees the table; otherwise a power of two in 2^10 .. 2^28
 * (48 bytes each; QD_ERR_INVALID).  Needs qd_set_plan and qd_set_barcodes first (QD_ERR_STATE), waits for the
 * context's outstanding work.  qd_set_plan and qd_set_barcodes turn the tally off; qd_reset_counts empties it.
 * qd_unknown_stats: out = {tallied pairs, short, dropped, distinct entries}; waits for the context's work;
 * QD_ERR_STATE when the tally is off.
 * qd_unknown_read: the occupied entries are packed on the device and only they are downloaded; entry i is
 * keys[i*key_width .. (i+1)*key_width) with counts[i], in no particular order (sort on the host).  Returns the number
 * of entries, or -(entries needed) when cap is too small (cap 0 with NULL arrays asks for the size), or a value
 * <= QD_UNKNOWN_READ_ERROR on failure: QD_UNKNOWN_READ_ERROR + QD_ERR_* (qd_last_error has the text). */
#define QD_UNKNOWN_READ_ERROR (-((int64_t)1 << 40))
int qd_unknown_enable(qd_ctx* ctx, int64_t slots);
int qd_unknown_stats(qd_ctx* ctx, uint64_t out[4]);
int64_t qd_unknown_read(qd_ctx* ctx, uint8_t* keys, uint64_t* counts, int64_t cap);

/* ---- index-hopping matrix (opt-in, additive: QD_ABI_VERSION stays 6; no reference counterpart) -------------------------
 * For a dual plan (qd_plan.dual == 1) with K = key_width, w1 = idx1_end - idx1_start and w2 = K - w1, both > 0.
 * Part lists: take the samples whose registered barcode is K bytes long, in ordinal order (a barcode of another length is
 * "off the matrix" and takes no part).  P1 = the distinct values of bc[0:w1] in order of first appearance, P2 = the same for
 * bc[w1:K]; n1 = |P1|, n2 = |P2|; sample s has part1[s] and part2[s], both -1 when it is off the matrix.  A cell (a, b) is
 * "on the sheet" when some sample has exactly that pair.
 * Table: uint64[(n1+1) * (n2+1) + 1], row-major; row n1 = "index 1 matches no part", column n2 = "index 2 matches no part";
 * the last value is `short`.
 * Counted is every pair whose FINAL routing code is 0xFFFF (after the exact kernels, the ragged fix-up and the mismatch
 * rescue): the pairs the unknown tally counts.  A pair with a read that ends inside its index window (the row is zero padded
 * there) adds 1 to `short`.  Otherwise a = the index in P1 of the pair's index-1 slice after the case fold, or n1 when it
 * equals none, b the same for index 2 (N and any other byte are ordinary symbols), and cell (a, b) += 1.
 * Matching per part is exact whatever the mismatch budgets are: a tolerant match per part is not unique (the collision rule
 * holds for whole barcodes only), so with budgets above 0 the rates derived from the table are lower bounds.
 * For all work launched since the matrix was enabled or zeroed: sum(table) == qd_get_counts()[3], and every on-sheet cell is 0
 * (such a pair would have matched exactly).  Limit: (n1+1) * (n2+1) <= 2^24 (128 MiB per context).
 * The matrix is one more post-pass of every launch (qd_demux_device, _ragged, qd_submit, qd_submit_ragged, qd_pipe_run) on the
 * launch's stream; it is updated with atomics only, so launches on different streams need no order among themselves.
 * Disabled, nothing is launched or allocated.
 *
 * qd_hop_index: host only, never touches the GPU -- the one definition of the part lists.  Writes part1[n_samples],
 * part2[n_samples], *n1, *n2.  QD_ERR_INVALID on bad arguments (1 <= w1 < key_width <= QD_MAX_KEY), QD_ERR_UNSUPPORTED when
 * the sheet is over the limit (the outputs are written all the same).
 * qd_hop_enable: on != 0 builds the part tables, allocates and zeroes the table; 0 frees everything.  Needs qd_set_plan and
 * qd_set_barcodes first (QD_ERR_STATE), a dual plan with w1, w2 > 0 (QD_ERR_INVALID) and a sheet within the limit
 * (QD_ERR_UNSUPPORTED); waits for the context's outstanding work.  qd_set_plan and qd_set_barcodes turn the matrix off;
 * qd_reset_counts zeroes it.
 * qd_hop_shape: n1 and n2; QD_ERR_STATE when off.
 * qd_hop_read: waits for the context's work, writes n_values = (n1+1)*(n2+1)+1 values (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).
 * qd_hop_add: another context's table (qd_hop_read's layout) joins this one's, as qd_qstats_add does. */
int qd_hop_index(int32_t n_samples, const uint8_t* barcodes, const int32_t* offsets, int32_t key_width, int32_t w1, int32_t* part1,
                 int32_t* part2, int32_t* n1, int32_t* n2);
int qd_hop_enable(qd_ctx* ctx, int32_t on);
int qd_hop_shape(const qd_ctx* ctx, int32_t* n1, int32_t* n2);
int qd_hop_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_hop_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- yield and quality per destination (opt-in; no reference counterpart: Quade 0.3.2 reports pair counts only) ------
 * A device-resident table of exact uint64 counters, [(2*S+1)][2][6], destination-major: destination d = routing code,
 * 0xFFFF -> 2*S (even = <sample>_pass, odd = <sample>_fail, as the files); read 0 = R1, 1 = R2; counters
 *   0 records    pairs routed to d
 *   1 bases      sum of the records' sequence lengths (without a trailing '\r')
 *   2 qual_sum   sum over the quality bytes b (unsigned, 0..255) of q = max(0, b - 33)
 *   3 q20_bases  quality bytes with q >= 20        4 q30_bases  ... with q >= 30
 *   5 n_bases    sequence bytes 'N' or 'n'
 * The insert reads only reach the device in the device pipeline: qd_pipe_run counts every pair it routes (one launch per
 * batch on its compute stream, no host sync), whatever the write flags say -- a destination that is not written is still
 * counted; a chunk part (skip_kept, max_pairs) counts exactly its pairs.  The other launch paths (qd_demux_device,
 * qd_submit*) never see the insert reads and count nothing.  Disabled, nothing is launched or allocated.
 *
 * qd_qstats_enable: on != 0 allocates and zeroes the table (96 * (2*S+1) bytes), 0 frees it.  Needs qd_set_plan and
 * qd_set_barcodes first (QD_ERR_STATE), waits for the context's outstanding work.  qd_set_plan and qd_set_barcodes turn
 * the counters off; qd_reset_counts zeroes them.
 * qd_qstats_read: waits for the context's work, writes n_values = (2*S+1)*12 values (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).
 * qd_qstats_add: another context's table (qd_qstats_read layout) joins this one's, as qd_add_counts does for the pair
 * counters of chunk workers.
 * qd_qstats_kind: how a launch of this context accumulates -- 1 = per-workgroup 32-bit partials in LDS, flushed once per
 * workgroup (2*S+1 <= 1365 destinations), 2 = 64-bit global atomics, equal destinations merged in the wave (more);
 * QD_ERR_STATE when off. */
int qd_qstats_enable(qd_ctx* ctx, int32_t on);
int qd_qstats_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_qstats_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);
int qd_qstats_kind(const qd_ctx* ctx);

/* ---- end clipping, sliding-window quality trimming and poly-G tail trimming of the insert reads (opt-in; no reference
 * counterpart: Quade 0.3.2 writes the insert reads as they came) ----------------------------------------------------------------
 * One stage in front of the 3' trimming below, in fastp's order: fixed trimming, cut_right, poly-G, then adapters.  For an insert
 * read r (R1 or R2) with sequence bytes s, quality bytes q (unsigned) and length L, with u(b) = b & 0xDF and
 * ph[i] = max(0, q[i] - 33); F_r = front_clip[r], T_r = tail_clip[r], W = window_size, Q = window_quality, P = poly_g_min_length.
 * Steps 1 to 3 are each skipped when not configured; their output length is then their input length.
 *   1 fixed clip: f = min(F_r, L) and Lc = max(0, L - f - T_r).  From here on position i means byte f + i of the line.
 *   2 window, W > 0 (Trimmomatic SLIDINGWINDOW, fastp cut_right): Lw = the smallest p in [0, Lc - W] with
 *     ph[p] + .. + ph[p+W-1] < Q * W; Lc when there is none, which includes every read with Lc < W
 *   3 poly-G, P > 0 (fastp's trimPolyG, folded to upper case): for t = 1 .. Lw let b_t = u(s[Lw - t]) and mm(t) the number of
 *     k <= t with b_k != 'G'; stop(t) is true when mm(t) > 5, or when t >= P and 8 * mm(t) > t; T = the smallest t with stop(t),
 *     Lw + 1 when there is none.  If T - 1 >= P then Lg = Lw - g, g being the largest t <= T - 1 with b_t == 'G' (one exists
 *     because P >= 6); otherwise Lg = Lw.  One mismatch per 8 bases, at most 5, a run of at least P, cut at the leftmost G reached
 *   4 floor: Lout = max(Lg, min(min_length, L - f)), min_length being the 3' trimming's.  A front clip is never given back;
 *     everything cut from the 3' end can be
 * and the read's record becomes seq + f, qual + f, seq_len = Lout; its other three fields stay.  Index reads, names and the
 * :IDX[:MOL] tag never change and no pair is dropped.  With the stage on, qd_pipe_run runs it over every pair it routes (one launch
 * per batch on its compute stream, no host sync) directly in front of the 3' trimming, so that the trimming stages, the read
 * filter, the quality and cycle counters and the output stages all see the clipped reads, and adds to a device table
 * uint64[2][12] (R1, R2), whatever the write flags say:
 *   0 reads   1 bases_in (sum of L)   2 bases_out (sum of Lout)   3 front_clipped_reads (f > 0)   4 front_clipped_bases
 *   5 tail_clipped_reads (Lc < L - f)   6 tail_clipped_bases   7 window_reads (Lw < Lc)   8 window_bases
 *   9 polyg_reads (Lg < Lw)   10 polyg_bases   11 floored_reads (Lout > Lg)
 * Off, nothing is allocated or launched.
 *
 * qd_clip_set: NULL, or every rule off (all clips 0, no window, no poly-G), turns the stage off and frees the table; otherwise
 * the values are checked (front_clip and tail_clip 0..1000, window_size 0 = off or 1..100, window_quality 1..93 and set together
 * with window_size or not at all, poly_g_min_length 0 = off or 6..100, min_length 0..65535: QD_ERR_INVALID, the state as before)
 * and a zeroed table allocated.  Waits for the context's outstanding work.  Independent of plan, barcodes and qd_trim_set.
 * qd_clip_get: the parameters in force (all zero and QD_OK when off).
 * qd_clip_read: waits for the context's work, writes n_values = 24 values (QD_ERR_INVALID on another size, QD_ERR_STATE when off).
 * qd_clip_add: another context's table (qd_clip_read's layout) joins this one's, as qd_trim_add does.  qd_reset_counts zeroes
 * the table. */
#define QD_CLIP_VALUES 24
typedef struct qd_clip_params {
    int32_t front_clip[2]; /* R1, R2 */
    int32_t tail_clip[2];
    int32_t window_size;    /* 0 = off */
    int32_t window_quality; /* 0 with window_size 0 */
    int32_t poly_g_min_length; /* 0 = off */
    int32_t min_length;
} qd_clip_params;
int qd_clip_set(qd_ctx* ctx, const qd_clip_params* params);
int qd_clip_get(const qd_ctx* ctx, qd_clip_params* out);
int qd_clip_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_clip_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- 3' quality and adapter trimming of the insert reads (opt-in; no reference counterpart: Quade 0.3.2 writes the insert
 * reads as they came) -----------------------------------------------------------------------------------------------------
 * For an insert read with sequence s, quality bytes q and length L (index reads, names and the :IDX[:MOL] tag never change):
 *   1 quality trim, quality_cutoff C > 0 (cutadapt's / BWA's rule): ph[i] = max(0, q[i] - 33), bytes unsigned; walking i from
 *     L-1 down with a running sum of C - ph[i], stop once it is negative; Lq = the i of its strict maximum above 0, else L
 *   2 adapter trim, an adapter a of length A set for the read: La = the leftmost p < Lq with ov = min(A, Lq - p) >= min_overlap
 *     and at most ov * max_mismatch_pct / 100 (rounded down) positions i < ov where upper(s[p+i]) != a[i] (N and every other
 *     byte mismatch; substitutions only); Lq when there is none
 *   3 floor: Lout = max(La, min(min_length, L))
 * and the read's sequence and quality lines become their first Lout bytes.  The reads only reach the device in the device
 * pipeline: with trimming on, qd_pipe_run trims every pair it routes (one launch per batch on its compute stream, no host sync)
 * before the quality counters (qd_qstats_enable) and the output stages see them, and adds to a device table uint64[2][8] (R1,
 * R2), whatever the write flags say:
 *   0 reads   1 bases_in (sum of L)   2 bases_out (sum of Lout)   3 quality_trimmed_reads (Lq < L)
 *   4 quality_trimmed_bases (sum of L - Lq)   5 adapter_reads (La < Lq)   6 adapter_bases (sum of Lq - La)
 *   7 floored_reads (Lout > La)
 * Off, nothing is allocated or launched.
 *
 * qd_trim_set: NULL, or neither an adapter nor a cutoff, turns trimming off and frees the table; otherwise the values are
 * checked (adapters 0..64 letters of ACGT in either case, quality_cutoff 0..93, min_overlap 1..64 and not above a set adapter's
 * length, max_mismatch_pct 0..50, min_length 0..65535: QD_ERR_INVALID, the state as before) and a zeroed table allocated.  Waits
 * for the context's outstanding work.  Independent of plan and barcodes.
 * qd_trim_get: the parameters in force (adapters upper case; all zero and QD_OK when off).
 * qd_trim_read: waits for the context's work, writes n_values = 16 values (QD_ERR_INVALID on another size, QD_ERR_STATE when off).
 * qd_trim_add: another context's table (qd_trim_read's layout) joins this one's, as qd_qstats_add does.  qd_reset_counts
 * zeroes the table. */
#define QD_TRIM_ADAPTER_MAX 64
typedef struct qd_trim_params {
    uint8_t adapter_r1[QD_TRIM_ADAPTER_MAX]; /* the first adapter_r1_len bytes count */
    uint8_t adapter_r2[QD_TRIM_ADAPTER_MAX];
    int32_t adapter_r1_len; /* 0 = none */
    int32_t adapter_r2_len;
    int32_t quality_cutoff; /* 0 = off */
    int32_t min_overlap;
    int32_t max_mismatch_pct;
    int32_t min_length;
} qd_trim_params;
int qd_trim_set(qd_ctx* ctx, const qd_trim_params* params);
int qd_trim_get(const qd_ctx* ctx, qd_trim_params* out);
int qd_trim_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_trim_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- paired-end overlap trimming of the insert reads with insert sizes (opt-in; no reference counterpart: Quade 0.3.2 never
 * looks at R1 and R2 of a pair together) ------------------------------------------------------------------------------------
 * When the insert is shorter than the reads, R1 and the reverse complement of R2 overlap over the whole insert and everything
 * behind it is adapter, whatever its sequence.  Per pair, the two insert reads as the stage receives them -- behind the 3'
 * trimming above when that is on, as scanned otherwise: sequences s1, s2 of current lengths L1, L2 (only the first L bytes of
 * each count).
 *   fold      : u(b) = b & 0xDF; a base is valid only if u(b) is one of A C G T; comp maps A<->T and C<->G
 *   candidate : an insert length I, 1 <= I <= L1 + L2, pairs position i of R1 with position j = I - 1 - i of R2 for all i with
 *               0 <= i < L1 and 0 <= j < L2; the number of such positions is ov(I) = min(L1, I) - max(0, I - L2).  A position
 *               matches iff u(s1[i]) is valid and u(s2[j]) == comp(u(s1[i])); everything else is a mismatch, N in either read
 *               and N opposite N included.  I is accepted iff ov(I) >= min_overlap and
 *               mismatches <= min(max_mismatches, ov(I) * max_mismatch_pct / 100) (rounded down)
 *   insert I* : with M = max(L1, L2): the smallest accepted I >= M if there is one (the reads overlap or the insert spans them;
 *               nothing is cut, and a tandem repeat that also matches at a shorter I causes no trim); otherwise the largest
 *               accepted I < M; otherwise there is none
 *   cut       : I* < M: Lp_r = min(L_r, I*) for each read; otherwise Lp_r = L_r
 *   floor     : Lout_r = max(Lp_r, min(min_length, L_r)), min_length being the 3' trimming's.  That stage applied the same floor:
 *               it left L_r >= min(min_length, L0_r) of a read of L0_r bases, so L_r < min_length only where L_r == L0_r and
 *               min(min_length, L_r) == min(min_length, L0_r) either way -- the stage's input length serves as L_r
 * and the read's sequence and quality lines become their first Lout_r bytes.  Index reads, names and the :IDX[:MOL] tag never
 * change and no pair is dropped.  With the stage on, qd_pipe_run runs it over every pair it routes (one launch per batch on its
 * compute stream, no host sync) directly behind the 3' trimming and before the quality counters (qd_qstats_enable) and the output
 * stages see the reads, and adds to a device table of 1040 uint64, whatever the write flags say:
 *   [2][6] per read R1, R2: 0 reads   1 bases_in (sum of L)   2 bases_out (sum of Lout)   3 overlap_trimmed_reads (Lp < L)
 *                           4 overlap_trimmed_bases (sum of L - Lp)   5 floored_reads (Lout > Lp)
 *   [12] pairs   [13] overlapped_pairs (an I* exists)   [14] short_insert_pairs (I* < M)
 *   [15 .. 1039] the insert sizes: bin I* for I* < 1024, the last bin for I* >= 1024
 * Off, nothing is allocated or launched.
 *
 * qd_pairtrim_set: NULL turns the stage off and frees the table; otherwise the values are checked (min_overlap 8..1000,
 * max_mismatches 0..64, max_mismatch_pct 0..50, min_length 0..65535: QD_ERR_INVALID, the state as before) and a zeroed table
 * allocated.  Waits for the context's outstanding work.  Independent of plan, barcodes and qd_trim_set.
 * qd_pairtrim_get: the parameters in force (all zero and QD_OK when off).
 * qd_pairtrim_read: waits for the context's work, writes n_values = 1040 values (QD_ERR_INVALID on another size, QD_ERR_STATE
 * when off).
 * qd_pairtrim_add: another context's table (qd_pairtrim_read's layout) joins this one's, as qd_trim_add does.  qd_reset_counts
 * zeroes the table. */
#define QD_PAIRTRIM_VALUES 1040
typedef struct qd_pairtrim_params {
    int32_t min_overlap;
    int32_t max_mismatches;
    int32_t max_mismatch_pct;
    int32_t min_length;
} qd_pairtrim_params;
int qd_pairtrim_set(qd_ctx* ctx, const qd_pairtrim_params* params);
int qd_pairtrim_get(const qd_ctx* ctx, qd_pairtrim_params* out);
int qd_pairtrim_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_pairtrim_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- overlap base correction of read pairs (opt-in; no reference counterpart: Quade 0.3.2 never looks at R1 and R2 of a pair
 * together) ---------------------------------------------------------------------------------------------------------------------
 * What fastp does under --correction: at a disagreeing position of an accepted overlap the instrument read the same base twice,
 * and the confident call, with its quality, is written over the doubtful one.  The first stage that edits the text itself.
 *
 * The rule (tests/paircorrect_model.py and quade_amd/csrc/quade_paircorrect.h state exactly this).  The stage runs directly behind the
 * overlap trimming stage and in front of post-trimming, over every pair for which that stage found an insert length I* (I* >= M and
 * I* < M alike), whatever its destination, the write flags and later filtering.  It uses the record tables the overlap stage
 * RECEIVED: sequences s1, s2 and quality lines q1, q2 of lengths L1, L2, starting at the tables' seq / qual (a 5' clip is respected).
 *   definitions : u(b) = b & 0xDF; valid(b) iff u(b) is one of A C G T; comp maps A<->T and C<->G; the phred of a quality byte c is
 *                 (int)c - 33, so a byte below 33 is negative and therefore "bad" (as in quade_pairtrim.h)
 *   positions   : i with max(0, I* - L2) <= i < min(L1, I*), with partner j = I* - 1 - i; every such i, j lies inside what the overlap
 *                 stage keeps of both reads (<= Lp <= Lout)
 *   mismatch    : a position mismatches iff not (valid(s1[i]) and u(s2[j]) == comp(u(s1[i]))): the overlap stage's definition exactly
 *   at a mismatching position, with G = good_quality and B = bad_quality (B < G, so at most one of the first two cases holds):
 *     1. if valid(s1[i]) and phred(q1[i]) >= G and phred(q2[j]) <= B: s2[j] = comp(u(s1[i])) and q2[j] = q1[i] -- R2 is corrected
 *     2. else if valid(s2[j]) and phred(q2[j]) >= G and phred(q1[i]) <= B: s1[i] = comp(u(s2[j])) and q1[i] = q2[j] -- R1 is corrected
 *     3. else nothing is written: the position is unresolved
 *   The written base is upper case.  The doubtful byte may be anything (N, lower case, any other byte); the trusted one must be a letter.
 *   properties  : nothing else in the text changes; no length changes and no pair is dropped; names, index reads and the :IDX[:MOL]
 *                 tag never change; a position's outcome depends on its own four bytes only; applying the rule twice equals applying it
 *                 once, because a corrected position matches afterwards
 * Everything behind the stage sees the corrected reads: post-trimming, the read filter, the k-mer screen, the quality, cycle and
 * duplication counters and the output files.  The adapter content still counts the raw reads, and the overlap trimming table is as
 * before.  With the stage on, qd_pipe_run hands every pair's I* from the overlap kernel to this one (64 bits a pair: exact for every
 * L1 + L2 the record tables can express) and launches it once per batch on its compute stream, no host sync; with overlap trimming
 * off it fails with QD_ERR_STATE.  The device table, 10 uint64, whatever the write flags say:
 *   [0] R1 corrected_reads   [1] R1 corrected_bases   [2] R2 corrected_reads   [3] R2 corrected_bases   [4] pairs
 *   [5] overlapped_pairs (I* != 0)   [6] overlap_bases (sum of ov(I*))   [7] mismatches   [8] unresolved
 *   [9] corrected_pairs (pairs with at least one write);   [7] == [1] + [3] + [8] by construction
 * Off, nothing is allocated or launched.
 *
 * qd_paircorrect_set: NULL turns the stage off and frees the table; otherwise the values are checked (good_quality 1..93,
 * bad_quality 0..good_quality - 1: QD_ERR_INVALID, the state as before) and a zeroed table allocated.  Waits for the context's
 * outstanding work.  Independent of plan, barcodes and, at set time, of qd_pairtrim_set.
 * qd_paircorrect_get: the parameters in force (all zero and QD_OK when off).
 * qd_paircorrect_read: waits for the context's work, writes n_values = 10 values (QD_ERR_INVALID on another size, QD_ERR_STATE when
 * off).
 * qd_paircorrect_add: another context's table joins this one's, as qd_trim_add does.  qd_reset_counts zeroes the table. */
#define QD_PAIRCORRECT_VALUES 10
typedef struct qd_paircorrect_params {
    int32_t good_quality;
    int32_t bad_quality;
} qd_paircorrect_params;
int qd_paircorrect_set(qd_ctx* ctx, const qd_paircorrect_params* params);
int qd_paircorrect_get(const qd_ctx* ctx, qd_paircorrect_params* out);
int qd_paircorrect_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_paircorrect_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- post-trimming of the insert reads: trailing N, a poly-X tail and a crop to max_length (opt-in; no reference counterpart:
 * Quade 0.3.2 writes the insert reads as they came) -----------------------------------------------------------------------------
 * One stage behind the clip, 3' trimming and overlap trimming stages above and in front of the read filter below, where fastp runs
 * trim_poly_x and max_len1 / max_len2 and cutadapt --trim-n: a poly-A tail sits between the insert and the adapter and shows only
 * once the adapter is gone.  For an insert read r (0 = R1, 1 = R2), take the record the stage receives, that is, what clip, trim and
 * pairtrim left: sequence bytes s, length L; u(b) = b & 0xDF; P = poly_x_min_length; M_r = max_length[r].  Each of steps 1 to 3 is
 * skipped when not configured; its output length is then its input length.
 *   1 trailing N (tail_n = 1): Ln = L - k, where k is the number of consecutive bytes at the 3' end with u(b) == 'N'
 *   2 poly-X (P > 0; 6..100): for each X in A, C, G, T, Lx(X) is the clip stage's step 3 exactly as stated above for poly-G, with
 *     X in place of 'G', over s[0 .. Ln).  Lp = min over X of Lx(X).  The read's tail base is the X with Lx(X) < Ln; at most one
 *     such X exists (a walk alive at t = P has at most P / 8 mismatches among the last P bytes, and every byte mismatches all bases
 *     but one).  N and every other byte count as a mismatch.  One pass only: a T run behind an A run loses the T run
 *   3 crop (M_r > 0): Lm = min(Lp, M_r)
 *   4 floor: Lout = max(Lm, min(min_length, L)), min_length being the 3' trimming's
 * and the read's record becomes seq_len = Lout; its other fields stay.  The stage never moves seq or qual and never drops a pair;
 * index reads, names and the :IDX[:MOL] tag never change.  Only the sequence line is read.  With the stage on, qd_pipe_run runs it
 * over every pair it routes (one launch per batch on its compute stream, no host sync) directly behind the overlap trimming, so that
 * the read filter, the quality and cycle counters, the duplication tally and the output stages all see the post-trimmed reads, and
 * adds to a device table uint64[2][16] (R1, R2), whatever the write flags say:
 *   0 reads   1 bases_in (sum of L)   2 bases_out (sum of Lout)   3 n_tail_reads (Ln < L)   4 n_tail_bases (sum of L - Ln)
 *   5 polya_reads (tail base A)   6 polya_bases (sum of Ln - Lp for tail base A)   7 polyc_reads   8 polyc_bases   9 polyg_reads
 *   10 polyg_bases   11 polyt_reads   12 polyt_bases   13 cropped_reads (Lm < Lp)   14 cropped_bases (sum of Lp - Lm)
 *   15 floored_reads (Lout > Lm)
 * Off, nothing is allocated or launched.
 *
 * qd_posttrim_set: NULL, or every rule off (tail_n 0, poly_x_min_length 0, both max_length 0), turns the stage off and frees the
 * table; otherwise the values are checked (tail_n 0 or 1, poly_x_min_length 0 = off or 6..100, max_length 0 = off or 1..65535,
 * min_length 0..65535: QD_ERR_INVALID, the state as before) and a zeroed table allocated.  Waits for the context's outstanding
 * work.  Independent of plan, barcodes and the other stages' setters.
 * qd_posttrim_get: the parameters in force (all zero and QD_OK when off).
 * qd_posttrim_read: waits for the context's work, writes n_values = 32 values (QD_ERR_INVALID on another size, QD_ERR_STATE when
 * off).
 * qd_posttrim_add: another context's table (qd_posttrim_read's layout) joins this one's, as qd_clip_add does.  qd_reset_counts
 * zeroes the table. */
#define QD_POSTTRIM_VALUES 32
typedef struct qd_posttrim_params {
    int32_t tail_n;            /* 1 = cut trailing N */
    int32_t poly_x_min_length; /* 0 = off */
    int32_t max_length[2];     /* R1, R2; 0 = off */
    int32_t min_length;
} qd_posttrim_params;
int qd_posttrim_set(qd_ctx* ctx, const qd_posttrim_params* params);
int qd_posttrim_get(const qd_ctx* ctx, qd_posttrim_params* out);
int qd_posttrim_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_posttrim_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- read filtering of the insert reads: length, N, quality, complexity (opt-in; no reference counterpart: Quade 0.3.2 writes
 * every pair it assigns) ----------------------------------------------------------------------------------------------------
 * The step cutadapt and fastp run directly behind trimming: discard the pairs that are not worth keeping, pair-aware, and say
 * how many went and why.  The stage sees the two insert reads as the trimming stages above left them (as scanned when those are
 * off).  For a read of length L with sequence bytes s and quality bytes q (unsigned):
 *   n_count = the number of bytes 'N' or 'n'
 *   unq     = the number of q[i] < 33 + qualified_quality
 *   qsum    = the sum of max(0, q[i] - 33) (QD_QS_QUAL_SUM's definition)
 *   diff    = the number of i in [0, L - 1) with (s[i] & 0xDF) != (s[i + 1] & 0xDF)
 * A pair is dropped for the first of these rules that either of its reads fails; a rule whose parameter is -1 is off and
 * skipped; all comparisons are in 64-bit integers:
 *   1 too_short         L < min_length                                   (fastp -l, cutadapt -m)
 *   2 too_many_n        n_count > max_n                                  (fastp -n)
 *   3 low_quality       unq * 100 > max_unqualified_pct * L              (fastp -u with -q)
 *   4 low_mean_quality  qsum < min_mean_quality * L                      (fastp -e)
 *   5 low_complexity    diff * 100 < min_complexity_pct * max(L - 1, 0)  (fastp -y with -Y)
 * An empty read fails rule 1 only.  The filter applies to every pair, Undetermined included.  A dropped pair appears in no output
 * file, neither its R1 nor its R2 record, and the quality counters (qd_qstats_enable) do not count it: they count the pairs that
 * are written.  The pair counters (qd_get_counts), the unknown-barcode tally and the two trimming tables are as without the
 * stage: they count what their stages saw.  A destination that loses all its pairs is treated exactly as a destination that
 * received none: the pipeline hands the sink no text for it, and since the sink creates a destination's two files when the first
 * text for it arrives, it has no files.
 * With the stage on, qd_pipe_run runs it over every pair it routes (one launch per batch on its compute stream, no host sync)
 * behind the trimming stages and in front of the quality counters, and adds to a device table uint64[2 * S + 1][8],
 * destination-major as qd_qstats_read's (destination = routing code, Undetermined last), whatever the write flags say:
 *   0 pairs   1 .. 5 the pairs dropped by rule 1 .. 5   6 bases_in (L of both reads, every pair)   7 bases_dropped (... of the
 *   dropped pairs)
 * Off, nothing is allocated or launched and no path changes.
 *
 * qd_filter_set: NULL, or every rule -1, turns the stage off and frees the table; otherwise the values are checked (min_length 1
 * .. 100000, max_n 0 .. 100000, max_unqualified_pct 0 .. 100, qualified_quality 1 .. 93 with -1 = 15, min_mean_quality 1 .. 93,
 * min_complexity_pct 1 .. 100: QD_ERR_INVALID, the state as before) and a zeroed table allocated, which needs the plan and the
 * barcodes (QD_ERR_STATE); a new plan or new barcodes turn the stage off, as they do the quality counters.  Waits for the
 * context's outstanding work.
 * qd_filter_get: the parameters in force (every rule -1, qualified_quality 15 and QD_OK when off).
 * qd_filter_read: waits for the context's work, writes n_values = (2 * S + 1) * 8 values (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).  qd_filter_add: another context's table joins this one's.  qd_reset_counts zeroes the table.
 * qd_filter_kind: which accumulation the kernel takes for this context's S: 1 = 32-bit partials in LDS (2 * S + 1 <= 2048),
 * 2 = 64-bit atomics on the table. */
#define QD_FILTER_VALUES 8
typedef struct qd_filter_params {
    int32_t min_length;
    int32_t max_n;
    int32_t max_unqualified_pct;
    int32_t qualified_quality;
    int32_t min_mean_quality;
    int32_t min_complexity_pct;
} qd_filter_params;
int qd_filter_set(qd_ctx* ctx, const qd_filter_params* params);
int qd_filter_get(const qd_ctx* ctx, qd_filter_params* out);
int qd_filter_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_filter_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);
int qd_filter_kind(const qd_ctx* ctx);

/* ---- k-mer screen of the insert reads against a reference: PhiX, a spike-in, a vector, a contaminant (opt-in;
 * no reference counterpart: Quade 0.3.2 knows no reference sequence) --------------------------------------------------------------
 * What bbduk does with ref=phix.fa k=31 in a pass of its own over every output file, done while the device pipeline holds the
 * reads' text.  The definition:
 *   u(b) = b & 0xDF.  A base is valid when u(b) is one of A, C, G, T.  Its code is c(b) = (u(b) >> 1) & 3, which gives A 0, C 1,
 *   T 2, G 3 (the duplication key's code); the complement is c ^ 2.  k = kmer, 15 to 32.
 *   The k-mer at position p of a sequence s exists when s[p .. p + k) are all valid.  Its forward word is
 *   w = sum c(s[p + i]) << 2 (k - 1 - i), its reverse-complement word rc = sum (c(s[p + k - 1 - i]) ^ 2) << 2 (k - 1 - i), its
 *   canonical word min(w, rc).
 *   The reference set R holds the distinct canonical words of every k-mer of every record of the reference FASTA.  Records are
 *   linear; a line starting with '>' separates records, so k-mers never span two records; lower case counts; any other letter
 *   breaks k-mers.
 *   hits(read) is the number of positions p in [0, L - k] whose k-mer exists and whose canonical word is in R.  A read shorter
 *   than k has 0 hits and 0 k-mers.  A pair is matched when hits(R1) + hits(R2) >= min_hits (1 to 65535).
 * The stage sees the pairs the output stages see: behind clip, trim, pairtrim, posttrim and the read filter, only pairs the filter
 * kept, the reads as those stages left them (seq, seq_len of the last table), every destination whatever its write flag.  With
 * action QD_SCREEN_REPORT nothing else changes.  With QD_SCREEN_DROP a matched pair leaves the run the way a filtered pair does:
 * output lengths 0, in no file, counted neither by the quality and cycle counters nor by the duplication tally; qd_get_counts
 * and the filter's table are exactly as without the stage.  With the stage on, qd_pipe_run runs it over every batch (one launch
 * on its compute stream, no host sync) between the read filter and the quality counters and adds to a device table
 * uint64[2 * S + 1][8], destination-major in routing code order as qd_qstats_read's:
 *   0 pairs   1 matched_pairs   2 r1_hit_reads (pairs whose R1 has at least one hit)   3 r2_hit_reads   4 kmers (k-mers that exist,
 *   over both reads)   5 hit_kmers   6 bases_in (sum of L over both reads)   7 bases_matched (... of the matched pairs)
 * Off, nothing is allocated or launched.
 *
 * qd_screen_set: params NULL or n_kmers 0 turns the stage off and frees everything.  Otherwise kmer (15 .. 32), min_hits
 * (1 .. 65535) and action (0, 1) are checked, and the list of R's words: strictly ascending, every word below 4^kmer, every word
 * canonical, n_kmers <= QD_SCREEN_MAX_KMERS; a bad value is QD_ERR_INVALID and leaves the state as before.  The library builds an
 * open-addressing table of 64-bit words on the host (linear probing, at most half full, the empty slot all ones, which no
 * canonical word equals) and uploads it: up to QD_SCREEN_LDS_MAX_KMERS words the kernel keeps the table in the workgroup's LDS
 * (16384 slots, 128 KiB, at most three eighths full), beyond that it probes it in global memory.  Compares are exact, so no result depends on the hash
 * function.  Needs qd_set_plan and qd_set_barcodes (QD_ERR_STATE), which turn the stage off, as they do the read filter.  Waits
 * for the context's outstanding work.
 * qd_screen_get: the parameters in force (all zero, *n_kmers 0 and QD_OK when off); n_kmers may be NULL.
 * qd_screen_kind: 1 = the table in LDS, 2 = in global memory; QD_ERR_STATE when off.
 * qd_screen_first_slot: the slot at which the probe for `word` starts in the table built for n_kmers words (for tests that build
 * long probe chains); QD_ERR_INVALID for an n_kmers outside 1 .. QD_SCREEN_MAX_KMERS.
 * qd_screen_read: waits for the context's work, writes n_values = (2 * S + 1) * 8 values (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).  qd_screen_add: another context's table joins this one's.  qd_reset_counts zeroes the table. */
#define QD_SCREEN_VALUES 8
#define QD_SCREEN_MAX_KMERS (1u << 22)
#define QD_SCREEN_LDS_MAX_KMERS 6144u
#define QD_SCREEN_REPORT 0
#define QD_SCREEN_DROP 1
#define QD_SCREEN_DROPPED 0x80u /* the flag byte of a pair the screen drops */
typedef struct qd_screen_params {
    int32_t kmer;
    int32_t min_hits;
    int32_t action; /* QD_SCREEN_REPORT | QD_SCREEN_DROP */
} qd_screen_params;
int qd_screen_set(qd_ctx* ctx, const qd_screen_params* params, const uint64_t* kmers, int64_t n_kmers);
int qd_screen_get(const qd_ctx* ctx, qd_screen_params* out, int64_t* n_kmers);
int qd_screen_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_screen_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);
int qd_screen_kind(const qd_ctx* ctx);
int64_t qd_screen_first_slot(uint64_t word, int64_t n_kmers);

/* ---- per-cycle quality and base content, per-read distributions (opt-in; no reference counterpart) -----------------------------
 * What the first plots of a read QC tool show: quality and base composition by cycle, and the distributions of read length,
 * per-read mean quality and GC content.  A device-resident table of exact uint64 counters over the insert reads as the output
 * stages see them -- behind the trimming stages, without the pairs the read filter dropped, whatever the write flags say: exactly
 * the reads the quality counters (qd_qstats_enable) count.
 *
 * Groups.  g comes from the routing code: an even code is pass (0), an odd code is fail (1), and 0xFFFF is Undetermined (2).
 * Reads.  r = 0 / 1 for R1 / R2.
 * Bytes.  Sequence bytes are s.  Quality bytes q are unsigned, with ph = max(0, q - 33), as in qd_qstats.
 * Per cycle, for c < QD_CS_CYCLES = 1024, every read with L > c adds to cycle[g][r][c][8]:
 *   0 A  1 C  2 G  3 T  4 N    (s[c] & 0xDF) == the letter
 *   5 qual_sum  += ph[c]       6 q20  ph[c] >= 20       7 q30  ph[c] >= 30
 * Cycles from 1024 on are not counted per cycle.
 * Per read:
 *   len[g][r][1025]    bin min(L, 1024)
 *   meanq[g][r][94]    for L > 0: bin min(93, sum(ph) / L), integer division over the whole read
 *   gc[g][r][101]      for L > 0: bin 100 * (G and C count, either case) / L, over the whole read
 * Derived values.  reads(c) is not stored: it is the sum of len minus the sum of len[0..c].  other(c) = reads(c) - A - C - G - T - N.
 * Table.  uint64, group-major, then read.  For each (g, r) the order is cycle, len, meanq, gc, which is 1024*8 + 1025 + 94 + 101
 * = QD_CS_GR_VALUES = 9412 values.  The whole table is QD_CS_VALUES = 56 472 values, independent of S.
 * Cross-checks.  For reads of at most 1024 bases, summed over cycles and groups, N, qual_sum, q20 and q30 equal the qd_qstats
 * table's columns, and the sum of L * len[L] equals its bases.
 *
 * With the table on, qd_pipe_run adds every pair it routes (one launch per batch on its compute stream, no host sync), directly
 * behind the quality counters; a chunk part (skip_kept, max_pairs) counts exactly its pairs.  Off, nothing is allocated or
 * launched.
 * qd_cstats_enable: on != 0 allocates and zeroes the table, 0 frees it.  Waits for the context's outstanding work.  Independent of
 * plan and barcodes (the table does not depend on S): neither turns it off.  qd_reset_counts zeroes the table.
 * qd_cstats_read: waits for the context's work, writes n_values = QD_CS_VALUES values (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).  qd_cstats_add: another context's table joins this one's (the same errors).
 * qd_cstats_lds_cycles: the cycles below which a workgroup of the kernel counts in LDS partials; later cycles go to the 64-bit
 * table directly (a constant of the build: tests straddle it). */
enum {
    QD_CS_A = 0,
    QD_CS_C = 1,
    QD_CS_G = 2,
    QD_CS_T = 3,
    QD_CS_N = 4,
    QD_CS_QUAL_SUM = 5,
    QD_CS_Q20 = 6,
    QD_CS_Q30 = 7,
    QD_CS_COUNTERS = 8,
    QD_CS_GROUPS = 3,
    QD_CS_CYCLES = 1024,
    QD_CS_LEN_BINS = 1025,
    QD_CS_MEANQ_BINS = 94,
    QD_CS_GC_BINS = 101,
    QD_CS_GR_VALUES = 9412,
    QD_CS_VALUES = 56472
};
int qd_cstats_enable(qd_ctx* ctx, int32_t on);
int qd_cstats_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_cstats_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);
int qd_cstats_lds_cycles(void);

/* ---- adapter content of the raw insert reads (opt-in; no reference counterpart) ------------------------------------------------
 * Which known adapter is in the library, in what share of the reads, from which cycle on and in which samples: what a user needs
 * before choosing adapter_R1 / adapter_R2 for the trimming stage.  A device-resident table of exact uint64 counters.
 *
 * Probes.  A probe is QD_ADAPTERS_K = 12 bytes, each one of A, C, G, T (upper case).  Up to QD_ADAPTERS_PROBES = 16 are in force;
 *   slot a is the a-th probe given to qd_adapters_set.  No two are equal.
 * Reads.  The insert reads AS THE SCAN LEFT THEM, R1 and R2 (r = 0 / 1): in front of clipping, trimming, overlap trimming,
 *   post-trimming, the read filter and the screen.  It is the only stage that counts raw reads: the table describes the library, not
 *   what the trimmers left.  Every pair the pipeline routes is counted, whatever the write flags say and whatever the filter or
 *   the screen do to it later.
 * Per read.  With u[i] = s[i] & 0xDF and L the sequence length, first(a) is the smallest p in [0, L - 12] with u[p .. p + 12)
 *   equal to probe a; otherwise it is none.  A byte that is not A, C, G or T after folding never matches, so an N inside the 12
 *   bases means no match at that p.  first(any) is the minimum over the probes in force.
 * Table.  uint64, two parts, QD_ADAPTERS_HIST_VALUES + (2 * S + 1) * QD_ADAPTERS_DEST_VALUES values:
 *   hist[r][a][bin]   a is one of 17 columns, the 16 slots then any; a read with first(a) adds one to bin = min(first(a), 1024);
 *                     2 x 17 x 1025 = 34 850 values; unused slots stay 0
 *   dest[d][r][c]     d the destination in routing code order, 0xFFFF -> 2 * S, as qd_qstats_read's; c = 0 the reads, c = 1 + a
 *                     the reads with first(a) not none: 18 columns, 36 values per destination
 * Cross-checks.  The sum over bins of hist[r][a] equals the sum over d of dest[d][r][1 + a]; the sum of dest[d][r][0] equals the
 *   pairs routed.
 *
 * With the stage on, qd_pipe_run adds every pair it routes: one launch per batch on its compute stream, no host sync, on the
 * scan's record tables and the final routing codes, in front of the stages that rewrite the tables; a chunk part (skip_kept,
 * max_pairs) counts exactly its pairs.  Off, nothing is allocated or launched.
 * qd_adapters_set: probes = n_probes x 12 bytes; NULL or n_probes 0 turns the stage off and frees the table.  A byte outside ACGT,
 *   two equal probes or n_probes outside 0 .. 16 is QD_ERR_INVALID and leaves the state as before.  Needs qd_set_plan and
 *   qd_set_barcodes (QD_ERR_STATE), which turn the stage off as they do the quality counters: the table has a row per destination.
 *   Waits for the context's outstanding work.
 * qd_adapters_get: the probes in force (*n_probes 0 and QD_OK when off); probes (room for 16 x 12 bytes) may be NULL.
 * qd_adapters_read: waits for the context's work, writes n_values = 34850 + (2 * S + 1) * 36 values (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).  qd_adapters_add: another context's table joins this one's.  qd_reset_counts zeroes the table. */
#define QD_ADAPTERS_K 12
#define QD_ADAPTERS_PROBES 16
#define QD_ADAPTERS_BINS 1025
#define QD_ADAPTERS_HIST_VALUES 34850
#define QD_ADAPTERS_DEST_VALUES 36
int qd_adapters_set(qd_ctx* ctx, const uint8_t* probes, int32_t n_probes);
int qd_adapters_get(const qd_ctx* ctx, uint8_t* probes, int32_t* n_probes);
int qd_adapters_read(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int qd_adapters_add(qd_ctx* ctx, const uint64_t* values, int64_t n_values);

/* ---- duplication report: read-pair keys tallied on the device (opt-in; no reference counterpart) -------------------------------
 * The library duplication rate: how many of a destination's pairs repeat an earlier pair's first bases.  It is no sum of per-read
 * counters: a device-resident hash table, fed by every batch, counts the pairs per key.  The pairs are those the output stages
 * see -- behind the trimming stages, without the pairs the read filter dropped, every destination whatever its write flag:
 * exactly the pairs the quality counters (qd_qstats_enable) count.
 *
 * Definition (quade_amd/csrc/quade_dup.h and tests/dup_model.py state the same; the kernels implement exactly this).
 * Parameters: B = bases (8 .. 32), sample (a power of two, 1 .. 1024), slots (a power of two, 2^10 .. 2^28).  Per pair that
 * carries no filter reason, with reads s1, s2 of current lengths L1, L2 and starts as the record tables in force give them (a
 * front clip moves the start):
 *   fold     u(b) = b & 0xDF; a base is valid when u(b) is one of A, C, G, T
 *   code     c(b) = (u(b) >> 1) & 3, which gives A 0, C 1, T 2, G 3
 *   class    the first that applies: short (L1 < B or L2 < B); with_n (an invalid base among the first B of either read); keyed
 *   key      three 64-bit words (w1, w2, d): w_r = sum over i < B of c(s_r[i]) << (2 i) (there is no shift by 64 at B = 32);
 *            d = the destination as qd_qstats numbers it (the routing code, 0xFFFF -> 2 * S).  Equal sequences in two
 *            destinations are two keys: duplicates are a per-library matter
 *   hash     h = the unknown tally's 64-bit tag function over the four words {w1, w2, d, 0}: h0 = 0x9E3779B97F4A7C15; per word
 *            h = (h ^ w) * 0xFF51AFD7ED558CCD, h ^= h >> 32; then h *= 0xC4CEB9FE1A85EC53, h ^= h >> 29 (mod 2^64)
 *   sampled  sample == 1, or h >> (64 - log2 sample) == 0.  This is key-space sampling: a sampled key keeps its exact
 *            multiplicity, and every context and rank samples the same keys because the test is a pure function of the key.
 *            Table and merge traffic fall by the factor `sample`; rates over the sample are unbiased estimates of the library's
 *   tally    sampled pairs are counted per key in a table of `slots` entries per context.  The slot tag is h (0 replaced by 1;
 *            the low dup_tag_bits of it under the test knob), the home slot and the probe limit min(slots, 1024) are the unknown
 *            tally's.  A pair that finds no entry within the probe limit, or whose tag belongs to another key, is not_tallied
 * Counters: uint64[2 * S + 1][QD_DUP_VALUES], destination-major as qd_qstats_read's:
 *   0 pairs   1 short   2 with_n   3 sampled   4 not_tallied      (keyed = pairs - short - with_n)
 * Per destination sampled == not_tallied + the sum of the counts of the table's entries with that d; every entry's count is exact.
 *
 * With the stage on, qd_pipe_run runs it over every pair it routes beside the quality counters (three launches per batch on its
 * compute stream, no host sync; launches of one context on different streams are ordered among themselves as the unknown tally's
 * are).  Off, nothing is allocated or launched.
 *
 * qd_dup_set: NULL turns the stage off and frees both tables; otherwise the values are checked (QD_ERR_INVALID, the state as
 * before) and zeroed tables allocated (20 bytes per destination and 48 bytes per slot), which needs the plan and the barcodes
 * (QD_ERR_STATE); a new plan or new barcodes turn the stage off, as they do the read filter.  Waits for the context's work.
 * qd_dup_get: the parameters in force (all 0 and QD_OK when off).
 * qd_dup_stats: waits for the context's work, writes n_values = (2 * S + 1) * 5 counters (QD_ERR_INVALID on another size,
 * QD_ERR_STATE when off).
 * qd_dup_read: the occupied entries are packed on the device and only they are downloaded; entry i is keys[3 i .. 3 i + 2] =
 * (w1, w2, d) with counts[i], in no particular order.  Returns the number of entries, or -(entries needed) when cap is too small
 * (cap 0 with NULL arrays asks for the size), or a value <= QD_DUP_READ_ERROR on failure: QD_DUP_READ_ERROR + QD_ERR_*.
 * qd_reset_counts empties both tables.  Tables of several contexts or ranks are merged on the host: equal keys summed. */
#define QD_DUP_VALUES 5
#define QD_DUP_READ_ERROR (-((int64_t)1 << 40))
typedef struct qd_dup_params {
    int32_t bases;  /* 8 .. 32 */
    int32_t sample; /* a power of two, 1 .. 1024 */
    int64_t slots;  /* a power of two, 2^10 .. 2^28 */
} qd_dup_params;
int qd_dup_set(qd_ctx* ctx, const qd_dup_params* params);
int qd_dup_get(const qd_ctx* ctx, qd_dup_params* out);
int qd_dup_stats(qd_ctx* ctx, uint64_t* out, int64_t n_values);
int64_t qd_dup_read(qd_ctx* ctx, uint64_t* keys, uint64_t* counts, int64_t cap);

/* ---- counters: replace the class counters of src/Sample.py:32,144 and feed Sample.REPORT ---------
 * qd_get_counts waits for outstanding work of this context (only), then writes 2*S+4 values. */
int qd_get_counts(qd_ctx* ctx, uint64_t* out, int32_t n_values);
int qd_reset_counts(qd_ctx* ctx);
/* Adds a counter vector (layout of qd_get_counts, e.g. another context's) to this context's totals.  The reference
 * keeps ONE set of class counters per run (src/Sample.py:32,144); a process that drives several contexts on one
 * device (chunk workers) folds the others into the context that is the member of its communicator before
 * qd_reduce_counts, or into any one of them before the report.  Waits for this context's outstanding work.
 * QD_ERR_INVALID when the vector's aggregates do not add up (TOTAL = PASS + FAIL + UNDETERMINED over the samples). */
int qd_add_counts(qd_ctx* ctx, const uint64_t* counts, int32_t n_values);
/* Waits for every outstanding launch / copy this context issued (on its own stream, its slots'
 * streams and the caller's streams it was handed) -- not for other contexts' work on the device. */
int qd_synchronize(qd_ctx* ctx);

/* ---- host-staged streaming: pinned slots, H2D || kernel || D2H -------------------------------------
 * Replaces the per-read loop body of Quade.double_index_parser / simple_index_parser
 * (src/Quade.py:210-221, 240-250) for host-resident rows.  The library owns pinned host and device
 * buffers of n_slots slots x max_pairs.  A slot's host buffers are caller-writable from qd_wait()
 * (or creation) until the next qd_submit() of that slot. */
typedef struct qd_slot_buffers {
    uint8_t* seq[2];
    uint8_t* qual[2];
    uint8_t* len[2];
    uint16_t* codes; /* valid after qd_wait */
    uint8_t* mol;    /* valid after qd_wait; NULL when mol_width == 0 */
    int64_t max_pairs;
    uint32_t* short_idx[2]; /* per stream: indices of the reads shorter than their window (qd_submit_ragged) */
    int64_t short_cap;      /* entries each short_idx array holds */
} qd_slot_buffers;
int qd_slots_create(qd_ctx* ctx, int32_t n_slots, int64_t max_pairs);
int qd_slots_destroy(qd_ctx* ctx);
int qd_slot_get(qd_ctx* ctx, int32_t slot, qd_slot_buffers* out);
/* has_len != 0: the len rows were filled and the generic kernel runs. Non-blocking. */
int qd_submit(qd_ctx* ctx, int32_t slot, int64_t n_pairs, int32_t has_len);
/* The len rows were filled and stream k's short reads are listed (ascending) in the slot's
 * short_idx[k][0..n_short[k]) -- what qd_pack_index_fastq writes.  Indices >= n_pairs are ignored.
 * Runs like qd_demux_device_ragged; a count above short_cap means "too many to list": the generic
 * kernel takes the batch.  Non-blocking. */
int qd_submit_ragged(qd_ctx* ctx, int32_t slot, int64_t n_pairs, const int64_t n_short[2]);
int qd_wait(qd_ctx* ctx, int32_t slot);

/* ---- host helpers: fastq text -> rows (replace what the path consumed from pyFastq, a9) -----------
 * Scans decompressed fastq text (4-line records).  A record whose sequence and quality lengths
 * differ is skipped inside its own stream (pinned by the reference's golden run);
 * a trailing partial record ends the scan.  For every kept record r (r < max_records):
 *   rec_off[r]  = byte offset of its '@' line,   rec_off[n] = offset one past the last kept record
 * Returns the number of kept records (>= 0) or a negative error code.  *consumed = bytes scanned
 * (start of the first record NOT consumed) so a caller can stream a file in pieces. */
int64_t qd_fastq_index(const uint8_t* text, int64_t text_len, int64_t max_records, int64_t* rec_off,
                       int64_t* consumed);

/* Packs stream `k` (0/1) of `layout` from fastq text: for kept record r writes seq row r, qual row
 * r and len row r (len_rows may be NULL).  *all_full is set to 0 when any read is shorter than its
 * window (then the caller must pass len rows to the device).  short_idx (may be NULL): the indices
 * r of those short reads, ascending, at most short_cap of them stored; *n_short = how many there
 * were (may exceed short_cap).  Same skipping rule and return value as qd_fastq_index. */
int64_t qd_pack_index_fastq(const qd_layout* layout, int32_t k, const uint8_t* text, int64_t text_len,
                            int64_t max_records, uint8_t* seq_rows, uint8_t* qual_rows,
                            uint8_t* len_rows, int32_t* all_full, int64_t* consumed,
                            uint32_t* short_idx, int64_t short_cap, int64_t* n_short);

/* Packs rows from already separated reads (concatenated sequence and quality bytes + offsets):
 * used by tests and by callers that hold records rather than text. */
int qd_pack_index_reads(const qd_layout* layout, int32_t k, int64_t n, const uint8_t* seq,
                        const uint8_t* qual, const int64_t* offsets, uint8_t* seq_rows,
                        uint8_t* qual_rows, uint8_t* len_rows, int32_t* all_full);

/* ---- host helpers: routed records -> output text (replace FastqWriter.__call__'s formatting) --------
 * qd_build_tags: the name suffix of every pair, ":IDX" or ":IDX:MOL" (src/FastqWriter.py:61-66):
 * IDX = fused barcode slice as read (NOT case folded), MOL = fused molecular slice; ":MOL" is
 * omitted when the molecular slice is empty (empty molecular index is falsy).  Slices
 * are clamped to the read length when len rows are given.  mol_rows (optional): the molecular
 * bytes written by the device (n x mol_width); when NULL they are sliced from seq_rows on the
 * host -- both give the same bytes.  tag row r = tag_rows + r*tag_stride,
 * tag_stride >= 2 + key_width + mol_width; tag_len[r] = bytes used. */
int qd_build_tags(const qd_layout* layout, const qd_plan* plan, int64_t n, const uint8_t* const seq_rows[2],
                  const uint8_t* const len_rows[2], const uint8_t* mol_rows, uint8_t* tag_rows,
                  int32_t tag_stride, uint8_t* tag_len);

/* qd_format_records: for the n_sel records sel[0..n_sel) (indices into rec_off, input order) of
 * fastq `text`, writes "@" + name + tag + "\n" + seq + "\n+\n" + qual + "\n" -- the record format
 * of the reference's output (src/FastqWriter.py:68-69 via FastqSeq.fastqstr; pinned by the bundled
 * goldens): name = header line without its first byte, cut at the first ASCII whitespace.
 * Returns bytes written, or -(bytes needed) when out_cap is too small. */
int64_t qd_format_records(const uint8_t* text, const int64_t* rec_off, const int64_t* sel, int64_t n_sel,
                          const uint8_t* tag_rows, int32_t tag_stride, const uint8_t* tag_len, uint8_t* out,
                          int64_t out_cap);

/* ---- multi-GPU: the one exchange of the path ------------------------------------------------------------
 * Read pairs are independent (src/Sample.py:56-91 touches nothing but counters) and chunks are
 * independent files (src/Quade.py:198,229), so work shards across GPUs with no data-path collective.
 * What is exchanged is what the reference keeps in class-level counters (src/Sample.py:32,144): one
 * sum of the uint64[2S+1] counters + TOTAL over all member contexts, an RCCL all-reduce over xGMI
 * (librccl.so.1 is loaded on first use; single-GPU users never load it).
 *   one process, several devices : qd_comm_create_local(contexts, n)            (ncclCommInitAll)
 *   one process per device       : rank 0 calls qd_comm_unique_id and hands the 128 bytes to the other
 *                                  ranks by any means; every rank calls qd_comm_create_rank (ncclCommInitRank)
 * qd_reduce_counts waits for the member contexts' outstanding work, sums, and gives every caller the
 * total in the layout of qd_get_counts.  Member contexts must hold the same sample table. */
typedef struct qd_comm qd_comm;
#define QD_UNIQUE_ID_BYTES 128
int qd_comm_unique_id(uint8_t id[QD_UNIQUE_ID_BYTES]);
int qd_comm_create_local(qd_ctx* const* contexts, int32_t n_contexts, qd_comm** out);
int qd_comm_create_rank(qd_ctx* ctx, int32_t world_size, int32_t rank, const uint8_t id[QD_UNIQUE_ID_BYTES],
                        qd_comm** out);
int qd_comm_world(const qd_comm* comm);
int qd_reduce_counts(qd_comm* comm, uint64_t* out, int32_t n_values);
int qd_comm_destroy(qd_comm* comm);
const char* qd_comm_last_error(void); /* text of the last qd_comm_* / qd_reduce_counts error on this thread */

/* ---- host I/O: routed records -> per-destination fastq.gz files ---------------------------------------
 * A sink is one output directory's set of destinations: "<name>_pass", "<name>_fail" per sample and
 * "Undetermined", each a pair of files <dest>_R1.fastq.gz / <dest>_R2.fastq.gz (src/FastqWriter.py:29-31,
 * src/Sample.py:44,147-148).  qd_sink_route replaces, for a whole batch, the routing tail of
 * Sample.FINDER (src/Sample.py:74-75,82-83,90-91: writer called when the write_* flag of the pair's
 * category is set) and FastqWriter.__call__/flush_buffers (src/FastqWriter.py:48-90): name tag,
 * record format (as qd_format_records), lazy creation of a destination's two files at its first
 * routed pair (truncating), gzip members appended in input order.  Compression runs on a thread pool
 * owned by the library (libdeflate when libdeflate.so.0 loads, zlib otherwise); no file descriptor
 * is held between members.  qd_sink_route returns once the batch's text has been consumed (the
 * caller's buffers are free again); compression and the appends continue behind it.  A sink is driven
 * by one thread at a time; different sinks may be driven concurrently. */
typedef struct qd_sink qd_sink;
typedef struct qd_text_batch qd_text_batch; /* a batch of the native reader, below */
/* Threads of the I/O pool: n_threads > 0 sets it (before the pool's first use), 0 = one per hardware
 * core this process may use (qd_host_cores), < 0 = query only.  Returns the size in effect. */
int qd_io_threads(int32_t n_threads);
int qd_io_backend(void); /* 1 = libdeflate, 0 = zlib */
int qd_host_cores(void); /* cores this process may use: affinity mask capped by the cgroup CPU quota */
/* names: n_samples sample names in ordinal order (SAMPLE_LIST order, src/Sample.py:153); gzip_level -1..9 (-1 = Huffman coding only, no string matching: ~3x the speed of level 1, larger files);
 * write_*: the [output] flags (src/Quade.py:125-129 -> Sample.CLASS_INIT). */
int qd_sink_create(const char* outdir, int32_t n_samples, const char* const* names, int32_t gzip_level,
                   int32_t write_pass, int32_t write_fail, int32_t write_undetermined, qd_sink** out);
int qd_sink_set_quiet(qd_sink* sink, int32_t quiet); /* 1: no "Create ... file" lines on stdout */
/* codes: the device's routing codes of the batch's n pairs; r1/r2 text + rec_off: the insert reads
 * as qd_fastq_index gives them (record i of both = pair i); tags as qd_build_tags gives them. */
int qd_sink_route(qd_sink* sink, int64_t n_pairs, const uint16_t* codes, const uint8_t* r1_text,
                  const int64_t* r1_rec_off, const uint8_t* r2_text, const int64_t* r2_rec_off,
                  const uint8_t* tag_rows, int32_t tag_stride, const uint8_t* tag_len);
/* Same, for insert reads that came from the native reader (qd_reader_next): the sink takes the two text
 * batches over (the caller must NOT free their handles afterwards, whatever the return code) and copies the
 * tags, so the call returns right after the scatter; formatting and compression run behind it. */
int qd_sink_route_batches(qd_sink* sink, int64_t n_pairs, const uint16_t* codes, const qd_text_batch* r1,
                          const qd_text_batch* r2, const uint8_t* tag_rows, int32_t tag_stride,
                          const uint8_t* tag_len);
int qd_sink_flush(qd_sink* sink); /* waits until every member is in its file (src/Sample.py:93-102 FLUSH_ALL) */
int qd_sink_stats(qd_sink* sink, int64_t* members, int64_t* text_bytes, int64_t* gzip_bytes, int64_t* files);
const char* qd_sink_last_error(const qd_sink* sink);
int qd_sink_close(qd_sink* sink); /* flush + destroy */

/* Writes n bytes as a gzip file, compressed on the library's pool: member_bytes > 0 = members of that much
 * text, 0 = one member, -1 = BGZF blocks (bgzip / htslib layout: 64 KiB members that carry their size in a
 * 'BC' extra subfield, closed by the empty end-of-file block).  Tooling (synthetic inputs); no reference
 * counterpart. */
/* Where the host's CPU time goes (measurement): thread-CPU seconds per stage of the reader, the sink and the pool since the
 * process started or since the last call with reset != 0, summed over all threads of the library.  names[i] (static strings)
 * and seconds[i] for i < the return value (<= cap); either array may be NULL. */
int qd_io_stage_seconds(const char** names, double* seconds, int32_t cap, int32_t reset);
int qd_write_gzip_file(const char* path, const uint8_t* data, int64_t n_bytes, int32_t level, int64_t member_bytes);

/* ---- host I/O: fastq(.gz) file -> batches of whole records ----------------------------------------------
 * Replaces pyFastq.FastqReader as the reference uses it (src/Quade.py:203-214: one .next() per record):
 * a reader owns two threads that read + inflate ("*.gz": gzip, any number of members; BGZF / bgzip files
 * are cut into blocks by their header fields and inflated in parallel on the library's pool; else plain
 * text) and scan + batch the file ahead of the consumer.  A batch holds exactly batch_records kept records
 * (fewer at the end of the file only); a record whose sequence and quality lengths differ is skipped
 * inside its own stream, a trailing partial record ends the stream, a last line
 * without newline counts.  text/rec_off stay valid until qd_text_batch_free(handle). */
typedef struct qd_reader qd_reader;
struct qd_text_batch {
    const uint8_t* text;    /* whole records, 4 lines each */
    int64_t text_len;
    const int64_t* rec_off; /* n_records + 1 offsets into text, as qd_fastq_index gives them */
    int64_t n_records;      /* 0 = end of the stream (handle is NULL then) */
    void* handle;
};
int qd_reader_open(const char* path, int64_t batch_records, int32_t queue_depth, qd_reader** out);
int qd_reader_next(qd_reader* reader, qd_text_batch* out); /* blocks until a batch is ready */
int qd_text_batch_free(void* handle);
int qd_reader_close(qd_reader* reader);
const char* qd_reader_last_error(const qd_reader* reader); /* reader == NULL: why qd_reader_open failed on this thread */

/* ---- ordinary gzip files: parallel inflate on the library's pool ------------------------------------------------
 * The reference opens ordinary .fastq.gz files (src/Quade.py:203-206, 234-236; its fixtures under test/dataset
 * are single gzip members): one DEFLATE stream, which a single thread inflates at a few hundred MB/s.  The reader
 * cuts such a file at fixed offsets, finds a block start behind every cut by trying every bit offset, inflates
 * the chunks in parallel into 16-bit symbols over a window of markers, proves every boundary by the chain from the
 * start of the stream, resolves the markers in file order and checks every member's CRC-32 and ISIZE
 * (quade_amd/csrc/quade_pgz.h).  Result: the bytes zlib would give, or an error.
 * qd_io_set_option names (process-wide; tests and tuning):
 *   "parallel_gunzip"        1 (default) / 0 = one thread per file (libdeflate per member, streaming zlib beyond 32 MB)
 *   "gunzip_chunk_bytes"     compressed bytes per chunk (default 4 MiB, at least 64 KiB)
 *   "gunzip_min_file_bytes"  smaller files are inflated by one thread (default 8 MiB)
 *   "gunzip_in_flight"       chunks in flight per file, 0 (default) = half the pool's threads, at least 4
 *   "test_deflate_fail_after" / "test_inflate_fail_after"  tests: a device lane of the sink / of a reader treats the device as
 *                            failed after this many batches / runs (-1, the default: never) */
int qd_io_set_option(const char* name, int64_t value);
/* Chunks of this reader's file that were inflated speculatively and proven / inflated by the coordinator itself. */
int qd_reader_gunzip_stats(const qd_reader* reader, int64_t* parallel_chunks, int64_t* serial_chunks);
/* A whole gzip file image in memory -> its text, by the same parallel inflater (chunk_bytes 0 = the option's value).
 * stats (may be NULL): int64[5] = pieces, of them speculative and proven, inflated by the coordinator, members whose
 * trailer was checked, bit offsets tried by the block searches.  QD_ERR_FORMAT: damaged or truncated stream
 * (qd_gunzip_last_error); QD_ERR_INVALID: out_cap too small. */
int qd_gunzip_buffer(const uint8_t* comp, int64_t comp_len, int64_t chunk_bytes, uint8_t* out, int64_t out_cap,
                     int64_t* out_len, int64_t* stats);
const char* qd_gunzip_last_error(void);

/* ---- BGZF inflate on the device ------------------------------------------------------------------------
 * The gunzip inside pyFastq.FastqReader (src/Quade.py:203-214), for BGZF (bgzip) files: their blocks are
 * independent gzip members of <= 64 KiB that carry their compressed and inflated sizes, so a run of them is
 * inflated one block per GPU lane.  An inflater owns a stream and grow-only staging buffers on one device and
 * is driven by one thread at a time (the native reader gives each of its files one).
 * qd_inflater_run: comp[0..comp_len) = whole BGZF blocks back to back, out_len = the sum of their ISIZE
 * fields; blocking.  Every block's CRC32 and length are checked on the host.  QD_ERR_FORMAT: not whole BGZF
 * blocks, sizes inconsistent, or a block did not inflate / check (*bad_block = its index, else -1) -- the
 * caller may inflate that run itself (the reader does).  No reference counterpart beyond the gunzip. */
typedef struct qd_inflater qd_inflater;
int qd_inflater_create(int device_id, qd_inflater** out);
int qd_inflater_run(qd_inflater* inflater, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_len,
                    int32_t* bad_block);
/* The same with `out` in page-locked memory from qd_pinned_alloc: the text is copied from the device straight
 * into it (no staging copy on the host). */
int qd_inflater_run_pinned(qd_inflater* inflater, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_len,
                           int32_t* bad_block);
void* qd_pinned_alloc(int64_t bytes); /* NULL on failure */
void qd_pinned_free(void* p);
/* ABI v4 (form 3: v6).  Which kernel inflates the blocks: 3 (the default) = one LANE decodes a block's symbols once into tokens, 64 blocks
 * per wave, then a workgroup per block resolves the tokens (quade_inflate3.hip); 2 = 1 024 lanes per block (spans decoded from guessed starts
 * that synchronise, matches resolved by pointer jumping: quade_inflate.hip); 1 = one wave per block, one symbol after the other (r02).  Same results, same status codes.
 * The environment variable QUADE_INFLATE_FORM sets the form new inflaters start with. */
int qd_inflater_set_form(qd_inflater* inflater, int32_t form);
int qd_inflater_destroy(qd_inflater* inflater);
const char* qd_inflater_last_error(const qd_inflater* inflater);
/* A reader whose BGZF runs go through an inflater on `device_id` (< 0: host threads, as qd_reader_open). */
int qd_reader_open_on(const char* path, int64_t batch_records, int32_t queue_depth, int32_t device_id, qd_reader** out);
/* BGZF runs of this reader inflated by the device / by host threads so far (read it after the last batch). */
int qd_reader_inflate_stats(const qd_reader* reader, int64_t* device_runs, int64_t* host_runs);

/* ---- Huffman-only gzip members on the device --------------------------------------------------------------------
 * The gzip inside FastqWriter.flush_buffers (src/FastqWriter.py:83-90 appends gzip members to the destination files),
 * for the driver's `gzip_level : -1`: a member is one dynamic-Huffman DEFLATE block of literals (a byte histogram, a
 * length-limited Huffman code, one table lookup per byte; no string matching) -- any gunzip reads it.  One workgroup
 * codes one piece of text (quade_amd/csrc/quade_deflate.hip); the CRC-32 of every piece is made by the caller.
 * A deflater owns a stream and grow-only staging buffers on one device and is driven by one thread at a time.
 * qd_deflater_run: piece i = text[i][0 .. text_len[i]) (text_pinned != 0: every text[i] is page-locked memory from
 * qd_pinned_alloc and is copied to the device without a staging copy); member i lands at out + i * out_stride
 * (ordinary memory, out_stride >= qd_huffman_member_bound(longest piece), a multiple of 4), its length in
 * member_len[i]; member_len[i] == 0: that member did not fit out_stride (make it on the host).  Blocking.
 * qd_sink_set_device_deflate: the sink's Huffman-only members are made on `device_id` while the process has
 * page-locked buffers to spare (576 x 2.75 MB, made as its six lanes come up); a piece that finds none is coded on its pool thread as before, so the
 * host and the device share the work; device_id < 0: host only (the default).  gzip_level -1 and 1 are affected (the levels
 * the device implements, qd_deflater_set_level); sinks at other levels ignore the device. */
typedef struct qd_deflater qd_deflater;
int qd_deflater_create(int device_id, qd_deflater** out);
int qd_deflater_run(qd_deflater* deflater, int32_t n_pieces, const uint8_t* const* text, const int64_t* text_len,
                    const uint32_t* crc32, int32_t text_pinned, uint8_t* out, int64_t out_stride, int64_t* member_len);
int64_t qd_huffman_member_bound(int64_t text_len);
/* ABI v4.  Which members the deflater makes: -1 (the default) = Huffman only, as above; 1 = LZ77 + dynamic Huffman, the
 * driver's `gzip_level : 1` (greedy parse, 4-byte hash of last positions + runs, 32 KiB window; the piece is coded as 64 KiB
 * dynamic-Huffman blocks joined by empty stored blocks in ONE member).  Same slots, same bound, same fallback rule
 * (member_len 0); other levels stay with the host's libdeflate / zlib: QD_ERR_INVALID.
 * At level 1 qd_deflater_run accepts crc32 == NULL: every member's CRC-32 then comes from the coder itself (each sub-block's,
 * taken while its text is staged, combined per piece on the device), as in the device pipeline.  At level -1 NULL stays
 * QD_ERR_INVALID. */
int qd_deflater_set_level(qd_deflater* deflater, int32_t level);
int qd_deflater_destroy(qd_deflater* deflater);
const char* qd_deflater_last_error(const qd_deflater* deflater);
int qd_sink_set_device_deflate(qd_sink* sink, int32_t device_id);
int qd_sink_device_members(qd_sink* sink, int64_t* device_members); /* of qd_sink_stats' members: made on the device */

/* ---- ordinary gzip files on the device (ABI v6) ----------------------------------------------------------------------
 * What it replaces: the gunzip inside pyFastq.FastqReader for the reference's real input format -- src/Quade.py:203-206, 234-236 open
 * plain .fastq.gz files, and its fixtures test/dataset/[*].fastq.gz are single gzip members.  The pipeline (qd_pipe_run) feeds such
 * files through these kernels; this entry point inflates a whole file image for tests and measurements: gz[0 .. gz_len) = one or more
 * gzip members -> out (at most out_cap bytes), *out_len = the text's size.  Every member's CRC-32 and ISIZE are checked.  step_bytes:
 * compressed bytes per step (what the pipeline takes per batch and stream); stretch_bytes / unit_text: 0 = the defaults (16 KiB of
 * compressed bytes per probed stretch, at most 2 MiB of text per resolving workgroup).  stats (may be NULL): int64[8] = members, steps,
 * stretches probed, units decoded, units dropped (a false block start: their predecessor ran through them), steps that ended inside
 * a block, decodes done again without the probe's text filter (the stream is not text), 0.
 * QD_ERR_FORMAT: not gzip, damaged, or beyond what the device decodes (the pipeline then hands the file to the host's inflater). */
int qd_dev_gunzip(int device_id, const uint8_t* gz, int64_t gz_len, uint8_t* out, int64_t out_cap, int64_t* out_len, int64_t step_bytes,
                  int64_t stretch_bytes, int64_t unit_text, int64_t* stats);

/* ---- device buffers kept across pipelines (ABI v6) -------------------------------------------------------------------
 * No counterpart in the reference (its buffers are Python objects).  The large device buffers of a pipeline -- windows, token slots,
 * upload rings -- go to a per-device free list of the process when the pipeline is destroyed, and the next pipeline is served from
 * it: hipMalloc of ~25 GB takes between 50 ms and over a second on this pool's boxes, which a process that runs several jobs pays
 * once.  The list holds at most QUADE_POOL_GB gigabytes (environment; default 64, 0 = no list); page-locked host buffers (the
 * feeders' read buffers, the collector's slabs) have a list of their own (QUADE_POOL_PINNED_GB, default 4).  qd_pool_trim gives
 * everything on both lists back to the driver (memory in use by live objects is not touched); always QD_OK. */
int qd_pool_trim(void);

/* ---- device-resident chunk pipeline (ABI v5) ---------------------------------------------------------------------
 * Replaces, for whole chunks, the per-pair loop of Quade.double_index_parser / simple_index_parser and everything it
 * calls (src/Quade.py:195-254: four FastqReader.next(), slice + fuse, Sample.FINDER; src/FastqWriter.py:48-90: name tag,
 * record format, gzip append) with the fastq TEXT staying on the device between the stages: BGZF blocks are inflated
 * there, records are found (a record whose sequence and quality lengths differ is dropped inside its own stream,
 * SURVEY.md F6), pairs are formed in lock step (the chunk ends with its first exhausted stream, Quade.py:223-224), index
 * rows are packed and matched (the context's counters move), records are scattered by routing code in input order,
 * formatted ("@name:IDX[:MOL]", FastqWriter.py:61-69), CRC-32'd and coded into gzip members; only compressed bytes
 * cross PCIe.  Inputs the device cannot inflate (ordinary gzip members, plain text) are inflated by the host's readers
 * and join the same path as text.  The sink must be at gzip_level 1 or -1 (the levels the device codes).
 * qd_pipe_run processes the chunks in order (input for the next chunks is read ahead) and returns when every member is
 * in its file; it is driven by one thread, the context must not be used by another meanwhile.  begin_message /
 * end_message (may be NULL) are printed to stdout when a chunk starts / when its last record is in its files. */
typedef struct qd_pipe qd_pipe;
typedef struct qd_pipe_chunk {
    const char* r1;  /* seq_R1 file of the chunk (src/Quade.py:119) */
    const char* r2;  /* seq_R2 */
    const char* i1;  /* index_R1 */
    const char* i2;  /* index_R2; NULL with a single-index plan */
    qd_sink* sink;   /* where the chunk's records go (one sink for the run, or one per chunk part directory) */
    const char* begin_message;
    const char* end_message;
    /* One part of a chunk that several ranks share (all zero: the whole chunk).  Stream s (r1, r2, i1, i2) is read from file offset
     * start_offset[s] on -- a BGZF block boundary --, the first skip_bytes[s] bytes of its text and then its first skip_kept[s] kept
     * records are dropped, and the part is over after max_pairs pairs (0: at the first exhausted stream).  qd_pipe_index gives the numbers. */
    int64_t start_offset[4];
    int64_t skip_bytes[4];
    int64_t skip_kept[4];
    int64_t max_pairs;
} qd_pipe_chunk;
typedef struct qd_pipe_stats {
    int64_t pairs, batches;
    int64_t bgzf_blocks;         /* inflated (and CRC-checked) on the device */
    int64_t host_inflated_runs;  /* runs of BGZF blocks the device refused and the host inflated */
    int64_t text_segments;       /* uploads of text inflated by the host's readers (ordinary gzip, plain files) */
    int64_t pieces;              /* gzip members made */
    int64_t host_coded_pieces;   /* of them by the host (a member that did not fit its slot on the device) */
    int64_t text_in_bytes, text_out_bytes, gzip_bytes;
    int64_t rescans;             /* window scans repeated (line table too small, host-inflated text) */
    /* wall seconds: the whole call; the driver waiting for input from the feeders, for its read-backs from the device, for an
     * output set the collector still holds, in device allocations; the collector waiting for the device, downloading, appending */
    double run_s, wait_input_s, wait_sync_s, wait_out_set_s, alloc_s, collector_wait_s, download_s, append_s;
    /* ABI v6: ordinary gzip files (the reference's input format) inflated on the device */
    int64_t gzip_steps;      /* inflate steps of such streams (one per stream and top-up) */
    int64_t gzip_units;      /* stretches decoded by a lane each, from a block start that the chain from the member's start proved */
    int64_t gzip_members;    /* members whose CRC-32 and ISIZE were checked */
    int64_t gzip_fallbacks;  /* streams the device gave up (damaged, or beyond what it decodes): the host's inflater took them over */
} qd_pipe_stats;
int qd_pipe_create(qd_ctx* ctx, qd_pipe** out); /* the context holds plan and barcodes */
/* A chunk that several ranks share ("large single chunks are split into contiguous row ranges").  The reference pairs
 * record j of every stream counted from the start of the chunk (src/Quade.py:210-221), and a dropped record shifts its stream, so a
 * rank cannot start in the middle of a file without knowing how many lines and kept records lie before.  qd_pipe_index is the first
 * pass: the BGZF file `path` is cut into world x grains_per_rank grains at block boundaries, this rank inflates its grains on the
 * device and reports, for each and for each residue of (lines before the grain) mod 4: the kept records that start in it, and how
 * many bytes into the grain the first of them starts (0xFFFFFFFF: none).  The ranks exchange these tables (any transport: they are a
 * few hundred bytes per grain), add the line counts up -- which fixes every grain's residue -- and the kept counts, and derive the
 * start_offset / skip_bytes / skip_kept / max_pairs of every rank's part (quade_amd/dist.py: plan_parts).  incomplete[q] != 0: a record
 * of the grain reaches beyond the text this rank looked at -- the caller falls back to one rank per chunk.  QD_ERR_UNSUPPORTED: the
 * file is not BGZF throughout, or a rank's share exceeds one window. */
typedef struct qd_grain_info {
    int64_t file_offset;   /* of the grain's first BGZF block */
    uint32_t n_lines;      /* newlines inside the grain */
    uint32_t kept[4];      /* kept records whose header line starts in the grain, by residue */
    uint32_t skip_bytes[4]; /* from the grain's first byte of text to its first kept record's header */
    uint32_t incomplete[4];
} qd_grain_info;
int qd_pipe_index(qd_pipe* pipe, const char* path, int32_t world, int32_t rank, int32_t grains_per_rank, qd_grain_info* out, int32_t cap,
                  int32_t* n_out);
/* "batch_pairs": pairs per batch at most (default 2 000 000; windows of text are sized from it, at most 1 GiB per stream);
 * "member_slots_bytes": device memory the member slots of one batch may take (default 12 GiB): a member holds 1 MiB of one destination's
 * text, less (down to 64 KiB) when thousands of destinations would need more slots than that;
 * "device_gunzip": 1 (default) = ordinary gzip files (one or more members that are not BGZF blocks) are inflated on the device too
 * (gz_probe / inflate3_tokens / gz_resolve / gz_windows / gz_fixup); 0 = by the host's parallel inflater, uploaded as text;
 * "test_fail_inflate_batch": tests -- the device's BGZF result of that batch is treated as refused;
 * "test_host_code_every": tests -- every k-th member is coded by the host, as one that did not fit its slot on the device would be.
 * Any other name is QD_ERR_INVALID -- also the names that selected variants which were measured, not kept and have been removed
 * (another BGZF inflate form, a second inflate stream, the coder on a stream of its own: DESIGN.md 7).  The pipeline inflates BGZF
 * blocks with quade_inflate3.hip on one stream and codes on the compute stream.  No exported function changed: QD_ABI_VERSION stays 6. */
int qd_pipe_set_option(qd_pipe* pipe, const char* name, int64_t value);
int qd_pipe_run(qd_pipe* pipe, const qd_pipe_chunk* chunks, int32_t n_chunks, qd_pipe_stats* stats);
const char* qd_pipe_last_error(const qd_pipe* pipe);
int qd_pipe_destroy(qd_pipe* pipe);
/* ---- the pipeline's device stages one at a time, over host buffers (bindings that hold text in memory; tests) ----------
 * qd_dev_fastq_scan: the record scan of qd_pipe_run on `device_id` (what qd_fastq_index does on the host, same rules): text
 * = whole lines from a record start on; at_eof: a last line without newline counts; need: reads shorter than this count as
 * short; line_cap: lines the scan's table holds (result[5] != 0: more than that -- result[0] says how many).  recs_out:
 * 6 uint32 per kept record (head, name_off, name_len, seq, seq_len, qual -- offsets into text), at most recs_cap records;
 * result_out: uint32[8] = n_lines, n_records, n_kept, n_short, tail_start, overflow, -, -.  Returns the kept records. */
int64_t qd_dev_fastq_scan(int device_id, const uint8_t* text, int64_t text_len, int32_t at_eof, int32_t want_names, int32_t need,
                          int64_t line_cap, uint32_t* recs_out, int64_t recs_cap, uint32_t* result_out);
/* CRC-32 (gzip's) of n bytes, made on the device from ranges of range_bytes (<= 65536) whose CRCs are combined */
int qd_dev_crc32(int device_id, const uint8_t* data, int64_t n, int64_t range_bytes, uint32_t* crc_out);
/* the stable sort by destination of the scatter stage: perm_out[k] = the pair at sorted position k; with len / offsets_out
 * (n + 1 values) also the exclusive sums of len in sorted order, i.e. where every pair's output record starts */
int qd_dev_sort_by_dest(int device_id, const uint16_t* dest, int64_t n, int32_t n_dest, const uint32_t* len, uint32_t* perm_out,
                        uint32_t* offsets_out);
/* the quality counters' stage (qd_qstats_enable above) over host buffers: pairs [0, n_pairs) of two texts with their record
 * tables (6 uint32 per record, qd_dev_fastq_scan's layout) and routing codes are uploaded, counted by the kernel qd_pipe_run
 * launches, and added to the context's table.  Every record's sequence and quality range is checked against len1 / len2 and
 * every code against 2*S (0xFFFF apart) before anything is launched: QD_ERR_INVALID.  QD_ERR_STATE when the counters are off.
 * Returns when the launch has finished. */
int qd_dev_qstats(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes);
/* the clip stage (qd_clip_set above; no reference counterpart) over host buffers, as qd_dev_trim: reads [0, n_pairs) of two texts
 * with their record tables are uploaded (the texts 3 bytes off alignment) and run through the kernel qd_pipe_run launches;
 * out_recs1 / out_recs2 receive the whole tables, seq and qual moved by the front clip and seq_len the length the read keeps, and
 * the context's table grows.  Every record's sequence and quality range is checked against len1 / len2 before anything is
 * launched: QD_ERR_INVALID.  QD_ERR_STATE when the stage is off.  Returns when the launch has finished. */
int qd_dev_clip(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2);
/* the trimming stage (qd_trim_set above; no reference counterpart) over host buffers: reads [0, n_pairs) of two texts with their
 * record tables (6 uint32 per record, qd_dev_fastq_scan's layout) are uploaded and trimmed by the kernel qd_pipe_run launches;
 * out_recs1 / out_recs2 receive the tables with every seq_len replaced by the length the read keeps, and the context's counters
 * grow.  Every record's sequence and quality range is checked against len1 / len2 before anything is launched: QD_ERR_INVALID.
 * QD_ERR_STATE when trimming is off.  Returns when the launch has finished. */
int qd_dev_trim(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2);
/* the overlap trimming stage (qd_pairtrim_set above; no reference counterpart) over host buffers, as qd_dev_trim: pairs
 * [0, n_pairs) of two texts with their record tables are uploaded and run through the kernel qd_pipe_run launches; out_recs1 /
 * out_recs2 receive the tables with every seq_len replaced by the length the read keeps, and the context's table grows.  Every
 * record's sequence and quality range is checked against len1 / len2 before anything is launched: QD_ERR_INVALID.  QD_ERR_STATE
 * when the stage is off.  Returns when the launch has finished. */
int qd_dev_pairtrim(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                    const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2);
/* the overlap base correction (qd_paircorrect_set above; no reference counterpart) over host buffers, as qd_dev_pairtrim: pairs
 * [0, n_pairs) of two texts with their record tables are uploaded (the texts 3 bytes off alignment) and run through the kernel
 * qd_pipe_run launches; out_text1 / out_text2 (len1 / len2 bytes) receive the whole texts as the stage leaves them, and the context's
 * table grows.  inserts != NULL: n_pairs insert lengths I (0 = none) used as given; every record's sequence and quality range is
 * checked against len1 / len2, and inserts[k] <= L1 + L2, before anything is launched: QD_ERR_INVALID.  inserts == NULL: the
 * overlap trimming kernel runs first with the context's parameters and supplies them, as in qd_pipe_run (QD_ERR_STATE when that stage
 * is off; its table grows too).  QD_ERR_STATE when the stage is off.  Returns when the launches have finished. */
int qd_dev_paircorrect(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                       const uint32_t* recs2, int64_t n_pairs, const uint64_t* inserts, uint8_t* out_text1, uint8_t* out_text2);
/* the post-trimming stage (qd_posttrim_set above; no reference counterpart) over host buffers, as qd_dev_trim: reads [0, n_pairs)
 * of two texts with their record tables are uploaded (the texts 3 bytes off alignment) and run through the kernel qd_pipe_run
 * launches; out_recs1 / out_recs2 receive the tables with every seq_len replaced by the length the read keeps, and the context's
 * table grows.  Every record's sequence and quality range is checked against len1 / len2 before anything is launched:
 * QD_ERR_INVALID.  QD_ERR_STATE when the stage is off.  Returns when the launch has finished. */
int qd_dev_posttrim(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                    const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2);
/* the read filter (qd_filter_set above; no reference counterpart) over host buffers, as qd_dev_qstats: pairs [0, n_pairs) of two
 * texts with their record tables and routing codes are uploaded (the texts 3 bytes off alignment) and run through the kernel
 * qd_pipe_run launches; reasons[j] receives 0 (kept) or the number of the rule that dropped pair j, and the context's table grows.
 * Every record's sequence and quality range is checked against len1 / len2 and every code against 2 * S before anything is
 * launched: QD_ERR_INVALID.  QD_ERR_STATE when the stage is off.  Returns when the launch has finished. */
int qd_dev_filter(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, uint8_t* reasons);
/* the k-mer screen (qd_screen_set above; no reference counterpart) over host buffers, as qd_dev_filter: pairs [0, n_pairs) of two
 * texts with their record tables and routing codes are uploaded (the texts 3 bytes off alignment) and run through the kernel
 * qd_pipe_run launches.  drop_in: NULL or a byte per pair; hits_out: uint32[n_pairs][2], hits(R1) and hits(R2); flag_out: a byte
 * per pair.  flag_out[j] is drop_in[j] when that is non-zero: the pair is then skipped and counted nowhere, with hits 0, 0.  Else
 * it is QD_SCREEN_DROPPED when the pair is matched and the action is QD_SCREEN_DROP, else 0.  The context's table grows.  Every
 * record's sequence and quality range is checked against len1 / len2 and every code against 2 * S before anything is launched:
 * QD_ERR_INVALID.  QD_ERR_STATE when the stage is off.  Returns when the launch has finished. */
int qd_dev_screen(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, const uint8_t* drop_in, uint32_t* hits_out,
                  uint8_t* flag_out);
/* the per-cycle counters' stage (qd_cstats_enable above; no reference counterpart) over host buffers, as qd_dev_qstats: pairs
 * [0, n_pairs) of two texts with their record tables and routing codes are uploaded (the texts 3 bytes off alignment), counted by
 * the kernel qd_pipe_run launches, and added to the context's table.  drop may be NULL; otherwise pair j is skipped where
 * drop[j] != 0 (the read filter's reason bytes).  Every record's sequence and quality range is checked against len1 / len2 and
 * every code against 2 * S (0xFFFF apart) before anything is launched: QD_ERR_INVALID.  QD_ERR_STATE when the table is off.
 * Returns when the launch has finished. */
int qd_dev_cstats(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, const uint8_t* drop);
/* the duplication tally (qd_dup_set above; no reference counterpart) over host buffers, as qd_dev_cstats: pairs [0, n_pairs) of
 * two texts with their record tables and routing codes are uploaded (the texts 3 bytes off alignment), keyed, listed and tallied
 * by the kernels qd_pipe_run launches, and added to the context's two tables.  drop may be NULL; otherwise pair j is skipped where
 * drop[j] != 0 (the read filter's reason bytes).  Every record's sequence and quality range is checked against len1 / len2 and
 * every code against 2 * S (0xFFFF apart) before anything is launched: QD_ERR_INVALID.  QD_ERR_STATE when the stage is off.
 * Returns when the launches have finished. */
int qd_dev_dup(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
               const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, const uint8_t* drop);
/* the adapter content stage (qd_adapters_set above; no reference counterpart) over host buffers, as qd_dev_qstats: pairs
 * [0, n_pairs) of two texts with their record tables and routing codes are uploaded (the texts 3 bytes off alignment), searched by
 * the kernel qd_pipe_run launches, and added to the context's table.  Every record's sequence and quality range is checked against
 * len1 / len2 and every code against 2 * S (0xFFFF apart) before anything is launched: QD_ERR_INVALID.  QD_ERR_STATE when the stage
 * is off.  Returns when the launch has finished. */
int qd_dev_adapters(qd_ctx* ctx, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                    const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes);
/* ---- the routing and format stages of qd_pipe_run one at a time (additive: QD_ABI_VERSION stays 6) ----------------------------
 * These three run the kernels between the record tables and the packed members on host buffers, for tests that compare every stage
 * with a plain model (tests/route_model.py).  They are stage harnesses: no reference counterpart (what the stages themselves
 * restate of the reference is said at qd_pipe_run above).  Each uses its own hipMalloc scratch on `device_id` and returns when its
 * launches have finished.  Record tables are uint32[n][6] in qd_dev_fastq_scan's layout; every range a table names is checked
 * against its text's length before anything is launched (QD_ERR_INVALID), so a bad table cannot become a bad address.
 * Bytes that no kernel owns hold QD_DEV_GUARD_BYTE when the entry returns.  qd_dev_pack_rows and qd_dev_route_format take n >= 1
 * pairs, qd_dev_pack_members n >= 0 members. */
#define QD_DEV_GUARD_BYTE 0xEE
/* qd_dev_pack_rows runs qd_text_pack_rows (quade_text.hip: pack_rows; no reference counterpart of its own, it makes the operands
 * of src/Quade.py:217-218): index rows of pairs [0, n) of `layout`'s one or two index streams, text[k] / recs[k] -> seq_rows[k]
 * (n x seq_stride[k]), qual_rows[k] (n x qual_stride[k]), len_rows[k] (n).  short_idx holds short_room >= short_cap entries, all
 * 0xFFFFFFFF before the launch: the kernel stores the pairs with a read shorter than its window (each once, any order) in the first
 * min(*n_short, short_cap) of them and *n_short says how many there are. */
int qd_dev_pack_rows(int device_id, const qd_layout* layout, const uint8_t* const text[2], const int64_t text_len[2],
                     const uint32_t* const recs[2], int64_t n, int64_t short_cap, uint8_t* const seq_rows[2], uint8_t* const qual_rows[2],
                     uint8_t* const len_rows[2], uint32_t* short_idx, int64_t short_room, uint32_t* n_short);
/* qd_dev_route_format runs the chain of qd_pipe_run's batches behind the routing codes (no reference counterpart as a stage: its
 * output is what src/Sample.py:74-91 and src/FastqWriter.py:61-69 write, per destination): qd_text_dest_lens, qd_text_sort_by_dest,
 * both qd_text_scan_gathered, qd_text_dest_bounds, the host's layout of the output text (qd_text_out_layout, the function the
 * pipeline calls) and qd_text_format with both reads' records in one buffer.  text / text_len / recs: R1, R2, I1, I2 (I2 is not
 * read with a single-index plan); byte o of a text lies at device address o + shift (mod 16), shift 0..15.  drop (may be NULL): a
 * pair with drop[j] != 0 gets no room.  Out: dest, len1, len2, perm, sdest (n each), g1, g2 (n + 1), first, g1_first, g2_first,
 * base1, base2 (2 * n_samples + 1 each; an entry of g1_first / g2_first whose destination has no pair is 0xFFFFFFFF), and the text
 * in out[0 .. out_cap), which is QD_DEV_GUARD_BYTE wherever no record lies; *out_used = the bytes the regions take (rounded up to
 * 16).  QD_ERR_INVALID with *out_used set when out_cap is below that: nothing was formatted. */
int qd_dev_route_format(int device_id, const qd_plan* plan, int32_t n_samples, int32_t write_pass, int32_t write_fail, int32_t write_undet,
                        const uint8_t* const text[4], const int64_t text_len[4], const uint32_t* const recs[4], const uint16_t* codes,
                        const uint8_t* drop, int64_t n, int32_t shift, uint16_t* dest, uint32_t* len1, uint32_t* len2, uint32_t* perm,
                        uint16_t* sdest, uint32_t* g1, uint32_t* g2, uint32_t* first, uint32_t* g1_first, uint32_t* g2_first, int64_t* base1,
                        int64_t* base2, uint8_t* out, int64_t out_cap, int64_t* out_used);
/* qd_dev_pack_members runs qd_text_pack_members (member_offsets + member_copy; no reference counterpart: the reference appends
 * whole gzip files): members of len[i] <= stride bytes in slots of `stride` bytes -> offsets[n + 1] (exclusive sums of len, the
 * total last) and packed[0 .. packed_cap) = the members back to back, QD_DEV_GUARD_BYTE behind offsets[n]. */
int qd_dev_pack_members(int device_id, const uint8_t* slots, int64_t stride, const uint32_t* len, int64_t n, uint64_t* offsets, uint8_t* packed,
                        int64_t packed_cap);
/* what a context was made with / holds (the pipeline reads them; bindings may too) */
int qd_get_plan(const qd_ctx* ctx, qd_plan* out);
int qd_context_device(const qd_ctx* ctx, int32_t* device_id);

#ifdef __cplusplus
}
#endif
#endif /* QUADE_HIP_H */
