// C ABI of libquade_hip.so: context, plan, barcode table, launches, counters, pinned slots.
// Host C++ over the HIP runtime; kernels live in quade_kernels.hip.  See include/quade_hip.h.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is bound at run time (dlopen), single-GPU users never load it

#include <algorithm>
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/quade_hip.h"
#include "quade_common.h"
#include "batch_sizes.h"
#include "gz_framing.h"
#include "quade_kernels.h"
#include "quade_inflate.h"
#include "quade_inflate3.h"
#include "quade_deflate.h"
#include "quade_text.h"
#include "quade_mismatch.h"
#include "quade_unknown.h"
#include "quade_hop.h"
#include "quade_qstats.h"
#include "quade_cstats.h"
#include "quade_adapters.h"
#include "quade_clip.h"
#include "quade_trim.h"
#include "quade_pairtrim.h"
#include "quade_paircorrect.h"
#include "quade_posttrim.h"
#include "quade_filter.h"
#include "quade_screen.h"
#include "quade_dup.h"
#include "quade_buf.h"

typedef uint64_t u64;

namespace {

// who owns what: quade_buf.h, DESIGN.md 7.0
template <class T>
using DevArr = qbuf::Arr<T, qbuf::DriverDev>;  // long-lived tables
template <class T>
using TrimArr = qbuf::Arr<T, qbuf::DriverDevTrim>;  // what is allocated while a pipeline's pool may hold the device's memory
template <class T>
using PinArr = qbuf::Arr<T, qbuf::DriverPin>;

thread_local std::string g_create_error;

struct Slot {
    hipStream_t stream = nullptr;   // kernel + downloads of this slot
    hipEvent_t uploaded = nullptr;  // recorded on the context's upload stream behind this slot's H2D copies
    PinArr<uint8_t> h_base;
    DevArr<uint8_t> d_base;
    qd_slot_buffers h{};        // host views
    qd_slot_buffers d{};        // device views (same struct, device pointers)
    // pinned + device: the two streams' lists merged (unique, ascending; 2 * short_cap indices), then the
    // listed reads' lengths per stream (2 * short_cap bytes each): all the fixup kernel needs of the len rows
    PinArr<uint32_t> h_short;
    DevArr<uint32_t> d_short;
    bool busy = false;
};

enum { K_FAST = 1, K_GENERIC = 2 };

// Per stream one device buffer that holds `units` units of a batch (pairs, here) and grows on demand: the rescue's list of a batch's
// undetermined pairs and the two tallies' batch scratch.
struct StreamScratch {
    struct Buf {
        hipStream_t stream;
        TrimArr<uint8_t> buf;
        size_t units;  // bytes_for(units) bytes; 0 beside an empty buf
    };
    std::vector<Buf> bufs;
    Buf* find(hipStream_t st);
    Buf* need(qd_ctx* c, hipStream_t st, size_t units, size_t (*bytes_for)(size_t));  // nullptr: failed, qd_last_error has the text
    void release() { bufs.clear(); }  // (the caller waited for the context's work)
};

// A tally of keys on the device (the unknown barcodes, the duplication report): the table (one allocation, quade_unknown.h), per
// stream the scratch of a batch, and the event behind the last launch's count kernel that a launch on another stream waits for
// before its claim kernel.  The tally_* functions work on it.
struct KeyTally {
    TrimArr<uint8_t> mem;  // empty = off
    int64_t slots = 0;
    UnknownTable t{};
    int tag_bits = 64;  // options "unknown_tag_bits" / "dup_tag_bits" (tests); outlives the table
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool recorded = false;
    StreamScratch scratch;
};

// A table of 64-bit counters on the device with what its messages call it: a read stage's (qd_ctx::stage) or the index-hopping
// matrix'.  The table_*, stage_* and stages_* functions work on it.
struct StageTable {
    const char* what;       // in an allocation's error
    const char* launch;     // in a launch's error (the matrix has none of its own)
    const char* off_text;   // the error text while the table is off
    const char* size_text;  // the error text for a caller's table of another size
    bool per_destination;   // a row per destination: a new plan and new barcodes switch it off
    TrimArr<u64> d;         // empty = off
    size_t n_values = 0;    // as allocated
};

// the read stages, in the pipeline's order
enum StageId { ST_ADAPTERS, ST_CLIP, ST_TRIM, ST_PAIRTRIM, ST_PAIRCORRECT, ST_POSTTRIM, ST_FILTER, ST_SCREEN, ST_QSTATS, ST_CSTATS, ST_DUP, ST_COUNT };

// a stage's parameters while it is off: all zero, but for the filter's, whose rules are off at -1 (and qualified_quality is 15)
constexpr qd_filter_params FILTER_OFF{-1, -1, -1, 15, -1, -1};
constexpr qd_filter_dev filter_dev_of(const qd_filter_params& P) {
    return qd_filter_dev{P.min_length, P.max_n, P.max_unqualified_pct, 33 + P.qualified_quality, P.min_mean_quality, P.min_complexity_pct};
}

}  // namespace

struct qd_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    mutable std::string err;
    char dev_name[256] = {0};
    int cu = 0;
    int64_t total_mem = 0;

    bool have_plan = false, have_table = false;
    qd_plan plan{};
    qd_layout lay{};

    // host copy of the barcodes
    int32_t S = 0;
    std::vector<uint8_t> bc;
    std::vector<int32_t> bc_off;

    // device table
    DevArr<uint32_t> d_slots_fast, d_slots_gen;
    DevArr<u64> d_bk16, d_bk32;
    DevArr<u64> d_bkv;      // wide plans: per barcode its two slices as the kernel extracts them (confirmation compare)
    DevArr<uint8_t> d_blen;
    uint32_t mask_fast = 0, mask_gen = 0, seed_fast = 0, seed_gen = 0;
    bool fast_ok = false;
    bool wide = false;      // the fast table holds nibble-packed keys (16 < K <= 32)
    uint32_t lds_bk_off = 0, lds_hist_off = 0, lds_strip_off = 0;
    size_t lds_bytes = 0;       // table image + histogram
    size_t lds_strip_bytes = 0; // per wave: 128*M bytes of molecular staging (M % 4 == 0), else 0
    int opt_wg_per_cu = 0;    // 0 = occupancy query
    int opt_force_generic = 0;
    int opt_block = 0;        // 0 = automatic
    int opt_slot_factor = 0;  // 0 = automatic: QD_SLOT_FACTOR slots per barcode, half that for sample sheets whose image then fits a CU three times
    int opt_mol_strips = 1;   // LDS-staged molecular stores in the fast kernel
    int opt_kernel = 0;       // 0 = automatic, K_FAST / K_GENERIC
    QdKernelCache kcache;     // per-context launch memo (attribute set, occupancy)
    // streams this context has work on (its own, its slots', the caller's) with an event recorded after
    // the last operation issued on each: waits are scoped to the context, never the whole device
    std::vector<std::pair<hipStream_t, hipEvent_t>> tracked;

    // counters
    DevArr<qd_row_t> d_partial;  // [partial_rows][cnt_stride] 32-bit rows the kernels flush into
    DevArr<u64> d_acc;         // [cnt_stride] 64-bit totals: rows folded so far + demux_fixup's signed moves
    DevArr<u64> d_counts;      // [cnt_stride + 4]: 2S+1 counters, then TOTAL at [cnt_stride] (reduce scratch)
    DevArr<u64> d_total;       // all-reduce result, same shape
    uint32_t partial_rows = 0, cnt_stride = 0;
    uint64_t total_pairs = 0;
    uint64_t pairs_in_rows = 0;             // pairs launched since the rows were last folded (bounds every row counter)
    uint64_t fold_limit = 0xFFFFFFFFull;    // option "fold_pairs": fold before pairs_in_rows would pass this
    uint64_t folds = 0;

    std::vector<Slot> slots;
    int64_t slot_pairs = 0;
    // One upload stream for all slots: their H2D copies run one after the other at the full link rate and a
    // slot's kernel starts as soon as ITS rows have arrived.  With the uploads on the slots' own streams the
    // copies of all submitted slots shared the link, finished together, and the link then idled while the
    // kernels, the downloads and the host's next submits went by (48.7 of the link's 57 GB/s, tools/h2d_probe.py).
    hipStream_t up_stream = nullptr;

    // mismatch-tolerant matching (qd_set_mismatches): budgets, device tables, the parameter block's fixed part, and per
    // stream the list of a batch's undetermined pairs ([0] = count, the list from [4]; grown on demand)
    int32_t mm_m1 = 0, mm_m2 = 0;
    MismatchParams mm{};
    DevArr<QdMmBucket> d_mm_htab;
    DevArr<uint16_t> d_mm_cand;
    StreamScratch mm_list;  // pairs + 4 uint32 entries

    // tally of the unknown barcodes (qd_unknown_enable); per stream the scratch of a batch: 2 * pairs + 4 uint32 entries ([0] = count
    // and the list of its undetermined pairs from [4], then from [4 + pairs] each listed pair's slot)
    KeyTally uk;

    // The read stages' tables, by StageId: what each is called, whether it has a row per destination, and, while the stage is on,
    // its counters.  adapters uint64[34850 + (2 * S + 1) * 36], clip uint64[2][12], trim [2][8], pairtrim [1040], paircorrect [10], posttrim [2][16], filter [(2 * S + 1)][8], screen
    // [(2 * S + 1)][8], qstats [(2 * S + 1)][2][6], cstats [QD_CS_VALUES], dup [(2 * S + 1)][5].  Everything that switches stages off,
    // zeroes, reads or adds to a table goes through this array; a new stage adds its row here.
    StageTable stage[ST_COUNT] = {
        {"adapter counters", "adapter content", "the adapter content is not on", "n_values must be 34850+(2*S+1)*36", true},
        {"clip counters", "clip", "clipping is not on", "n_values must be 24", false},
        {"trim counters", "trim", "trimming is not on", "n_values must be 16", false},
        {"overlap trimming table", "overlap trimming", "overlap trimming is not on", "n_values must be 1040", false},
        {"overlap correction counters", "overlap correction", "overlap base correction is not on", "n_values must be 10", false},
        {"post-trim counters", "post-trim", "post-trimming is not on", "n_values must be 32", false},
        {"filter table", "filter", "the read filter is not on", "n_values must be (2*S+1)*8", true},
        {"screen counters", "screen", "the k-mer screen is not on", "n_values must be (2*S+1)*8", true},
        {"quality counters", "quality counters", "the quality counters are not enabled", "n_values must be (2*S+1)*12", true},
        {"cycle counters", "cycle counters", "the cycle counters are not enabled", "n_values must be QD_CS_VALUES", false},
        {"duplication counters", "duplication tally", "the duplication tally is not on", "n_values must be (2*S+1)*5", true},
    };
    // The stages' parameters as given (qd_*_set) and as the kernels take them; a stage that is off holds the off values (stage_off).
    uint8_t adapters[QD_AD_PROBES * QD_AD_K] = {0};  // adapter content of the raw insert reads: the probes as given, and their words
    qd_adapters_dev adapters_dev{};
    qd_clip_params clip{};  // end clipping, window and poly-G trimming of the insert reads
    qd_clip_dev clip_dev{};
    qd_trim_params trim{};  // 3' trimming of the insert reads
    qd_trim_dev trim_dev{};
    qd_pairtrim_params pairtrim{};  // paired-end overlap trimming with insert sizes
    qd_pairtrim_dev pairtrim_dev{};
    qd_paircorrect_params paircorrect{};  // overlap base correction behind it
    qd_paircorrect_dev paircorrect_dev{};
    qd_posttrim_params posttrim{};  // trailing-N, poly-X and max_length trimming behind the three stages above
    qd_posttrim_dev posttrim_dev{};
    qd_filter_params filter = FILTER_OFF;  // read filtering
    qd_filter_dev filter_dev = filter_dev_of(FILTER_OFF);
    // k-mer screen against a reference: besides the parameters the reference's hash table (1 << screen_dev.slots_lg words)
    qd_screen_params screen{};
    qd_screen_dev screen_dev{};
    int64_t screen_kmers = 0;
    TrimArr<u64> d_screen_slots;
    // duplication tally: besides the parameters the key tally; per stream its scratch is the batch list, qd_dup_list_bytes(pairs)
    // bytes (quade_dup.h)
    qd_dup_params dup{};
    qd_dup_dev dup_dev{};
    KeyTally dup_keys;

    // index-hopping matrix (qd_hop_enable): the table uint64[(hop_n1 + 1) * (hop_n2 + 1) + 1] (hop.d == nullptr = off), the two
    // part lookup tables in one allocation (slots of part 1, slots of part 2, then their key words), and per stream a list of
    // a batch's undetermined pairs (pairs + 4 uint32 entries) for the launches that neither rescue nor tally
    StageTable hop{"index-hopping matrix", nullptr, "the index-hopping matrix is not enabled", "n_values must be (n1+1)*(n2+1)+1", true};
    TrimArr<uint8_t> d_hop_parts;
    HopPart hop_part[2]{};
    int32_t hop_n1 = 0, hop_n2 = 0;
    StreamScratch hop_list;
};

namespace {

int fail(const qd_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), QD_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));     \
    } while (0)

hipStream_t resolve_stream(const qd_ctx* c, void* stream) {
    return stream == QD_STREAM_CONTEXT ? c->stream : (hipStream_t)stream;  // NULL = HIP's null stream
}

// remember that `st` carries work of this context up to now
hipError_t track(qd_ctx* c, hipStream_t st) {
    for (auto& t : c->tracked)
        if (t.first == st) return hipEventRecord(t.second, st);
    hipEvent_t ev;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    c->tracked.emplace_back(st, ev);
    return hipEventRecord(ev, st);
}

// host waits for everything this context issued
hipError_t wait_all(qd_ctx* c) {
    for (auto& t : c->tracked) {
        hipError_t e = hipEventSynchronize(t.second);
        if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(c->stream);
}

// the context's own stream waits (on the device) for everything this context issued elsewhere
hipError_t join_into_own_stream(qd_ctx* c) {
    for (auto& t : c->tracked) {
        if (t.first == c->stream) continue;
        hipError_t e = hipStreamWaitEvent(c->stream, t.second, 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void forget_stream(qd_ctx* c, hipStream_t st) {
    for (size_t i = 0; i < c->tracked.size(); ++i)
        if (c->tracked[i].first == st) {
            (void)hipEventDestroy(c->tracked[i].second);
            c->tracked.erase(c->tracked.begin() + (long)i);
            return;
        }
}

// canonical key of a byte string: little-endian packed, zero padded
void canon(const uint8_t* b, int len, u64 w[QD_KEY_WORDS]) {
    for (int i = 0; i < QD_KEY_WORDS; ++i) w[i] = 0;
    for (int i = 0; i < len && i < QD_MAX_KEY; ++i) w[i >> 3] |= (u64)b[i] << (8 * (i & 7));
}

// open-addressing table over the given barcode ordinals; picks the seed with the shortest
// worst-case probe sequence.  Returns slots (size mask+1).
std::vector<uint32_t> build_slots(const std::vector<int>& ids, const std::vector<u64>& keys32,
                                  const std::vector<uint8_t>& blen, uint32_t& mask, uint32_t& seed,
                                  const std::vector<u64>* packed16 = nullptr, uint32_t K = 0, uint32_t slot_factor = QD_SLOT_FACTOR) {
    // >= 4 slots per barcode (half that many cost +8 % on S = 1536 and +13 % on S = 96, twice as many nothing:
    // profiles/r02_slot_table_load.txt), and never fewer than 256: a dozen barcodes in 64 slots have every lane of
    // a wave probing the same few LDS words (S = 12: -7 % with 256 slots)
    uint32_t m = 256;
    while (m < slot_factor * (uint32_t)ids.size()) m <<= 1;
    mask = m - 1;
    std::vector<uint32_t> best;
    uint32_t best_worst = ~0u;
    for (uint32_t sd = 0; sd < 8; ++sd) {
        std::vector<uint32_t> t(m, QD_EMPTY_SLOT);
        uint32_t worst = 0;
        for (int id : ids) {
            const uint32_t h = packed16 ? qd_hash_wide((*packed16)[2 * (size_t)id], (*packed16)[2 * (size_t)id + 1], K, sd)
                                        : qd_hash_key(&keys32[(size_t)id * QD_KEY_WORDS], blen[id], sd);
            uint32_t s = h & mask, probes = 1;
            while (t[s] != QD_EMPTY_SLOT) {
                s = (s + 1) & mask;
                ++probes;
            }
            t[s] = qd_slot_entry(h, (uint32_t)id);
            worst = std::max(worst, probes);
        }
        if (worst < best_worst) {
            best_worst = worst;
            best.swap(t);
            seed = sd;
        }
        if (best_worst <= 2) break;
    }
    return best;
}

void free_table(qd_ctx* c) {
    for (auto* b : {&c->d_slots_fast, &c->d_slots_gen}) b->release();
    for (auto* b : {&c->d_bk16, &c->d_bk32, &c->d_bkv, &c->d_acc, &c->d_counts, &c->d_total}) b->release();
    c->d_blen.release();
    c->d_partial.release();
    c->have_table = false;
}

StreamScratch::Buf* StreamScratch::find(hipStream_t st) {
    for (auto& b : bufs)
        if (b.stream == st) return &b;
    return nullptr;
}

// the stream's buffer with room for `units` units at least, grown (to twice what it held, at least) when it has not
StreamScratch::Buf* StreamScratch::need(qd_ctx* c, hipStream_t st, size_t units, size_t (*bytes_for)(size_t)) {
    Buf* b = find(st);
    if (!b) {
        bufs.emplace_back();
        b = &bufs.back();
        b->stream = st;
        b->units = 0;
    }
    if (b->buf && b->units >= units) return b;
    hipError_t e = hipStreamSynchronize(st);  // the old buffer may still be read by this stream's previous batch
    if (e == hipSuccess) {
        const size_t grown = qbuf::twice(units, b->units);
        b->units = 0;  // should the allocation fail, the next batch allocates again
        e = b->buf.alloc(bytes_for(grown));
        if (e == hipSuccess) b->units = grown;
    }
    if (e == hipSuccess) return b;
    fail(c, QD_ERR_HIP, std::string("stream scratch: ") + hipGetErrorString(e));
    return nullptr;
}

bool tally_slots_ok(int64_t slots) {  // a power of two in 2^10 .. 2^28
    return slots >= ((int64_t)1 << QD_UK_MIN_LG) && slots <= ((int64_t)1 << QD_UK_MAX_LG) && !(slots & (slots - 1));
}

// the tally off and its memory freed (the caller waited for the context's work)
void tally_close(KeyTally& T) {
    T.mem.release();
    T.slots = 0;
    T.recorded = false;
    T.scratch.release();
    if (T.done) (void)hipEventDestroy(T.done);
    T.done = nullptr;
}

// a closed tally on: a zeroed table of `slots` entries and its event; `what` names the table in the error text
int tally_open(qd_ctx* c, KeyTally& T, int64_t slots, const char* what) {
    hipError_t e = T.mem.alloc(qd_uk_bytes(slots));
    if (e == hipSuccess) e = hipMemsetAsync(T.mem, 0, qd_uk_bytes(slots), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&T.done, hipEventDisableTiming);
    if (e != hipSuccess) {
        tally_close(T);
        return fail(c, QD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    qd_uk_carve(T.mem, slots, T.t);
    T.slots = slots;
    return QD_OK;
}

// an empty table again, on `st` (qd_reset_counts)
hipError_t tally_zero(const KeyTally& T, hipStream_t st) { return hipMemsetAsync(T.mem, 0, qd_uk_bytes(T.slots), st); }

// the table as the kernels take it
UnknownTable tally_view(const KeyTally& T) {
    UnknownTable t = T.t;
    t.tag_mask = T.tag_bits >= 64 ? ~0ull : ((1ull << T.tag_bits) - 1);
    return t;
}

// what a launch on `st` waits for before its claim kernel: the last launch's count kernel when that ran on another stream
hipEvent_t tally_before(const KeyTally& T, hipStream_t st) { return T.recorded && T.last != st ? T.done : nullptr; }

// behind a launch's count kernel on `st`
int tally_after(qd_ctx* c, KeyTally& T, hipStream_t st) {
    HIPCHK(c, hipEventRecord(T.done, st));
    T.recorded = true;
    T.last = st;
    return QD_OK;
}

// (the caller waited for the stream: its event, should it be the last one recorded, is not waited for any more)
void tally_retired(KeyTally& T, hipStream_t st) {
    if (T.last == st) T.recorded = false;
}

// What qd_unknown_read and qd_dup_read share: D entries, D <= cap: their key words (QD_KEY_WORDS each) into hk and their counts
// into counts; returns D, -D when cap is too small, or QD_UNKNOWN_READ_ERROR + QD_ERR_* with "<what> read: ..." as the text
int64_t tally_gather(qd_ctx* c, const KeyTally& T, const char* what, int64_t cap, std::vector<u64>& hk, uint64_t* counts) {
    auto bad = [&](const char* msg) { return QD_UNKNOWN_READ_ERROR + (int64_t)fail(c, QD_ERR_HIP, std::string(what) + " read: " + msg); };
    uint64_t tot[4];
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = wait_all(c);
    if (e == hipSuccess) e = hipMemcpy(tot, T.t.totals, sizeof tot, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return bad(hipGetErrorString(e));
    const int64_t D = (int64_t)tot[QD_UK_DISTINCT];
    if (D > cap) return -D;
    if (D == 0) return 0;
    // the occupied entries packed on the device (uk_gather works on the table alone): only they cross the link
    TrimArr<uint8_t> d_out;
    const size_t kbytes = (size_t)D * QD_KEY_WORDS * 8, cbytes = (size_t)D * 8;
    if ((e = d_out.alloc(kbytes + cbytes + 16)) != hipSuccess) return bad(hipGetErrorString(e));
    u64* d_keys = reinterpret_cast<u64*>(d_out.p);
    u64* d_counts = reinterpret_cast<u64*>(d_out + kbytes);
    uint32_t* d_n = reinterpret_cast<uint32_t*>(d_out + kbytes + cbytes);
    hk.resize((size_t)D * QD_KEY_WORDS);
    uint32_t got = 0;
    e = qd_launch_unknown_gather(T.t, d_keys, d_counts, d_n, (uint32_t)D, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hk.data(), d_keys, kbytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, cbytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&got, d_n, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return bad(hipGetErrorString(e));
    if ((int64_t)got != D) return bad("the table's entry count and its occupied entries differ");
    return D;
}

// budgets back to 0 and the rescue's tables freed (the caller waited for the context's work)
void free_mismatch(qd_ctx* c, bool scratch) {
    c->d_mm_htab.release();
    c->d_mm_cand.release();
    c->mm_m1 = c->mm_m2 = 0;
    if (scratch) c->mm_list.release();
}

// the rescue post-pass of a batch on `st` (launch(), budgets set): the stream's list holds n + 4 entries at least
int launch_mismatch(qd_ctx* c, int64_t n, const qd_rows* rows, uint16_t* codes, hipStream_t st) {
    StreamScratch::Buf* sc = c->mm_list.need(c, st, (size_t)n, [](size_t pairs) { return (pairs + 4) * 4; });
    if (!sc) return QD_ERR_HIP;
    uint32_t* list = sc->buf.as<uint32_t>();
    MismatchParams p = c->mm;
    for (int k = 0; k < c->lay.n_streams; ++k) {
        p.seq[k] = rows->seq[k];
        p.qual[k] = rows->qual[k];
    }
    p.codes = codes;
    p.adjust = c->d_acc;
    p.bk32 = c->d_bk32;
    p.htab = c->d_mm_htab;
    p.cand = c->d_mm_cand;
    p.miss = list;
    p.n = n;
    hipError_t e = qd_launch_mismatch(p, list, c->cu, st);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("mismatch launch: ") + hipGetErrorString(e));
    return QD_OK;
}

// ---- the read stages (StageId): their tables' lifecycle, the harness of their qd_*_device launches and of their qd_dev_* entries ----

// T on: n_values 64-bit counters on the device, zero
int table_alloc(qd_ctx* c, StageTable& T, size_t n_values) {
    hipError_t e = T.d.alloc(n_values * 8);
    if (e != hipSuccess) {
        return fail(c, QD_ERR_HIP, std::string(T.what) + ": " + hipGetErrorString(e));
    }
    T.n_values = n_values;
    HIPCHK(c, hipMemsetAsync(T.d, 0, n_values * 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return QD_OK;
}

// (the caller waited for the context's work)
void table_free(StageTable& T) {
    T.d.release();
    T.n_values = 0;
}

// qd_*_read
int table_read(qd_ctx* c, const StageTable& T, uint64_t* out, int64_t n_values) {
    if (!out) return QD_ERR_INVALID;
    if (!T.d) return fail(c, QD_ERR_STATE, T.off_text);
    if (n_values != (int64_t)T.n_values) return fail(c, QD_ERR_INVALID, T.size_text);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));
    HIPCHK(c, hipMemcpy(out, T.d, T.n_values * 8, hipMemcpyDeviceToHost));
    return QD_OK;
}

// qd_*_add: another context's table joins this one
int table_add(qd_ctx* c, const StageTable& T, const uint64_t* values, int64_t n_values) {
    if (!values) return QD_ERR_INVALID;
    if (!T.d) return fail(c, QD_ERR_STATE, T.off_text);
    if (n_values != (int64_t)T.n_values) return fail(c, QD_ERR_INVALID, T.size_text);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // the kernels add to the table: nothing of this context may be in flight
    std::vector<u64> h(T.n_values);
    HIPCHK(c, hipMemcpy(h.data(), T.d, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) h[i] += values[i];
    HIPCHK(c, hipMemcpy(T.d, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    return QD_OK;
}

// a stage off: its table freed, its parameters at their off values, and what screen and dup hold besides (the caller waited for
// the context's work)
void stage_off(qd_ctx* c, int id) {
    table_free(c->stage[id]);
    switch (id) {
        case ST_ADAPTERS: std::memset(c->adapters, 0, sizeof c->adapters); c->adapters_dev = {}; break;
        case ST_CLIP: c->clip = {}; c->clip_dev = {}; break;
        case ST_TRIM: c->trim = {}; c->trim_dev = {}; break;
        case ST_PAIRTRIM: c->pairtrim = {}; c->pairtrim_dev = {}; break;
        case ST_PAIRCORRECT: c->paircorrect = {}; c->paircorrect_dev = {}; break;
        case ST_POSTTRIM: c->posttrim = {}; c->posttrim_dev = {}; break;
        case ST_FILTER: c->filter = FILTER_OFF; c->filter_dev = filter_dev_of(FILTER_OFF); break;
        case ST_SCREEN:
            c->screen = {}; c->screen_dev = {};
            c->d_screen_slots.release();
            c->screen_kmers = 0;
            break;
        case ST_DUP:
            c->dup = {}; c->dup_dev = {};
            tally_close(c->dup_keys);
            break;
        default: break;  // qstats, cstats: a table and nothing else
    }
}

// whether any stage is on, or any of those whose tables have a row per destination
bool stages_on(const qd_ctx* c, bool per_destination_only) {
    for (const StageTable& T : c->stage)
        if (T.d && (T.per_destination || !per_destination_only)) return true;
    return false;
}

// every stage off, or those only whose tables have a row per destination (the caller waited for the context's work)
void stages_off(qd_ctx* c, bool per_destination_only) {
    for (int id = 0; id < ST_COUNT; ++id)
        if (c->stage[id].per_destination || !per_destination_only) stage_off(c, id);
}

// What every qd_*_enable and qd_*_set does behind its own checks: the stage goes off, and when it is to be on its table of n_values
// is allocated.  The caller stores the parameters behind QD_OK with `on`.
int stage_install(qd_ctx* c, int id, bool on, size_t n_values) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // nothing of this context may still read the old parameters or add to the old table
    stage_off(c, id);
    return on ? table_alloc(c, c->stage[id], n_values) : QD_OK;
}

// What every qd_*_device does around its launch: launch(table, stream) fills the stage's qd_*_args and launches.  A stage that is off
// is an error with its off text (off_is_error) or has nothing to do.
template <typename LAUNCH>
int stage_launch(qd_ctx* c, int id, bool off_is_error, uint32_t n, void* stream, LAUNCH launch) {
    if (!c) return QD_ERR_INVALID;
    const StageTable& T = c->stage[id];
    if (!T.d) return off_is_error ? fail(c, QD_ERR_STATE, T.off_text) : QD_OK;
    if (!n) return QD_OK;
    hipStream_t st = resolve_stream(c, stream);
    hipError_t e = launch(T.d, st);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string(T.launch) + " launch: " + hipGetErrorString(e));
    HIPCHK(c, track(c, st));
    return QD_OK;
}

// the four pointers every qd_*_args begins with
template <typename ARGS>
void fill_pair_args(ARGS& a, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2) {
    a.text[0] = text1;
    a.text[1] = text2;
    a.recs[0] = recs1;
    a.recs[1] = recs2;
}

// What every qd_dev_* does around its stage: a batch in host memory is checked, copied to scratch on the device, and after the
// stage what it wrote comes back; the scratch is freed with the object.
//     PairUpload up(c);
//     rc = up.open(...);  if (rc != QD_OK || up.empty()) return rc;
//     return up.close(qd_<stage>_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), ..., QD_STREAM_CONTEXT));
class PairUpload {
public:
    // what the stage needs besides the texts and record tables.  SCRATCH_RECS: the out tables on the device only (nothing comes
    // back); INSERTS: a uint64 per pair on the device; TEXT_BACK: close() copies the two texts to texts_back()'s buffers
    enum { CODES = 1, OUT_RECS = 2, REASONS = 4, HITS = 8, SCRATCH_RECS = 16, INSERTS = 32, TEXT_BACK = 64 };

    explicit PairUpload(qd_ctx* ctx) : c(ctx) {}

    // Every size, range and code is checked here, before anything is allocated: a bad table cannot become a bad address.  want:
    // which of codes, out_recs1 / out_recs2 and reasons must be given; drop is uploaded when it is.
    int open(const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2, const uint32_t* recs2,
             int64_t n_pairs, int want, const uint16_t* codes, const uint8_t* drop, uint32_t* out_recs1, uint32_t* out_recs2, uint8_t* reasons,
             uint32_t* hits = nullptr) {
        const int64_t len[2] = {len1, len2};
        const uint8_t* text[2] = {text1, text2};
        const uint32_t* recs[2] = {recs1, recs2};
        if (n_pairs < 0 || n_pairs > 0x7FFFFFFF || len1 < 0 || len2 < 0 || len1 > ((int64_t)1 << 30) || len2 > ((int64_t)1 << 30))
            return fail(c, QD_ERR_INVALID, "bad sizes");
        if (n_pairs == 0) return QD_OK;
        if (!recs1 || !recs2 || ((want & CODES) && !codes) || ((want & OUT_RECS) && (!out_recs1 || !out_recs2)) || ((want & REASONS) && !reasons) ||
            ((want & HITS) && !hits) ||
            (!text1 && len1) || (!text2 && len2))
            return fail(c, QD_ERR_INVALID, "null argument");
        static_assert(sizeof(qd_rec) == 6 * sizeof(uint32_t), "qd_dev_fastq_scan's record layout");
        for (int r = 0; r < 2; ++r)
            for (int64_t j = 0; j < n_pairs; ++j) {
                const qd_rec* q = reinterpret_cast<const qd_rec*>(recs[r]) + j;
                if ((int64_t)q->seq + q->seq_len > len[r] || (int64_t)q->qual + q->seq_len > len[r])
                    return fail(c, QD_ERR_INVALID, "a record's sequence or quality line reaches beyond its text");
            }
        for (int64_t j = 0; (want & CODES) && j < n_pairs; ++j)
            if (codes[j] != QD_CODE_UNDETERMINED && (int)codes[j] >= 2 * c->S) return fail(c, QD_ERR_INVALID, "a routing code is not below 2*S");
        HIPCHK(c, hipSetDevice(c->device));
        const size_t rec_bytes = (size_t)n_pairs * sizeof(qd_rec);
        // the texts start 3 bytes into their buffers: the kernels' aligned words must not depend on an aligned window (and reach up to
        // 15 bytes beyond a line: 32 bytes of slack)
        for (int r = 0; r < 2; ++r) {
            HIPCHK(c, d_text[r].alloc((size_t)len[r] + 32));
            HIPCHK(c, d_recs[r].alloc(rec_bytes));
            if (want & (OUT_RECS | SCRATCH_RECS)) HIPCHK(c, d_out[r].alloc(rec_bytes));
            if (len[r]) HIPCHK(c, hipMemcpyAsync(d_text[r].p + 3, text[r], (size_t)len[r], hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_recs[r].p, recs[r], rec_bytes, hipMemcpyHostToDevice, c->stream));
        }
        if (want & CODES) {
            HIPCHK(c, d_codes.alloc((size_t)n_pairs * 2));
            HIPCHK(c, hipMemcpyAsync(d_codes.p, codes, (size_t)n_pairs * 2, hipMemcpyHostToDevice, c->stream));
        }
        if (drop) {
            HIPCHK(c, d_drop.alloc((size_t)n_pairs));
            HIPCHK(c, hipMemcpyAsync(d_drop.p, drop, (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
        }
        if (want & REASONS) HIPCHK(c, d_reason.alloc((size_t)n_pairs));
        if (want & HITS) HIPCHK(c, d_hits.alloc((size_t)n_pairs * 8));
        if (want & INSERTS) HIPCHK(c, d_inserts.alloc((size_t)n_pairs * 8));
        if (want & TEXT_BACK) {
            text_len[0] = (size_t)len1;
            text_len[1] = (size_t)len2;
        }
        pairs = n_pairs;
        h_out[0] = out_recs1;
        h_out[1] = out_recs2;
        h_reason = reasons;
        h_hits = hits;
        return QD_OK;
    }
    bool empty() const { return pairs == 0; }  // open() found no pairs: nothing was uploaded, there is nothing to launch

    uint32_t n() const { return (uint32_t)pairs; }
    const uint8_t* text(int r) const { return d_text[r].p + 3; }
    const qd_rec* recs(int r) const { return d_recs[r].as<const qd_rec>(); }
    const uint16_t* codes() const { return d_codes.as<const uint16_t>(); }
    const uint8_t* drop() const { return d_drop.as<const uint8_t>(); }  // nullptr when none was given
    qd_rec* out(int r) const { return d_out[r].as<qd_rec>(); }
    uint8_t* reason() const { return d_reason.as<uint8_t>(); }
    uint32_t* hits() const { return d_hits.as<uint32_t>(); }  // uint32[n][2]
    uint64_t* inserts() const { return d_inserts.as<uint64_t>(); }
    uint8_t* mutable_text(int r) const { return d_text[r].p + 3; }  // for the stage that writes into the text
    void texts_back(uint8_t* out1, uint8_t* out2) {
        h_text[0] = out1;
        h_text[1] = out2;
    }

    // behind the stage, which returned rc: what it wrote goes to the host when it succeeded, and the stream is waited for
    int close(int rc) {
        if (rc == QD_OK) {
            for (int r = 0; r < 2; ++r)
                if (d_out[r].p && h_out[r]) HIPCHK(c, hipMemcpyAsync(h_out[r], d_out[r].p, (size_t)pairs * sizeof(qd_rec), hipMemcpyDeviceToHost, c->stream));
            for (int r = 0; r < 2; ++r)
                if (h_text[r] && text_len[r]) HIPCHK(c, hipMemcpyAsync(h_text[r], mutable_text(r), text_len[r], hipMemcpyDeviceToHost, c->stream));
            if (d_reason.p) HIPCHK(c, hipMemcpyAsync(h_reason, d_reason.p, (size_t)pairs, hipMemcpyDeviceToHost, c->stream));
            if (d_hits.p) HIPCHK(c, hipMemcpyAsync(h_hits, d_hits.p, (size_t)pairs * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the scratch is freed on return
        return rc;
    }

private:
    qd_ctx* c;
    int64_t pairs = 0;
    TrimArr<uint8_t> d_text[2], d_recs[2], d_codes, d_drop, d_out[2], d_reason, d_hits, d_inserts;
    uint32_t* h_out[2] = {nullptr, nullptr};
    uint8_t* h_text[2] = {nullptr, nullptr};
    size_t text_len[2] = {0, 0};
    uint8_t* h_reason = nullptr;
    uint32_t* h_hits = nullptr;
};

// qd_dev_clip, qd_dev_trim, qd_dev_pairtrim, qd_dev_posttrim: the stages that write new record tables, whose qd_*_device have one
// signature
typedef int (*rewrite_device_fn)(qd_ctx*, const uint8_t*, const qd_rec*, const uint8_t*, const qd_rec*, uint32_t, qd_rec*, qd_rec*, void*);
int dev_rewrite(qd_ctx* c, int id, rewrite_device_fn device, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2,
                int64_t len2, const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[id].d) return fail(c, QD_ERR_STATE, c->stage[id].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::OUT_RECS, nullptr, nullptr, out_recs1, out_recs2,
                           nullptr);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.out(0), up.out(1), QD_STREAM_CONTEXT));
}

// the tally off and its memory freed (the caller waited for the context's work)
void free_unknown(qd_ctx* c) {
    tally_close(c->uk);
}

// the tally post-pass of a batch on `st` (launch(), tally enabled), behind the rescue when one ran (`rescued`: its list is reused)
int launch_unknown(qd_ctx* c, int64_t n, const qd_rows* rows, const uint16_t* codes, hipStream_t st, bool rescued) {
    StreamScratch::Buf* sc = c->uk.scratch.need(c, st, (size_t)n, [](size_t pairs) { return (2 * pairs + 4) * 4; });
    if (!sc) return QD_ERR_HIP;
    uint32_t* const buf = sc->buf.as<uint32_t>();
    uint32_t* list = buf;
    if (rescued) {
        if (const StreamScratch::Buf* m = c->mm_list.find(st)) list = m->buf.as<uint32_t>();
    } else {
        hipError_t e = qd_launch_compact(codes, n, list, st);
        if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("unknown tally list: ") + hipGetErrorString(e));
    }
    UnknownParams p{};
    const qd_layout& L = c->lay;
    const qd_plan& P = c->plan;
    const int is[2] = {P.idx1_start, P.idx2_start}, ie[2] = {P.idx1_end, P.idx2_end};
    p.n_streams = L.n_streams;
    p.K = L.key_width;
    for (int k = 0; k < L.n_streams; ++k) {
        p.seq[k] = rows->seq[k];
        p.seq_stride[k] = L.seq_stride[k];
        p.idx_w[k] = ie[k] - is[k];
        p.idx_off[k] = p.idx_w[k] ? is[k] - L.seq_off[k] : 0;
    }
    p.codes = codes;
    p.miss = list;
    p.where = buf + 4 + sc->units;
    p.t = tally_view(c->uk);
    p.n = n;
    hipError_t e = qd_launch_unknown(p, c->cu, tally_before(c->uk, st), st);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("unknown tally launch: ") + hipGetErrorString(e));
    return tally_after(c, c->uk, st);
}

// Host: the part lists of a sheet, the one definition (include/quade_hip.h qd_hop_index).  part1 / part2: per sample the
// ordinal of its index-1 / index-2 value among the distinct values in order of first appearance, -1 for a barcode whose length is
// not K; key1 / key2 (may be NULL): per distinct value its canonical key words.
void hop_parts(int32_t S, const uint8_t* bc, const int32_t* off, int32_t K, int32_t w1, int32_t* part1, int32_t* part2, int32_t& n1,
               int32_t& n2, std::vector<u64>* key1, std::vector<u64>* key2) {
    std::map<std::string, int32_t> seen[2];
    int32_t* part[2] = {part1, part2};
    std::vector<u64>* key[2] = {key1, key2};
    const int from[2] = {0, w1}, width[2] = {w1, K - w1};
    for (int32_t i = 0; i < S; ++i) {
        const uint8_t* b = bc + off[i];
        const bool on = off[i + 1] - off[i] == K;
        for (int h = 0; h < 2; ++h) {
            if (!on) {
                part[h][i] = -1;
                continue;
            }
            const std::string v((const char*)b + from[h], (size_t)width[h]);
            auto it = seen[h].find(v);
            if (it == seen[h].end()) {
                it = seen[h].emplace(v, (int32_t)seen[h].size()).first;
                if (key[h]) {
                    u64 w[QD_KEY_WORDS];
                    canon(b + from[h], width[h], w);
                    key[h]->insert(key[h]->end(), w, w + QD_KEY_WORDS);
                }
            }
            part[h][i] = it->second;
        }
    }
    n1 = (int32_t)seen[0].size();
    n2 = (int32_t)seen[1].size();
}

size_t hop_values(const qd_ctx* c) { return (size_t)(c->hop_n1 + 1) * (size_t)(c->hop_n2 + 1) + 1; }

// the matrix off and its memory freed (the caller waited for the context's work)
void free_hop(qd_ctx* c) {
    table_free(c->hop);
    c->d_hop_parts.release();
    c->hop_n1 = c->hop_n2 = 0;
    c->hop_list.release();
}

// the matrix post-pass of a batch on `st` (launch(), matrix enabled), behind the rescue and the tally: the rescue's list when one ran
// (`rescued`), else the tally's (`tallied`: launch_unknown has listed the batch on this stream), else a compaction of its own
int launch_hop(qd_ctx* c, int64_t n, const qd_rows* rows, const uint16_t* codes, hipStream_t st, bool rescued, bool tallied) {
    const StreamScratch::Buf* have = rescued ? c->mm_list.find(st) : (tallied ? c->uk.scratch.find(st) : nullptr);
    const uint32_t* list = have ? have->buf.as<const uint32_t>() : nullptr;
    if (!list) {
        StreamScratch::Buf* sc = c->hop_list.need(c, st, (size_t)n, [](size_t pairs) { return (pairs + 4) * 4; });
        if (!sc) return QD_ERR_HIP;
        uint32_t* own = sc->buf.as<uint32_t>();
        hipError_t e = qd_launch_compact(codes, n, own, st);
        if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("index-hopping list: ") + hipGetErrorString(e));
        list = own;
    }
    HopParams p{};
    const qd_layout& L = c->lay;
    const qd_plan& P = c->plan;
    const int is[2] = {P.idx1_start, P.idx2_start}, ie[2] = {P.idx1_end, P.idx2_end};
    for (int k = 0; k < 2; ++k) {  // (a dual plan: two streams, both windows non-empty)
        p.seq[k] = rows->seq[k];
        p.seq_stride[k] = L.seq_stride[k];
        p.idx_w[k] = ie[k] - is[k];
        p.idx_off[k] = is[k] - L.seq_off[k];
        p.part[k] = c->hop_part[k];
    }
    p.codes = codes;
    p.miss = list;
    p.table = c->hop.d;
    p.n = n;
    p.K = L.key_width;
    p.n1 = (uint32_t)c->hop_n1;
    p.n2 = (uint32_t)c->hop_n2;
    hipError_t e = qd_launch_hop(p, c->cu, st);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("index-hopping launch: ") + hipGetErrorString(e));
    return QD_OK;
}

// What a new plan and new barcodes do first: the mismatch budgets are reset, as the counters are, and everything with a row or a key
// per destination goes off -- the unknown tally, the index-hopping matrix and the read stages whose tables say so
int destinations_change(qd_ctx* c) {
    if (!(c->mm_m1 + c->mm_m2 > 0 || c->uk.mem || c->hop.d || stages_on(c, true))) return QD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));
    free_mismatch(c, false);
    free_unknown(c);
    free_hop(c);
    stages_off(c, true);
    return QD_OK;
}

// (re)build the device table from the host barcodes and the current plan
int rebuild(qd_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // nothing of this context may still read the old table
    free_table(c);
    const int S = c->S;
    const int K = c->lay.key_width;
    std::vector<u64> k32((size_t)std::max(S, 1) * QD_KEY_WORDS, 0), k16((size_t)std::max(S, 1) * 2, 0);
    std::vector<uint8_t> blen(std::max(S, 1), 0);
    std::vector<int> ids_fast, ids_gen;
    std::map<std::string, int> seen;
    // Wide plan: 16 < K <= 32 with every slice and window inside 16 bytes (so both index reads carry a part of
    // the key) and at most 8 molecular bytes per read; its fast table is built over nibble-packed keys, which
    // is injective only on the alphabet the reference admits (src/Sample.py:40,141): any K-long barcode with
    // another byte sends the plan to the generic kernel.
    const qd_layout& Lw = c->lay;
    const int w1 = c->plan.idx1_end - c->plan.idx1_start, w2 = c->plan.dual ? c->plan.idx2_end - c->plan.idx2_start : 0;
    bool wide = K > 16 && K <= 32 && Lw.n_streams == 2 && w1 <= 16 && w2 <= 16 && Lw.mol_width <= 16;
    for (int k = 0; wide && k < Lw.n_streams; ++k) {
        const int mw = (k == 0 ? c->plan.mol1_end - c->plan.mol1_start : c->plan.mol2_end - c->plan.mol2_start);
        wide = Lw.seq_stride[k] <= 16 && Lw.qual_stride[k] <= 16 && mw <= 8;
    }
    std::vector<u64> kv((size_t)std::max(S, 1) * 4, 0);
    for (int i = 0; i < S; ++i) {
        const uint8_t* b = c->bc.data() + c->bc_off[i];
        const int len = c->bc_off[i + 1] - c->bc_off[i];
        std::string s((const char*)b, (size_t)len);
        if (seen.count(s)) {
            char m[128];
            snprintf(m, sizeof m, "barcode %d duplicates barcode %d (Index is not unique)", i, seen[s]);
            return fail(c, QD_ERR_BARCODE, m);
        }
        seen[s] = i;
        blen[i] = (uint8_t)std::min(len, 255);
        if (len == 0 || len > QD_MAX_KEY) continue;  // can never equal a slice (empty: see DESIGN.md)
        canon(b, len, &k32[(size_t)i * QD_KEY_WORDS]);
        ids_gen.push_back(i);
        if (len == K && K <= 16) {
            k16[2 * (size_t)i] = k32[(size_t)i * QD_KEY_WORDS];
            k16[2 * (size_t)i + 1] = k32[(size_t)i * QD_KEY_WORDS + 1];
            ids_fast.push_back(i);
        } else if (len == K && wide) {
            for (int j = 0; j < len; ++j)
                if (!strchr("ACGTN", b[j]) || b[j] == 0) wide = false;
            u64 s1[QD_KEY_WORDS], s2[QD_KEY_WORDS];
            canon(b, w1, s1);           // the barcode's part in index read 1, then in index read 2
            canon(b + w1, len - w1, s2);
            u64* v = &kv[(size_t)i * 4];
            v[0] = s1[0];
            v[1] = s1[1];
            v[2] = s2[0];
            v[3] = s2[1];
            qd_wide_key(v[0], v[1], v[2], v[3], w1, &k16[2 * (size_t)i], &k16[2 * (size_t)i + 1]);
            ids_fast.push_back(i);
        }
    }
    if (K > 16 && !wide) ids_fast.clear();
    c->wide = wide;
    const uint32_t slot_factor = c->opt_slot_factor > 0 ? (uint32_t)c->opt_slot_factor : (uint32_t)QD_SLOT_FACTOR;
    std::vector<uint32_t> sf = wide ? build_slots(ids_fast, k32, blen, c->mask_fast, c->seed_fast, &k16, (uint32_t)K, slot_factor)
                                    : build_slots(ids_fast, k32, blen, c->mask_fast, c->seed_fast, nullptr, 0, slot_factor);
    std::vector<uint32_t> sg = build_slots(ids_gen, k32, blen, c->mask_gen, c->seed_gen);

    HIPCHK(c, c->d_slots_fast.alloc(sf.size() * 4));
    HIPCHK(c, c->d_slots_gen.alloc(sg.size() * 4));
    HIPCHK(c, c->d_bk16.alloc(k16.size() * 8));
    HIPCHK(c, c->d_bk32.alloc(k32.size() * 8));
    HIPCHK(c, c->d_blen.alloc(blen.size()));
    HIPCHK(c, c->d_bkv.alloc(kv.size() * 8));
    HIPCHK(c, hipMemcpy(c->d_bkv, kv.data(), kv.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_slots_fast, sf.data(), sf.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_slots_gen, sg.data(), sg.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_bk16, k16.data(), k16.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_bk32, k32.data(), k32.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_blen, blen.data(), blen.size(), hipMemcpyHostToDevice));

    // LDS image of the fast kernel: slots | keys (16 B each) | histogram (2S+1)
    c->lds_bk_off = (uint32_t)(((size_t)(c->mask_fast + 1) * 4 + 15) & ~(size_t)15);
    c->lds_hist_off = c->lds_bk_off + (uint32_t)S * 16;
    c->lds_bytes = ((size_t)c->lds_hist_off + (size_t)(2 * S + 1) * 4 + 15) & ~(size_t)15;
    c->lds_strip_off = (uint32_t)c->lds_bytes;
    // "UMI in index read 1" shapes (quade_kernels.hip StaticUmi1): 8-base barcodes at the start of both index reads, a molecular
    // index of 9..12 bases right behind the first one, none in the second -- rows of 18 / 20 bytes, static kernels only
    const bool umi1 = [&] {
        const qd_layout& Lu = c->lay;
        const qd_plan& Pu = c->plan;
        const int mw = Pu.mol1_end - Pu.mol1_start;
        return Lu.n_streams == 2 && K == 16 && Pu.idx1_end - Pu.idx1_start == 8 && Pu.idx2_end - Pu.idx2_start == 8 && mw >= 9 && mw <= 12 &&
               Pu.mol2_end == Pu.mol2_start && Lu.mol_width == mw && Pu.mol1_start == Pu.idx1_end && Lu.seq_off[0] == Pu.idx1_start &&
               Lu.seq_off[1] == Pu.idx2_start && Lu.seq_stride[0] == ((8 + mw + 1) & ~1) && Lu.seq_stride[1] == 8 && Lu.qual_stride[0] == 8 &&
               Lu.qual_stride[1] == 8;
    }();
    // "UMI in both index reads" (StaticUmi2, r05): the same in both reads -- rows of 18 / 20 bytes in both streams, 18 .. 24 bytes of
    // molecular index per pair
    const bool umi2 = [&] {
        const qd_layout& Lu = c->lay;
        const qd_plan& Pu = c->plan;
        const int mw = Pu.mol1_end - Pu.mol1_start;
        return Lu.n_streams == 2 && K == 16 && Pu.idx1_end - Pu.idx1_start == 8 && Pu.idx2_end - Pu.idx2_start == 8 && mw >= 9 && mw <= 12 &&
               Pu.mol2_end - Pu.mol2_start == mw && Lu.mol_width == 2 * mw && Pu.mol1_start == Pu.idx1_end && Pu.mol2_start == Pu.idx2_end &&
               Lu.seq_off[0] == Pu.idx1_start && Lu.seq_off[1] == Pu.idx2_start && Lu.seq_stride[0] == ((8 + mw + 1) & ~1) &&
               Lu.seq_stride[1] == ((8 + mw + 1) & ~1) && Lu.qual_stride[0] == 8 && Lu.qual_stride[1] == 8;
    }();
    c->lds_strip_bytes = (c->lay.mol_width > 0 && (c->lay.mol_width % 4 == 0 || umi1 || umi2) && c->opt_mol_strips) ? (size_t)128 * c->lay.mol_width : 0;
    if (c->lds_bytes + 16 * c->lds_strip_bytes > 150 * 1024) c->lds_strip_bytes = 0;  // 16 waves per workgroup at most

    const qd_layout& L = c->lay;
    bool ok = (K >= 1 && K <= 16 && L.mol_width <= 16 && c->lds_bytes <= 150 * 1024);
    for (int k = 0; k < L.n_streams; ++k) {
        // rows of two reads in at most two 16-byte loads; slices of at most 8 bytes
        ok = ok && L.seq_stride[k] <= 16 && L.qual_stride[k] <= 8;
        const int mw = (k == 0 ? c->plan.mol1_end - c->plan.mol1_start : c->plan.mol2_end - c->plan.mol2_start);
        ok = ok && mw <= 8 && L.qual_width[k] <= 8;
    }
    c->fast_ok = ok || ((c->wide || umi1 || umi2) && c->lds_bytes <= 150 * 1024);

    c->cnt_stride = (uint32_t)((2 * S + 1 + 3) & ~3);
    // one counter row per workgroup (modulo), capped at 64 MiB of rows for very large tables
    c->partial_rows = (uint32_t)std::max<size_t>(8, std::min<size_t>((size_t)c->cu * 8, ((size_t)64 << 20) / ((size_t)c->cnt_stride * sizeof(qd_row_t))));
    HIPCHK(c, c->d_partial.alloc((size_t)c->partial_rows * c->cnt_stride * sizeof(qd_row_t)));
    HIPCHK(c, c->d_acc.alloc((size_t)c->cnt_stride * 8));
    HIPCHK(c, c->d_counts.alloc(((size_t)c->cnt_stride + 4) * 8));
    HIPCHK(c, c->d_total.alloc(((size_t)c->cnt_stride + 4) * 8));
    HIPCHK(c, hipMemset(c->d_partial, 0, (size_t)c->partial_rows * c->cnt_stride * sizeof(qd_row_t)));
    HIPCHK(c, hipMemset(c->d_acc, 0, (size_t)c->cnt_stride * 8));
    c->total_pairs = 0;
    c->pairs_in_rows = 0;
    c->have_table = true;
    return QD_OK;
}

void fill_params(const qd_ctx* c, DemuxParams& p, bool fast) {
    memset(&p, 0, sizeof p);
    const qd_layout& L = c->lay;
    const qd_plan& P = c->plan;
    p.partial = c->d_partial;
    p.adjust = c->d_acc;
    p.slots = fast ? c->d_slots_fast : c->d_slots_gen;
    p.slot_mask = fast ? c->mask_fast : c->mask_gen;
    p.seed = fast ? c->seed_fast : c->seed_gen;
    p.gslots = c->d_slots_gen;
    p.gmask = c->mask_gen;
    p.gseed = c->seed_gen;
    p.bk16 = c->d_bk16;
    p.bk32 = c->d_bk32;
    p.bkv = c->d_bkv;
    p.wide = (fast && c->wide) ? 1 : 0;
    p.blen = c->d_blen;
    p.n_samples = (uint32_t)c->S;
    p.cnt_stride = c->cnt_stride;
    p.partial_rows = c->partial_rows;
    p.lds_bk_off = c->lds_bk_off;
    p.lds_hist_off = c->lds_hist_off;
    p.mol_strip_off = (fast && c->lds_strip_bytes) ? c->lds_strip_off : 0;
    p.thr = (uint32_t)(P.min_qual + 33);
    p.n_streams = L.n_streams;
    p.K = L.key_width;
    p.M = L.mol_width;
    const int is[2] = {P.idx1_start, P.idx2_start}, ie[2] = {P.idx1_end, P.idx2_end};
    const int ms[2] = {P.mol1_start, P.mol2_start}, me[2] = {P.mol1_end, P.mol2_end};
    for (int k = 0; k < 2; ++k) {
        p.seq_stride[k] = L.seq_stride[k];
        p.qual_stride[k] = L.qual_stride[k];
        const bool used = k < L.n_streams;
        p.idx_w[k] = used ? ie[k] - is[k] : 0;
        p.mol_w[k] = used ? me[k] - ms[k] : 0;
        p.idx_col[k] = is[k];
        p.mol_col[k] = ms[k];
        p.idx_off[k] = p.idx_w[k] ? is[k] - L.seq_off[k] : 0;
        p.mol_off[k] = p.mol_w[k] ? ms[k] - L.seq_off[k] : 0;
        p.idx_mask[k] = p.idx_w[k] >= 8 ? ~0ull : ((1ull << (8 * p.idx_w[k])) - 1);
        p.idx_mask_hi[k] = p.idx_w[k] >= 16 ? ~0ull : (p.idx_w[k] > 8 ? ((1ull << (8 * (p.idx_w[k] - 8))) - 1) : 0);
        p.mol_mask[k] = p.mol_w[k] >= 8 ? ~0ull : ((1ull << (8 * p.mol_w[k])) - 1);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// which kernel takes a batch: dense = per-read lengths apply to (potentially) every pair
int pick_kernel(const qd_ctx* c, bool dense_len) {
    if (!c->fast_ok || dense_len || c->opt_force_generic || c->opt_kernel == K_GENERIC) return K_GENERIC;
    return K_FAST;
}

// n_short < 0: no exception list (len rows, if any, apply to every pair -> generic kernel)
// short_len: the listed reads' lengths, compact ([k][i] for short_idx[i]); NULL: rows->len holds them per pair
// The kernels count into 32-bit rows.  A row counter never exceeds the number of pairs launched since the rows
// were last emptied, so before that number could pass 2^32 - 1 the rows are added to the 64-bit totals and
// zeroed: once per ~4.3 G pairs, behind everything the context has in flight (a host wait, ~tens of us).
int fold_rows(qd_ctx* c) {
    HIPCHK(c, wait_all(c));
    const uint32_t ncnt = (uint32_t)(2 * c->S + 1);
    hipError_t e = qd_launch_reduce(c->d_partial, c->partial_rows, c->cnt_stride, ncnt, c->d_acc, c->d_acc, c->stream);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("fold launch: ") + hipGetErrorString(e));
    HIPCHK(c, hipMemsetAsync(c->d_partial, 0, (size_t)c->partial_rows * c->cnt_stride * sizeof(qd_row_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pairs_in_rows = 0;
    ++c->folds;
    return QD_OK;
}

int launch(qd_ctx* c, int64_t n, const qd_rows* rows, uint16_t* codes, uint8_t* mol, hipStream_t st,
           int64_t n_short = -1, const uint32_t* short_idx = nullptr, const uint8_t* const* short_len = nullptr) {
    const qd_layout& L = c->lay;
    bool has_len = false;
    for (int k = 0; k < L.n_streams; ++k) {
        if (!rows->seq[k] || !rows->qual[k]) return fail(c, QD_ERR_INVALID, "NULL row pointer");
        if (!aligned16(rows->seq[k]) || !aligned16(rows->qual[k]))
            return fail(c, QD_ERR_INVALID, "row buffers must be 16-byte aligned");
        has_len = has_len || rows->len[k] != nullptr;
    }
    if (short_len) has_len = true;
    if (!codes || !aligned16(codes)) return fail(c, QD_ERR_INVALID, "codes buffer NULL or not 16-byte aligned");
    if (L.mol_width > 0 && (!mol || !aligned16(mol)))
        return fail(c, QD_ERR_INVALID, "mol buffer NULL or not 16-byte aligned");
    if (n > (int64_t)0xFFFFFFFF) return fail(c, QD_ERR_INVALID, "more than 2^32-1 pairs in one batch");
    if (c->pairs_in_rows + (uint64_t)n > c->fold_limit) {
        const int r = fold_rows(c);
        if (r != QD_OK) return r;
    }
    // a listed minority of short reads: fast kernel for everybody, the listed pairs redone afterwards
    const bool sparse = has_len && n_short >= 0 && n_short <= n / 2;
    const int kind = pick_kernel(c, has_len && !sparse);
    DemuxParams p;
    fill_params(c, p, kind != K_GENERIC);
    for (int k = 0; k < L.n_streams; ++k) {
        p.seq[k] = rows->seq[k];
        p.qual[k] = rows->qual[k];
        p.len[k] = rows->len[k];
    }
    p.codes = codes;
    p.mol = mol;
    p.n = n;
    hipError_t e;
    bool fast_done = false;
    if (kind == K_FAST) {
        e = qd_launch_fast(p, c->kcache, c->cu, c->opt_wg_per_cu, c->opt_block, c->lds_bytes, c->lds_strip_bytes, st);
        fast_done = e == hipSuccess;
        if (e == hipErrorInvalidValue) {  // no instantiation for this layout in this build (tuning builds leave static shapes out): the generic kernel takes it
            (void)hipGetLastError();
            fill_params(c, p, false);
            for (int k = 0; k < L.n_streams; ++k) {
                p.seq[k] = rows->seq[k];
                p.qual[k] = rows->qual[k];
                p.len[k] = rows->len[k];
            }
            p.codes = codes;
            p.mol = mol;
            p.n = n;
        }
    }
    if (!fast_done && (kind != K_FAST || e == hipErrorInvalidValue)) {
        const int64_t nb = (n + QD_GEN_BLOCK - 1) / QD_GEN_BLOCK;
        const int grid = (int)std::min<int64_t>(nb, (int64_t)c->cu * 8);
        e = qd_launch_generic(p, grid, st);
    }
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    if (fast_done && sparse && n_short > 0) {
        p.exc = short_idx;
        p.n_exc = (uint32_t)n_short;
        for (int k = 0; k < L.n_streams; ++k) p.exc_len[k] = short_len ? short_len[k] : nullptr;
        e = qd_launch_fixup(p, st);
        if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("fixup launch: ") + hipGetErrorString(e));
    }
    if (c->mm_m1 + c->mm_m2 > 0) {  // opt-in rescue of the undetermined pairs, behind whatever took the batch
        const int r = launch_mismatch(c, n, rows, codes, st);
        if (r != QD_OK) return r;
    }
    if (c->uk.mem) {  // opt-in tally of the pairs that stay undetermined, behind the rescue
        const int r = launch_unknown(c, n, rows, codes, st, c->mm_m1 + c->mm_m2 > 0);
        if (r != QD_OK) return r;
    }
    if (c->hop.d) {  // opt-in index-hopping matrix over the same pairs, behind both
        const int r = launch_hop(c, n, rows, codes, st, c->mm_m1 + c->mm_m2 > 0, c->uk.mem != nullptr);
        if (r != QD_OK) return r;
    }
    c->total_pairs += (uint64_t)n;
    c->pairs_in_rows += (uint64_t)n;
    e = track(c, st);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
    return QD_OK;
}

}  // namespace

extern "C" {

int qd_version(void) { return QD_ABI_VERSION; }

const char* qd_strerror(int code) {
    switch (code) {
        case QD_OK: return "ok";
        case QD_ERR_INVALID: return "invalid argument";
        case QD_ERR_NO_DEVICE: return "no usable gfx950 HIP device";
        case QD_ERR_HIP: return "HIP runtime error";
        case QD_ERR_STATE: return "plan and barcodes must be set first";
        case QD_ERR_UNSUPPORTED: return "plan outside the supported envelope";
        case QD_ERR_BARCODE: return "barcode table rejected";
        case QD_ERR_FORMAT: return "malformed fastq text";
    }
    return "unknown error";
}

const char* qd_last_error(const qd_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int qd_device_count(int32_t* n_devices) {
    if (!n_devices) return fail(nullptr, QD_ERR_INVALID, "n_devices is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *n_devices = 0;
        return fail(nullptr, QD_ERR_NO_DEVICE, std::string("no HIP device visible (") + hipGetErrorString(e) + ")");
    }
    *n_devices = n;
    return QD_OK;
}

int qd_create(int device_id, qd_ctx** out) {
    if (!out) return fail(nullptr, QD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, QD_ERR_NO_DEVICE,
                    std::string("no HIP device visible (") + hipGetErrorString(e) + "); this library has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, QD_ERR_INVALID, "device_id out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
        return fail(nullptr, QD_ERR_HIP, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, QD_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    if ((e = hipSetDevice(device_id)) != hipSuccess)
        return fail(nullptr, QD_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    qd_ctx* c = new qd_ctx();
    c->device = device_id;
    c->cu = prop.multiProcessorCount;
    c->total_mem = (int64_t)prop.totalGlobalMem;
    snprintf(c->dev_name, sizeof c->dev_name, "%s (%s)", prop.name, prop.gcnArchName);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return fail(nullptr, QD_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = c;
    return QD_OK;
}

int qd_destroy(qd_ctx* c) {
    if (!c) return QD_OK;
    (void)hipSetDevice(c->device);
    (void)wait_all(c);
    qd_slots_destroy(c);
    tally_close(c->uk);  // (their events; every table and scratch buffer goes back with `delete c`, the device being current)
    tally_close(c->dup_keys);
    for (auto& t : c->tracked) (void)hipEventDestroy(t.second);
    c->tracked.clear();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return QD_OK;
}

int qd_device_info(const qd_ctx* c, char* name, int32_t cap, int32_t* cus, int64_t* mem) {
    if (!c) return QD_ERR_INVALID;
    if (name && cap > 0) snprintf(name, (size_t)cap, "%s", c->dev_name);
    if (cus) *cus = c->cu;
    if (mem) *mem = c->total_mem;
    return QD_OK;
}

int qd_set_plan(qd_ctx* c, const qd_plan* plan) {
    if (!c || !plan) return QD_ERR_INVALID;
    qd_layout L;
    const int r = qd_plan_layout(plan, &L);
    if (r != QD_OK) return fail(c, r, "plan rejected: positions must satisfy 0 <= start <= end <= 255, window <= 64, "
                                       "fused barcode <= 32, 0 <= minimal_qual <= 40");
    if (!c->slots.empty()) return fail(c, QD_ERR_STATE, "destroy the slots before changing the plan");
    const int rc = destinations_change(c);
    if (rc != QD_OK) return rc;
    c->plan = *plan;
    c->lay = L;
    c->have_plan = true;
    if (c->S > 0 || c->have_table) return rebuild(c);
    return QD_OK;
}

int qd_get_layout(const qd_ctx* c, qd_layout* out) {
    if (!c || !out) return QD_ERR_INVALID;
    if (!c->have_plan) return fail(c, QD_ERR_STATE, "qd_set_plan first");
    *out = c->lay;
    return QD_OK;
}

int qd_get_plan(const qd_ctx* c, qd_plan* out) {
    if (!c || !out) return QD_ERR_INVALID;
    if (!c->have_plan) return fail(c, QD_ERR_STATE, "no plan set");
    *out = c->plan;
    return QD_OK;
}

int qd_context_device(const qd_ctx* c, int32_t* device_id) {
    if (!c || !device_id) return QD_ERR_INVALID;
    *device_id = c->device;
    return QD_OK;
}

int qd_set_barcodes(qd_ctx* c, int32_t S, const uint8_t* barcodes, const int32_t* offsets) {
    if (!c || S < 0 || S > QD_MAX_SAMPLES || (S > 0 && (!barcodes || !offsets)))
        return fail(c, QD_ERR_INVALID, "bad barcode arguments (0 <= n_samples <= 32767)");
    if (!c->have_plan) return fail(c, QD_ERR_STATE, "qd_set_plan first");
    for (int i = 0; i < S; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(c, QD_ERR_INVALID, "offsets must be non-decreasing");
    const int rc = destinations_change(c);
    if (rc != QD_OK) return rc;
    c->S = S;
    c->bc.assign(barcodes, barcodes + (S ? offsets[S] : 0));
    c->bc_off.assign(offsets, offsets + (S ? S + 1 : 0));
    if (S == 0) c->bc_off.assign(1, 0);
    return rebuild(c);
}

int qd_check_mismatch_collisions(int32_t S, const uint8_t* barcodes, const int32_t* offsets, int32_t K, int32_t w1, int32_t m1,
                                 int32_t m2, int32_t* first, int32_t* second) {
    if (S < 0 || S > QD_MAX_SAMPLES || (S > 0 && (!barcodes || !offsets)) || !first || !second || K < 1 || K > QD_MAX_KEY ||
        w1 < 0 || w1 > K || m1 < 0 || m1 > 2 || m2 < 0 || m2 > 2)
        return QD_ERR_INVALID;
    for (int i = 0; i < S; ++i)
        if (offsets[i + 1] < offsets[i]) return QD_ERR_INVALID;
    *first = *second = -1;
    return qd_mm_first_collision(S, barcodes, offsets, K, w1, m1, m2, first, second) ? QD_ERR_BARCODE : QD_OK;
}

int qd_set_mismatches(qd_ctx* c, int32_t m1, int32_t m2) {
    if (!c) return QD_ERR_INVALID;
    if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    if (m1 < 0 || m1 > 2 || m2 < 0 || m2 > 2) return fail(c, QD_ERR_INVALID, "mismatch budgets must be 0, 1 or 2");
    if (!c->plan.dual && m2 != 0) return fail(c, QD_ERR_INVALID, "index2_mismatches needs a dual-index plan");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // nothing of this context may still read the old tables
    free_mismatch(c, false);
    if (m1 + m2 == 0) return QD_OK;
    const int K = c->lay.key_width, w1 = c->plan.idx1_end - c->plan.idx1_start;
    int32_t a = -1, b = -1;
    if (qd_mm_first_collision(c->S, c->bc.data(), c->bc_off.data(), K, w1, m1, m2, &a, &b)) {
        char m[160];
        snprintf(m, sizeof m, "barcodes %d and %d collide with index1_mismatches=%d index2_mismatches=%d", a, b, m1, m2);
        return fail(c, QD_ERR_BARCODE, m);
    }
    MismatchParams& p = c->mm;
    memset(&p, 0, sizeof p);
    std::vector<QdMmBucket> htab;
    std::vector<uint16_t> cand;
    qd_mm_build(c->S, c->bc.data(), c->bc_off.data(), K, w1, m1, m2, p, htab, cand);
    const qd_layout& L = c->lay;
    const qd_plan& P = c->plan;
    const int is[2] = {P.idx1_start, P.idx2_start}, ie[2] = {P.idx1_end, P.idx2_end};
    p.n_streams = L.n_streams;
    p.K = K;
    for (int k = 0; k < L.n_streams; ++k) {
        p.seq_stride[k] = L.seq_stride[k];
        p.qual_stride[k] = L.qual_stride[k];
        p.idx_w[k] = ie[k] - is[k];
        p.idx_off[k] = p.idx_w[k] ? is[k] - L.seq_off[k] : 0;
    }
    p.thr = (uint32_t)(P.min_qual + 33);
    p.n_samples = (uint32_t)c->S;
    p.hist_entries = 2 * c->S <= 16000 ? (uint32_t)(2 * c->S) : 0;  // <= 64 KB of LDS, else global 64-bit adds per pair
    HIPCHK(c, c->d_mm_htab.alloc(htab.size() * sizeof(QdMmBucket)));
    HIPCHK(c, c->d_mm_cand.alloc(cand.size() * sizeof(uint16_t)));
    HIPCHK(c, hipMemcpy(c->d_mm_htab, htab.data(), htab.size() * sizeof(QdMmBucket), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_mm_cand, cand.data(), cand.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->mm_m1 = m1;
    c->mm_m2 = m2;
    return QD_OK;
}

int qd_unknown_enable(qd_ctx* c, int64_t slots) {
    if (!c) return QD_ERR_INVALID;
    if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    if (slots != 0 && !tally_slots_ok(slots))
        return fail(c, QD_ERR_INVALID, "unknown-barcode slots must be 0 (off) or a power of two in 2^10 .. 2^28");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // nothing of this context may still use the old table
    free_unknown(c);
    if (slots == 0) return QD_OK;
    return tally_open(c, c->uk, slots, "unknown-barcode table");
}

int qd_unknown_stats(qd_ctx* c, uint64_t out[4]) {
    if (!c || !out) return QD_ERR_INVALID;
    if (!c->uk.mem) return fail(c, QD_ERR_STATE, "the unknown-barcode tally is not enabled");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));
    HIPCHK(c, hipMemcpy(out, c->uk.t.totals, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return QD_OK;
}

int64_t qd_unknown_read(qd_ctx* c, uint8_t* keys, uint64_t* counts, int64_t cap) {
    auto bad = [&](int code, const std::string& msg) { return QD_UNKNOWN_READ_ERROR + (int64_t)fail(c, code, msg); };
    if (!c || cap < 0 || (cap > 0 && (!keys || !counts))) return bad(QD_ERR_INVALID, "bad arguments");
    if (!c->uk.mem) return bad(QD_ERR_STATE, "the unknown-barcode tally is not enabled");
    std::vector<u64> hk;
    const int64_t D = tally_gather(c, c->uk, "unknown-barcode", cap, hk, counts);
    const int K = c->lay.key_width;
    for (int64_t i = 0; i < D; ++i)  // (D <= 0: nothing was gathered)
        for (int b = 0; b < K; ++b) keys[i * K + b] = (uint8_t)(hk[(size_t)i * QD_KEY_WORDS + (b >> 3)] >> (8 * (b & 7)));
    return D;
}

int qd_hop_index(int32_t S, const uint8_t* barcodes, const int32_t* offsets, int32_t K, int32_t w1, int32_t* part1, int32_t* part2,
                 int32_t* n1, int32_t* n2) {
    if (S < 0 || S > QD_MAX_SAMPLES || (S > 0 && (!barcodes || !offsets || !part1 || !part2)) || !n1 || !n2 || K < 2 || K > QD_MAX_KEY ||
        w1 < 1 || w1 >= K)
        return QD_ERR_INVALID;
    for (int i = 0; i < S; ++i)
        if (offsets[i + 1] < offsets[i]) return QD_ERR_INVALID;
    hop_parts(S, barcodes, offsets, K, w1, part1, part2, *n1, *n2, nullptr, nullptr);
    return (int64_t)(*n1 + 1) * (int64_t)(*n2 + 1) > QD_HOP_MAX_CELLS ? QD_ERR_UNSUPPORTED : QD_OK;
}

int qd_hop_enable(qd_ctx* c, int32_t on) {
    if (!c) return QD_ERR_INVALID;
    if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    const int K = c->lay.key_width, w1 = c->plan.idx1_end - c->plan.idx1_start;
    if (on && (!c->plan.dual || w1 < 1 || w1 >= K))
        return fail(c, QD_ERR_INVALID, "the index-hopping matrix needs a dual-index plan with both index windows non-empty");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // nothing of this context may still add to the old table
    free_hop(c);
    if (!on) return QD_OK;
    std::vector<int32_t> part1((size_t)std::max(c->S, 1)), part2((size_t)std::max(c->S, 1));
    std::vector<u64> key[2];
    int32_t n[2] = {0, 0};
    hop_parts(c->S, c->bc.data(), c->bc_off.data(), K, w1, part1.data(), part2.data(), n[0], n[1], &key[0], &key[1]);
    if ((int64_t)(n[0] + 1) * (int64_t)(n[1] + 1) > QD_HOP_MAX_CELLS) {
        char m[160];
        snprintf(m, sizeof m, "index-hopping matrix: %d x %d distinct index values are more than (n1+1)*(n2+1) <= 2^24 admits", n[0], n[1]);
        return fail(c, QD_ERR_UNSUPPORTED, m);
    }
    // one allocation: [slots of part 1][slots of part 2][keys of part 1][keys of part 2] (entries of 16 bytes first: aligned)
    std::vector<HopSlot> slots[2];
    for (int h = 0; h < 2; ++h) {
        qd_hop_build(key[h], n[h], slots[h], c->hop_part[h].mask, c->hop_part[h].lg);
        if (key[h].empty()) key[h].assign(QD_KEY_WORDS, 0);  // never read (no entry names it), keeps the device array non-empty
    }
    const size_t sb[2] = {slots[0].size() * sizeof(HopSlot), slots[1].size() * sizeof(HopSlot)};
    const size_t kb[2] = {key[0].size() * 8, key[1].size() * 8};
    hipError_t e = c->d_hop_parts.alloc(sb[0] + sb[1] + kb[0] + kb[1]);
    if (e != hipSuccess) {
        return fail(c, QD_ERR_HIP, std::string("index-hopping part tables: ") + hipGetErrorString(e));
    }
    uint8_t* base = c->d_hop_parts;
    const size_t so[2] = {0, sb[0]}, ko[2] = {sb[0] + sb[1], sb[0] + sb[1] + kb[0]};
    for (int h = 0; h < 2 && e == hipSuccess; ++h) {
        c->hop_part[h].slots = reinterpret_cast<const HopSlot*>(base + so[h]);
        c->hop_part[h].keys = reinterpret_cast<const u64*>(base + ko[h]);
        e = hipMemcpy(base + so[h], slots[h].data(), sb[h], hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(base + ko[h], key[h].data(), kb[h], hipMemcpyHostToDevice);
    }
    c->hop_n1 = n[0];
    c->hop_n2 = n[1];
    int rc = e == hipSuccess ? table_alloc(c, c->hop, hop_values(c))
                             : fail(c, QD_ERR_HIP, std::string("index-hopping part tables: ") + hipGetErrorString(e));
    if (rc != QD_OK) free_hop(c);
    return rc;
}

int qd_hop_shape(const qd_ctx* c, int32_t* n1, int32_t* n2) {
    if (!c || !n1 || !n2) return QD_ERR_INVALID;
    if (!c->hop.d) return fail(c, QD_ERR_STATE, c->hop.off_text);
    *n1 = c->hop_n1;
    *n2 = c->hop_n2;
    return QD_OK;
}

int qd_hop_read(qd_ctx* c, uint64_t* out, int64_t n_values) {
    if (!c) return QD_ERR_INVALID;
    return table_read(c, c->hop, out, n_values);
}

int qd_hop_add(qd_ctx* c, const uint64_t* values, int64_t n_values) {
    if (!c) return QD_ERR_INVALID;
    return table_add(c, c->hop, values, n_values);
}

int qd_qstats_enable(qd_ctx* c, int32_t on) {
    if (!c) return QD_ERR_INVALID;
    if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    return stage_install(c, ST_QSTATS, on != 0, qd_qstats_values((uint32_t)c->S));
}

int qd_qstats_kind(const qd_ctx* c) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_QSTATS].d) return fail(c, QD_ERR_STATE, c->stage[ST_QSTATS].off_text);
    return qd_qstats_path((uint32_t)c->S);
}

int qd_qstats_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_QSTATS], out, n_values) : QD_ERR_INVALID; }

int qd_qstats_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_QSTATS], values, n_values) : QD_ERR_INVALID; }

int qd_qstats_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                     const uint16_t* codes, const uint8_t* drop, void* stream) {
    return stage_launch(c, ST_QSTATS, false, n, stream, [&](u64* table, hipStream_t st) {
        qd_qstats_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.codes = codes;
        a.drop = drop;
        a.table = table;
        return qd_qstats_launch(a, (uint32_t)c->S, n, st);
    });
}

int qd_dev_qstats(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_QSTATS].d) return fail(c, QD_ERR_STATE, c->stage[ST_QSTATS].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::CODES, codes, nullptr, nullptr, nullptr, nullptr);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(qd_qstats_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.codes(), nullptr, QD_STREAM_CONTEXT));
}

int qd_cstats_enable(qd_ctx* c, int32_t on) {
    if (!c) return QD_ERR_INVALID;
    return stage_install(c, ST_CSTATS, on != 0, QD_CS_VALUES);
}

int qd_cstats_lds_cycles(void) { return (int)QD_CS_LDS_CYCLES; }

int qd_cstats_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_CSTATS], out, n_values) : QD_ERR_INVALID; }

int qd_cstats_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_CSTATS], values, n_values) : QD_ERR_INVALID; }

int qd_cstats_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                     const uint16_t* codes, const uint8_t* drop, void* stream) {
    return stage_launch(c, ST_CSTATS, false, n, stream, [&](u64* table, hipStream_t st) {
        qd_cstats_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.codes = codes;
        a.drop = drop;
        a.table = table;
        return qd_cstats_launch(a, n, st);
    });
}

int qd_dev_cstats(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, const uint8_t* drop) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_CSTATS].d) return fail(c, QD_ERR_STATE, c->stage[ST_CSTATS].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::CODES, codes, drop, nullptr, nullptr, nullptr);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(qd_cstats_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.codes(), up.drop(), QD_STREAM_CONTEXT));
}

static_assert(QD_ADAPTERS_PROBES == QD_AD_PROBES && QD_ADAPTERS_K == QD_AD_K && QD_ADAPTERS_HIST_VALUES == QD_AD_HIST_VALUES &&
                  QD_ADAPTERS_DEST_VALUES == QD_AD_DEST_VALUES,
              "the public table sizes are the kernel's");

int qd_adapters_set(qd_ctx* c, const uint8_t* probes, int32_t n_probes) {
    if (!c) return QD_ERR_INVALID;
    const bool on = probes && n_probes != 0;
    qd_adapters_dev D{};
    if (on) {
        if (n_probes < 0 || n_probes > (int32_t)QD_AD_PROBES) return fail(c, QD_ERR_INVALID, "n_probes must be 0 to 16");
        if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
        for (uint32_t a = 0; a < QD_AD_PROBES; ++a) D.word[a] = QD_AD_NO_PROBE;
        for (int32_t a = 0; a < n_probes; ++a) {
            uint32_t w = 0;
            for (uint32_t i = 0; i < QD_AD_K; ++i) {
                const uint8_t b = probes[a * QD_AD_K + i];
                if (b != 'A' && b != 'C' && b != 'G' && b != 'T') return fail(c, QD_ERR_INVALID, "a probe holds a byte that is not A, C, G or T");
                w = (w << 2) | ((b >> 1) & 3u);
            }
            for (int32_t e = 0; e < a; ++e)
                if (D.word[e] == w) return fail(c, QD_ERR_INVALID, "two probes are equal");
            D.word[a] = w;
        }
        D.n_probes = (uint32_t)n_probes;
    }
    uint8_t given[sizeof c->adapters] = {0};  // (probes may be the context's own copy)
    if (on) std::memcpy(given, probes, (size_t)n_probes * QD_AD_K);
    const int rc = stage_install(c, ST_ADAPTERS, on, qd_adapters_values((uint32_t)c->S));
    if (rc != QD_OK || !on) return rc;
    std::memcpy(c->adapters, given, sizeof given);
    c->adapters_dev = D;
    return QD_OK;
}

int qd_adapters_get(const qd_ctx* c, uint8_t* probes, int32_t* n_probes) {
    if (!c || !n_probes) return QD_ERR_INVALID;
    *n_probes = (int32_t)c->adapters_dev.n_probes;
    if (probes) std::memcpy(probes, c->adapters, (size_t)c->adapters_dev.n_probes * QD_AD_K);
    return QD_OK;
}

int qd_adapters_active(const qd_ctx* c) { return c && c->stage[ST_ADAPTERS].d ? 1 : 0; }

int qd_adapters_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_ADAPTERS], out, n_values) : QD_ERR_INVALID; }

int qd_adapters_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_ADAPTERS], values, n_values) : QD_ERR_INVALID; }

int qd_adapters_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                       const uint16_t* codes, void* stream) {
    return stage_launch(c, ST_ADAPTERS, false, n, stream, [&](u64* table, hipStream_t st) {
        qd_adapters_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.codes = codes;
        a.table = table;
        return qd_adapters_launch(c->adapters_dev, a, (uint32_t)c->S, n, st);
    });
}

int qd_dev_adapters(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                    const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_ADAPTERS].d) return fail(c, QD_ERR_STATE, c->stage[ST_ADAPTERS].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::CODES, codes, nullptr, nullptr, nullptr, nullptr);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(qd_adapters_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.codes(), QD_STREAM_CONTEXT));
}

static_assert(QD_CLIP_VALUES == QD_CLIP_TABLE, "the public table size is the kernel's");

int qd_clip_set(qd_ctx* c, const qd_clip_params* params) {
    if (!c) return QD_ERR_INVALID;
    qd_clip_params P{};
    qd_clip_dev D{};
    const bool on = params && (params->front_clip[0] || params->front_clip[1] || params->tail_clip[0] || params->tail_clip[1] ||
                               params->window_size || params->window_quality || params->poly_g_min_length);
    if (on) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        for (int r = 0; r < 2; ++r) {
            if (P.front_clip[r] < 0 || P.front_clip[r] > 1000) return fail(c, QD_ERR_INVALID, "front_clip: 0 to 1000");
            if (P.tail_clip[r] < 0 || P.tail_clip[r] > 1000) return fail(c, QD_ERR_INVALID, "tail_clip: 0 to 1000");
            D.front[r] = (uint32_t)P.front_clip[r];
            D.tail[r] = (uint32_t)P.tail_clip[r];
        }
        if (P.window_size < 0 || P.window_size > QD_CLIP_MAX_WINDOW) return fail(c, QD_ERR_INVALID, "window_size: 0 (off) or 1 to 100");
        if (P.window_size ? (P.window_quality < 1 || P.window_quality > 93) : P.window_quality != 0)
            return fail(c, QD_ERR_INVALID, "window_quality: 1 to 93, set together with window_size");
        if (P.poly_g_min_length && (P.poly_g_min_length < 6 || P.poly_g_min_length > QD_CLIP_MAX_POLYG))
            return fail(c, QD_ERR_INVALID, "poly_g_min_length: 0 (off) or 6 to 100");
        if (P.min_length < 0 || P.min_length > 65535) return fail(c, QD_ERR_INVALID, "min_length: 0 to 65535");
        D.window = (uint32_t)P.window_size;
        D.window_sum = (uint32_t)(P.window_size * P.window_quality);
        D.poly_g = (uint32_t)P.poly_g_min_length;
        D.min_length = (uint32_t)P.min_length;
    }
    const int rc = stage_install(c, ST_CLIP, on, QD_CLIP_TABLE);
    if (rc != QD_OK || !on) return rc;
    c->clip = P;
    c->clip_dev = D;
    return QD_OK;
}

int qd_clip_get(const qd_ctx* c, qd_clip_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->clip;
    return QD_OK;
}

int qd_clip_active(const qd_ctx* c) { return c && c->stage[ST_CLIP].d ? 1 : 0; }

int qd_clip_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_CLIP], out, n_values) : QD_ERR_INVALID; }

int qd_clip_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_CLIP], values, n_values) : QD_ERR_INVALID; }

int qd_clip_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                   qd_rec* out1, qd_rec* out2, void* stream) {
    return stage_launch(c, ST_CLIP, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_clip_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.out[0] = out1;
        a.out[1] = out2;
        a.table = table;
        return qd_clip_launch(c->clip_dev, a, n, st);
    });
}

int qd_dev_clip(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2) {
    return dev_rewrite(c, ST_CLIP, qd_clip_device, text1, len1, recs1, text2, len2, recs2, n_pairs, out_recs1, out_recs2);
}

int qd_trim_set(qd_ctx* c, const qd_trim_params* params) {
    if (!c) return QD_ERR_INVALID;
    qd_trim_params P{};
    qd_trim_dev D{};
    const bool on = params && (params->adapter_r1_len || params->adapter_r2_len || params->quality_cutoff);
    if (on) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        const int32_t len[2] = {P.adapter_r1_len, P.adapter_r2_len};
        uint8_t* ad[2] = {P.adapter_r1, P.adapter_r2};
        for (int r = 0; r < 2; ++r) {
            if (len[r] < 0 || len[r] > QD_TRIM_ADAPTER_MAX) return fail(c, QD_ERR_INVALID, "an adapter has 1 to 64 letters");
            for (int i = 0; i < QD_TRIM_ADAPTER_MAX; ++i) {
                if (i >= len[r]) {
                    ad[r][i] = 0;
                    continue;
                }
                ad[r][i] &= 0xDF;  // upper case
                if (ad[r][i] != 'A' && ad[r][i] != 'C' && ad[r][i] != 'G' && ad[r][i] != 'T')
                    return fail(c, QD_ERR_INVALID, "an adapter holds letters of ACGT only");
                D.adapter[r][i >> 2] |= (uint32_t)ad[r][i] << (8 * (i & 3));
            }
            D.adapter_len[r] = (uint32_t)len[r];
            if (len[r] && P.min_overlap > len[r]) return fail(c, QD_ERR_INVALID, "min_overlap is above the length of a set adapter");
        }
        if (P.quality_cutoff < 0 || P.quality_cutoff > 93) return fail(c, QD_ERR_INVALID, "quality_cutoff: 0 to 93");
        if (P.min_overlap < 1 || P.min_overlap > QD_TRIM_ADAPTER_MAX) return fail(c, QD_ERR_INVALID, "min_overlap: 1 to 64");
        if (P.max_mismatch_pct < 0 || P.max_mismatch_pct > 50) return fail(c, QD_ERR_INVALID, "max_mismatch_pct: 0 to 50");
        if (P.min_length < 0 || P.min_length > 65535) return fail(c, QD_ERR_INVALID, "min_length: 0 to 65535");
        D.cutoff = (uint32_t)P.quality_cutoff;
        D.min_overlap = (uint32_t)P.min_overlap;
        D.mismatch_pct = (uint32_t)P.max_mismatch_pct;
        D.min_length = (uint32_t)P.min_length;
    }
    const int rc = stage_install(c, ST_TRIM, on, QD_TRIM_VALUES);
    if (rc != QD_OK || !on) return rc;
    c->trim = P;
    c->trim_dev = D;
    return QD_OK;
}

int qd_trim_get(const qd_ctx* c, qd_trim_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->trim;
    return QD_OK;
}

int qd_trim_active(const qd_ctx* c) { return c && c->stage[ST_TRIM].d ? 1 : 0; }

int qd_trim_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_TRIM], out, n_values) : QD_ERR_INVALID; }

int qd_trim_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_TRIM], values, n_values) : QD_ERR_INVALID; }

int qd_trim_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                   qd_rec* out1, qd_rec* out2, void* stream) {
    return stage_launch(c, ST_TRIM, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_trim_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.out[0] = out1;
        a.out[1] = out2;
        a.table = table;
        return qd_trim_launch(c->trim_dev, a, n, st);
    });
}

int qd_dev_trim(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2) {
    return dev_rewrite(c, ST_TRIM, qd_trim_device, text1, len1, recs1, text2, len2, recs2, n_pairs, out_recs1, out_recs2);
}

static_assert(QD_PAIRTRIM_VALUES == QD_PT_VALUES, "the public table size is the kernel's");

int qd_pairtrim_set(qd_ctx* c, const qd_pairtrim_params* params) {
    if (!c) return QD_ERR_INVALID;
    qd_pairtrim_params P{};
    qd_pairtrim_dev D{};
    if (params) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        if (P.min_overlap < 8 || P.min_overlap > 1000) return fail(c, QD_ERR_INVALID, "pair min_overlap: 8 to 1000");
        if (P.max_mismatches < 0 || P.max_mismatches > 64) return fail(c, QD_ERR_INVALID, "pair max_mismatches: 0 to 64");
        if (P.max_mismatch_pct < 0 || P.max_mismatch_pct > 50) return fail(c, QD_ERR_INVALID, "pair max_mismatch_pct: 0 to 50");
        if (P.min_length < 0 || P.min_length > 65535) return fail(c, QD_ERR_INVALID, "min_length: 0 to 65535");
        D.min_overlap = (uint32_t)P.min_overlap;
        D.max_mismatches = (uint32_t)P.max_mismatches;
        D.mismatch_pct = (uint32_t)P.max_mismatch_pct;
        D.min_length = (uint32_t)P.min_length;
    }
    const int rc = stage_install(c, ST_PAIRTRIM, params, QD_PT_VALUES);
    if (rc != QD_OK || !params) return rc;
    c->pairtrim = P;
    c->pairtrim_dev = D;
    return QD_OK;
}

int qd_pairtrim_get(const qd_ctx* c, qd_pairtrim_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->pairtrim;
    return QD_OK;
}

int qd_pairtrim_active(const qd_ctx* c) { return c && c->stage[ST_PAIRTRIM].d ? 1 : 0; }

int qd_pairtrim_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_PAIRTRIM], out, n_values) : QD_ERR_INVALID; }

int qd_pairtrim_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_PAIRTRIM], values, n_values) : QD_ERR_INVALID; }

int qd_pairtrim_device_inserts(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                               qd_rec* out1, qd_rec* out2, uint64_t* inserts, void* stream) {
    return stage_launch(c, ST_PAIRTRIM, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_pairtrim_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.out[0] = out1;
        a.out[1] = out2;
        a.table = table;
        a.insert = inserts;
        return qd_pairtrim_launch(c->pairtrim_dev, a, n, st);
    });
}

int qd_pairtrim_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                       qd_rec* out1, qd_rec* out2, void* stream) {
    return qd_pairtrim_device_inserts(c, text1, recs1, text2, recs2, n, out1, out2, nullptr, stream);
}

int qd_dev_pairtrim(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                    const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2) {
    return dev_rewrite(c, ST_PAIRTRIM, qd_pairtrim_device, text1, len1, recs1, text2, len2, recs2, n_pairs, out_recs1, out_recs2);
}

static_assert(QD_PAIRCORRECT_VALUES == QD_PC_VALUES, "the public table size is the kernel's");

int qd_paircorrect_set(qd_ctx* c, const qd_paircorrect_params* params) {
    if (!c) return QD_ERR_INVALID;
    qd_paircorrect_params P{};
    qd_paircorrect_dev D{};
    if (params) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        if (P.good_quality < 1 || P.good_quality > 93) return fail(c, QD_ERR_INVALID, "pair_correct good_quality: 1 to 93");
        if (P.bad_quality < 0 || P.bad_quality >= P.good_quality) return fail(c, QD_ERR_INVALID, "pair_correct bad_quality: 0 to good_quality - 1");
        D.good_byte = 33u + (uint32_t)P.good_quality;
        D.bad_byte = 33u + (uint32_t)P.bad_quality;
    }
    const int rc = stage_install(c, ST_PAIRCORRECT, params, QD_PC_VALUES);
    if (rc != QD_OK || !params) return rc;
    c->paircorrect = P;
    c->paircorrect_dev = D;
    return QD_OK;
}

int qd_paircorrect_get(const qd_ctx* c, qd_paircorrect_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->paircorrect;
    return QD_OK;
}

int qd_paircorrect_active(const qd_ctx* c) { return c && c->stage[ST_PAIRCORRECT].d ? 1 : 0; }

int qd_paircorrect_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_PAIRCORRECT], out, n_values) : QD_ERR_INVALID; }

int qd_paircorrect_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_PAIRCORRECT], values, n_values) : QD_ERR_INVALID; }

int qd_paircorrect_device(qd_ctx* c, uint8_t* text1, const qd_rec* recs1, uint8_t* text2, const qd_rec* recs2, const uint64_t* inserts,
                          uint32_t n, void* stream) {
    if (c && !inserts && n) return fail(c, QD_ERR_INVALID, "overlap correction: no insert lengths");
    return stage_launch(c, ST_PAIRCORRECT, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_paircorrect_args a{};
        a.text[0] = text1;
        a.text[1] = text2;
        a.recs[0] = recs1;
        a.recs[1] = recs2;
        a.insert = inserts;
        a.table = table;
        return qd_paircorrect_launch(c->paircorrect_dev, a, n, st);
    });
}

int qd_dev_paircorrect(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                       const uint32_t* recs2, int64_t n_pairs, const uint64_t* inserts, uint8_t* out_text1, uint8_t* out_text2) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_PAIRCORRECT].d) return fail(c, QD_ERR_STATE, c->stage[ST_PAIRCORRECT].off_text);
    if (!inserts && !c->stage[ST_PAIRTRIM].d) return fail(c, QD_ERR_STATE, c->stage[ST_PAIRTRIM].off_text);
    if ((len1 > 0 && (!text1 || !out_text1)) || (len2 > 0 && (!text2 || !out_text2))) return fail(c, QD_ERR_INVALID, "null argument");
    if (inserts && recs1 && recs2 && n_pairs > 0 && n_pairs <= 0x7FFFFFFF)  // (open() below refuses the other cases)
        for (int64_t j = 0; j < n_pairs; ++j)
            if (inserts[j] > (uint64_t)recs1[6 * j + 4] + recs2[6 * j + 4]) return fail(c, QD_ERR_INVALID, "an insert length is above L1 + L2");
    PairUpload up(c);
    const int want = PairUpload::INSERTS | PairUpload::TEXT_BACK | (inserts ? 0 : PairUpload::SCRATCH_RECS);
    int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, want, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != QD_OK) return rc;
    if (up.empty()) {  // no pairs: the texts as they came
        if (len1 > 0) std::memcpy(out_text1, text1, (size_t)len1);
        if (len2 > 0) std::memcpy(out_text2, text2, (size_t)len2);
        return QD_OK;
    }
    up.texts_back(out_text1, out_text2);
    if (inserts) {
        HIPCHK(c, hipMemcpyAsync(up.inserts(), inserts, (size_t)up.n() * 8, hipMemcpyHostToDevice, c->stream));
    } else {  // the hand-over: the overlap kernel with the context's parameters supplies them (its table grows too)
        rc = qd_pairtrim_device_inserts(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.out(0), up.out(1), up.inserts(), QD_STREAM_CONTEXT);
    }
    if (rc == QD_OK)
        rc = qd_paircorrect_device(c, up.mutable_text(0), up.recs(0), up.mutable_text(1), up.recs(1), up.inserts(), up.n(), QD_STREAM_CONTEXT);
    return up.close(rc);
}

static_assert(QD_POSTTRIM_VALUES == QD_POST_TABLE, "the public table size is the kernel's");

int qd_posttrim_set(qd_ctx* c, const qd_posttrim_params* params) {
    if (!c) return QD_ERR_INVALID;
    qd_posttrim_params P{};
    qd_posttrim_dev D{};
    const bool on = params && (params->tail_n || params->poly_x_min_length || params->max_length[0] || params->max_length[1]);
    if (on) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        if (P.tail_n < 0 || P.tail_n > 1) return fail(c, QD_ERR_INVALID, "tail_n: 0 or 1");
        if (P.poly_x_min_length && (P.poly_x_min_length < QD_POST_MIN_POLYX || P.poly_x_min_length > QD_POST_MAX_POLYX))
            return fail(c, QD_ERR_INVALID, "poly_x_min_length: 0 (off) or 6 to 100");
        for (int r = 0; r < 2; ++r) {
            if (P.max_length[r] < 0 || P.max_length[r] > 65535) return fail(c, QD_ERR_INVALID, "max_length: 0 (off) or 1 to 65535");
            D.max_length[r] = (uint32_t)P.max_length[r];
        }
        if (P.min_length < 0 || P.min_length > 65535) return fail(c, QD_ERR_INVALID, "min_length: 0 to 65535");
        D.tail_n = (uint32_t)P.tail_n;
        D.poly_x = (uint32_t)P.poly_x_min_length;
        D.min_length = (uint32_t)P.min_length;
    }
    const int rc = stage_install(c, ST_POSTTRIM, on, QD_POST_TABLE);
    if (rc != QD_OK || !on) return rc;
    c->posttrim = P;
    c->posttrim_dev = D;
    return QD_OK;
}

int qd_posttrim_get(const qd_ctx* c, qd_posttrim_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->posttrim;
    return QD_OK;
}

int qd_posttrim_active(const qd_ctx* c) { return c && c->stage[ST_POSTTRIM].d ? 1 : 0; }

int qd_posttrim_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_POSTTRIM], out, n_values) : QD_ERR_INVALID; }

int qd_posttrim_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_POSTTRIM], values, n_values) : QD_ERR_INVALID; }

int qd_posttrim_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                       qd_rec* out1, qd_rec* out2, void* stream) {
    return stage_launch(c, ST_POSTTRIM, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_posttrim_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.out[0] = out1;
        a.out[1] = out2;
        a.table = table;
        return qd_posttrim_launch(c->posttrim_dev, a, n, st);
    });
}

int qd_dev_posttrim(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                    const uint32_t* recs2, int64_t n_pairs, uint32_t* out_recs1, uint32_t* out_recs2) {
    return dev_rewrite(c, ST_POSTTRIM, qd_posttrim_device, text1, len1, recs1, text2, len2, recs2, n_pairs, out_recs1, out_recs2);
}

static_assert(QD_FILTER_VALUES == QD_FL_VALUES, "the public table width is the kernel's");

int qd_filter_set(qd_ctx* c, const qd_filter_params* params) {
    if (!c) return QD_ERR_INVALID;
    qd_filter_params P = FILTER_OFF;
    bool on = false;
    if (params) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        if (P.qualified_quality == -1) P.qualified_quality = FILTER_OFF.qualified_quality;
        if (P.min_length != -1 && (P.min_length < 1 || P.min_length > 100000)) return fail(c, QD_ERR_INVALID, "filter min_length: 1 to 100000 (-1: off)");
        if (P.max_n != -1 && (P.max_n < 0 || P.max_n > 100000)) return fail(c, QD_ERR_INVALID, "filter max_n: 0 to 100000 (-1: off)");
        if (P.max_unqualified_pct != -1 && (P.max_unqualified_pct < 0 || P.max_unqualified_pct > 100))
            return fail(c, QD_ERR_INVALID, "filter max_unqualified_pct: 0 to 100 (-1: off)");
        if (P.qualified_quality < 1 || P.qualified_quality > 93) return fail(c, QD_ERR_INVALID, "filter qualified_quality: 1 to 93 (-1: 15)");
        if (P.min_mean_quality != -1 && (P.min_mean_quality < 1 || P.min_mean_quality > 93)) return fail(c, QD_ERR_INVALID, "filter min_mean_quality: 1 to 93 (-1: off)");
        if (P.min_complexity_pct != -1 && (P.min_complexity_pct < 1 || P.min_complexity_pct > 100))
            return fail(c, QD_ERR_INVALID, "filter min_complexity_pct: 1 to 100 (-1: off)");
        on = P.min_length >= 0 || P.max_n >= 0 || P.max_unqualified_pct >= 0 || P.min_mean_quality >= 0 || P.min_complexity_pct >= 0;
    }
    if (on && (!c->have_plan || !c->have_table)) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    const int rc = stage_install(c, ST_FILTER, on, qd_filter_values((uint32_t)c->S));
    if (rc != QD_OK || !on) return rc;
    c->filter = P;
    c->filter_dev = filter_dev_of(P);
    return QD_OK;
}

int qd_filter_get(const qd_ctx* c, qd_filter_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->filter;
    return QD_OK;
}

int qd_filter_active(const qd_ctx* c) { return c && c->stage[ST_FILTER].d ? 1 : 0; }

int qd_filter_kind(const qd_ctx* c) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_FILTER].d) return fail(c, QD_ERR_STATE, c->stage[ST_FILTER].off_text);
    return qd_filter_path((uint32_t)c->S);
}

int qd_filter_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_FILTER], out, n_values) : QD_ERR_INVALID; }

int qd_filter_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_FILTER], values, n_values) : QD_ERR_INVALID; }

int qd_filter_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                     const uint16_t* codes, uint8_t* reason, void* stream) {
    return stage_launch(c, ST_FILTER, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_filter_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.codes = codes;
        a.reason = reason;
        a.table = table;
        return qd_filter_launch(c->filter_dev, a, (uint32_t)c->S, n, st);
    });
}

int qd_dev_filter(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, uint8_t* reasons) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_FILTER].d) return fail(c, QD_ERR_STATE, c->stage[ST_FILTER].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::CODES | PairUpload::REASONS, codes, nullptr,
                           nullptr, nullptr, reasons);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(qd_filter_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.codes(), up.reason(), QD_STREAM_CONTEXT));
}

static_assert(QD_SCREEN_VALUES == QD_SC_VALUES, "the public table width is the kernel's");
static_assert(QD_SCREEN_MAX_KMERS == QD_SC_MAX_KMERS && QD_SCREEN_LDS_MAX_KMERS == QD_SC_LDS_MAX_KMERS, "the public caps are the kernel's");
static_assert(QD_SCREEN_DROPPED == QD_SC_DROPPED, "the public flag byte is the kernel's");

namespace {
// the reverse-complement word of a k-mer's forward word, base by base (the kernel reverses bit pairs)
uint64_t screen_revcomp(uint64_t w, int k) {
    uint64_t rc = 0;
    for (int i = 0; i < k; ++i) rc = (rc << 2) | (((w >> (2 * i)) & 3u) ^ 2u);
    return rc;
}
}  // namespace

int qd_screen_set(qd_ctx* c, const qd_screen_params* params, const uint64_t* kmers, int64_t n_kmers) {
    if (!c) return QD_ERR_INVALID;
    const bool on = params && n_kmers != 0;
    qd_screen_params P{};
    std::vector<u64> slots;
    uint32_t lg = 0;
    if (on) {  // checked as the configuration file's values are, before anything changes
        P = *params;
        if (P.kmer < QD_SC_MIN_K || P.kmer > QD_SC_MAX_K) return fail(c, QD_ERR_INVALID, "screen kmer: 15 to 32");
        if (P.min_hits < 1 || P.min_hits > 65535) return fail(c, QD_ERR_INVALID, "screen min_hits: 1 to 65535");
        if (P.action != QD_SC_REPORT && P.action != QD_SC_DROP) return fail(c, QD_ERR_INVALID, "screen action: 0 (report) or 1 (drop)");
        if (!kmers || n_kmers < 0 || n_kmers > (int64_t)QD_SC_MAX_KMERS) return fail(c, QD_ERR_INVALID, "screen k-mers: 1 to 4194304 words");
        for (int64_t i = 0; i < n_kmers; ++i) {
            const uint64_t w = kmers[i];
            if (i && kmers[i - 1] >= w) return fail(c, QD_ERR_INVALID, "screen k-mers: the words must ascend strictly");
            if (P.kmer < 32 && (w >> (2 * P.kmer))) return fail(c, QD_ERR_INVALID, "screen k-mers: a word is not below 4^kmer");
            if (screen_revcomp(w, P.kmer) < w) return fail(c, QD_ERR_INVALID, "screen k-mers: a word is not canonical");
        }
        if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
        lg = qd_screen_slots_lg((uint64_t)n_kmers);
        slots.assign((size_t)1 << lg, QD_SC_EMPTY);
        const uint32_t mask = (1u << lg) - 1u;
        for (int64_t i = 0; i < n_kmers; ++i) {  // at most half full: a free slot is never far
            uint32_t s = qd_screen_slot(kmers[i], lg);
            while (slots[s] != QD_SC_EMPTY) s = (s + 1) & mask;
            slots[s] = kmers[i];
        }
    }
    const int rc = stage_install(c, ST_SCREEN, on, qd_screen_values((uint32_t)c->S));
    if (rc != QD_OK || !on) return rc;
    hipError_t e = c->d_screen_slots.alloc(slots.size() * 8);
    if (e != hipSuccess) {
        stage_off(c, ST_SCREEN);
        return fail(c, QD_ERR_HIP, std::string("screen hash table: ") + hipGetErrorString(e));
    }
    HIPCHK(c, hipMemcpy(c->d_screen_slots, slots.data(), slots.size() * 8, hipMemcpyHostToDevice));
    c->screen = P;
    c->screen_dev = qd_screen_dev{(uint32_t)P.kmer, (uint32_t)P.min_hits, (uint32_t)P.action, lg};
    c->screen_kmers = n_kmers;
    return QD_OK;
}

int qd_screen_get(const qd_ctx* c, qd_screen_params* out, int64_t* n_kmers) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->screen;
    if (n_kmers) *n_kmers = c->screen_kmers;
    return QD_OK;
}

int qd_screen_active(const qd_ctx* c) { return c && c->stage[ST_SCREEN].d ? (c->screen.action == QD_SC_DROP ? 2 : 1) : 0; }

int qd_screen_kind(const qd_ctx* c) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_SCREEN].d) return fail(c, QD_ERR_STATE, c->stage[ST_SCREEN].off_text);
    return qd_screen_path((uint64_t)c->screen_kmers);
}

int64_t qd_screen_first_slot(uint64_t word, int64_t n_kmers) {
    if (n_kmers < 1 || n_kmers > (int64_t)QD_SC_MAX_KMERS) return QD_ERR_INVALID;
    return qd_screen_slot(word, qd_screen_slots_lg((uint64_t)n_kmers));
}

int qd_screen_read(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_SCREEN], out, n_values) : QD_ERR_INVALID; }

int qd_screen_add(qd_ctx* c, const uint64_t* values, int64_t n_values) { return c ? table_add(c, c->stage[ST_SCREEN], values, n_values) : QD_ERR_INVALID; }

int qd_screen_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                     const uint16_t* codes, const uint8_t* drop_in, uint32_t* hits, uint8_t* flag, void* stream) {
    return stage_launch(c, ST_SCREEN, true, n, stream, [&](u64* table, hipStream_t st) {
        qd_screen_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.codes = codes;
        a.drop_in = drop_in;
        a.hits = hits;
        a.flag = flag;
        a.slots = c->d_screen_slots;
        a.table = table;
        return qd_screen_launch(c->screen_dev, a, (uint32_t)c->S, n, qd_screen_path((uint64_t)c->screen_kmers), (uint32_t)c->cu, st);
    });
}

int qd_dev_screen(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
                  const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, const uint8_t* drop_in, uint32_t* hits_out, uint8_t* flag_out) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_SCREEN].d) return fail(c, QD_ERR_STATE, c->stage[ST_SCREEN].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::CODES | PairUpload::REASONS | PairUpload::HITS, codes,
                           drop_in, nullptr, nullptr, flag_out, hits_out);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(qd_screen_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.codes(), up.drop(), up.hits(), up.reason(),
                                     QD_STREAM_CONTEXT));
}

static_assert(QD_DUP_VALUES == QD_DP_VALUES, "the public row size is the kernels'");
static_assert(QD_DUP_READ_ERROR == QD_UNKNOWN_READ_ERROR, "one sizing protocol");

int qd_dup_set(qd_ctx* c, const qd_dup_params* params) {
    if (!c) return QD_ERR_INVALID;
    int sample_lg = 0;
    if (params) {  // checked as the configuration file's values are, before anything changes
        const qd_dup_params& P = *params;
        if (P.bases < 8 || P.bases > 32) return fail(c, QD_ERR_INVALID, "duplication bases: 8 to 32");
        if (P.sample < 1 || P.sample > 1024 || (P.sample & (P.sample - 1))) return fail(c, QD_ERR_INVALID, "duplication sample: a power of two, 1 to 1024");
        if (!tally_slots_ok(P.slots)) return fail(c, QD_ERR_INVALID, "duplication slots: a power of two in 2^10 .. 2^28");
        while ((1 << sample_lg) < P.sample) ++sample_lg;
        if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    }
    int rc = stage_install(c, ST_DUP, params != nullptr, qd_dup_values((uint32_t)c->S));
    if (rc != QD_OK || !params) return rc;
    rc = tally_open(c, c->dup_keys, params->slots, "duplication table");
    if (rc != QD_OK) {
        stage_off(c, ST_DUP);
        return rc;
    }
    c->dup = *params;
    c->dup_dev = qd_dup_dev{params->bases, sample_lg};
    return QD_OK;
}

int qd_dup_get(const qd_ctx* c, qd_dup_params* out) {
    if (!c || !out) return QD_ERR_INVALID;
    *out = c->dup;
    return QD_OK;
}

int qd_dup_active(const qd_ctx* c) { return c && c->stage[ST_DUP].d ? 1 : 0; }

int qd_stream_retired(qd_ctx* c, void* stream) {
    if (!c) return QD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    forget_stream(c, st);  // (the caller waited for the stream: nothing of it is outstanding)
    tally_retired(c->uk, st);
    tally_retired(c->dup_keys, st);
    return QD_OK;
}

int qd_dup_stats(qd_ctx* c, uint64_t* out, int64_t n_values) { return c ? table_read(c, c->stage[ST_DUP], out, n_values) : QD_ERR_INVALID; }

int64_t qd_dup_read(qd_ctx* c, uint64_t* keys, uint64_t* counts, int64_t cap) {
    auto bad = [&](int code, const std::string& msg) { return QD_DUP_READ_ERROR + (int64_t)fail(c, code, msg); };
    if (!c || cap < 0 || (cap > 0 && (!keys || !counts))) return bad(QD_ERR_INVALID, "bad arguments");
    if (!c->stage[ST_DUP].d) return bad(QD_ERR_STATE, c->stage[ST_DUP].off_text);
    std::vector<u64> hk;
    const int64_t D = tally_gather(c, c->dup_keys, "duplication", cap, hk, counts);
    for (int64_t i = 0; i < D; ++i)  // (D <= 0: nothing was gathered)
        for (int q = 0; q < QD_DUP_KEY_WORDS; ++q) keys[i * QD_DUP_KEY_WORDS + q] = hk[(size_t)i * QD_KEY_WORDS + q];
    return D;
}

int qd_dup_device(qd_ctx* c, const uint8_t* text1, const qd_rec* recs1, const uint8_t* text2, const qd_rec* recs2, uint32_t n,
                  const uint16_t* codes, const uint8_t* drop, void* stream) {
    int own = QD_OK;  // what the scratch or the handshake refused: qd_last_error has their text
    const int rc = stage_launch(c, ST_DUP, false, n, stream, [&](u64* table, hipStream_t st) {
        StreamScratch::Buf* sc = c->dup_keys.scratch.need(c, st, n, qd_dup_list_bytes);
        if (!sc) {
            own = QD_ERR_HIP;
            return hipSuccess;
        }
        qd_dup_args a{};
        fill_pair_args(a, text1, recs1, text2, recs2);
        a.codes = codes;
        a.drop = drop;
        a.table = table;
        a.list_n = sc->buf.as<uint32_t>();
        a.list = reinterpret_cast<uint64_t*>(sc->buf + QD_DUP_LIST_HEAD);
        a.where = reinterpret_cast<uint32_t*>(sc->buf + QD_DUP_LIST_HEAD + sc->units * QD_DUP_KEY_WORDS * 8);
        a.t = tally_view(c->dup_keys);
        hipError_t e = qd_dup_launch(c->dup_dev, a, (uint32_t)c->S, n, c->cu, tally_before(c->dup_keys, st), st);
        if (e == hipSuccess) own = tally_after(c, c->dup_keys, st);
        return e;
    });
    return own != QD_OK ? own : rc;
}

int qd_dev_dup(qd_ctx* c, const uint8_t* text1, int64_t len1, const uint32_t* recs1, const uint8_t* text2, int64_t len2,
               const uint32_t* recs2, int64_t n_pairs, const uint16_t* codes, const uint8_t* drop) {
    if (!c) return QD_ERR_INVALID;
    if (!c->stage[ST_DUP].d) return fail(c, QD_ERR_STATE, c->stage[ST_DUP].off_text);
    PairUpload up(c);
    const int rc = up.open(text1, len1, recs1, text2, len2, recs2, n_pairs, PairUpload::CODES, codes, drop, nullptr, nullptr, nullptr);
    if (rc != QD_OK || up.empty()) return rc;
    return up.close(qd_dup_device(c, up.text(0), up.recs(0), up.text(1), up.recs(1), up.n(), up.codes(), up.drop(), QD_STREAM_CONTEXT));
}

int qd_kernel_kind(const qd_ctx* c, int has_len) {
    if (!c || !c->have_table) return QD_ERR_STATE;
    return pick_kernel(c, has_len != 0);
}

int qd_set_option(qd_ctx* c, const char* name, int64_t value) {
    if (!c || !name) return QD_ERR_INVALID;
    if (!strcmp(name, "fast_workgroups_per_cu")) {
        if (value < 0 || value > 4096) return fail(c, QD_ERR_INVALID, "fast_workgroups_per_cu must be 0..4096");
        c->opt_wg_per_cu = (int)value;
        return QD_OK;
    }
    if (!strcmp(name, "fast_block")) {
        if (value != 0 && value != 256 && value != 512 && value != 1024)
            return fail(c, QD_ERR_INVALID, "fast_block must be 0, 256, 512 or 1024");
        c->opt_block = (int)value;
        return QD_OK;
    }
    if (!strcmp(name, "slot_factor")) {  // open-addressing slots per barcode of the fast kernel's table (before rounding up to a power of two)
        if (value < 0 || value > 16) return fail(c, QD_ERR_INVALID, "slot_factor must be 0 (automatic) .. 16");
        c->opt_slot_factor = (int)value;
        return c->have_table ? rebuild(c) : QD_OK;
    }
    if (!strcmp(name, "mol_strips")) {
        c->opt_mol_strips = value != 0;
        return c->have_table ? rebuild(c) : QD_OK;
    }
    if (!strcmp(name, "force_generic")) {
        c->opt_force_generic = value != 0;
        return QD_OK;
    }
    if (!strcmp(name, "kernel")) {
        if (value < 0 || value > 2) return fail(c, QD_ERR_INVALID, "kernel must be 0 (automatic), 1 (fast) or 2 (generic)");
        c->opt_kernel = (int)value;
        return QD_OK;
    }
    if (!strcmp(name, "fold_pairs")) {  // test knob: fold the 32-bit counter rows this often (default 2^32 - 1)
        if (value < 1 || value > (int64_t)0xFFFFFFFF) return fail(c, QD_ERR_INVALID, "fold_pairs must be 1..2^32-1");
        c->fold_limit = (uint64_t)value;
        return QD_OK;
    }
    if (!strcmp(name, "unknown_tag_bits")) {  // test knob: the tally keeps this many low bits of a key's tag (default 64), so tag collisions can be made
        if (value < 1 || value > 64) return fail(c, QD_ERR_INVALID, "unknown_tag_bits must be 1..64");
        c->uk.tag_bits = (int)value;
        return QD_OK;
    }
    if (!strcmp(name, "dup_tag_bits")) {  // test knob: the same for the duplication tally's table
        if (value < 1 || value > 64) return fail(c, QD_ERR_INVALID, "dup_tag_bits must be 1..64");
        c->dup_keys.tag_bits = (int)value;
        return QD_OK;
    }
    return fail(c, QD_ERR_INVALID, std::string("unknown option ") + name);
}


int qd_demux_device(qd_ctx* c, int64_t n, const qd_rows* rows, uint16_t* codes, uint8_t* mol, void* stream) {
    if (!c || !rows || n < 0) return fail(c, QD_ERR_INVALID, "bad arguments");
    if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    if (n == 0) return QD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return launch(c, n, rows, codes, mol, resolve_stream(c, stream));
}

int qd_demux_device_ragged(qd_ctx* c, int64_t n, const qd_rows* rows, uint16_t* codes, uint8_t* mol, int64_t n_short,
                           const uint32_t* short_idx, void* stream) {
    if (!c || !rows || n < 0 || n_short < 0 || (n_short > 0 && !short_idx)) return fail(c, QD_ERR_INVALID, "bad arguments");
    if (!c->have_plan || !c->have_table) return fail(c, QD_ERR_STATE, "qd_set_plan and qd_set_barcodes first");
    for (int k = 0; k < c->lay.n_streams; ++k)
        if (!rows->len[k]) return fail(c, QD_ERR_INVALID, "qd_demux_device_ragged needs the len rows of every stream");
    if (n == 0) return QD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return launch(c, n, rows, codes, mol, resolve_stream(c, stream), n_short, short_idx);
}

int qd_synchronize(qd_ctx* c) {
    if (!c) return QD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));
    return QD_OK;
}

// counters of this context summed on its device: d_counts[0..2S] + TOTAL at d_counts[cnt_stride], on c->stream
static int counts_to_device(qd_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, join_into_own_stream(c));  // the reduce runs behind this context's launches, whatever stream they used
    const uint32_t ncnt = (uint32_t)(2 * c->S + 1);
    hipError_t e = qd_launch_reduce(c->d_partial, c->partial_rows, c->cnt_stride, ncnt, c->d_acc, c->d_counts, c->stream);
    if (e != hipSuccess) return fail(c, QD_ERR_HIP, std::string("reduce launch: ") + hipGetErrorString(e));
    HIPCHK(c, hipMemcpyAsync(c->d_counts + c->cnt_stride, &c->total_pairs, 8, hipMemcpyHostToDevice, c->stream));
    return QD_OK;
}

// h = device layout [cnt_stride + 1] -> the ABI's vector [2S + 4]
static void compose_counts(const qd_ctx* c, const u64* h, uint64_t* out) {
    uint64_t pass = 0, failq = 0;
    for (int i = 0; i < c->S; ++i) {
        out[4 + 2 * i] = h[2 * i];
        out[5 + 2 * i] = h[2 * i + 1];
        pass += h[2 * i];
        failq += h[2 * i + 1];
    }
    out[0] = h[c->cnt_stride];  // TOTAL: pairs submitted (Sample.py:62)
    out[1] = pass;
    out[2] = failq;
    out[3] = h[2 * c->S];       // UNDETERMINED: counted on the device, not derived
}

int qd_get_counts(qd_ctx* c, uint64_t* out, int32_t n_values) {
    if (!c || !out) return QD_ERR_INVALID;
    if (!c->have_table) return fail(c, QD_ERR_STATE, "qd_set_barcodes first");
    if (n_values != 2 * c->S + 4) return fail(c, QD_ERR_INVALID, "n_values must be 2*S+4");
    const int r = counts_to_device(c);
    if (r != QD_OK) return r;
    std::vector<u64> h((size_t)c->cnt_stride + 1);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_counts, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    compose_counts(c, h.data(), out);
    return QD_OK;
}

// Counters another context of this process gathered (qd_get_counts layout) join this context's 64-bit totals: what
// a process with several contexts on one device does before qd_reduce_counts, whose communicator holds one of them.
int qd_add_counts(qd_ctx* c, const uint64_t* counts, int32_t n_values) {
    if (!c || !counts) return QD_ERR_INVALID;
    if (!c->have_table) return fail(c, QD_ERR_STATE, "qd_set_barcodes first");
    if (n_values != 2 * c->S + 4) return fail(c, QD_ERR_INVALID, "n_values must be 2*S+4");
    uint64_t pass = 0, failq = 0;
    for (int i = 0; i < c->S; ++i) {
        pass += counts[4 + 2 * i];
        failq += counts[5 + 2 * i];
    }
    if (pass != counts[1] || failq != counts[2] || counts[0] != pass + failq + counts[3])
        return fail(c, QD_ERR_INVALID, "counter vector is not self-consistent (TOTAL = PASS + FAIL + UNDETERMINED over the samples)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, wait_all(c));  // demux_fixup adds to d_acc on the device: nothing of this context may be in flight
    std::vector<u64> h((size_t)c->cnt_stride);
    HIPCHK(c, hipMemcpy(h.data(), c->d_acc, h.size() * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < 2 * c->S; ++i) h[(size_t)i] += counts[4 + i];
    h[(size_t)(2 * c->S)] += counts[3];
    HIPCHK(c, hipMemcpy(c->d_acc, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    c->total_pairs += counts[0];
    return QD_OK;
}

int qd_reset_counts(qd_ctx* c) {
    if (!c) return QD_ERR_INVALID;
    if (!c->have_table) {  // no barcodes, no pair counters; the stages that need none (clip, trim, pairtrim, paircorrect, posttrim, cstats) may be on
        if (!stages_on(c, false)) return QD_OK;
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, wait_all(c));
        for (const StageTable& T : c->stage)
            if (T.d) HIPCHK(c, hipMemset(T.d, 0, T.n_values * 8));
        return QD_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, join_into_own_stream(c));
    HIPCHK(c, hipMemsetAsync(c->d_partial, 0,(size_t)c->partial_rows * c->cnt_stride * sizeof(qd_row_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_acc, 0, (size_t)c->cnt_stride * 8, c->stream));
    if (c->uk.mem) HIPCHK(c, tally_zero(c->uk, c->stream));  // sum(counts) + short + dropped == UNDETERMINED stays true
    if (c->hop.d) HIPCHK(c, hipMemsetAsync(c->hop.d, 0, c->hop.n_values * 8, c->stream));  // sum(table) == UNDETERMINED stays true
    for (const StageTable& T : c->stage)  // (the quality counters: records stay equal to the pair counters)
        if (T.d) HIPCHK(c, hipMemsetAsync(T.d, 0, T.n_values * 8, c->stream));
    if (c->dup_keys.mem) HIPCHK(c, tally_zero(c->dup_keys, c->stream));  // both of dup's tables: sampled == tallied + not_tallied stays true
    HIPCHK(c, track(c, c->stream));  // later launches on other streams are not ordered behind this: wait here
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->total_pairs = 0;
    c->pairs_in_rows = 0;
    return QD_OK;
}

// ---- pinned slots ---------------------------------------------------------------------------------
static size_t carve(qd_slot_buffers& v, uint8_t* base, const qd_layout& L, int64_t n) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* p = base ? base + off : nullptr;
        off += (bytes + 255) & ~(size_t)255;
        return p;
    };
    for (int k = 0; k < 2; ++k) {
        const bool used = k < L.n_streams;
        v.seq[k] = used ? take((size_t)n * L.seq_stride[k]) : nullptr;
        v.qual[k] = used ? take((size_t)n * L.qual_stride[k]) : nullptr;
        v.len[k] = used ? take((size_t)n) : nullptr;
    }
    v.codes = (uint16_t*)take((size_t)n * 2);
    v.mol = L.mol_width ? take((size_t)n * L.mol_width) : nullptr;
    v.max_pairs = n;
    v.short_cap = n / 8 + 64;
    for (int k = 0; k < 2; ++k) v.short_idx[k] = (k < L.n_streams) ? (uint32_t*)take((size_t)v.short_cap * 4) : nullptr;
    return off;
}

int qd_slots_create(qd_ctx* c, int32_t n_slots, int64_t max_pairs) {
    if (!c || n_slots < 1 || n_slots > 64 || max_pairs < 1) return fail(c, QD_ERR_INVALID, "bad slot arguments");
    if (!c->have_plan) return fail(c, QD_ERR_STATE, "qd_set_plan first");
    if (!c->slots.empty()) return fail(c, QD_ERR_STATE, "slots already exist");
    HIPCHK(c, hipSetDevice(c->device));
    qd_slot_buffers probe{};
    const size_t bytes = carve(probe, nullptr, c->lay, max_pairs);
    c->slots.resize((size_t)n_slots);
    c->slot_pairs = max_pairs;
    HIPCHK(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    for (auto& s : c->slots) {
        HIPCHK(c, hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
        HIPCHK(c, s.h_base.alloc(bytes));
        HIPCHK(c, s.d_base.alloc(bytes));
        carve(s.h, s.h_base, c->lay, max_pairs);
        carve(s.d, s.d_base, c->lay, max_pairs);
        HIPCHK(c, s.h_short.alloc((size_t)s.h.short_cap * 12));
        HIPCHK(c, s.d_short.alloc((size_t)s.h.short_cap * 12));
    }
    return QD_OK;
}

int qd_slots_destroy(qd_ctx* c) {
    if (!c) return QD_ERR_INVALID;
    (void)hipSetDevice(c->device);
    for (auto& s : c->slots) {
        if (s.stream) {
            (void)hipStreamSynchronize(s.stream);
            forget_stream(c, s.stream);
            (void)hipStreamDestroy(s.stream);
        }
        if (s.uploaded) (void)hipEventDestroy(s.uploaded);
    }
    c->slots.clear();  // (their buffers go back here)
    if (c->up_stream) {
        (void)hipStreamSynchronize(c->up_stream);
        (void)hipStreamDestroy(c->up_stream);
        c->up_stream = nullptr;
    }
    return QD_OK;
}

int qd_slot_get(qd_ctx* c, int32_t slot, qd_slot_buffers* out) {
    if (!c || !out || slot < 0 || slot >= (int)c->slots.size()) return fail(c, QD_ERR_INVALID, "bad slot");
    *out = c->slots[(size_t)slot].h;
    return QD_OK;
}

// n_short: NULL = no exception lists (has_len decides between the fast and the generic kernel)
static int submit_impl(qd_ctx* c, int32_t slot, int64_t n, int32_t has_len, const int64_t* n_short) {
    if (!c || slot < 0 || slot >= (int)c->slots.size()) return fail(c, QD_ERR_INVALID, "bad slot");
    if (n < 0 || n > c->slot_pairs) return fail(c, QD_ERR_INVALID, "n_pairs exceeds the slot capacity");
    if (!c->have_table) return fail(c, QD_ERR_STATE, "qd_set_barcodes first");
    Slot& s = c->slots[(size_t)slot];
    if (s.busy) return fail(c, QD_ERR_STATE, "slot already submitted; qd_wait it first");
    HIPCHK(c, hipSetDevice(c->device));
    s.busy = true;
    if (n == 0) return QD_OK;
    const qd_layout& L = c->lay;
    // exception lists of the streams -> one ascending list without duplicates (a pair short in both
    // index reads is redone once), indices beyond the batch dropped
    int64_t m = -1;
    if (n_short) {
        bool listed = true;
        for (int k = 0; k < L.n_streams; ++k) listed = listed && n_short[k] >= 0 && n_short[k] <= s.h.short_cap;
        if (listed) {
            const uint32_t* a = s.h.short_idx[0];
            const uint32_t* b = L.n_streams > 1 ? s.h.short_idx[1] : nullptr;
            int64_t na = n_short[0], nb = b ? n_short[1] : 0, i = 0, j = 0;
            m = 0;
            while (i < na || j < nb) {
                uint32_t v;
                if (j >= nb || (i < na && a[i] <= b[j])) {
                    v = a[i++];
                    if (j < nb && b[j] == v) ++j;
                } else {
                    v = b[j++];
                }
                if ((int64_t)v < n) s.h_short[m++] = v;
            }
            if (m == 0) has_len = 0;  // every short read lies beyond the batch
        }
    }
    // a listed minority on a fast-eligible plan: only their lengths travel, not the len rows (the generic
    // kernel, which reads a length per pair, gets the rows)
    const bool listed = has_len && m > 0 && m <= n / 2 && pick_kernel(c, false) == K_FAST;
    qd_rows rows{};
    for (int k = 0; k < L.n_streams; ++k) {
        HIPCHK(c, hipMemcpyAsync(s.d.seq[k], s.h.seq[k], (size_t)n * L.seq_stride[k], hipMemcpyHostToDevice, c->up_stream));
        HIPCHK(c, hipMemcpyAsync(s.d.qual[k], s.h.qual[k], (size_t)n * L.qual_stride[k], hipMemcpyHostToDevice, c->up_stream));
        rows.seq[k] = s.d.seq[k];
        rows.qual[k] = s.d.qual[k];
        if (has_len && !listed) {
            HIPCHK(c, hipMemcpyAsync(s.d.len[k], s.h.len[k], (size_t)n, hipMemcpyHostToDevice, c->up_stream));
            rows.len[k] = s.d.len[k];
        }
    }
    const uint8_t* dlen[2] = {nullptr, nullptr};
    if (listed) {
        const size_t cap2 = (size_t)s.h.short_cap * 2;
        uint8_t* hl = reinterpret_cast<uint8_t*>(s.h_short + cap2);
        uint8_t* dl = reinterpret_cast<uint8_t*>(s.d_short + cap2);
        for (int k = 0; k < L.n_streams; ++k) {
            for (int64_t i = 0; i < m; ++i) hl[k * cap2 + (size_t)i] = s.h.len[k][s.h_short[i]];
            dlen[k] = dl + k * cap2;
        }
        HIPCHK(c, hipMemcpyAsync(s.d_short, s.h_short, (size_t)m * 4, hipMemcpyHostToDevice, c->up_stream));
        for (int k = 0; k < L.n_streams; ++k)
            HIPCHK(c, hipMemcpyAsync(dl + k * cap2, hl + k * cap2, (size_t)m, hipMemcpyHostToDevice, c->up_stream));
    }
    HIPCHK(c, hipEventRecord(s.uploaded, c->up_stream));
    HIPCHK(c, hipStreamWaitEvent(s.stream, s.uploaded, 0));
    const int r = launch(c, n, &rows, s.d.codes, s.d.mol, s.stream, listed ? m : -1, s.d_short, listed ? dlen : nullptr);
    if (r != QD_OK) return r;
    HIPCHK(c, hipMemcpyAsync(s.h.codes, s.d.codes, (size_t)n * 2, hipMemcpyDeviceToHost, s.stream));
    if (L.mol_width)
        HIPCHK(c, hipMemcpyAsync(s.h.mol, s.d.mol, (size_t)n * L.mol_width, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(c, track(c, s.stream));
    return QD_OK;
}

int qd_submit(qd_ctx* c, int32_t slot, int64_t n, int32_t has_len) { return submit_impl(c, slot, n, has_len, nullptr); }

int qd_submit_ragged(qd_ctx* c, int32_t slot, int64_t n, const int64_t n_short[2]) {
    if (!n_short) return fail(c, QD_ERR_INVALID, "n_short is NULL");
    return submit_impl(c, slot, n, 1, n_short);
}

int qd_wait(qd_ctx* c, int32_t slot) {
    if (!c || slot < 0 || slot >= (int)c->slots.size()) return fail(c, QD_ERR_INVALID, "bad slot");
    Slot& s = c->slots[(size_t)slot];
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(s.stream));
    s.busy = false;
    return QD_OK;
}

}  // extern "C"

// ---- multi-GPU: the one exchange of the path --------------------------------------------------------
namespace {
struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
    bool ok = false;
    Rccl() {
        handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!handle) handle = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!handle) {
            why = std::string("librccl.so.1: ") + dlerror();
            return;
        }
#define QD_SYM(field, name) field = reinterpret_cast<decltype(field)>(dlsym(handle, name))
        QD_SYM(GetUniqueId, "ncclGetUniqueId");
        QD_SYM(CommInitRank, "ncclCommInitRank");
        QD_SYM(CommInitAll, "ncclCommInitAll");
        QD_SYM(CommDestroy, "ncclCommDestroy");
        QD_SYM(AllReduce, "ncclAllReduce");
        QD_SYM(GroupStart, "ncclGroupStart");
        QD_SYM(GroupEnd, "ncclGroupEnd");
        QD_SYM(GetErrorString, "ncclGetErrorString");
#undef QD_SYM
        ok = GetUniqueId && CommInitRank && CommInitAll && CommDestroy && AllReduce && GroupStart && GroupEnd && GetErrorString;
        if (!ok) why = "librccl.so.1 lacks an expected symbol";
    }
};
Rccl& rccl() {
    static Rccl R;
    return R;
}
thread_local std::string g_comm_error;
int comm_fail(int code, const std::string& msg) {
    g_comm_error = msg;
    return code;
}
}  // namespace

struct qd_comm {
    std::vector<qd_ctx*> ctxs;       // this process's member contexts (one per local device)
    std::vector<ncclComm_t> comms;   // their communicators
    int world = 0, rank0 = 0;        // ranks of the whole communicator; rank of ctxs[0]
};

extern "C" {

const char* qd_comm_last_error(void) { return g_comm_error.c_str(); }

int qd_comm_unique_id(uint8_t id[QD_UNIQUE_ID_BYTES]) {
    if (!id) return comm_fail(QD_ERR_INVALID, "id is NULL");
    Rccl& R = rccl();
    if (!R.ok) return comm_fail(QD_ERR_HIP, R.why);
    static_assert(QD_UNIQUE_ID_BYTES == sizeof(ncclUniqueId), "unique id size");
    ncclUniqueId u;
    const ncclResult_t r = R.GetUniqueId(&u);
    if (r != ncclSuccess) return comm_fail(QD_ERR_HIP, std::string("ncclGetUniqueId: ") + R.GetErrorString(r));
    memcpy(id, &u, sizeof u);
    return QD_OK;
}

int qd_comm_create_local(qd_ctx* const* ctxs, int32_t n, qd_comm** out) {
    if (!ctxs || n < 1 || !out) return comm_fail(QD_ERR_INVALID, "bad arguments");
    *out = nullptr;
    Rccl& R = rccl();
    if (!R.ok) return comm_fail(QD_ERR_HIP, R.why);
    std::vector<int> devs;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return comm_fail(QD_ERR_INVALID, "NULL context");
        for (int d : devs)
            if (d == ctxs[i]->device) return comm_fail(QD_ERR_INVALID, "two member contexts share a device (RCCL wants one rank per device)");
        devs.push_back(ctxs[i]->device);
    }
    std::unique_ptr<qd_comm> cm(new qd_comm());
    cm->ctxs.assign(ctxs, ctxs + n);
    cm->comms.resize((size_t)n);
    cm->world = n;
    const ncclResult_t r = R.CommInitAll(cm->comms.data(), n, devs.data());  // one process, the n local devices
    if (r != ncclSuccess) return comm_fail(QD_ERR_HIP, std::string("ncclCommInitAll: ") + R.GetErrorString(r));
    *out = cm.release();
    return QD_OK;
}

int qd_comm_create_rank(qd_ctx* ctx, int32_t world, int32_t rank, const uint8_t id[QD_UNIQUE_ID_BYTES], qd_comm** out) {
    if (!ctx || world < 1 || rank < 0 || rank >= world || !id || !out) return comm_fail(QD_ERR_INVALID, "bad arguments");
    *out = nullptr;
    Rccl& R = rccl();
    if (!R.ok) return comm_fail(QD_ERR_HIP, R.why);
    if (hipSetDevice(ctx->device) != hipSuccess) return comm_fail(QD_ERR_HIP, "hipSetDevice failed");
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    std::unique_ptr<qd_comm> cm(new qd_comm());
    cm->ctxs.push_back(ctx);
    cm->comms.resize(1);
    cm->world = world;
    cm->rank0 = rank;
    const ncclResult_t r = R.CommInitRank(&cm->comms[0], world, u, rank);  // one process per GPU
    if (r != ncclSuccess) return comm_fail(QD_ERR_HIP, std::string("ncclCommInitRank: ") + R.GetErrorString(r));
    *out = cm.release();
    return QD_OK;
}

int qd_comm_world(const qd_comm* cm) { return cm ? cm->world : QD_ERR_INVALID; }

int qd_reduce_counts(qd_comm* cm, uint64_t* out, int32_t n_values) {
    if (!cm || !out) return comm_fail(QD_ERR_INVALID, "bad arguments");
    Rccl& R = rccl();
    qd_ctx* c0 = cm->ctxs[0];
    if (!c0->have_table) return comm_fail(QD_ERR_STATE, "qd_set_barcodes first");
    if (n_values != 2 * c0->S + 4) return comm_fail(QD_ERR_INVALID, "n_values must be 2*S+4");
    for (qd_ctx* c : cm->ctxs) {
        if (!c->have_table || c->S != c0->S) return comm_fail(QD_ERR_STATE, "member contexts hold different sample tables");
        const int r = counts_to_device(c);  // every member's counters + TOTAL, summed on its own device
        if (r != QD_OK) return comm_fail(r, c->err);
    }
    // one all-reduce (sum, uint64) of 2S+1 counters + TOTAL over xGMI; latency-bound (<= 24.6 KB at S = 1536)
    const size_t count = (size_t)c0->cnt_stride + 1;
    ncclResult_t r = R.GroupStart();
    for (size_t i = 0; r == ncclSuccess && i < cm->ctxs.size(); ++i) {
        qd_ctx* c = cm->ctxs[i];
        if (hipSetDevice(c->device) != hipSuccess) return comm_fail(QD_ERR_HIP, "hipSetDevice failed");
        r = R.AllReduce(c->d_counts, c->d_total, count, ncclUint64, ncclSum, cm->comms[i], c->stream);
    }
    const ncclResult_t r2 = R.GroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
        return comm_fail(QD_ERR_HIP, std::string("ncclAllReduce: ") + R.GetErrorString(r != ncclSuccess ? r : r2));
    std::vector<u64> h(count);
    if (hipSetDevice(c0->device) != hipSuccess) return comm_fail(QD_ERR_HIP, "hipSetDevice failed");
    hipError_t e = hipMemcpyAsync(h.data(), c0->d_total, count * 8, hipMemcpyDeviceToHost, c0->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c0->stream);
    for (size_t i = 1; e == hipSuccess && i < cm->ctxs.size(); ++i) {  // every member's collective has completed on return
        if (hipSetDevice(cm->ctxs[i]->device) != hipSuccess) return comm_fail(QD_ERR_HIP, "hipSetDevice failed");
        e = hipStreamSynchronize(cm->ctxs[i]->stream);
    }
    if (e != hipSuccess) return comm_fail(QD_ERR_HIP, std::string("count reduce: ") + hipGetErrorString(e));
    compose_counts(c0, h.data(), out);
    return QD_OK;
}

int qd_comm_destroy(qd_comm* cm) {
    if (!cm) return QD_OK;
    Rccl& R = rccl();
    for (size_t i = 0; i < cm->comms.size(); ++i) {
        (void)hipSetDevice(cm->ctxs[i]->device);
        if (R.ok && cm->comms[i]) (void)R.CommDestroy(cm->comms[i]);
    }
    delete cm;
    return QD_OK;
}

}  // extern "C"

// ---- BGZF inflate on the device (include/quade_hip.h; kernel: quade_inflate.hip) ------------------------------
uint32_t qd_io_crc32(const uint8_t* p, size_t n);  // quade_io.cpp: libdeflate's when loaded, else zlib's

struct __attribute__((visibility("hidden"))) qd_inflater {  // (hidden: its destructor is no symbol of the library)
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;  // blocking-sync event: the calling thread sleeps while the device works
    std::string err;
    // grow-only staging: pinned host + device, for the compressed run, its text, the block table and the states
    qbuf::Pair<uint8_t> comp, out;
    qbuf::Pair<qd_inflate_block> blk;
    qbuf::Pair<int32_t> st;
    std::vector<uint32_t> crc;
    // which kernel: 3 (the default, below), 2 = 512 lanes per block, 1 = one wave per block (QUADE_INFLATE_FORM / qd_inflater_set_form); the second form's match lists
    int form = 3;
    DevArr<unsigned long long> d_matches;  // QD_INFLATE_MATCHES_PER_BLOCK per block
    // the third form (3: one lane decodes a block's symbols once, a workgroup resolves its tokens -- quade_inflate3.hip): its scratch
    DevArr<uint8_t> d_scratch3;
};

namespace {
int inf_fail(qd_inflater* f, int code, const std::string& msg) {
    if (f) f->err = msg;
    return code;
}
#define INFCHK(f, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return inf_fail((f), QD_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// the stand-alone coders' staging pairs grow to n + n/4 + 4096 elements
template <class T>
hipError_t need_pair(qbuf::Pair<T>& b, size_t n) {
    return b.need(n, qbuf::quarter(n, 4096));
}
thread_local std::string g_inflater_error;

// quade_buf.h's wait with naps of 100 us
hipError_t wait_event_napping(hipEvent_t ev) {
    static const int nap_us = [] {
        const char* e = getenv("QUADE_NAP_US");  // measurement knob
        const int v = e && *e ? atoi(e) : 100;
        return v < 10 ? 10 : (v > 5000 ? 5000 : v);
    }();
    return qbuf::wait_event_napping(ev, (unsigned)nap_us);
}
// The first n blocks of f->blk.d (states to f->st.d) through the speculative spans (form 2) when that form is allowed and the longest
// payload leaves its workgroup room in 160 KB of LDS -- beyond ~52 KB, stored blocks, it does not -- else a wave per block (form 1).
int inflate_spans_or_wave(qd_inflater* f, uint32_t n, uint32_t longest, bool spans_allowed) {
    if (!spans_allowed || qd_inflate2_lds(longest) > 160 * 1024) {
        INFCHK(f, qd_launch_inflate(f->comp.d, f->blk.d, n, f->out.d, f->st.d, f->stream));
        return QD_OK;
    }
    const size_t per_block = (size_t)QD_INFLATE_MATCHES_PER_BLOCK * 8;
    INFCHK(f, f->d_matches.need(n * per_block, qbuf::quarter(n, 16) * per_block));
    static const bool debug_rounds = getenv("QUADE_INFLATE_DEBUG") != nullptr;  // measurement: rounds per block on stderr
    DevArr<uint32_t> d_rounds;
    if (debug_rounds) INFCHK(f, d_rounds.alloc((size_t)n * 32));
    INFCHK(f, qd_launch_inflate2(f->comp.d, f->blk.d, n, f->out.d, f->st.d, f->d_matches, QD_INFLATE_MATCHES_PER_BLOCK, longest,
                                 f->stream, d_rounds));
    if (debug_rounds) {
        std::vector<uint32_t> r((size_t)n * 8);
        INFCHK(f, hipMemcpy(r.data(), d_rounds, (size_t)n * 32, hipMemcpyDeviceToHost));
        uint64_t sum = 0, db = 0, tk[8] = {0};
        uint32_t mx = 0, over8 = 0;
        for (size_t q = 0; q < n; ++q) {
            const uint32_t v = r[8 * q];
            sum += v & 0xFFFF;
            db += v >> 16;
            mx = std::max(mx, v & 0xFFFF);
            over8 += (v & 0xFFFF) > 8;
            for (int k = 1; k < 8; ++k) tk[k] += r[8 * q + k];
        }
        const double us = 0.01 / (double)n;  // 100 MHz ticks -> microseconds per block
        fprintf(stderr, "[inflate form 2] %u blocks: %.2f rounds and %.2f deflate blocks per block, most %u, %u blocks over 8 rounds; us per block: stage %.0f "
                        "header+tables %.0f rounds %.0f scan+write %.0f matches %.0f flush %.0f; %.0f matches per block\n", n, (double)sum / n,
                (double)db / n, mx, over8, tk[1] * us, tk[2] * us, tk[3] * us, tk[4] * us, tk[5] * us, tk[6] * us, (double)tk[7] / n);
    }
    return QD_OK;
}
}  // namespace

extern "C" {

int qd_inflater_create(int device_id, qd_inflater** out) {
    if (!out) return QD_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) {
        g_inflater_error = "no such HIP device";
        return QD_ERR_NO_DEVICE;
    }
    qd_inflater* f = new qd_inflater();
    f->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&f->done, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) {
        g_inflater_error = "hipStreamCreate failed";
        delete f;
        return QD_ERR_HIP;
    }
    if (const char* e = getenv("QUADE_INFLATE_FORM")) f->form = atoi(e) == 1 ? 1 : (atoi(e) == 2 ? 2 : 3);
    *out = f;
    return QD_OK;
}

const char* qd_inflater_last_error(const qd_inflater* f) { return f ? f->err.c_str() : g_inflater_error.c_str(); }

int qd_inflater_destroy(qd_inflater* f) {
    if (!f) return QD_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) {
        (void)hipStreamSynchronize(f->stream);
        (void)hipStreamDestroy(f->stream);
    }
    if (f->done) (void)hipEventDestroy(f->done);
    delete f;
    return QD_OK;
}

int qd_inflater_set_form(qd_inflater* f, int32_t form) {
    if (!f || form < 1 || form > 3) return QD_ERR_INVALID;
    f->form = form;
    return QD_OK;
}

// page-locked host memory for callers that want the text to land in their buffer without a staging copy
void* qd_pinned_alloc(int64_t bytes) {
    void* p = nullptr;
    if (bytes <= 0 || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void qd_pinned_free(void* p) {
    if (p) (void)hipHostFree(p);
}

static int inflater_run(qd_inflater* f, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_len, int32_t* bad_block,
                        bool out_pinned);
int qd_inflater_run(qd_inflater* f, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_len, int32_t* bad_block) {
    return inflater_run(f, comp, comp_len, out, out_len, bad_block, false);
}
int qd_inflater_run_pinned(qd_inflater* f, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_len, int32_t* bad_block) {
    return inflater_run(f, comp, comp_len, out, out_len, bad_block, true);
}

static int inflater_run(qd_inflater* f, const uint8_t* comp, int64_t comp_len, uint8_t* out, int64_t out_len, int32_t* bad_block,
                        bool out_pinned) {
    if (bad_block) *bad_block = -1;
    if (!f || !comp || comp_len < 0 || out_len < 0 || (out_len > 0 && !out)) return inf_fail(f, QD_ERR_INVALID, "bad arguments");
    if (comp_len > (int64_t)0xFFFF0000ll || out_len > (int64_t)0xFFFF0000ll) return inf_fail(f, QD_ERR_INVALID, "run larger than 4 GiB");
    // 1. walk the block headers: gzip member with the 'BC' extra subfield = total block size - 1
    std::vector<qd_inflate_block> blk;
    f->crc.clear();
    size_t pos = 0, opos = 0;
    while (pos < (size_t)comp_len) {
        const gzf::BgzfBlock b = gzf::bgzf_block(comp + pos, (size_t)comp_len - pos);
        if (!b.framed()) return inf_fail(f, QD_ERR_FORMAT, "not a run of whole BGZF blocks");  // (other gzip flags -- name, comment, hcrc: not bgzip's)
        if (!b.is_bgzip_layout() || opos + b.isize > (size_t)out_len) return inf_fail(f, QD_ERR_FORMAT, "BGZF block sizes do not add up");
        blk.push_back(qd_inflate_block{(uint32_t)(pos + b.payload_off), (uint32_t)b.payload_len, (uint32_t)opos, b.isize});
        f->crc.push_back(b.crc);
        pos += b.bsize;
        opos += b.isize;
    }
    if (opos != (size_t)out_len) return inf_fail(f, QD_ERR_FORMAT, "BGZF block sizes do not add up");
    if (blk.empty()) return QD_OK;
    // 2. stage, inflate one block per lane, fetch
    INFCHK(f, hipSetDevice(f->device));
    INFCHK(f, need_pair(f->comp, (size_t)comp_len));
    INFCHK(f, need_pair(f->out, (size_t)out_len + 16));
    uint8_t* const text = out_pinned ? out : f->out.h;  // where the D2H copy lands
    INFCHK(f, need_pair(f->blk, blk.size()));
    INFCHK(f, need_pair(f->st, blk.size()));
    memcpy(f->comp.h, comp, (size_t)comp_len);
    memcpy(f->blk.h, blk.data(), blk.size() * sizeof(qd_inflate_block));
    INFCHK(f, hipMemcpyAsync(f->comp.d, f->comp.h, (size_t)comp_len, hipMemcpyHostToDevice, f->stream));
    INFCHK(f, hipMemcpyAsync(f->blk.d, f->blk.h, blk.size() * sizeof(qd_inflate_block), hipMemcpyHostToDevice, f->stream));
    uint32_t longest = 0;
    for (const qd_inflate_block& bk : blk) longest = std::max(longest, bk.in_len);
    bool form3_ran = false;
    if (f->form == 3) {
        const size_t need = qd_inflate3_scratch_bytes((uint32_t)blk.size());
        INFCHK(f, f->d_scratch3.need(need, qbuf::quarter(need, 0)));
        INFCHK(f, qd_launch_inflate3(f->comp.d, (size_t)comp_len, f->blk.d, (uint32_t)blk.size(), f->out.d, f->st.d, f->d_scratch3, f->stream));
        form3_ran = true;
    } else {
        const int rc = inflate_spans_or_wave(f, (uint32_t)blk.size(), longest, f->form == 2);
        if (rc != QD_OK) return rc;
    }
    INFCHK(f, hipMemcpyAsync(f->st.h, f->st.d, blk.size() * 4, hipMemcpyDeviceToHost, f->stream));
    if (form3_ran) {
        // blocks whose Huffman codes hold more long symbols than a lane's table takes (byte soup, not fastq) go through the second
        // form -- or the first, when their payload leaves no room for it: a second launch over just those blocks
        INFCHK(f, hipEventRecord(f->done, f->stream));
        INFCHK(f, wait_event_napping(f->done));
        std::vector<qd_inflate_block> redo;
        std::vector<size_t> redo_at;
        uint32_t redo_longest = 0;
        for (size_t i = 0; i < blk.size(); ++i)
            if (f->st.h[i] == QD_INFLATE_TABLE_SPACE) {
                redo.push_back(blk[i]);
                redo_at.push_back(i);
                redo_longest = std::max(redo_longest, blk[i].in_len);
            }
        if (!redo.empty()) {
            // (the first launch is done with the block table and has handed its states over: the redo's go through the same buffers)
            memcpy(f->blk.h, redo.data(), redo.size() * sizeof(qd_inflate_block));
            INFCHK(f, hipMemcpyAsync(f->blk.d, f->blk.h, redo.size() * sizeof(qd_inflate_block), hipMemcpyHostToDevice, f->stream));
            const int rc = inflate_spans_or_wave(f, (uint32_t)redo.size(), redo_longest, true);
            if (rc != QD_OK) return rc;
            std::vector<int32_t> rst(redo.size());
            INFCHK(f, hipMemcpyAsync(rst.data(), f->st.d, redo.size() * 4, hipMemcpyDeviceToHost, f->stream));
            INFCHK(f, hipStreamSynchronize(f->stream));
            for (size_t k = 0; k < redo.size(); ++k) f->st.h[redo_at[k]] = rst[k];
        }
    }
    if (out_len) INFCHK(f, hipMemcpyAsync(text, f->out.d, (size_t)out_len, hipMemcpyDeviceToHost, f->stream));
    INFCHK(f, hipEventRecord(f->done, f->stream));
    INFCHK(f, wait_event_napping(f->done));
    if (f->form != 1) {
        // The second form's match list holds QD_INFLATE_MATCHES_PER_BLOCK matches; a block with more (GNU gzip -1 makes 16 000 of 64 KiB
        // of fastq) comes back as QD_INFLATE_OVERRUN, like one whose codes stand for more text than its ISIZE.  The one-wave form has no
        // such list and tells the two apart: a launch over just those blocks.
        std::vector<qd_inflate_block> redo;
        std::vector<size_t> redo_at;
        for (size_t i = 0; i < blk.size(); ++i)
            if (f->st.h[i] == QD_INFLATE_OVERRUN) {
                redo.push_back(blk[i]);
                redo_at.push_back(i);
            }
        if (!redo.empty()) {
            memcpy(f->blk.h, redo.data(), redo.size() * sizeof(qd_inflate_block));
            INFCHK(f, hipMemcpyAsync(f->blk.d, f->blk.h, redo.size() * sizeof(qd_inflate_block), hipMemcpyHostToDevice, f->stream));
            INFCHK(f, qd_launch_inflate(f->comp.d, f->blk.d, (uint32_t)redo.size(), f->out.d, f->st.d, f->stream));
            std::vector<int32_t> rst(redo.size());
            INFCHK(f, hipMemcpyAsync(rst.data(), f->st.d, redo.size() * 4, hipMemcpyDeviceToHost, f->stream));
            for (const qd_inflate_block& b : redo)
                if (b.out_len) INFCHK(f, hipMemcpyAsync(text + b.out_off, f->out.d + b.out_off, b.out_len, hipMemcpyDeviceToHost, f->stream));
            INFCHK(f, hipStreamSynchronize(f->stream));
            for (size_t k = 0; k < redo.size(); ++k) f->st.h[redo_at[k]] = rst[k];
        }
    }
    // 3. every block: decoder status, then the CRC32 of its text
    for (size_t i = 0; i < blk.size(); ++i) {
        if (f->st.h[i] != 0 || qd_io_crc32(text + blk[i].out_off, blk[i].out_len) != f->crc[i]) {
            if (bad_block) *bad_block = (int32_t)i;
            char m[128];
            if (f->st.h[i])
                snprintf(m, sizeof m, "BGZF block %zu: did not inflate (decoder status %d)", i, (int)f->st.h[i]);
            else
                snprintf(m, sizeof m, "BGZF block %zu: CRC32 mismatch", i);
            return inf_fail(f, QD_ERR_FORMAT, m);
        }
    }
    if (!out_pinned) memcpy(out, f->out.h, (size_t)out_len);
    return QD_OK;
}

}  // extern "C"

// ---- Huffman-only gzip members on the device (include/quade_hip.h; kernel: quade_deflate.hip) -------------------------
struct __attribute__((visibility("hidden"))) qd_deflater {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    std::string err;
    // grow-only staging: pinned host + device, for the text, the members, the piece table and the member lengths
    PinArr<uint8_t> h_text;  // (only for pageable callers, and then as large as d_text)
    DevArr<uint8_t> d_text;
    qbuf::Pair<uint8_t> out;
    qbuf::Pair<qd_deflate_piece> pc;
    qbuf::Pair<uint32_t> len;
    // level 1 (LZ77 + dynamic Huffman, quade_deflate.hip): sub-block table, piece -> first sub-block, device scratch
    int level = -1;
    qbuf::Pair<qd_lz_sub> sub;
    qbuf::Pair<uint32_t> first;
    DevArr<uint32_t> d_tokens, d_sub_bytes;  // these and the next two hold the same number of sub-blocks
    DevArr<uint8_t> d_sub_out;
    // crc32 == NULL at level 1: the sub-blocks' CRC-32s out of the coder, their lengths for the combine
    DevArr<uint32_t> d_sub_crc;
    qbuf::Pair<qd_crc_range> rg;
};

namespace {
thread_local std::string g_deflater_error;
// The coder's launches are short (2 ms per 64 MB) and everything downstream waits for them: its stream gets the device's
// highest priority, so that its workgroups are placed before those of long-running kernels that share the GPU (the BGZF
// inflater's launches hold their CUs for ~16 ms).
hipError_t make_priority_stream(hipStream_t* st) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest);
}
int def_fail(qd_deflater* f, int code, const std::string& msg) {
    if (f) f->err = msg;
    else g_deflater_error = msg;
    return code;
}
#define DEFCHK(f, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return def_fail((f), QD_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
}  // namespace

extern "C" {

int64_t qd_huffman_member_bound(int64_t text_len) {
    return bsz::huffman_member_bound(text_len);  // (the formula and its reasons: batch_sizes.h)
}

int qd_deflater_create(int device_id, qd_deflater** out) {
    if (!out) return QD_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return def_fail(nullptr, QD_ERR_NO_DEVICE, "no such HIP device");
    qd_deflater* f = new qd_deflater();
    f->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || make_priority_stream(&f->stream) != hipSuccess ||
        hipEventCreateWithFlags(&f->done, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) {
        delete f;
        return def_fail(nullptr, QD_ERR_HIP, "hipStreamCreate failed");
    }
    *out = f;
    return QD_OK;
}

const char* qd_deflater_last_error(const qd_deflater* f) { return f ? f->err.c_str() : g_deflater_error.c_str(); }

int qd_deflater_destroy(qd_deflater* f) {
    if (!f) return QD_OK;
    (void)hipSetDevice(f->device);
    if (f->stream) {
        (void)hipStreamSynchronize(f->stream);
        (void)hipStreamDestroy(f->stream);
    }
    if (f->done) (void)hipEventDestroy(f->done);
    delete f;
    return QD_OK;
}

int qd_deflater_set_level(qd_deflater* f, int32_t level) {
    if (!f || (level != -1 && level != 1)) return def_fail(f, QD_ERR_INVALID, "the device makes members at gzip_level -1 (Huffman only) and 1 (LZ77 + Huffman)");
    f->level = level;
    return QD_OK;
}

int qd_deflater_run(qd_deflater* f, int32_t n_pieces, const uint8_t* const* text, const int64_t* text_len, const uint32_t* crc32,
                    int32_t text_pinned, uint8_t* out, int64_t out_stride, int64_t* member_len) {
    if (!f || n_pieces < 0 || (n_pieces && (!text || !text_len || !out || !member_len)) || out_stride < 64 || (out_stride & 3))
        return def_fail(f, QD_ERR_INVALID, "bad arguments");
    if (n_pieces == 0) return QD_OK;
    if (!crc32 && f->level != 1) return def_fail(f, QD_ERR_INVALID, "only the level-1 coder makes the members' CRC-32s itself");
    size_t total = 0;
    for (int i = 0; i < n_pieces; ++i) {
        if (text_len[i] < 0 || text_len[i] > (int64_t)0x7FFFFFFF || (text_len[i] && !text[i])) return def_fail(f, QD_ERR_INVALID, "bad piece");
        total += ((size_t)text_len[i] + 15) & ~(size_t)15;
    }
    DEFCHK(f, hipSetDevice(f->device));
    DEFCHK(f, need_pair(f->pc, (size_t)n_pieces));
    DEFCHK(f, need_pair(f->len, (size_t)n_pieces));
    DEFCHK(f, need_pair(f->out, (size_t)n_pieces * (size_t)out_stride));
    // device text always; the pinned staging copy only for pageable callers, and as large as the device text
    if (total + 16 > f->d_text.cap) f->h_text.release();
    DEFCHK(f, f->d_text.need(total + 16, qbuf::quarter(total, 4096)));
    if (!text_pinned && !f->h_text) DEFCHK(f, f->h_text.alloc(f->d_text.cap));
    size_t at = 0;
    for (int i = 0; i < n_pieces; ++i) {
        f->pc.h[i] = qd_deflate_piece{(uint64_t)at, (uint32_t)text_len[i], crc32 ? crc32[i] : 0u};
        if (text_len[i]) {
            const uint8_t* src = text[i];
            if (!text_pinned) {
                memcpy(f->h_text + at, text[i], (size_t)text_len[i]);
                src = f->h_text + at;
            }
            DEFCHK(f, hipMemcpyAsync(f->d_text + at, src, (size_t)text_len[i], hipMemcpyHostToDevice, f->stream));
        }
        at += ((size_t)text_len[i] + 15) & ~(size_t)15;
    }
    DEFCHK(f, hipMemcpyAsync(f->pc.d, f->pc.h, (size_t)n_pieces * sizeof(qd_deflate_piece), hipMemcpyHostToDevice, f->stream));
    if (f->level == 1) {  // LZ77 + dynamic Huffman: one workgroup per 64 KiB sub-block, then the members are strung together
        size_t n_subs = 0;
        for (int i = 0; i < n_pieces; ++i) n_subs += outplan::subs_of((uint64_t)text_len[i]);
        const int64_t sub_stride = qd_huffman_member_bound(QD_LZ_SUB);
        DEFCHK(f, need_pair(f->sub, n_subs + 1));
        DEFCHK(f, need_pair(f->first, (size_t)n_pieces + 1));
        const size_t grown = qbuf::quarter(n_subs, 16);  // sub-blocks the four scratch arrays hold behind a growth
        DEFCHK(f, f->d_tokens.need(n_subs * (size_t)QD_LZ_SUB * 4, grown * (size_t)QD_LZ_SUB * 4));
        DEFCHK(f, f->d_sub_bytes.need(n_subs * 4, grown * 4));
        DEFCHK(f, f->d_sub_out.need(n_subs * (size_t)sub_stride, grown * (size_t)sub_stride));
        DEFCHK(f, f->d_sub_crc.need(n_subs * 4, grown * 4));
        if (!crc32) DEFCHK(f, need_pair(f->rg, n_subs + 1));  // (the sub-blocks' CRC-32s out of the coder: their ranges for the combine)
        size_t js = 0;
        for (int i = 0; i < n_pieces; ++i) {  // the pieces' sub-blocks, cut as the pipeline cuts them (out_plan.h)
            f->first.h[i] = (uint32_t)js;
            outplan::cut_piece(f->pc.h[i].text_off, f->pc.h[i].text_len, (uint32_t)i, [&](const qd_lz_sub& s, const qd_crc_range& r) {
                if (!crc32) f->rg.h[js] = r;
                f->sub.h[js++] = s;
            });
        }
        f->first.h[n_pieces] = (uint32_t)js;
        if (js) DEFCHK(f, hipMemcpyAsync(f->sub.d, f->sub.h, js * sizeof(qd_lz_sub), hipMemcpyHostToDevice, f->stream));
        DEFCHK(f, hipMemcpyAsync(f->first.d, f->first.h, ((size_t)n_pieces + 1) * 4, hipMemcpyHostToDevice, f->stream));
        if (crc32) {
            DEFCHK(f, qd_launch_lz(f->d_text, f->pc.d, (uint32_t)n_pieces, f->sub.d, f->first.d, (uint32_t)js, f->d_tokens, f->d_sub_out, sub_stride,
                                   f->d_sub_bytes, f->out.d, out_stride, f->len.d, f->stream));
        } else {  // as the pipeline (quade_pipe.cpp): the sub-blocks' CRC-32s out of the coder, combined per piece into the piece table
            static_assert(sizeof(qd_deflate_piece) == 16 && offsetof(qd_deflate_piece, crc32) == 12, "the combined CRCs land in the piece table");
            if (js) DEFCHK(f, hipMemcpyAsync(f->rg.d, f->rg.h, js * sizeof(qd_crc_range), hipMemcpyHostToDevice, f->stream));
            DEFCHK(f, qd_launch_lz_subblocks(f->d_text, f->sub.d, (uint32_t)js, f->d_tokens, f->d_sub_out, sub_stride, f->d_sub_bytes, f->d_sub_crc, f->stream));
            DEFCHK(f, qd_text_crc32_combine(f->rg.d, f->d_sub_crc, f->first.d, (uint32_t)n_pieces, f->pc.d.as<uint32_t>() + 3, 4, f->stream));
            DEFCHK(f, qd_launch_lz_members(f->pc.d, (uint32_t)n_pieces, f->sub.d, f->first.d, (uint32_t)js, f->d_sub_out, sub_stride, f->d_sub_bytes,
                                           f->out.d, out_stride, f->len.d, f->stream));
        }
    } else {
        DEFCHK(f, qd_launch_huffman(f->d_text, f->pc.d, (uint32_t)n_pieces, f->out.d, out_stride, f->len.d, f->stream));
    }
    DEFCHK(f, hipMemcpyAsync(f->len.h, f->len.d, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, f->stream));
    DEFCHK(f, hipEventRecord(f->done, f->stream));
    DEFCHK(f, wait_event_napping(f->done));
    for (int i = 0; i < n_pieces; ++i) {  // the used bytes of every member
        if (f->len.h[i] > (uint64_t)out_stride) return def_fail(f, QD_ERR_HIP, "member longer than its slot");
        if (f->len.h[i])
            DEFCHK(f, hipMemcpyAsync(f->out.h + (size_t)i * (size_t)out_stride, f->out.d + (size_t)i * (size_t)out_stride, f->len.h[i],
                                     hipMemcpyDeviceToHost, f->stream));
    }
    DEFCHK(f, hipEventRecord(f->done, f->stream));
    DEFCHK(f, wait_event_napping(f->done));
    for (int i = 0; i < n_pieces; ++i) {
        member_len[i] = f->len.h[i];  // 0: this member did not fit out_stride (the caller makes it itself)
        if (f->len.h[i]) memcpy(out + (size_t)i * (size_t)out_stride, f->out.h + (size_t)i * (size_t)out_stride, f->len.h[i]);
    }
    return QD_OK;
}

}  // extern "C"

// ---- a whole gzip file image through the device's gzip inflater (include/quade_hip.h: qd_dev_gunzip) -----------------------------------
extern "C" int qd_dev_gunzip(int device_id, const uint8_t* gz, int64_t gz_len, uint8_t* out, int64_t out_cap, int64_t* out_len, int64_t step_bytes,
                             int64_t stretch_bytes, int64_t unit_text, int64_t* stats) {
    if (!gz || gz_len < 0 || !out_len || (out_cap > 0 && !out) || step_bytes < 4096) return QD_ERR_INVALID;
    *out_len = 0;
    if (hipSetDevice(device_id) != hipSuccess) return QD_ERR_NO_DEVICE;
    hipStream_t st = nullptr;
    DevArr<uint8_t> d_gz, d_out, d_win;  // (freed on return: done() has drained the stream by then)
    int rc = QD_OK;
    qd_gz G;
    if (stretch_bytes > 0) G.stretch_bytes = (uint64_t)stretch_bytes;
    if (unit_text > 0) G.unit_text = (uint64_t)unit_text, G.unit_text_given = true;
    int64_t members = 0, steps_run = 0;
    auto done = [&](int code) {
        if (st) (void)hipStreamSynchronize(st);
        if (st) (void)hipStreamDestroy(st);
        if (stats) {
            const qd_gz_stats s = G.stats();
            stats[0] = members;
            stats[1] = steps_run;
            stats[2] = s.stretches;
            stats[3] = s.units;
            stats[4] = s.chain_retries;
            stats[5] = s.partial_last;
            stats[6] = s.plain_probes;
            stats[7] = 0;
        }
        return code;
    };
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return done(QD_ERR_HIP);
    if (d_gz.alloc((size_t)gz_len + 4096) != hipSuccess || d_out.alloc((size_t)std::max<int64_t>(out_cap, 1) + 4096) != hipSuccess ||
        d_win.alloc(32768) != hipSuccess)
        return done(QD_ERR_HIP);
    if (hipMemset(d_gz + gz_len, 0, 4096) != hipSuccess || (gz_len && hipMemcpy(d_gz, gz, (size_t)gz_len, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemset(d_win, 0, 32768) != hipSuccess)
        return done(QD_ERR_HIP);
    gzf::MemberWalk walk;  // the whole image is on hand: comp_off 0, comp_len gz_len
    int64_t opos = 0;      // text so far
    while ((int64_t)walk.hdr_off < gz_len && rc == QD_OK) {
        // (zero padding behind the last member is refused here, unlike the readers: DESIGN.md 7.1)
        const int64_t hb = gzf::gzip_header_len(gz + walk.hdr_off, (size_t)gz_len - walk.hdr_off);
        if (hb <= 0) {
            rc = QD_ERR_FORMAT;
            break;
        }
        walk.begin((uint64_t)hb);
        qd_gz_step s{};
        s.carried = d_win;
        s.carried_valid = 0;
        int64_t step = step_bytes;
        bool ended = false;
        while (!ended) {
            const gzf::MemberWalk::Window win = walk.window(0, (uint64_t)gz_len, (uint64_t)step);
            s.comp = d_gz + win.byte0;
            s.comp_bytes = win.comp_bytes;
            s.bit_start = win.bit_start;
            s.at_end = win.byte0 + win.comp_bytes >= (uint64_t)gz_len;
            if (G.decode(&s, 1, st) != hipSuccess) return done(QD_ERR_HIP);
            ++steps_run;
            if (s.failed) {
                rc = QD_ERR_FORMAT;
                break;
            }
            if (walk.stalled(s)) {  // a block longer than the step: more input, if there is any
                if (s.at_end) {
                    rc = QD_ERR_FORMAT;
                    break;
                }
                step *= 2;
                continue;
            }
            if (opos + (int64_t)s.text_len > out_cap) {
                rc = QD_ERR_INVALID;
                break;
            }
            uint8_t* dst = d_out + opos;
            if (G.resolve(&s, 1, &dst, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess || G.finish(&s, 1) != hipSuccess) return done(QD_ERR_HIP);
            if (s.failed) {
                rc = QD_ERR_FORMAT;
                break;
            }
            walk.account(s, win);
            opos += (int64_t)s.text_len;
            ended = s.member_end != 0;
        }
        if (rc != QD_OK) break;
        if (!walk.trailer_inside((uint64_t)gz_len)) {
            rc = QD_ERR_FORMAT;
            break;
        }
        const uint64_t tr = walk.trailer_off();
        const gzf::MemberWalk::Trailer t = walk.end_member(gz + tr);  // CRC-32 and ISIZE of the member's text
        if (!t.ok) {
            if (getenv("QUADE_GZ_DEBUG")) fprintf(stderr, "[qd_dev_gunzip] trailer at %lld: crc %08x (text's %08x), isize %u (text %llu)\n", (long long)tr, t.crc, walk.crc, t.isize, (unsigned long long)walk.text);
            rc = QD_ERR_FORMAT;
            break;
        }
        ++members;
    }
    if (rc == QD_OK && opos && hipMemcpy(out, d_out, (size_t)opos, hipMemcpyDeviceToHost) != hipSuccess) rc = QD_ERR_HIP;
    if (rc == QD_OK) *out_len = opos;
    return done(rc);
}
