// Host-side checks of the feeder's cut (quade_amd/csrc/feed_cut.h): which BGZF blocks go into which segment, what is carried into the
// next buffer, where the host's text path takes over, the split at the text cap, and what a file's first buffer is -- on streams of
// small blocks made here with zlib's raw deflate, cut with buffers of a few hundred bytes, every result held against the file's own
// bytes.  fill_and_cut() stands in for the feeder's loop (Feeder::feed_bgzf): it reads as the feeder reads, and every buffer reaches the
// cutter in a heap block of exactly its length.  Built and run by tests/test_host_feed_cut.py, plain and under ASan + UBSan (no GPU).
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../quade_amd/csrc/feed_cut.h"

static int fails = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            if (++fails <= 40) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                     \
    } while (0)

typedef std::vector<uint8_t> Bytes;
static void put16(Bytes& b, uint32_t v) { b.push_back((uint8_t)v), b.push_back((uint8_t)(v >> 8)); }
static void put32(Bytes& b, uint32_t v) { put16(b, v & 0xffff), put16(b, v >> 16); }
static void append(Bytes& to, const Bytes& b) { to.insert(to.end(), b.begin(), b.end()); }
static uint32_t rnd_state = 12345;
static uint32_t rnd(uint32_t n) {
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return (rnd_state >> 8) % n;
}

static Bytes deflate_raw(const std::string& text) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    Bytes out(deflateBound(&z, (uLong)text.size()) + 16);
    z.next_in = (Bytef*)text.data();
    z.avail_in = (uInt)text.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) abort();
    out.resize(out.size() - z.avail_out);
    deflateEnd(&z);
    return out;
}
static bool inflate_raw(const uint8_t* p, size_t n, size_t want, std::string* text) {
    text->assign(want + 1, '\0');  // (room for one byte too many: a payload that holds more text is seen)
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) abort();
    z.next_in = (Bytef*)p;
    z.avail_in = (uInt)n;
    z.next_out = (Bytef*)&(*text)[0];
    z.avail_out = (uInt)text->size();
    const int rc = inflate(&z, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && z.avail_in == 0 && z.total_out == want;
    inflateEnd(&z);
    text->resize(want);
    return ok;
}

// ---- streams of blocks ------------------------------------------------------------------------------------------------------------------
struct Block {
    size_t off, size, payload_off, payload_len, xlen;  // in the file; payload_off from the block's start
    size_t text_off, text_len;
    uint32_t crc;
};
struct Stream {
    Bytes file;
    std::string text;
    std::vector<Block> blocks;
    size_t largest = 0;
};
// one block: `before` bytes of a 'ZZ' subfield in front of 'BC' (0: 'BC' first); deflate = false: no payload at all (26 bytes, no text)
static Bytes bgzf_block(const std::string& text, size_t before, bool deflate = true, int flg = 4, int64_t isize = -1) {
    const Bytes payload = deflate ? deflate_raw(text) : Bytes();
    Bytes x;
    if (before) {
        x.push_back('Z'), x.push_back('Z');
        put16(x, (uint32_t)before);
        for (size_t i = 0; i < before; ++i) x.push_back((uint8_t)(i % 3 == 0 ? 0x1f : i % 3 == 1 ? 0x8b : 8));  // (looks like magic all over)
    }
    x.push_back('B'), x.push_back('C');
    put16(x, 2);
    const size_t name = flg & 8 ? 2 : 0;
    put16(x, (uint32_t)(12 + x.size() + 2 + name + payload.size() + 8 - 1));
    Bytes b = {0x1f, 0x8b, 8, (uint8_t)flg, 0, 0, 0, 0, 0, 0xff};
    put16(b, (uint32_t)x.size());
    append(b, x);
    if (name) b.push_back('n'), b.push_back(0);
    append(b, payload);
    put32(b, (uint32_t)crc32(crc32(0, nullptr, 0), (const Bytef*)text.data(), (uInt)text.size()));
    put32(b, isize < 0 ? (uint32_t)text.size() : (uint32_t)isize);
    return b;
}
static void add_block(Stream& s, const std::string& text, size_t before, bool deflate = true) {
    const Bytes b = bgzf_block(text, before, deflate);
    Block k;
    k.off = s.file.size();
    k.size = b.size();
    k.xlen = (before ? 4 + before : 0) + 6;
    k.payload_off = 12 + k.xlen;
    k.payload_len = b.size() - k.payload_off - 8;
    k.text_off = s.text.size();
    k.text_len = text.size();
    k.crc = (uint32_t)crc32(crc32(0, nullptr, 0), (const Bytef*)text.data(), (uInt)text.size());
    s.blocks.push_back(k);
    append(s.file, b);
    s.text += text;
    s.largest = std::max(s.largest, b.size());
}
static std::string bases(size_t n) {
    std::string t(n, 'A');
    for (char& c : t) c = "ACGTN\n"[rnd(6)];
    return t;
}
// a few dozen blocks of 26 to ~300 bytes; every fourth with a long extra field in front of 'BC'
static Stream mixed_stream(int n_blocks) {
    Stream s;
    for (int i = 0; i < n_blocks; ++i) {
        if (i == 3 || i == n_blocks - 2) add_block(s, "", 0, false);  // 26 bytes
        else if (i == 5) add_block(s, "", 0);                        // 28 bytes: what bgzip ends a file with
        else add_block(s, bases(1 + rnd(600)), i % 4 == 1 ? 40 + rnd(160) : 0);
    }
    return s;
}

// ---- the feeder's loop around the cutter ----------------------------------------------------------------------------------------------
struct Emitted {
    feed::Cut cut;
    Bytes bytes;
};
struct Run {
    feed::FirstBuffer first = feed::FIRST_BGZF;
    std::vector<Emitted> segs;
    std::vector<size_t> buffer_ends;  // file offsets at which a buffer that did not reach the end of the file ended
    int64_t switch_at = -1;
    feed::Outcome last = feed::CUT_GO_ON;
    int emit_calls = 0;
    bool cut_ran = false;
};
constexpr int CHUNK = 7;
// S: bytes per buffer; fail_at: the emit call (from 0) that fails; classify: look at the first buffer as the feeder does
static Run fill_and_cut(const Bytes& file, size_t S, size_t cap, size_t largest, int64_t start = 0, int fail_at = -1, bool classify = true) {
    Run r;
    feed::Cutter cutter(S, cap, start, CHUNK, largest);
    Bytes buf(S);
    bool eof = false, first = true;
    size_t read_end = (size_t)start;
    while (!eof) {
        size_t fill = cutter.carry_into(buf.data());
        const size_t from = (size_t)cutter.read_from(), want = S - fill;
        CHECK(from == read_end);  // every byte of the file is read once: what is not cut yet is carried, not read again
        const size_t got = std::min(want, file.size() - std::min(from, file.size()));
        read_end = from + got;
        if (got) memcpy(buf.data() + fill, file.data() + from, got);
        fill += got;
        eof = got < want;  // (a file that ends with a buffer: the next read says so)
        if (!eof) r.buffer_ends.push_back(from + got);
        const Bytes exact(buf.begin(), buf.begin() + (long)fill);
        if (first && classify) {
            r.first = feed::classify_first(exact.data(), fill);
            if (r.first != feed::FIRST_BGZF) {
                r.switch_at = 0;
                return r;
            }
        }
        first = false;
        r.cut_ran = true;
        r.last = cutter.cut(exact.data(), fill, eof, [&](feed::Cut&& c, const uint8_t* at, size_t n) {
            CHECK(at >= exact.data() && at + n <= exact.data() + fill);
            if (r.emit_calls++ == fail_at) return false;
            r.segs.push_back(Emitted{std::move(c), Bytes(at, at + n)});
            return true;
        });
        if (r.last != feed::CUT_GO_ON) break;
    }
    r.switch_at = cutter.switch_at();
    CHECK((r.last == feed::CUT_TEXT_FROM) == (r.switch_at >= 0) || r.last == feed::CUT_EMIT_FAILED);
    return r;
}

// the segments are the stream's blocks [first_block, first_block + n_blocks), each once, with everything the cut says of them true
static void check_segments(const Stream& s, const Run& r, size_t first_block, size_t n_blocks, size_t cap) {
    size_t g = first_block;
    int64_t at = first_block < s.blocks.size() ? (int64_t)s.blocks[first_block].off : (int64_t)s.file.size();
    for (const Emitted& e : r.segs) {
        const feed::Cut& c = e.cut;
        CHECK(c.kind == feed::SEG_BGZF && c.chunk == CHUNK);
        CHECK(c.file_off == at);
        CHECK(!c.blocks.empty() && c.blocks.size() == c.crcs.size() && c.blocks.size() == c.starts.size());
        CHECK(c.text_bytes <= cap || c.blocks.size() == 1);
        CHECK((size_t)at + e.bytes.size() <= s.file.size() && !memcmp(e.bytes.data(), s.file.data() + at, e.bytes.size()));
        size_t text = 0, bytes = 0;
        for (size_t k = 0; k < c.blocks.size(); ++k, ++g) {
            if (g >= first_block + n_blocks) {
                CHECK(!"more blocks than the file's BGZF prefix holds");
                return;
            }
            const Block& b = s.blocks[g];
            const qd_inflate_block& q = c.blocks[k];
            CHECK(c.starts[k] == b.off - (size_t)at && c.starts[k] == bytes);
            CHECK(q.in_off == c.starts[k] + b.payload_off && q.in_len == b.payload_len);
            CHECK(q.out_off == text && q.out_len == b.text_len);
            CHECK(c.crcs[k] == b.crc);
            std::string t;
            if (q.in_len) {
                CHECK((size_t)q.in_off + q.in_len <= e.bytes.size() && inflate_raw(e.bytes.data() + q.in_off, q.in_len, q.out_len, &t));
                CHECK(t == s.text.substr(b.text_off, b.text_len));
            } else {
                CHECK(q.out_len == 0);
            }
            text += b.text_len;
            bytes += b.size;
        }
        CHECK(c.text_bytes == text && e.bytes.size() == bytes);
        at += (int64_t)bytes;
    }
    CHECK(g == first_block + n_blocks);
}

// ---- every seam position --------------------------------------------------------------------------------------------------------------
enum Seam { AT_BOUNDARY, IN_FIXED_HEADER, IN_LONG_EXTRA, IN_PAYLOAD, IN_TRAILER, N_SEAMS };
static void test_seams() {
    const Stream s = mixed_stream(40);
    CHECK(s.largest > 200 && s.largest < 500);
    size_t seen[N_SEAMS] = {0}, header_byte[18] = {0}, runs = 0;
    for (size_t S = 2 * s.largest; S <= 3 * s.largest; ++S) {
        const Run r = fill_and_cut(s.file, S, (size_t)1 << 30, s.largest);
        ++runs;
        CHECK(r.first == feed::FIRST_BGZF && r.switch_at < 0 && r.last == feed::CUT_GO_ON);
        check_segments(s, r, 0, s.blocks.size(), (size_t)1 << 30);
        for (size_t end : r.buffer_ends)
            for (const Block& b : s.blocks) {
                if (end == b.off) ++seen[AT_BOUNDARY];
                if (end <= b.off || end >= b.off + b.size) continue;
                const size_t in = end - b.off;  // bytes of the block inside the buffer
                if (in <= 17) ++seen[IN_FIXED_HEADER], ++header_byte[in];
                else if (in < 12 + b.xlen) ++seen[IN_LONG_EXTRA];
                else ++seen[in <= b.size - 8 && b.payload_len ? IN_PAYLOAD : IN_TRAILER];
            }
    }
    for (int k = 0; k < N_SEAMS; ++k) CHECK(seen[k] > 0);
    for (int k = 1; k <= 17; ++k) CHECK(header_byte[k] > 0);
    printf("seams: %zu buffer sizes; buffer ends at a boundary %zu, in the first 17 bytes %zu, in a long extra field %zu, in a payload %zu, in a trailer %zu\n",
           runs, seen[AT_BOUNDARY], seen[IN_FIXED_HEADER], seen[IN_LONG_EXTRA], seen[IN_PAYLOAD], seen[IN_TRAILER]);
    // a file that ends exactly with a buffer: the read behind it finds nothing, and nothing is emitted twice
    Stream two;
    const std::string same = bases(300);
    add_block(two, same, 0);
    add_block(two, same, 0);
    const Run r = fill_and_cut(two.file, two.file.size(), (size_t)1 << 30, two.largest);
    CHECK(r.switch_at < 0 && r.last == feed::CUT_GO_ON && r.buffer_ends.size() == 1);
    check_segments(two, r, 0, 2, (size_t)1 << 30);
}

// ---- every reason to switch -------------------------------------------------------------------------------------------------------------
static Bytes gzip_member(const std::string& text) {
    Bytes m = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};
    append(m, deflate_raw(text));
    put32(m, (uint32_t)crc32(crc32(0, nullptr, 0), (const Bytef*)text.data(), (uInt)text.size()));
    put32(m, (uint32_t)text.size());
    return m;
}
static void test_switches() {
    struct Damage {
        const char* what;
        Bytes bytes;
        bool more_behind;                 // two whole blocks follow (they must not be emitted)
        feed::FirstBuffer at_file_start;  // what the classifier says when no block stands in front
    };
    const std::string t = bases(400);
    Bytes truncated = bgzf_block(t, 0), cut_header = bgzf_block(t, 0), cut_extra = bgzf_block(t, 120);
    truncated.resize(truncated.size() - 5);
    cut_header.resize(10);
    cut_extra.resize(60);
    const Damage damages[] = {
        {"garbage", Bytes(40, 0x55), true, feed::FIRST_OTHER},
        {"an ordinary gzip member", gzip_member(t), true, feed::FIRST_GZIP},
        {"a block with FNAME set", bgzf_block(t, 0, true, 12), true, feed::FIRST_BGZF},
        {"ISIZE above 65536", bgzf_block(t, 0, true, 4, 65537), true, feed::FIRST_BGZF},
        {"a truncated block at the end of the file", truncated, false, feed::FIRST_BGZF},
        {"a header cut off at the end of the file", cut_header, false, feed::FIRST_OTHER},
        {"a long extra field cut off at the end of the file", cut_extra, false, feed::FIRST_GZIP},  // (short is not BGZF: gzip by its magic)
    };
    for (const Damage& d : damages)
        for (size_t k : {(size_t)0, (size_t)1, (size_t)9}) {
            Stream s = mixed_stream((int)k);
            const size_t prefix = s.file.size();
            append(s.file, d.bytes);
            if (d.more_behind) {
                append(s.file, bgzf_block(t, 0));
                append(s.file, bgzf_block(t, 30));
            }
            const size_t largest = std::max<size_t>(s.largest, 600);
            for (size_t S : {2 * largest, 2 * largest + 1, 2 * largest + 13, 2 * largest + prefix % 97, 3 * largest, std::max(2 * largest, s.file.size() + 50)}) {
                const Run r = fill_and_cut(s.file, S, (size_t)1 << 30, largest);
                if (k == 0) CHECK(r.first == d.at_file_start);
                if (k == 0 && d.at_file_start != feed::FIRST_BGZF) {
                    CHECK(!r.cut_ran && r.switch_at == 0);
                } else {
                    if (r.switch_at != (int64_t)prefix) printf("  %s after %zu blocks, buffers of %zu: switch at %lld, not %zu\n", d.what, k, S, (long long)r.switch_at, prefix);
                    CHECK(r.last == feed::CUT_TEXT_FROM && r.switch_at == (int64_t)prefix);
                    check_segments(s, r, 0, k, (size_t)1 << 30);  // (a switch in the middle of a buffer: the blocks in front still go out)
                }
                // the cutter's own rule where no block stands in front, without the first look
                if (k == 0) {
                    const Run bare = fill_and_cut(s.file, S, (size_t)1 << 30, largest, 0, -1, false);
                    CHECK(bare.last == feed::CUT_TEXT_FROM && bare.switch_at == 0 && bare.segs.empty());
                }
            }
        }
}

// ---- files that never get going, the first look, a ranged start --------------------------------------------------------------------------
static void test_first_buffer() {
    const std::string t = bases(100);
    const Bytes block = bgzf_block(t, 0), long_block = bgzf_block(t, 150), member = gzip_member(t);
    const Bytes empty;
    const Run e = fill_and_cut(empty, 1200, 1000, 600);
    CHECK(e.first == feed::FIRST_OTHER && e.switch_at == 0 && !e.cut_ran && e.segs.empty());
    for (size_t n = 0; n < 18; ++n) {  // shorter than 18 bytes: whatever it starts like
        for (const Bytes* src : {&block, &member}) {
            const Bytes head(src->begin(), src->begin() + (long)n);
            CHECK(feed::classify_first(head.data(), n) == feed::FIRST_OTHER);
            const Run r = fill_and_cut(head, 1200, 1000, 600);
            CHECK(r.first == feed::FIRST_OTHER && r.switch_at == 0 && r.segs.empty());
        }
    }
    auto first = [](const Bytes& b, size_t n) {
        const Bytes head(b.begin(), b.begin() + (long)n);
        return feed::classify_first(head.data(), n);
    };
    CHECK(first(block, 18) == feed::FIRST_BGZF && first(block, block.size()) == feed::FIRST_BGZF);
    CHECK(first(long_block, 12 + 160) == feed::FIRST_BGZF);
    for (size_t n = 18; n < 12 + 160; ++n) CHECK(first(long_block, n) == feed::FIRST_GZIP);  // short is not BGZF: an ordinary gzip file by its magic
    CHECK(first(member, 18) == feed::FIRST_GZIP && first(member, member.size()) == feed::FIRST_GZIP);
    Bytes other_cm = member, no_magic = member, no_bc = bgzf_block(t, 0);
    other_cm[2] = 7;
    no_magic[1] = 0x8c;
    no_bc[12] = 'X';
    CHECK(first(other_cm, other_cm.size()) == feed::FIRST_OTHER && first(no_magic, no_magic.size()) == feed::FIRST_OTHER);
    CHECK(first(no_bc, no_bc.size()) == feed::FIRST_GZIP);
    const Bytes plain(200, '@');
    CHECK(first(plain, 200) == feed::FIRST_OTHER);

    // a ranged file starts at its start offset: at a block boundary the blocks from there on, with their true offsets
    const Stream s = mixed_stream(20);
    for (size_t from : {(size_t)1, (size_t)3, (size_t)6, (size_t)19}) {
        for (size_t S : {2 * s.largest, 2 * s.largest + 31, s.file.size()}) {
            const Run r = fill_and_cut(s.file, S, (size_t)1 << 30, s.largest, (int64_t)s.blocks[from].off);
            CHECK(r.first == feed::FIRST_BGZF && r.switch_at < 0 && r.last == feed::CUT_GO_ON);
            CHECK(!r.segs.empty() && r.segs[0].cut.file_off == (int64_t)s.blocks[from].off);
            check_segments(s, r, from, s.blocks.size() - from, (size_t)1 << 30);
        }
    }
    // ... and inside a block there is no block header
    const Run mid = fill_and_cut(s.file, 2 * s.largest, (size_t)1 << 30, s.largest, (int64_t)s.blocks[2].off + 20);
    CHECK(mid.first != feed::FIRST_BGZF && !mid.cut_ran);
}

// ---- the text cap -----------------------------------------------------------------------------------------------------------------------
static void test_text_cap() {
    const size_t cap = 1000;
    Stream s;
    const size_t lens[] = {400, 400, 400, 999, 1, 1, 1000, 1500, 300, 0, 700, 1001, 2, 998, 400, 400};
    for (size_t n : lens) add_block(s, std::string(n, 'A'), s.blocks.size() % 5 == 2 ? 60 : 0);
    CHECK(s.file.size() < 1200);  // (highly compressible: all of it is one buffer)
    const Run r = fill_and_cut(s.file, s.file.size() + 100, cap, s.largest);
    CHECK(r.switch_at < 0 && r.last == feed::CUT_GO_ON);
    check_segments(s, r, 0, s.blocks.size(), cap);
    // a new segment starts exactly where the next block's text would pass the cap
    std::vector<size_t> want_blocks;
    size_t text = 0, n = 0;
    for (const Block& b : s.blocks) {
        if (text + b.text_len > cap && n) want_blocks.push_back(n), text = 0, n = 0;
        text += b.text_len, ++n;
    }
    want_blocks.push_back(n);
    CHECK(r.segs.size() == want_blocks.size() && r.segs.size() >= 8);
    for (size_t i = 0; i < std::min(r.segs.size(), want_blocks.size()); ++i) CHECK(r.segs[i].cut.blocks.size() == want_blocks[i]);
    bool alone = false;
    for (const Emitted& e : r.segs) alone |= e.cut.text_bytes == 1500 && e.cut.blocks.size() == 1 && e.cut.blocks[0].out_off == 0 && e.cut.starts[0] == 0;
    CHECK(alone);  // a single block above the cap goes out alone
    // with small buffers on top: the offsets stay segment-relative across both kinds of seam
    for (size_t S = 2 * s.largest; S <= 3 * s.largest; ++S) check_segments(s, fill_and_cut(s.file, S, cap, s.largest), 0, s.blocks.size(), cap);
}

// ---- an upload that fails -----------------------------------------------------------------------------------------------------------------
static void test_emit_failure() {
    Stream s;
    for (int i = 0; i < 12; ++i) add_block(s, std::string(400, 'C'), 0);
    const size_t prefix = s.file.size();
    append(s.file, Bytes(40, 0x55));
    for (size_t S : {2 * s.largest, s.file.size() + 10})
        for (size_t cap : {(size_t)1000, (size_t)1 << 30}) {
            const Run whole = fill_and_cut(s.file, S, cap, s.largest);
            CHECK(whole.last == feed::CUT_TEXT_FROM && whole.switch_at == (int64_t)prefix);
            for (int k = 0; k < whole.emit_calls; ++k) {
                const Run r = fill_and_cut(s.file, S, cap, s.largest, 0, k);
                CHECK(r.last == feed::CUT_EMIT_FAILED && r.emit_calls == k + 1 && (int)r.segs.size() == k);
                for (int i = 0; i < k; ++i) CHECK(r.segs[(size_t)i].bytes == whole.segs[(size_t)i].bytes);
                // the upload behind a switch fails: the verdict stands (the feeder's text path still runs from there, as it always did)
                // (one buffer: its last segment goes out behind the switch; small buffers: the garbage may stand alone in the last one)
                if (k == whole.emit_calls - 1 && S > s.file.size()) CHECK(r.switch_at == (int64_t)prefix);
                if (k < whole.emit_calls - 1) CHECK(r.switch_at < 0);
            }
        }
}

int main() {
    test_seams();
    test_switches();
    test_first_buffer();
    test_text_cap();
    test_emit_failure();
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
