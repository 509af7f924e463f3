// Host-side checks of the input side's one framing reader (quade_amd/csrc/gz_framing.h): the gzip header parser and the BGZF block
// reader on forged headers and every prefix of them, the member-start classifier, and the member walk that qd_dev_gunzip and the
// pipeline's gz_steps drive -- here around a stand-in for the device's decoder written with zlib (raw inflate, Z_BLOCK: a step ends at
// a block boundary).  Built and run by tests/test_host_framing.py, plain and under ASan + UBSan (no GPU).
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../quade_amd/csrc/gz_framing.h"

uint32_t qd_crc32_combine_host(uint32_t crc1, uint32_t crc2, uint64_t len2) { return (uint32_t)crc32_combine((uLong)crc1, (uLong)crc2, (z_off_t)len2); }

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
// the parsers see exactly n bytes in a heap block of their own: a read past the end is the sanitizer's to report
template <class F>
static auto on_prefix(const Bytes& b, size_t n, F f) {
    Bytes c(b.begin(), b.begin() + (long)std::min(n, b.size()));
    c.resize(n, 0xA5);
    return f(c.data(), n);
}

// ---- gzip headers ---------------------------------------------------------------------------------------------------------------
static Bytes gzip_header(int flg, size_t xlen, const std::string& name, const std::string& comment) {
    Bytes h = {0x1f, 0x8b, 8, (uint8_t)flg, 1, 2, 3, 4, 0, 0xff};
    if (flg & 4) {
        put16(h, (uint32_t)xlen);
        for (size_t i = 0; i < xlen; ++i) h.push_back((uint8_t)(i * 7 + 1));  // (zero bytes among them: no terminator here)
    }
    if (flg & 8) h.insert(h.end(), name.begin(), name.end()), h.push_back(0);
    if (flg & 16) h.insert(h.end(), comment.begin(), comment.end()), h.push_back(0);
    if (flg & 2) put16(h, 0xBEEF);
    return h;
}

static void test_gzip_headers() {
    const std::string long_name(700, 'n');
    int n_headers = 0;
    for (int bits = 0; bits < 16; ++bits) {
        const int flg = ((bits & 1) ? 4 : 0) | ((bits & 2) ? 8 : 0) | ((bits & 4) ? 16 : 0) | ((bits & 8) ? 2 : 0);
        for (size_t xlen : {(size_t)0, (size_t)1, (size_t)300})
            for (const std::string& name : {std::string(), long_name}) {
                const Bytes h = gzip_header(flg, xlen, name, name.empty() ? "c" : "");
                ++n_headers;
                for (size_t n = 0; n <= h.size() + 3; ++n) {
                    const int64_t got = on_prefix(h, n, gzf::gzip_header_len);
                    CHECK(got == (n < h.size() ? -1 : (int64_t)h.size()));
                }
                for (int at = 0; at < 3; ++at) {  // magic, magic, CM
                    Bytes m = h;
                    m[(size_t)at] ^= 0x10;
                    CHECK(on_prefix(m, m.size(), gzf::gzip_header_len) == 0);
                }
                for (int reserved : {0x20, 0x40, 0x80}) {
                    Bytes m = h;
                    m[3] |= (uint8_t)reserved;
                    CHECK(on_prefix(m, m.size(), gzf::gzip_header_len) == 0);
                    CHECK(!gzf::looks_like_gzip(m.data(), m.size()));
                }
                CHECK(gzf::looks_like_gzip(h.data(), h.size()) && gzf::has_magic_cm(h.data(), 3) && !gzf::has_magic_cm(h.data(), 2) && gzf::has_magic(h.data(), 2));
            }
    }
    CHECK(n_headers == 96);
    const uint8_t le[4] = {0x78, 0x56, 0x34, 0x92};
    CHECK(gzf::le16(le) == 0x5678 && gzf::le32(le) == 0x92345678u);
}

// ---- BGZF block headers -----------------------------------------------------------------------------------------------------------
struct Sub {
    char a, b;
    uint32_t slen;  // as written
    size_t data;    // bytes that follow
};
// a block whose BSIZE field (where there is a well-formed 'BC') says its true size
static Bytes bgzf(int flg, const std::vector<Sub>& subs, size_t payload, uint32_t isize, size_t* xlen_out) {
    Bytes x;
    size_t bc_at = 0;
    for (const Sub& s : subs) {
        x.push_back((uint8_t)s.a), x.push_back((uint8_t)s.b);
        put16(x, s.slen);
        if (s.a == 'B' && s.b == 'C' && s.slen == 2 && s.data == 2 && !bc_at) bc_at = x.size();
        for (size_t i = 0; i < s.data; ++i) x.push_back((uint8_t)(0x40 + i % 50));
    }
    Bytes h = {0x1f, 0x8b, 8, (uint8_t)flg, 0, 0, 0, 0, 0, 0xff};
    put16(h, (uint32_t)x.size());
    h.insert(h.end(), x.begin(), x.end());
    if (flg & 8) h.push_back('n'), h.push_back(0);
    for (size_t i = 0; i < payload; ++i) h.push_back((uint8_t)(i * 13 + 5));
    put32(h, 0xC0FFEE11u);
    put32(h, isize);
    if (bc_at) h[12 + bc_at] = (uint8_t)(h.size() - 1), h[12 + bc_at + 1] = (uint8_t)((h.size() - 1) >> 8);
    *xlen_out = x.size();
    return h;
}

static void test_bgzf_headers() {
    struct Case {
        const char* what;
        int flg;
        std::vector<Sub> subs;
        uint32_t isize;
        gzf::BgzfAnswer is;
        bool layout;
    } cases[] = {
        {"BC first", 4, {{'B', 'C', 2, 2}}, 1000, gzf::BGZF_BLOCK, true},
        {"BC behind a 190-byte subfield", 4, {{'X', 'Y', 190, 190}, {'B', 'C', 2, 2}}, 1000, gzf::BGZF_BLOCK, true},
        {"no BC", 4, {{'X', 'Y', 2, 2}}, 1000, gzf::BGZF_NOT, false},
        {"BC with SLEN 3", 4, {{'B', 'C', 3, 3}}, 1000, gzf::BGZF_NOT, false},
        {"a subfield that runs past XLEN", 4, {{'X', 'Y', 100, 2}}, 1000, gzf::BGZF_NOT, false},
        {"a subfield that runs past XLEN, BC behind it", 4, {{'X', 'Y', 100, 2}, {'B', 'C', 2, 2}}, 1000, gzf::BGZF_NOT, false},
        {"FNAME also set", 4 | 8, {{'B', 'C', 2, 2}}, 1000, gzf::BGZF_BLOCK, false},
        {"ISIZE 65536", 4, {{'B', 'C', 2, 2}}, 65536, gzf::BGZF_BLOCK, true},
        {"ISIZE 65537", 4, {{'B', 'C', 2, 2}}, 65537, gzf::BGZF_BLOCK, false},
    };
    for (const Case& c : cases) {
        size_t xlen = 0;
        const Bytes b = bgzf(c.flg, c.subs, 37, c.isize, &xlen);
        if (!strcmp(c.what, "BC behind a 190-byte subfield")) CHECK(xlen == 200);
        Bytes followed = b;  // "whatever follows": another header's start, then noise
        for (int i = 0; i < 64; ++i) followed.push_back(i < 4 ? b[(size_t)i] : (uint8_t)(i * 31));
        for (size_t n = 0; n <= followed.size(); ++n) {
            const gzf::BgzfBlock r = on_prefix(followed, n, gzf::bgzf_block);
            const bool is_short = n < 18 || n < 12 + xlen;
            if (is_short) {
                CHECK(r.is == gzf::BGZF_SHORT && !r.whole && r.size() == 0 && !r.is_bgzip_layout());
                continue;
            }
            CHECK(r.is == c.is);
            if (c.is != gzf::BGZF_BLOCK) {
                CHECK(!r.whole && r.size() == 0 && !r.is_bgzip_layout());
                continue;
            }
            CHECK(r.bsize == b.size() && r.size() == b.size() && r.xlen == xlen);
            CHECK(r.whole == (n >= b.size()));
            CHECK(r.is_bgzip_layout() == (r.whole && c.layout));
            if (r.whole) {
                CHECK(r.crc == 0xC0FFEE11u && r.isize == c.isize && r.only_fextra == !(c.flg & ~4));
                CHECK(r.payload_off == 12 + xlen && r.payload_off + r.payload_len + 8 == b.size());
                CHECK(r.framed() == r.only_fextra);
            }
        }
        // without the magic, CM or FEXTRA: not BGZF as soon as 18 bytes are there
        for (int at : {0, 1, 2, 3}) {
            Bytes m = b;
            m[(size_t)at] = at == 3 ? (uint8_t)(m[3] & ~4) : (uint8_t)(m[(size_t)at] ^ 1);
            for (size_t n = 0; n <= m.size(); ++n) CHECK(on_prefix(m, n, gzf::bgzf_block).is == (n < 18 ? gzf::BGZF_SHORT : gzf::BGZF_NOT));
        }
    }
    // a BSIZE smaller than the header and trailer it stands in: a block header, whole, never bgzip's layout (and nothing read in front of p)
    size_t xlen = 0;
    Bytes b = bgzf(4, {{'B', 'C', 2, 2}}, 37, 10, &xlen);
    for (uint32_t bsize_m1 : {0u, 6u, 7u, 24u}) {
        b[16] = (uint8_t)bsize_m1, b[17] = 0;
        const gzf::BgzfBlock r = on_prefix(b, b.size(), gzf::bgzf_block);
        CHECK(r.is == gzf::BGZF_BLOCK && r.whole && r.bsize == bsize_m1 + 1 && !r.framed() && !r.is_bgzip_layout() && r.payload_len == 0);
    }
}

// ---- what stands where a member should begin --------------------------------------------------------------------------------------
static void test_member_start() {
    const Bytes h = gzip_header(4 | 8, 5, "name", "");
    int64_t hl = 0;
    CHECK(gzf::member_start(h.data(), h.size(), false, &hl) == gzf::START_HEADER && hl == (int64_t)h.size());
    CHECK(gzf::member_start(h.data(), h.size() - 1, true, &hl) == gzf::START_CUT && hl == -1);
    CHECK(gzf::member_start(h.data() + 1, h.size() - 1, true, &hl) == gzf::START_GARBAGE && hl == 0);
    const Bytes zeros(4096, 0);
    CHECK(gzf::member_start(zeros.data(), zeros.size(), true) == gzf::START_PADDING);
    CHECK(gzf::member_start(zeros.data(), 0, true) == gzf::START_PADDING);
    CHECK(gzf::member_start(zeros.data(), zeros.size(), false) == gzf::START_GARBAGE);  // (more of the file follows: not known to be padding)
    Bytes z1 = zeros;
    z1.back() = 1;
    CHECK(gzf::member_start(z1.data(), z1.size(), true) == gzf::START_GARBAGE);
}

// ---- the member walk ----------------------------------------------------------------------------------------------------------------
struct Step {  // the fields of qd_gz_step that the walk reads
    uint64_t comp_bytes = 0, bit_start = 0;
    int at_end = 0, starved = 0;
    uint64_t text_len = 0, bit_next = 0;
    int member_end = 0;
    uint32_t crc32 = 0;
};
// qd_gz::decode's stand-in: the whole blocks inside comp[0 .. comp_bytes) from bit_start on; `before`: the member's text so far
static bool decode(const uint8_t* comp, Step& s, const std::string& before, std::string* text) {
    s.text_len = 0, s.bit_next = s.bit_start, s.member_end = 0, s.crc32 = 0;
    text->clear();
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    const size_t dict = std::min<size_t>(before.size(), 32768);
    if (dict) inflateSetDictionary(&z, (const Bytef*)before.data() + before.size() - dict, (uInt)dict);
    size_t at = (size_t)(s.bit_start >> 3);
    if (at >= s.comp_bytes) {
        inflateEnd(&z);
        return true;
    }
    if (s.bit_start & 7) {
        inflatePrime(&z, 8 - (int)(s.bit_start & 7), comp[at] >> (s.bit_start & 7));
        ++at;
    }
    std::vector<uint8_t> out((size_t)4 << 20);
    z.next_in = const_cast<Bytef*>(comp + at);
    z.avail_in = (uInt)(s.comp_bytes - at);
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    bool good = true;
    for (;;) {
        const int rc = inflate(&z, Z_BLOCK);
        if (rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR) {
            good = false;
            break;
        }
        if (rc == Z_OK && (z.data_type & 128)) {  // the end of a block
            s.bit_next = 8 * (uint64_t)(z.next_in - comp) - (uint64_t)(z.data_type & 63);
            s.text_len = z.total_out;
            if (z.data_type & 64) {  // ... of the last one
                s.member_end = 1;
                break;
            }
            continue;
        }
        break;  // out of input inside a block (or of room: the tests' members are small)
    }
    inflateEnd(&z);
    text->assign((const char*)out.data(), (size_t)s.text_len);
    s.crc32 = (uint32_t)crc32(0L, out.data(), (uInt)s.text_len);
    return good;
}

enum Outcome { WALK_OK, WALK_MISMATCH, WALK_CUT, WALK_GARBAGE, WALK_DAMAGED };
struct Walked {
    Outcome what = WALK_OK;
    int members = 0;
    bool padding = false;
    std::string text;
    int stalls = 0, boundary_ends = 0, trailer_ends = 0;
    std::vector<uint64_t> block_ends, trailers;  // byte offsets: behind each block (rounded up), of each trailer
};
// the loop of qd_dev_gunzip (the whole image on hand, the step grows when it stalls), with the readers' tolerance of padding.
// cuts: file offsets at which a step ends when it would reach beyond them
static Walked walk_file(const Bytes& f, uint64_t step_bytes, const std::vector<uint64_t>& cuts = {}) {
    Walked r;
    gzf::MemberWalk walk;
    const uint64_t size = f.size();
    while (walk.hdr_off < size) {
        int64_t hl = 0;
        const Bytes rest(f.begin() + (long)walk.hdr_off, f.end());
        const gzf::MemberStart ms = gzf::member_start(rest.data(), rest.size(), true, &hl);
        if (ms == gzf::START_PADDING) {
            r.padding = true;
            break;
        }
        if (ms != gzf::START_HEADER) {
            r.what = ms == gzf::START_CUT ? WALK_CUT : WALK_GARBAGE;
            return r;
        }
        const uint64_t at = walk.hdr_off;
        walk.begin((uint64_t)hl);
        CHECK(walk.member_off == at && walk.bit == 8 * (at + (uint64_t)hl) && walk.text == 0 && walk.crc == 0 && !walk.need_header);
        std::string member;
        uint64_t step = step_bytes, floor_end = 0;
        for (bool ended = false; !ended;) {
            gzf::MemberWalk::Window win = walk.window(0, size, step);
            CHECK(win.byte0 % 16 == 0 && win.base == win.byte0 && 8 * win.base + win.bit_start == walk.bit && win.bit_start < 128);
            CHECK(win.base + win.comp_bytes <= size);
            uint64_t end = std::max(win.base + win.comp_bytes, std::min(floor_end, size));
            for (uint64_t c : cuts)
                if (c > (walk.bit >> 3) && c >= floor_end && c < end) end = c;
            win.comp_bytes = end - win.base;
            Step s;
            s.comp_bytes = win.comp_bytes;
            s.bit_start = win.bit_start;
            s.at_end = end >= size;
            std::string text;
            Bytes held(f.begin() + (long)win.base, f.begin() + (long)end);  // (the step sees its bytes alone)
            if (!decode(held.data(), s, member, &text)) {
                r.what = WALK_DAMAGED;
                return r;
            }
            if (gzf::MemberWalk::stalled(s)) {  // the step ends inside a block: more input, if there is any
                ++r.stalls;
                if (s.at_end) {
                    r.what = WALK_CUT;
                    return r;
                }
                floor_end = end + 1;
                step *= 2;
                continue;
            }
            const uint64_t text_before = walk.text;
            CHECK(walk.account(s, win));
            CHECK(walk.text == text_before + s.text_len && walk.bit == 8 * win.base + s.bit_next);
            r.block_ends.push_back((walk.bit + 7) >> 3);
            if (end == ((walk.bit + 7) >> 3)) ++r.boundary_ends;
            member += text;
            ended = s.member_end != 0;
            if (ended && end > walk.trailer_off() && end < walk.trailer_off() + 8) ++r.trailer_ends;
        }
        CHECK(walk.crc == (uint32_t)crc32(0L, (const Bytef*)member.data(), (uInt)member.size()));  // (0 for an empty member)
        r.text += member;
        if (!walk.trailer_inside(size)) {
            r.what = WALK_CUT;
            return r;
        }
        const uint64_t tr = walk.trailer_off();
        r.trailers.push_back(tr);
        const gzf::MemberWalk::Trailer t = walk.end_member(f.data() + tr);
        if (!t.ok) {
            CHECK(!walk.need_header && walk.trailer_off() == tr);  // (the walk stays where it was)
            r.what = WALK_MISMATCH;
            return r;
        }
        CHECK(walk.need_header && walk.hdr_off == tr + 8 && walk.bit == 8 * walk.hdr_off);
        ++r.members;
    }
    return r;
}

static Bytes member_of(const Bytes& header, const std::string& text, int level) {
    z_stream z;
    memset(&z, 0, sizeof z);
    deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
    Bytes body(deflateBound(&z, (uLong)text.size()) + 64);
    z.next_in = (Bytef*)text.data();
    z.avail_in = (uInt)text.size();
    z.next_out = body.data();
    z.avail_out = (uInt)body.size();
    deflate(&z, Z_FINISH);
    body.resize(z.total_out);
    deflateEnd(&z);
    Bytes m = header;
    m.insert(m.end(), body.begin(), body.end());
    put32(m, (uint32_t)crc32(0L, (const Bytef*)text.data(), (uInt)text.size()));
    put32(m, (uint32_t)text.size());
    return m;
}

static void test_member_walk() {
    srand(11);
    auto fastq = [](size_t records) {
        std::string t;
        for (size_t i = 0; i < records; ++i) {
            t += "@SIM:1:FC:" + std::to_string(rand() % 100000) + " 1:N:0\n";
            for (int k = 0; k < 100; ++k) t += "ACGT"[rand() & 3];
            t += "\n+\n";
            for (int k = 0; k < 100; ++k) t += (char)('#' + rand() % 40);
            t += "\n";
        }
        return t;
    };
    const std::string t0 = fastq(2000), t2 = fastq(300), t3 = fastq(50);
    const std::vector<Bytes> members = {member_of(gzip_header(0, 0, "", ""), t0, 6), member_of(gzip_header(0, 0, "", ""), "", 6),
                                        member_of(gzip_header(8, 0, "stored.fastq", ""), t2, 0),
                                        member_of(gzip_header(4 | 8 | 16 | 2, 300, "all.fastq", "every optional field"), t3, 6)};
    const std::string text = t0 + t2 + t3;
    Bytes file;
    std::vector<size_t> member_end;
    for (const Bytes& m : members) file.insert(file.end(), m.begin(), m.end()), member_end.push_back(file.size());
    const Bytes unpadded = file;
    file.resize(file.size() + 4096, 0);

    const Walked whole = walk_file(file, ~(uint64_t)0 >> 1);
    CHECK(whole.what == WALK_OK && whole.members == 4 && whole.padding && whole.text == text && whole.stalls == 0);
    CHECK(whole.trailers.size() == 4);
    for (size_t k = 0; k < whole.trailers.size() && k < 4; ++k) CHECK(whole.trailers[k] + 8 == member_end[k]);
    // every block boundary, from a walk that stops behind every block it can
    const Walked fine = walk_file(file, 17);
    CHECK(fine.what == WALK_OK && fine.members == 4 && fine.padding && fine.text == text && fine.stalls > 0);
    CHECK(fine.block_ends.size() >= 8);  // the level-6 member alone has several blocks
    // step sizes of every kind; steps that end exactly behind a block, one byte short of that, and inside every trailer
    for (uint64_t step : {(uint64_t)17, (uint64_t)100, (uint64_t)1000, (uint64_t)4096, (uint64_t)65536}) {
        const Walked w = walk_file(file, step);
        CHECK(w.what == WALK_OK && w.members == 4 && w.padding && w.text == text);
    }
    std::vector<uint64_t> cuts;
    for (uint64_t e : fine.block_ends) cuts.push_back(e - 1), cuts.push_back(e);
    for (uint64_t t : fine.trailers) cuts.push_back(t + 3);
    std::sort(cuts.begin(), cuts.end());
    for (uint64_t step : {(uint64_t)1000, (uint64_t)1 << 40}) {
        const Walked w = walk_file(file, step, cuts);
        CHECK(w.what == WALK_OK && w.members == 4 && w.padding && w.text == text);
        CHECK(w.stalls > 0 && w.boundary_ends >= 4);
    }
    for (size_t k = 0; k < 4; ++k) {  // a step that ends inside a trailer: the member's last block and three bytes more
        const Walked w = walk_file(file, (uint64_t)1 << 40, {fine.trailers[k] + 3});
        CHECK(w.what == WALK_OK && w.members == 4 && w.text == text && w.trailer_ends == 1);
    }
    // the unpadded file ends where the last member does
    {
        const Walked w = walk_file(unpadded, 4096);
        CHECK(w.what == WALK_OK && w.members == 4 && !w.padding && w.text == text);
    }
    // one CRC byte, one ISIZE byte of every member in turn: a mismatch at that member
    for (size_t k = 0; k < 4; ++k)
        for (size_t back : {(size_t)8, (size_t)5, (size_t)4, (size_t)1}) {
            Bytes bad = file;
            bad[member_end[k] - back] ^= 0x04;
            for (uint64_t step : {(uint64_t)1000, (uint64_t)1 << 40}) {
                const Walked w = walk_file(bad, step);
                CHECK(w.what == WALK_MISMATCH && w.members == (int)k);
            }
        }
    // cut inside the last trailer (every length of it), inside the last member's blocks, inside its header: cut off
    for (size_t lose = 1; lose <= 8; ++lose) {
        const Bytes cut(unpadded.begin(), unpadded.end() - (long)lose);
        const Walked w = walk_file(cut, 1000);
        CHECK(w.what == WALK_CUT && w.members == 3);
    }
    {
        const Bytes cut(unpadded.begin(), unpadded.end() - 200);
        const Walked w = walk_file(cut, 1000);
        CHECK(w.what == WALK_CUT && w.members == 3);
        const Bytes in_header(unpadded.begin(), unpadded.begin() + (long)member_end[2] + 100);
        const Walked h = walk_file(in_header, 1000);
        CHECK(h.what == WALK_CUT && h.members == 3);
    }
    // something that is no header behind a member
    {
        Bytes bad = file;
        bad[member_end[1]] = 0x1e;
        const Walked w = walk_file(bad, 1000);
        CHECK(w.what == WALK_GARBAGE && w.members == 2);
        Bytes dirty = file;  // padding that is not all zeros
        dirty.back() = 1;
        const Walked d = walk_file(dirty, 1000);
        CHECK(d.what == WALK_GARBAGE && d.members == 4);
    }
}

int main() {
    test_gzip_headers();
    test_bgzf_headers();
    test_member_start();
    test_member_walk();
    printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
