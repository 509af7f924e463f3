// The container framing of the input side, read in ONE place: the gzip member header (RFC 1952), BGZF's 'BC' subfield, the
// CRC-32 / ISIZE trailer, zero padding behind the last member, and the walk from member to member around the device's gzip
// steps (qd_gz).  Host only: no GPU include, builds with plain g++ (tests/native/gz_framing_test.cpp).  Who uses what, and what
// each caller does with every answer: DESIGN.md 7.1.
#pragma once
#include <stddef.h>
#include <stdint.h>

uint32_t qd_crc32_combine_host(uint32_t crc1, uint32_t crc2, uint64_t len2);  // quade_io.cpp (zlib's)

namespace gzf {

inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }

// ---- the gzip member header ------------------------------------------------------------------------------------------------------
inline bool has_magic(const uint8_t* p, size_t n) { return n >= 2 && p[0] == 0x1f && p[1] == 0x8b; }
// magic and CM = 8 (deflate)
inline bool has_magic_cm(const uint8_t* p, size_t n) { return n >= 3 && has_magic(p, n) && p[2] == 8; }
// the ten fixed bytes of a member: magic, CM = 8, no reserved flag bits
inline bool looks_like_gzip(const uint8_t* p, size_t n) { return n >= 10 && has_magic_cm(p, n) && !(p[3] & 0xe0); }

// gzip member header at p -> its length; 0 = not a header, -1 = consistent so far but cut off by n
// (fewer than ten bytes: only the two magic bytes can refute it)
inline int64_t gzip_header_len(const uint8_t* p, size_t n) {
    if (n < 10) return (n >= 1 && p[0] != 0x1f) || (n >= 2 && p[1] != 0x8b) ? 0 : -1;
    if (!looks_like_gzip(p, n)) return 0;
    const uint8_t flg = p[3];
    size_t o = 10;
    if (flg & 4) {  // FEXTRA
        if (o + 2 > n) return -1;
        o += 2 + le16(p + o);
        if (o > n) return -1;
    }
    for (int f = 8; f <= 16; f <<= 1)  // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (o < n && p[o]) ++o;
            if (o >= n) return -1;
            ++o;
        }
    if (flg & 2) o += 2;  // FHCRC
    return o > n ? -1 : (int64_t)o;
}

// ---- BGZF (bgzip, htslib): gzip members of <= 64 KiB of text whose header carries their own size in an extra subfield 'B','C' --
// so a file can be cut into blocks without inflating it.  'BC' may stand anywhere in the extra field.
enum BgzfAnswer {
    BGZF_BLOCK,  // a complete block header: bsize and xlen are known
    BGZF_SHORT,  // fewer than 18 bytes, or fewer than 12 + XLEN bytes of something with the magic and FEXTRA: more bytes will tell
    BGZF_NOT     // whatever follows, this is no BGZF block
};
constexpr size_t BGZF_MIN_BLOCK = 26;  // header with only 'BC' in its extra field (18) and the trailer (8), no payload
struct BgzfBlock {
    BgzfAnswer is = BGZF_NOT;
    size_t bsize = 0, xlen = 0;  // BGZF_BLOCK: the block's total size (header .. ISIZE) and its extra field's
    bool whole = false;          // the block lies inside avail: what follows is set
    bool only_fextra = false;    // no FLG bit besides FEXTRA (bgzip sets none: no name, comment or header CRC)
    size_t payload_off = 0, payload_len = 0;  // the raw deflate stream between the header and the trailer
    uint32_t crc = 0, isize = 0;              // the trailer's
    // what bgzip writes: room for the header and the trailer, no other header fields (framed), at most 64 KiB of text
    bool framed() const { return whole && bsize >= 12 + xlen + 8 && only_fextra; }
    bool is_bgzip_layout() const { return framed() && isize <= 65536; }
    size_t size() const { return is == BGZF_BLOCK ? bsize : 0; }  // 0: no complete BGZF block header here (yet)
};
inline BgzfBlock bgzf_block(const uint8_t* p, size_t avail) {
    BgzfBlock b;
    if (avail < 18) {
        b.is = BGZF_SHORT;
        return b;
    }
    if (!has_magic_cm(p, avail) || !(p[3] & 4)) return b;
    b.xlen = le16(p + 10);
    if (avail < 12 + b.xlen) {
        b.is = BGZF_SHORT;
        return b;
    }
    for (size_t o = 12; o + 4 <= 12 + b.xlen;) {  // the extra field's subfields: SI1 SI2 SLEN data
        const size_t slen = le16(p + o + 2);
        if (p[o] == 'B' && p[o + 1] == 'C' && slen == 2 && o + 6 <= 12 + b.xlen) {
            b.is = BGZF_BLOCK;
            b.bsize = (size_t)le16(p + o + 4) + 1;
            break;
        }
        o += 4 + slen;
    }
    if (b.is != BGZF_BLOCK || b.bsize > avail) return b;
    b.whole = true;
    b.only_fextra = !(p[3] & ~4);
    b.payload_off = 12 + b.xlen;
    b.payload_len = b.bsize >= 12 + b.xlen + 8 ? b.bsize - 12 - b.xlen - 8 : 0;
    if (b.bsize >= 8) {
        b.crc = le32(p + b.bsize - 8);
        b.isize = le32(p + b.bsize - 4);
    }
    return b;
}

// ---- what stands where a member should begin ----------------------------------------------------------------------------------------
enum MemberStart {
    START_HEADER,   // a member header, *header_len bytes long
    START_PADDING,  // nothing but zero bytes up to the end of the file (none at all included): tolerated, as by gzip itself
    START_GARBAGE,  // not a gzip header
    START_CUT       // a header so far, cut off by n
};
// p[0 .. n): the bytes on hand; to_eof: they reach the end of the file
inline MemberStart member_start(const uint8_t* p, size_t n, bool to_eof, int64_t* header_len = nullptr) {
    if (to_eof) {
        size_t i = 0;
        while (i < n && p[i] == 0) ++i;
        if (i == n) return START_PADDING;
    }
    const int64_t h = gzip_header_len(p, n);
    if (header_len) *header_len = h;
    return h > 0 ? START_HEADER : h < 0 ? START_CUT : START_GARBAGE;
}

// ---- the walk over the members of a gzip file whose deflate blocks something else decodes step by step (qd_gz on the device, zlib in
// the test).  Offsets count from the start of the file.  The caller holds the compressed bytes [comp_off, comp_off + comp_len) -- the
// whole image, or what has been uploaded and not yet used -- and decides what to do when a step makes no progress.
struct MemberWalk {
    uint64_t hdr_off = 0;     // where the next member's header stands (need_header), or the current member's trailer ended last
    uint64_t member_off = 0;  // the current member's header
    uint64_t bit = 0;         // the next block header of the current member (bits from the start of the file); 8 * hdr_off between members
    uint64_t text = 0;        // text of the current member so far
    uint32_t crc = 0;         // CRC-32 of that text (0 while there is none: an empty member's CRC is 0)
    bool need_header = true;

    // a member begins at hdr_off with a header of header_len bytes (gzip_header_len); 0: nothing is known of it but where it stands
    void begin(uint64_t header_len) {
        member_off = hdr_off;
        text = 0;
        crc = 0;
        bit = 8 * (hdr_off + header_len);
        need_header = header_len == 0;
    }
    // one step's input: the bytes from the 16-byte boundary (counted from comp_off) in front of `bit` on
    struct Window {
        uint64_t byte0;       // from comp_off
        uint64_t bit_start;   // from byte0
        uint64_t comp_bytes;  // what is on hand behind byte0, at most max_bytes
        uint64_t base;        // byte0 from the start of the file
    };
    Window window(uint64_t comp_off, uint64_t comp_len, uint64_t max_bytes = ~(uint64_t)0) const {
        Window w;
        w.byte0 = ((bit >> 3) - comp_off) & ~(uint64_t)15;
        w.base = comp_off + w.byte0;
        w.bit_start = bit - 8 * w.base;
        w.comp_bytes = comp_len - w.byte0 < max_bytes ? comp_len - w.byte0 : max_bytes;
        return w;
    }
    // a step that decoded no block although all of its input went into the launch: it ends inside a block, more input is needed
    template <class Step>
    static bool stalled(const Step& s) {
        return s.bit_next == s.bit_start && !s.member_end && !s.starved;
    }
    // a finished step (its text_len, crc32, bit_next, member_end) joins the member; true: it made progress (or was starved)
    template <class Step>
    bool account(const Step& s, const Window& w) {
        if (s.text_len) {
            crc = text ? qd_crc32_combine_host(crc, s.crc32, s.text_len) : s.crc32;
            text += s.text_len;
        }
        bit = 8 * w.base + s.bit_next;
        return !stalled(s);
    }
    // behind the member's last block: CRC-32 and ISIZE of its text at the next byte boundary
    uint64_t trailer_off() const { return (bit + 7) >> 3; }
    bool trailer_inside(uint64_t file_size) const { return trailer_off() + 8 <= file_size; }
    struct Trailer {
        bool ok;
        uint32_t crc, isize;  // what the file says
    };
    // t: the 8 bytes at trailer_off().  ok: the next member's header (or the end of the file) stands at hdr_off
    Trailer end_member(const uint8_t* t) {
        const Trailer r{le32(t) == crc && le32(t + 4) == (uint32_t)text, le32(t), le32(t + 4)};
        if (r.ok) {
            hdr_off = trailer_off() + 8;
            bit = 8 * hdr_off;
            need_header = true;
        }
        return r;
    }
};

}  // namespace gzf
