// Where an upload ends: the cut of a feeder's buffers into segments of whole BGZF blocks, and what a file's first buffer is.  Host
// only: no GPU include, builds with plain g++ (tests/native/feed_cut_test.cpp).  The feeder (quade_pipe.cpp) keeps the reads, the
// page-locked buffers and the uploads; the rules, once: DESIGN.md 7.2.
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

#include "gz_framing.h"
#include "quade_inflate_block.h"

namespace feed {

enum { SEG_BGZF, SEG_TEXT, SEG_END, SEG_ERROR, SEG_GZIP };

// what the cut decides of a segment (the feeder adds the ring slot, the byte count and an error's text)
struct Cut {
    int kind = SEG_END;
    int chunk = 0;
    size_t text_bytes = 0;  // BGZF: what the blocks inflate to
    std::vector<qd_inflate_block> blocks;  // in_off inside the segment's bytes, out_off inside the segment's text
    std::vector<uint32_t> crcs;
    std::vector<uint32_t> starts;  // where every block starts in the segment's bytes (its file offset = file_off + that)
    int64_t file_off = 0;   // BGZF: where the blocks start in the file (a run the device refuses is read again by the host)
};

// ---- a file's first buffer ----------------------------------------------------------------------------------------------------------
enum FirstBuffer {
    FIRST_BGZF,  // a complete BGZF block header stands at its start
    FIRST_GZIP,  // ordinary gzip: the device can take the file's bytes as they are
    FIRST_OTHER  // neither (also: too short to tell): the host's readers from offset 0
};
inline FirstBuffer classify_first(const uint8_t* p, size_t fill) {
    if (gzf::bgzf_block(p, fill).is == gzf::BGZF_BLOCK) return FIRST_BGZF;
    return fill >= 18 && gzf::has_magic_cm(p, fill) ? FIRST_GZIP : FIRST_OTHER;
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------------------
// the most bytes gzf::bgzf_block asks for before it decides: a header with the longest extra field (a block is 64 KiB at most)
constexpr size_t BGZF_LARGEST = 12 + 65535;

enum Outcome {
    CUT_GO_ON,      // fill the next buffer (behind carry_into's bytes, from read_from()), unless this one reached the end of the file
    CUT_TEXT_FROM,  // not (or no longer) BGZF: the host's text path takes over at switch_at()
    CUT_EMIT_FAILED
};

// One per file.  Buffer after buffer: carry_into(buf), the caller reads the file from read_from() on behind those bytes, cut().
class Cutter {
  public:
    // buf_bytes: what a buffer holds; text_cap: text one segment inflates to at most; start: the file offset of the first buffer's
    // first byte; largest: no block and no block header of the file is longer.  A partial block is carried into the next buffer, so a
    // buffer must hold one largest block behind a carried tail: the block at its front is then whole (or decided otherwise) and every
    // buffer moves on.  A smaller buffer would be carried as it is, for ever.
    Cutter(size_t buf_bytes, size_t text_cap, int64_t start, int chunk, size_t largest = BGZF_LARGEST)
        : buf_bytes_(buf_bytes), text_cap_(text_cap), chunk_(chunk), file_pos_(start) {
        assert(buf_bytes >= 2 * largest);
        (void)largest;
    }

    // the partial block behind the last whole one of the previous buffer -> the front of the next; how many bytes that is
    size_t carry_into(uint8_t* buf) const {
        if (!tail_.empty()) memcpy(buf, tail_.data(), tail_.size());
        return tail_.size();
    }
    int64_t read_from() const { return file_pos_ + (int64_t)tail_.size(); }  // file offset of the byte behind the carried ones
    int64_t switch_at() const { return switch_at_; }  // >= 0: not (or no longer) BGZF from this file offset on

    // buf[0 .. fill): the carried bytes and what was read behind them; eof: they reach the end of the file (or of the byte range).
    // emit(Cut&&, first byte, bytes) uploads one segment and says whether that worked; after a failure nothing more is emitted.
    // switch_at() is set (or not) whatever the outcome: an emit can fail behind the switch it follows.
    template <class Emit>
    Outcome cut(const uint8_t* buf, size_t fill, bool eof, Emit&& emit) {
        tail_.clear();
        Cut seg = fresh(file_pos_);
        size_t pos = 0, seg_start = 0;  // seg holds the blocks of buf[seg_start, pos)
        while (pos < fill) {
            const gzf::BgzfBlock b = gzf::bgzf_block(buf + pos, fill - pos);
            if (b.is != gzf::BGZF_BLOCK) {
                // short: fewer bytes than a header, or than a header with its extra field ('BC' may stand anywhere in it): the
                // next read completes it
                if (b.is != gzf::BGZF_SHORT || eof) switch_at_ = file_pos_ + (int64_t)pos;
                break;
            }
            if (!b.whole) {
                if (eof) switch_at_ = file_pos_ + (int64_t)pos;  // a truncated block: the member loop reports it
                break;
            }
            if (!b.is_bgzip_layout()) {
                switch_at_ = file_pos_ + (int64_t)pos;
                break;
            }
            if (seg.text_bytes + b.isize > text_cap_ && !seg.blocks.empty()) {
                // text that compresses far better than fastq does: the buffer goes out in several segments, so that no window
                // has to take more than text_cap bytes of text in one step (its offsets are 32 bit)
                if (!emit(std::move(seg), buf + seg_start, pos - seg_start)) return CUT_EMIT_FAILED;
                seg = fresh(file_pos_ + (int64_t)pos);
                seg_start = pos;
            }
            seg.blocks.push_back(qd_inflate_block{(uint32_t)(pos - seg_start + b.payload_off), (uint32_t)b.payload_len, (uint32_t)seg.text_bytes, b.isize});
            seg.crcs.push_back(b.crc);
            seg.starts.push_back((uint32_t)(pos - seg_start));
            seg.text_bytes += b.isize;
            pos += b.bsize;
        }
        assert(pos > 0 || fill < buf_bytes_ || switch_at_ >= 0);  // (the constructor's condition: a full buffer moves on)
        if (switch_at_ < 0 && pos < fill) tail_.assign(buf + pos, buf + fill);
        file_pos_ += (int64_t)pos;
        if (!seg.blocks.empty() && !emit(std::move(seg), buf + seg_start, pos - seg_start)) return CUT_EMIT_FAILED;
        return switch_at_ >= 0 ? CUT_TEXT_FROM : CUT_GO_ON;
    }

  private:
    Cut fresh(int64_t file_off) const {
        Cut c;
        c.kind = SEG_BGZF;
        c.chunk = chunk_;
        c.file_off = file_off;
        return c;
    }
    const size_t buf_bytes_, text_cap_;
    const int chunk_;
    int64_t file_pos_;        // file offset of the buffer's first byte
    int64_t switch_at_ = -1;
    std::vector<uint8_t> tail_;
};

}  // namespace feed
