// How many bytes every buffer of a batch needs, said once.  Host only: no GPU include, builds with plain g++
// (tests/native/batch_plan_test.cpp).  The pipeline's reservation and its per-batch path apply these through the same helpers
// (quade_pipe.cpp: need_pair_buffers, need_scan_tables, need_out_buffers).  Every size is monotone in every argument.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/quade_hip.h"
#include "quade_out_records.h"

namespace bsz __attribute__((visibility("hidden"))) {  // (the library exports nothing of this)

constexpr size_t TEXT_TILE = 16384, REC_BYTES = 24;  // QD_TEXT_TILE and sizeof(qd_rec) (quade_text.h)

// Bytes per record where no scan has told yet: the reservation of an insert and of an index stream, and the chunk loop's top-ups
// (three defaults, kept apart: merging them would change what a run asks for)
constexpr double RECORD_INSERT = 400.0, RECORD_INDEX = 64.0, RECORD_TOP_UP = 256.0;
inline double record_bytes(double avg, double fallback) { return avg > 0 ? avg : fallback; }

// the text a window should hold: what it has, `pairs` more records, 3 % and a page on top -- three quarters of a window at most
inline size_t want_text(size_t len, uint64_t pairs, double bytes_per_record, size_t window_max) {
    return std::min<size_t>(len + (size_t)((double)pairs * bytes_per_record * 1.03) + 4096, window_max * 3 / 4);
}
// the pairs the reservation is made for: a batch, or what the run's largest seq_R1 file can hold (gzip at its best makes 1 byte of 8)
inline uint32_t most_pairs(uint32_t B, int64_t max_r1_bytes, bool r1_compressed, double avg1) {
    return (uint32_t)std::min<double>((double)B, (double)max_r1_bytes * (r1_compressed ? 8.0 : 1.0) / record_bytes(avg1, RECORD_INSERT) + 1024.0);
}

struct ScanSizes {  // the tables of a window's scan (qd_scan_scratch); tiles: tile_counts and tile_base, each
    size_t tiles, lines, rec_tile, recs;
};
inline ScanSizes scan_sizes(size_t text_bytes, size_t line_cap) {
    return ScanSizes{(text_bytes / TEXT_TILE + 3) * 4, line_cap * 4 + 64, (line_cap / 4 / 1024 + 4) * 4, (line_cap / 4 + 1) * REC_BYTES};
}

// ---- everything that is a function of the pair count ---------------------------------------------------------------------------------
inline uint32_t short_cap(size_t n) { return (uint32_t)(n / 2 + 64); }  // pairs qd_text_pack_rows may list in short_idx
struct StagesOn {  // which opt-in stages have tables of their own: clip, trim, overlap trim, post-trim; correction; filter / screen drop
    bool recs_out[4] = {false, false, false, false}, inserts = false, drop = false;
};
struct PairSizes {
    size_t rows_seq[2], rows_qual[2], rows_len[2], mol;  // per index stream; 0: no such stream, no molecular slice
    size_t halves;                                       // codes, dest, sdest
    size_t words;                                        // len1, len2, tmp, perm, g1, g2 (the total behind them)
    size_t short_idx, hist, scan_tiles;
    size_t dest_words, dest_longs, h_first;              // first, g1_first, g2_first; base1, base2; their page-locked read-back
    size_t recs_out[4], inserts, drop;                   // 0: the stage is off
};
inline PairSizes pair_sizes(const qd_layout& L, size_t n, size_t n_dest, const StagesOn& on) {
    PairSizes z{};
    for (int k = 0; k < L.n_streams; ++k) {
        z.rows_seq[k] = n * (size_t)L.seq_stride[k] + 64;
        z.rows_qual[k] = n * (size_t)L.qual_stride[k] + 64;
        z.rows_len[k] = n + 64;
    }
    z.mol = L.mol_width ? n * (size_t)L.mol_width + 64 : 0;
    z.halves = n * 2 + 64;
    z.words = (n + 1) * 4 + 64;
    z.short_idx = (size_t)short_cap(n) * 4;
    const size_t H = 256 * ((n + 1023) / 1024);  // qd_text_sort_by_dest's histograms
    z.hist = (H + H / 4096 + 8) * 4;
    z.scan_tiles = (n / 4096 + 4) * 4;
    z.dest_words = n_dest * 4;
    z.dest_longs = n_dest * 8;
    z.h_first = n_dest * 12 + 16;
    for (int s = 0; s < 4; ++s) z.recs_out[s] = on.recs_out[s] ? n * REC_BYTES + 64 : 0;
    z.inserts = on.inserts ? n * 8 + 64 : 0;
    z.drop = on.drop ? n + 64 : 0;
    return z;
}

// ---- the output side ---------------------------------------------------------------------------------------------------------------
// qd_huffman_member_bound: a code for 257 symbols never needs more than 9 bits per byte on average (the fixed 9-bit code is a
// candidate); the 15-bit limit's repair and the header (149 bytes), end-of-block code and trailer ride in the slack
inline int64_t huffman_member_bound(int64_t text_len) { return text_len < 0 ? -1 : ((text_len * 9 + 7) / 8 + text_len / 64 + 1024 + 3) & ~(int64_t)3; }

// the reservation's bounds on what out_plan.h makes of T bytes in 2 * n_dest regions (a region's last piece, a piece's last sub-block are short)
inline size_t max_pieces(size_t T, uint32_t piece_bytes, size_t n_dest) { return T / piece_bytes + 2 * n_dest + 2; }
inline size_t max_subs(size_t T, size_t n_pieces) { return T / QD_LZ_SUB + n_pieces; }

// Text per gzip member: 1 MiB -- less when so many destinations take members in one batch that their slots (every member gets one of
// the longest member's bound) would not fit member_slots_bytes: thousands of samples make thousands of small members per batch.
inline uint32_t piece_bytes_for(int64_t member_slots_bytes, uint64_t text_bytes, uint64_t n_dest) {
    uint32_t pb = 1u << 20;
    while (pb > QD_LZ_SUB && (uint64_t)max_pieces(text_bytes, pb, n_dest) * (uint64_t)huffman_member_bound(pb) > (uint64_t)member_slots_bytes) pb >>= 1;
    return pb;
}
// The coder's scratch of candidates / tokens is 4 bytes per byte of text: a batch's sub-blocks go through it a quarter at a time (a
// launch of some thousand workgroups still fills the device several times over), which keeps 2.5 GB of a 2 M-pair batch's 3.3 unallocated.
inline size_t lz_slice_subs(size_t n_subs) { return std::max<size_t>(2048, (n_subs + 3) / 4); }

struct OutSizes {
    size_t text, pieces, members, member_len, member_off, packed;  // of one output set
    size_t subs, ranges, crc, first_sub;                            // the format / CRC / coder launches' tables
    size_t tokens, sub_out, sub_bytes;                              // the level-1 coder's scratch
    int64_t out_stride, sub_stride;                                 // a member's and a sub-block's slot
};
inline OutSizes out_sizes(size_t text_bytes, size_t n_pieces, size_t n_subs, uint32_t piece_bytes) {
    OutSizes z;
    z.out_stride = huffman_member_bound(piece_bytes);
    z.sub_stride = huffman_member_bound(QD_LZ_SUB);
    z.text = text_bytes + 64;
    z.pieces = n_pieces * sizeof(qd_deflate_piece);
    z.members = z.packed = n_pieces * (size_t)z.out_stride;
    z.member_len = n_pieces * 4;
    z.member_off = (n_pieces + 1) * 8;
    z.subs = (n_subs + 1) * sizeof(qd_lz_sub);
    z.ranges = (n_subs + 1) * sizeof(qd_crc_range);
    z.crc = (n_subs + 1) * 4;
    z.first_sub = (n_pieces + 1) * 4;
    z.tokens = lz_slice_subs(n_subs) * QD_LZ_SUB * 4;
    z.sub_out = n_subs * (size_t)z.sub_stride;
    z.sub_bytes = n_subs * 4;
    return z;
}

}  // namespace bsz
