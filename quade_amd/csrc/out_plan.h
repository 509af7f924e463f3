// The host's plan of a batch's output: where every destination's text lies, and how it is cut into gzip members ("pieces"), the
// level-1 coder's 64 KiB sub-blocks and the CRC-32 ranges.  Host only: no GPU include (tests/native/batch_plan_test.cpp).  The pipeline
// and qd_dev_route_format share the layout, the pipeline and qd_deflater_run the cut of a piece.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/quade_hip.h"
#include "quade_out_records.h"

// Where every destination's text lies in a batch's output buffer (host; the pipeline and qd_dev_route_format share it): the R1
// regions of destinations 0 .. n_dest-1 in ascending order, then their R2 regions, each non-empty region starting on a multiple of
// 16.  first / g1_first / g2_first: qd_text_dest_bounds' tables read back, tot1 / tot2 = G1[n] / G2[n].  A destination without
// pairs starts where the next one does, so its region is empty.  base1[d] / base2[d] = where d's region starts minus G at d's
// first position (qd_text_format adds G back); the non-empty regions are appended to `regions` in buffer order.  Returns the
// bytes of the buffer the regions take, rounded up to 16.
struct qd_out_region {
    uint32_t dest;
    int k;  // 0: R1, 1: R2
    uint64_t at, bytes;
};
inline uint64_t qd_text_out_layout(uint32_t n_dest, const uint32_t* first, const uint32_t* g1_first, const uint32_t* g2_first, uint32_t tot1,
                                   uint32_t tot2, int64_t* base1, int64_t* base2, std::vector<qd_out_region>* regions) {
    std::vector<uint32_t> g1s(n_dest + 1), g2s(n_dest + 1);
    g1s[n_dest] = tot1;
    g2s[n_dest] = tot2;
    for (int64_t d = (int64_t)n_dest - 1; d >= 0; --d) {
        const bool none = first[d] == 0xFFFFFFFFu;
        g1s[d] = none ? g1s[d + 1] : g1_first[d];
        g2s[d] = none ? g2s[d + 1] : g2_first[d];
    }
    uint64_t at = 0;
    for (int k = 0; k < 2; ++k)
        for (uint32_t d = 0; d < n_dest; ++d) {
            const std::vector<uint32_t>& gs = k ? g2s : g1s;
            const uint64_t bytes = gs[d + 1] - gs[d];
            (k ? base2 : base1)[d] = (int64_t)at - (int64_t)gs[d];
            if (!bytes) continue;
            regions->push_back(qd_out_region{d, k, at, bytes});
            at = (at + bytes + 15) & ~(uint64_t)15;
        }
    return at;
}

namespace outplan __attribute__((visibility("hidden"))) {  // (the library exports nothing of this)

inline size_t subs_of(uint64_t text_len) { return (size_t)((text_len + QD_LZ_SUB - 1) / QD_LZ_SUB); }

// one piece -> its subs_of(text_len) sub-blocks in text order, each with the CRC-32 range of the same bytes: emit(qd_lz_sub, qd_crc_range)
template <class Emit>
inline void cut_piece(uint64_t text_off, uint32_t text_len, uint32_t piece, Emit&& emit) {
    for (uint64_t q = 0; q < text_len; q += QD_LZ_SUB) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(QD_LZ_SUB, text_len - q);
        emit(qd_lz_sub{text_off + q, n, piece}, qd_crc_range{text_off + q, n, 0});
    }
}

struct FileRun {  // the members of one output file made by one batch: pieces [first, first + n)
    uint32_t code;
    int k;
    uint32_t first, n;
    uint64_t text_bytes;
};

struct Plan {
    std::vector<qd_deflate_piece> pieces;  // text_off / text_len; the CRC-32s are made on the device
    std::vector<qd_lz_sub> subs;
    std::vector<qd_crc_range> ranges;      // ranges[k] = subs[k]'s bytes
    std::vector<uint32_t> first_sub;       // piece i = sub-blocks first_sub[i] .. first_sub[i + 1]: n_pieces + 1 entries
    std::vector<FileRun> files;            // one per region, in buffer order
};

// the regions of qd_text_out_layout, each cut into pieces of at most piece_bytes: a file run per region (destination 2 * n_samples: Undetermined)
inline Plan plan_output(const std::vector<qd_out_region>& regions, uint32_t piece_bytes, uint32_t n_samples) {
    Plan pl;
    for (const qd_out_region& rg : regions) {
        FileRun fr;
        fr.code = rg.dest == 2 * n_samples ? QD_CODE_UNDETERMINED : rg.dest;
        fr.k = rg.k;
        fr.first = (uint32_t)pl.pieces.size();
        fr.text_bytes = rg.bytes;
        for (uint64_t a = 0; a < rg.bytes; a += piece_bytes) {
            const uint32_t plen = (uint32_t)std::min<uint64_t>(piece_bytes, rg.bytes - a);
            pl.first_sub.push_back((uint32_t)pl.subs.size());
            cut_piece(rg.at + a, plen, (uint32_t)pl.pieces.size(), [&pl](const qd_lz_sub& s, const qd_crc_range& r) {
                pl.subs.push_back(s);
                pl.ranges.push_back(r);
            });
            pl.pieces.push_back(qd_deflate_piece{rg.at + a, plen, 0});
        }
        fr.n = (uint32_t)pl.pieces.size() - fr.first;
        pl.files.push_back(fr);
    }
    pl.first_sub.push_back((uint32_t)pl.subs.size());
    return pl;
}

}  // namespace outplan
