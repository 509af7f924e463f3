// The tables of a batch's output side, as the host describes them to the device: gzip members ("pieces"), the level-1 coder's
// sub-blocks and the CRC-32 ranges.  No GPU include: out_plan.h fills these on the host, quade_deflate.h and quade_text.h hand them
// to the kernels.
#pragma once
#include <stdint.h>

struct qd_deflate_piece {
    uint64_t text_off;  // where the piece's text starts in the text buffer, 16-byte aligned
    uint32_t text_len;
    uint32_t crc32;     // of the piece's text, made on the host
};

#ifndef QD_LZ_SUB
#define QD_LZ_SUB 65536 /* text per sub-block = per workgroup = per dynamic-Huffman block */
#endif
struct qd_lz_sub {
    uint64_t text_off;  // where the sub-block's text starts in the text buffer, 16-byte aligned
    uint32_t text_len;  // 1 .. QD_LZ_SUB
    uint32_t piece;
};

// CRC-32 (the gzip / zlib polynomial) of a range of text, at most 64 KiB
struct qd_crc_range {
    uint64_t off;
    uint32_t len;
    uint32_t pad;
};
