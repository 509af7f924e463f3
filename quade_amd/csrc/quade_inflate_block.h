// One BGZF block of an inflate launch, as the host describes it to the device.  No GPU include: the feeder's cutter (feed_cut.h)
// fills these on the host, quade_inflate.h hands them to the kernels.
#pragma once
#include <stdint.h>

struct qd_inflate_block {
    uint32_t in_off, in_len;    // raw deflate payload of the block inside the compressed buffer
    uint32_t out_off, out_len;  // where its text goes, and how much there must be (ISIZE)
};
