# -*- coding: utf-8 -*-
"""
Quade_unknown_barcodes.csv: the most frequent barcodes of the Undetermined pairs ([output] top_unknown_barcodes, conf.UNKNOWN_HELP).
The reference has no counterpart (Quade 0.3.2 only writes the Undetermined files); bcl2fastq and BCL Convert call the same table
"Top Unknown Barcodes".  The counts come from the device (include/quade_hip.h, qd_unknown_*); everything here is host work on at
most 1000 rows: the order, the nearest sample of every row and the text.
"""
from __future__ import annotations

import numpy as np

REPORT_NAME = "Quade_unknown_barcodes.csv"


def escape(key):
    """bytes -> text: bytes outside 0x21-0x7E as \\xNN"""
    return "".join(chr(b) if 0x21 <= b <= 0x7E else "\\x%02X" % b for b in bytes(key))


def nearest_sample(key, mat, ordinals, w1):
    """key: uint8[K]; mat: uint8[n, K], the (upper-cased) barcodes of length K, of the samples `ordinals` (ascending).
    Returns (ordinal, d1, d2) of the sample with the smallest d1 + d2 (per-part Hamming distances), lowest ordinal on a tie;
    None when no barcode has length K."""
    if mat.shape[0] == 0:
        return None
    diff = mat != np.asarray(key, dtype=np.uint8)[None, :]
    d1 = diff[:, :w1].sum(1)
    d2 = diff[:, w1:].sum(1)
    i = int(np.argmin(d1 + d2))  # the first minimum: rows are in ordinal order
    return int(ordinals[i]), int(d1[i]), int(d2[i])


def report_order(keys, counts):
    """count descending, then key bytes ascending"""
    counts = np.asarray(counts, dtype=np.uint64)
    if len(counts) == 0:
        return np.zeros((0, 0), dtype=np.uint8), counts
    keys = np.asarray(keys, dtype=np.uint8).reshape(len(counts), -1)
    cols = [keys[:, j] for j in reversed(range(keys.shape[1]))] + [-counts.astype(np.int64)]  # lexsort: the last column leads
    rows = np.lexsort(cols)
    return keys[rows], counts[rows]


def report_lines(keys, counts, short, dropped, undetermined, top, w1, dual, samples):
    """The file's lines.  keys uint8[n, K] / counts uint64[n]: the merged table; samples: (name, barcode) in ordinal order;
    w1: bytes of index read 1's part of the key; dual: the plan has an index read 2."""
    keys, counts = report_order(keys, counts)
    K = keys.shape[1] if len(counts) else 0
    same = [(i, b) for i, (_, b) in enumerate(samples) if len(b) == K and K > 0]
    ordinals = [i for i, _ in same]
    mat = np.array([np.frombuffer(b.upper().encode("latin-1"), np.uint8) for _, b in same], dtype=np.uint8).reshape(len(same), K)
    lines = ["Pair Undetermined\t{}".format(int(undetermined)), "Short index slice\t{}".format(int(short)),
             "Not tallied\t{}".format(int(dropped)), "Distinct barcodes tallied\t{}".format(len(counts)), ""]
    head = ["index1_seq"] + (["index2_seq"] if dual else []) + ["count", "percent_of_undetermined", "nearest_sample",
                                                              "index1_distance"] + (["index2_distance"] if dual else [])
    lines.append("\t".join(head))
    for r in range(min(int(top), len(counts))):
        key, c = keys[r], int(counts[r])
        row = [escape(key[:w1])] + ([escape(key[w1:])] if dual else [])
        row += [str(c), str(c * 100 // int(undetermined) if undetermined else 0)]
        near = nearest_sample(key, mat, ordinals, w1)
        if near is None:
            row += [""] * (3 if dual else 2)
        else:
            row += [samples[near[0]][0], str(near[1])] + ([str(near[2])] if dual else [])
        lines.append("\t".join(row))
    return lines


def write_report(path, *args, **kw):
    with open(path, "w") as fh:
        fh.write("\n".join(report_lines(*args, **kw)) + "\n")
