"""The truth for the per-cycle counters (qd_cstats_*, Quade_cycle_report.csv): plain Python over the records as bytes, by the
definition of include/quade_hip.h.

Groups: g from the routing code -- an even code is pass (0), an odd code is fail (1), 0xFFFF is Undetermined (2).  Reads: r = 0 / 1
for R1 / R2.  Sequence bytes s; quality bytes q unsigned, ph = max(0, q - 33).  Per cycle c < 1024, every read with L > c adds to
cycle[g][r][c][8]: A, C, G, T, N by (s[c] & 0xDF) == the letter, qual_sum += ph[c], q20 (ph[c] >= 20), q30 (ph[c] >= 30).  Per
read: len[g][r] bin min(L, 1024); for L > 0 meanq[g][r] bin min(93, sum(ph) // L) and gc[g][r] bin 100 * (G and C count, either
case) // L, both over the whole read."""
import os

import numpy as np

from tests import qstats_model as QM

UNDETERMINED = 0xFFFF
CYCLES, LEN_BINS, MEANQ_BINS, GC_BINS = 1024, 1025, 94, 101
LETTERS = b"ACGTN"
QUAL_SUM, Q20, Q30 = 5, 6, 7


def group(code):
    return 2 if code == UNDETERMINED else code & 1


_K = bytes(LETTERS.find(bytes([b & 0xDF])) & 0xFF for b in range(256))  # sequence byte -> counter 0 .. 4, or 255


def _lists():
    return {"cycle": [[[[0] * 8 for _ in range(CYCLES)] for _ in range(2)] for _ in range(3)],
            "len": [[[0] * LEN_BINS for _ in range(2)] for _ in range(3)], "meanq": [[[0] * MEANQ_BINS for _ in range(2)] for _ in range(3)],
            "gc": [[[0] * GC_BINS for _ in range(2)] for _ in range(3)]}


def _arrays(t):
    return {k: np.array(v, dtype=np.uint64) for k, v in t.items()}


def empty():
    return _arrays(_lists())


def add_read(t, g, r, seq, qual):
    """t: _lists()' nested lists of Python integers"""
    assert len(seq) == len(qual)
    L = len(seq)
    ph = qual.translate(QM._Q)  # max(0, q - 33) of the unsigned byte
    cyc = t["cycle"][g][r]
    for c, (k, p) in enumerate(zip(seq[:CYCLES].translate(_K), ph)):
        row = cyc[c]
        if k < 5:
            row[k] += 1
        row[QUAL_SUM] += p
        row[Q20] += p >= 20
        row[Q30] += p >= 30
    t["len"][g][r][min(L, CYCLES)] += 1
    if L:
        t["meanq"][g][r][min(MEANQ_BINS - 1, sum(ph) // L)] += 1
        t["gc"][g][r][100 * sum(1 for s in seq if s & 0xDF in b"GC") // L] += 1


def table(pairs):
    """pairs: (code, drop, (seq1, qual1), (seq2, qual2)); a pair with drop != 0 adds nothing -> dict of uint64 arrays cycle[3, 2,
    1024, 8], len[3, 2, 1025], meanq[3, 2, 94], gc[3, 2, 101]"""
    t = _lists()
    for code, drop, r1, r2 in pairs:
        if drop:
            continue
        for r, (seq, qual) in enumerate((r1, r2)):
            add_read(t, group(code), r, seq, qual)
    return _arrays(t)


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def equal(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and (a[k] == b[k]).all() for k in a)


def table_from_outputs(outdir, samples):
    """The table of a run from its per-destination output files (all three write flags on): <name>_pass/_fail_R1/_R2.fastq.gz
    and Undetermined_R1/_R2.fastq.gz; a missing file is an empty destination."""
    t = _lists()
    stems = [(n + q, g) for n in samples for g, q in enumerate(("_pass", "_fail"))] + [("Undetermined", 2)]
    for stem, g in stems:
        for r, read in enumerate(("_R1", "_R2")):
            p = os.path.join(outdir, stem + read + ".fastq.gz")
            if os.path.exists(p):
                for seq, qual in QM.fastq_records(p):
                    add_read(t, g, r, seq, qual)
    return _arrays(t)


def qstats_columns(t):
    """What the qd_qstats table holds of the same reads (none longer than 1024 bases), per read r, summed over destinations:
    [records, bases, qual_sum, q20_bases, q30_bases, n_bases] (tests/qstats_model.py's counters)"""
    out = []
    for r in range(2):
        cyc = t["cycle"][:, r].sum(axis=(0, 1))
        length = t["len"][:, r].sum(axis=0)
        out.append([int(length.sum()), int(sum(int(L) * int(v) for L, v in enumerate(length))), int(cyc[QUAL_SUM]), int(cyc[Q20]),
                    int(cyc[Q30]), int(cyc[4])])
    return out
