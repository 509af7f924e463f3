"""The truth for the adapter content (qd_adapters_*, Quade_adapter_report.csv): plain Python over the reads as bytes, by the
definition of include/quade_hip.h, with no shortcut -- every start is tried, base by base.

A probe is 12 bytes of ACGT; up to 16 are in force, slot a = the a-th.  With u[i] = s[i] & 0xDF and L the length, first(a) is the
smallest p in [0, L - 12] with u[p .. p + 12) equal to probe a, else None; a byte that is not A, C, G or T after folding matches
nothing.  first(any) is the minimum over the probes in force.  Table: hist[r][a][min(first(a), 1024)] over 17 columns (16 slots,
any) for r = R1, R2; dest[d][r][c], d the routing code (0xFFFF -> 2 * S), c = 0 the reads and c = 1 + a the reads with first(a)."""
import os

import numpy as np

from tests import qstats_model as QM

UNDETERMINED = 0xFFFF
K, PROBES, BINS = 12, 16, 1025
COLUMNS = PROBES + 1
ANY = PROBES
HIST_VALUES = 2 * COLUMNS * BINS
DEST_VALUES = 2 * (COLUMNS + 1)
BUILTIN = (("illumina_universal", b"AGATCGGAAGAG"), ("illumina_small_rna_3p", b"TGGAATTCTCGG"), ("illumina_small_rna_5p", b"GATCGTCGGACT"),
           ("nextera_transposase", b"CTGTCTCTTATA"), ("poly_a", b"AAAAAAAAAAAA"), ("poly_g", b"GGGGGGGGGGGG"))


def first(seq, probe):
    """the smallest start at which the 12 bases of probe stand in seq (bytes), or None"""
    assert len(probe) == K and all(b in b"ACGT" for b in probe)
    for p in range(len(seq) - K + 1):
        ok = True
        for i in range(K):
            u = seq[p + i] & 0xDF
            if u not in b"ACGT" or u != probe[i]:
                ok = False
                break
        if ok:
            return p
    return None


def firsts(seq, probes):
    """[first(a) for every probe] + [first(any)]"""
    f = [first(seq, p) for p in probes]
    found = [x for x in f if x is not None]
    return f + [min(found) if found else None]


def values(S):
    return HIST_VALUES + (2 * S + 1) * DEST_VALUES


def _lists(S):
    return {"hist": [[[0] * BINS for _ in range(COLUMNS)] for _ in range(2)],
            "dest": [[[0] * (COLUMNS + 1) for _ in range(2)] for _ in range(2 * S + 1)]}


def add_read(t, S, code, r, seq, probes):
    d = 2 * S if code == UNDETERMINED else code
    t["dest"][d][r][0] += 1
    f = firsts(seq, probes)
    for a, p in list(enumerate(f[:-1])) + [(ANY, f[-1])]:
        if p is not None:
            t["hist"][r][a][min(p, BINS - 1)] += 1
            t["dest"][d][r][1 + a] += 1


def _arrays(t):
    return {k: np.array(v, dtype=np.uint64) for k, v in t.items()}


def table(S, probes, pairs):
    """pairs: (code, seq of R1, seq of R2) -> dict of uint64 arrays hist[2, 17, 1025], dest[2S+1, 2, 18]"""
    assert len(probes) <= PROBES and len(set(probes)) == len(probes)
    t = _lists(S)
    for code, s1, s2 in pairs:
        add_read(t, S, code, 0, s1, probes)
        add_read(t, S, code, 1, s2, probes)
    return _arrays(t)


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def table_from_outputs(outdir, samples, probes):
    """The table of a run whose stages leave the reads alone, from its per-destination output files (all three write flags on):
    the files hold the raw reads, by the routing.  A missing file is an empty destination."""
    S = len(samples)
    t = _lists(S)
    stems = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    for d, stem in enumerate(stems):
        for r, read in enumerate(("_R1", "_R2")):
            p = os.path.join(outdir, stem + read + ".fastq.gz")
            if os.path.exists(p):
                for seq, _ in QM.fastq_records(p):
                    add_read(t, S, UNDETERMINED if d == 2 * S else d, r, seq, probes)
    return _arrays(t)
