"""The truth for the quality counters (qd_qstats_*, Quade_quality_report.csv): plain Python over the records as bytes, by the
definitions of include/quade_hip.h.  Per (destination, read) six integers: records, bases, qual_sum, q20_bases, q30_bases,
n_bases; destination = routing code (2 * i = sample i's pass, 2 * i + 1 = its fail), Undetermined (0xFFFF) last."""
import gzip
import os

import numpy as np

UNDETERMINED = 0xFFFF


_Q = bytes(max(0, b - 33) for b in range(256))          # quality byte (unsigned) -> q
_Q20 = bytes(1 if q >= 20 else 0 for q in _Q)
_Q30 = bytes(1 if q >= 30 else 0 for q in _Q)


def read_stats(seq, qual):
    """seq, qual: bytes of one record's sequence and quality line (no line end, no trailing '\\r'), of one length"""
    assert len(seq) == len(qual)
    return [1, len(seq), sum(qual.translate(_Q)), sum(qual.translate(_Q20)), sum(qual.translate(_Q30)),
            seq.count(b"N") + seq.count(b"n")]


def table(n_samples, pairs):
    """pairs: (code, (seq1, qual1), (seq2, qual2)) -> numpy uint64[2 * n_samples + 1, 2, 6]"""
    t = [[[0] * 6 for _ in range(2)] for _ in range(2 * n_samples + 1)]
    for code, r1, r2 in pairs:
        d = 2 * n_samples if code == UNDETERMINED else code
        assert 0 <= d <= 2 * n_samples
        for r, (seq, qual) in enumerate((r1, r2)):
            t[d][r] = [a + b for a, b in zip(t[d][r], read_stats(seq, qual))]
    return np.array(t, dtype=np.uint64)


def fastq_records(path):
    """(seq, qual) of every record of a fastq.gz file"""
    with gzip.open(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0, path
    return [(lines[i + 1].rstrip(b"\r"), lines[i + 3].rstrip(b"\r")) for i in range(0, len(lines), 4)]


def table_from_outputs(outdir, samples, only=None):
    """The table of a run from its per-destination output files (all three write flags on): <name>_pass/_fail_R1/_R2.fastq.gz
    and Undetermined_R1/_R2.fastq.gz; a missing file is an empty destination.  only: stems to read (the others stay zero)."""
    stems = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    t = np.zeros((len(stems), 2, 6), dtype=np.uint64)
    for d, stem in enumerate(stems):
        if only is not None and stem not in only:
            continue
        for r, read in enumerate(("_R1", "_R2")):
            p = os.path.join(outdir, stem + read + ".fastq.gz")
            if os.path.exists(p):
                for seq, qual in fastq_records(p):
                    t[d, r] += np.array(read_stats(seq, qual), dtype=np.uint64)
    return t
