"""The read filter in plain Python: the definition the device stage (quade_amd/csrc/quade_filter.hip) and the filter report are
tested against (include/quade_hip.h states it in the same words).  For a read of length L with sequence bytes s and quality bytes
q (unsigned):
  n_count = bytes 'N' or 'n'            unq  = the q[i] < 33 + qualified_quality
  qsum    = sum of max(0, q[i] - 33)    diff = the i in [0, L - 1) with (s[i] & 0xDF) != (s[i + 1] & 0xDF)
A pair is dropped for the first of these rules that either of its reads fails (a rule whose parameter is None is off):
  1 too_short L < min_length   2 too_many_n n_count > max_n   3 low_quality unq * 100 > max_unqualified_pct * L
  4 low_mean_quality qsum < min_mean_quality * L   5 low_complexity diff * 100 < min_complexity_pct * max(L - 1, 0)
A dropped pair is in no output file; a destination that loses all its pairs has no files, as one that received none (the sink
creates a destination's files when the first text for it arrives)."""
import os

from tests.trim_model import read_fastq, read_of

REASONS = ("too_short", "too_many_n", "low_quality", "low_mean_quality", "low_complexity")
COUNTERS = ("pairs",) + REASONS + ("bases_in", "bases_dropped")
KEYS = ("min_length", "max_n", "max_unqualified_pct", "qualified_quality", "min_mean_quality", "min_complexity_pct")
PAIRS, BASES_IN, BASES_DROPPED = 0, 6, 7
UNDETERMINED = 0xFFFF


class Params(object):
    def __init__(self, min_length=None, max_n=None, max_unqualified_pct=None, qualified_quality=15, min_mean_quality=None,
                 min_complexity_pct=None):
        self.min_length = min_length
        self.max_n = max_n
        self.max_unqualified_pct = max_unqualified_pct
        self.qualified_quality = qualified_quality
        self.min_mean_quality = min_mean_quality
        self.min_complexity_pct = min_complexity_pct

    def keywords(self):
        return {k: getattr(self, k) for k in KEYS}

    @property
    def on(self):
        return any(getattr(self, k) is not None for k in KEYS if k != "qualified_quality")


def read_counts(seq, qual, P):
    """-> (L, n_count, unq, qsum, diff) of one read"""
    seq, qual = bytes(seq), bytes(qual)
    assert len(seq) == len(qual)
    L = len(seq)
    n_count = sum(1 for b in seq if b in (ord("N"), ord("n")))
    unq = sum(1 for b in qual if b < 33 + P.qualified_quality)
    qsum = sum(max(0, b - 33) for b in qual)
    diff = sum(1 for i in range(L - 1) if (seq[i] & 0xDF) != (seq[i + 1] & 0xDF))
    return L, n_count, unq, qsum, diff


def read_fails(seq, qual, P):
    """the rules (1 .. 5) that are on and that the read fails, ascending"""
    L, n_count, unq, qsum, diff = read_counts(seq, qual, P)
    out = []
    if P.min_length is not None and L < P.min_length:
        out.append(1)
    if P.max_n is not None and n_count > P.max_n:
        out.append(2)
    if P.max_unqualified_pct is not None and unq * 100 > P.max_unqualified_pct * L:
        out.append(3)
    if P.min_mean_quality is not None and qsum < P.min_mean_quality * L:
        out.append(4)
    if P.min_complexity_pct is not None and diff * 100 < P.min_complexity_pct * max(L - 1, 0):
        out.append(5)
    return out


def reason(r1, r2, P):
    """r1, r2: (seq, qual) -> 0 (kept) or the first rule that either read fails"""
    fails = read_fails(r1[0], r1[1], P) + read_fails(r2[0], r2[1], P)
    return min(fails) if fails else 0


def new_table(n_samples):
    return [[0] * len(COUNTERS) for _ in range(2 * n_samples + 1)]


def count(table, code, r1, r2, P):
    """adds one pair to its destination's row and returns its reason"""
    d = len(table) - 1 if code == UNDETERMINED else code
    assert 0 <= d < len(table)
    why = reason(r1, r2, P)
    bases = len(r1[0]) + len(r2[0])
    table[d][PAIRS] += 1
    table[d][BASES_IN] += bases
    if why:
        table[d][why] += 1
        table[d][BASES_DROPPED] += bases
    return why


def add_tables(a, b):
    return [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a, b)]


def filtered_outputs(outdir, samples, P, trim=None, pair=None):
    """{file name: text} of what a run with the filter writes, from the <dest>_R1 / _R2 fastq.gz of a run made without it (all three
    write flags on), the two files of a destination zipped record by record, and the filter's table.  A destination all of whose
    pairs are dropped has no files.  trim / pair: tests/trim_model.py's and tests/pairtrim_model.py's Params of stages that run
    first (the filter sees what they left); -> (texts, table, trim table or None, pair trim table or None)."""
    from tests import pairtrim_model as PM
    from tests import trim_model as TM
    stems = [n + q for n in samples for q in ("_pass", "_fail")] + ["Undetermined"]
    table, texts = new_table(len(samples)), {}
    first = TM.new_table() if trim is not None else None
    second = PM.new_table() if pair is not None else None
    for f in sorted(os.listdir(outdir)):
        if read_of(f) != 0:
            continue
        stem = f[:-len("_R1.fastq.gz")]
        f2 = stem + "_R2.fastq.gz"
        d = stems.index(stem)
        recs = [read_fastq(os.path.join(outdir, x)) for x in (f, f2)]
        assert len(recs[0]) == len(recs[1])
        out = ([], [])
        for a, b in zip(*recs):
            if trim is not None:
                a, b = [(head, seq[:n], qual[:n]) for r, (head, seq, qual) in enumerate((a, b)) for n in [TM.count(first, seq, qual, r, trim)]]
            if pair is not None:
                keep = PM.count(second, a[1], b[1], pair)
                a, b = [(head, seq[:n], qual[:n]) for (head, seq, qual), n in zip((a, b), keep)]
            if count(table, UNDETERMINED if d == len(stems) - 1 else d, a[1:], b[1:], P):
                continue
            for r, (head, seq, qual) in enumerate((a, b)):
                out[r].append(head + b"\n" + seq + b"\n+\n" + qual + b"\n")
        if out[0]:
            texts[f], texts[f2] = b"".join(out[0]), b"".join(out[1])
    return texts, table, first, second
