"""The paired-end overlap trimming of insert reads in plain Python: the definition the device stage
(quade_amd/csrc/quade_pairtrim.hip) and the pair trim report are tested against (include/quade_hip.h states it in the same words).
An insert length I pairs position i of R1 with position I - 1 - i of R2; it is accepted when enough positions overlap and few
enough of them fail to be complementary letters of ACGT.  The smallest accepted I >= max(L1, L2) cuts nothing; otherwise the
largest accepted I below it cuts both reads to I; then the min_length floor."""
import os

from tests.trim_model import read_fastq, read_of

COUNTERS = ("reads", "bases_in", "bases_out", "overlap_trimmed_reads", "overlap_trimmed_bases", "floored_reads")
PAIR_COUNTERS = ("pairs", "overlapped_pairs", "short_insert_pairs")
BINS = 1025
VALUES = 2 * len(COUNTERS) + len(PAIR_COUNTERS) + BINS
PAIRS, HIST = 2 * len(COUNTERS), 2 * len(COUNTERS) + len(PAIR_COUNTERS)
COMP = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


class Params(object):
    def __init__(self, min_overlap=30, max_mismatches=5, max_mismatch_pct=20, min_length=0):
        self.min_overlap = min_overlap
        self.max_mismatches = max_mismatches
        self.max_mismatch_pct = max_mismatch_pct
        self.min_length = min_length

    def keywords(self):
        return dict(min_overlap=self.min_overlap, max_mismatches=self.max_mismatches, max_mismatch_pct=self.max_mismatch_pct,
                    min_length=self.min_length)


def matches(b1, b2):
    """a base of R1 opposite a base of R2"""
    u1, u2 = b1 & 0xDF, b2 & 0xDF
    return u1 in COMP and u2 == COMP[u1]


def overlap(I, L1, L2):
    return min(L1, I) - max(0, I - L2)


def mismatches(s1, s2, I):
    """over every position i of R1 whose partner j = I - 1 - i lies in R2"""
    mm = 0
    for i in range(len(s1)):
        j = I - 1 - i
        if 0 <= j < len(s2) and not matches(s1[i], s2[j]):
            mm += 1
    return mm


# R1 folded, every byte that is no letter of ACGT as 0; R2 complemented, every such byte as 1: a position matches iff they are equal
FOLD1 = bytes((b & 0xDF) if (b & 0xDF) in COMP else 0 for b in range(256))
COMP2 = bytes(COMP[b & 0xDF] if (b & 0xDF) in COMP else 1 for b in range(256))


def accepted(s1, s2, I, P):
    """s1 = R1 through FOLD1, s2 = R2 through COMP2"""
    ov = overlap(I, len(s1), len(s2))
    if ov < P.min_overlap:
        return False
    budget, mm = min(P.max_mismatches, ov * P.max_mismatch_pct // 100), 0
    for i in range(max(0, I - len(s2)), min(len(s1), I)):
        if s1[i] != s2[I - 1 - i]:
            mm += 1
            if mm > budget:  # (only saves time: more mismatches cannot bring it back under the budget)
                return False
    return True


def insert_size(s1, s2, P):
    """I* of the pair, None when there is none"""
    s1, s2 = bytes(s1).translate(FOLD1), bytes(s2).translate(COMP2)
    M = max(len(s1), len(s2))
    for I in range(max(M, 1), len(s1) + len(s2) + 1):
        if accepted(s1, s2, I, P):
            return I
    for I in range(M - 1, 0, -1):
        if accepted(s1, s2, I, P):
            return I
    return None


def insert_size_plain(s1, s2, P):
    """insert_size once more without the translated copies and without the early exit: every candidate counted in full by
    mismatches().  Slow; the tests hold insert_size against it on full-length reads."""
    s1, s2 = bytes(s1), bytes(s2)
    L1, L2 = len(s1), len(s2)
    ok = [I for I in range(1, L1 + L2 + 1) if overlap(I, L1, L2) >= P.min_overlap
          and mismatches(s1, s2, I) <= min(P.max_mismatches, overlap(I, L1, L2) * P.max_mismatch_pct // 100)]
    M = max(L1, L2)
    up, down = [I for I in ok if I >= M], [I for I in ok if I < M]
    return min(up) if up else max(down) if down else None


def trim_pair(s1, s2, P):
    """-> (I* or None, (Lp1, Lp2), (Lout1, Lout2))"""
    L = (len(s1), len(s2))
    I = insert_size(s1, s2, P)
    Lp = tuple(min(x, I) for x in L) if I is not None and I < max(L) else L
    return I, Lp, tuple(max(p, min(P.min_length, x)) for p, x in zip(Lp, L))


def new_table():
    return [0] * VALUES


def count(table, s1, s2, P):
    """adds one pair to the table (1040 values) and returns the lengths its two reads keep"""
    L = (len(s1), len(s2))
    I, Lp, Lout = trim_pair(s1, s2, P)
    for r in (0, 1):
        t = r * len(COUNTERS)
        table[t + 0] += 1
        table[t + 1] += L[r]
        table[t + 2] += Lout[r]
        table[t + 3] += Lp[r] < L[r]
        table[t + 4] += L[r] - Lp[r]
        table[t + 5] += Lout[r] > Lp[r]
    table[PAIRS] += 1
    if I is not None:
        table[PAIRS + 1] += 1
        table[PAIRS + 2] += I < max(L)
        table[HIST + min(I, BINS - 1)] += 1
    return Lout


def trimmed_outputs(outdir, P, trim=None):
    """{file name: text} for every <dest>_R1 / _R2 fastq.gz of a run made without the option, the two files of a destination
    zipped record by record and cut by the model, and the table of all of them.  trim: tests/trim_model.py's Params of a 3'
    trimming that runs first (the stage then sees what that left); its table is returned as a third value."""
    from tests import trim_model as TM
    table, first, texts = new_table(), TM.new_table(), {}
    for f in sorted(os.listdir(outdir)):
        if read_of(f) != 0:
            continue
        f2 = f[:-len("_R1.fastq.gz")] + "_R2.fastq.gz"
        recs = [read_fastq(os.path.join(outdir, x)) for x in (f, f2)]
        assert len(recs[0]) == len(recs[1])
        out = ([], [])
        for a, b in zip(*recs):
            if trim is not None:
                a, b = [(head, seq[:n], qual[:n]) for r, (head, seq, qual) in enumerate((a, b)) for n in [TM.count(first, seq, qual, r, trim)]]
            keep = count(table, a[1], b[1], P)
            for r, (head, seq, qual) in enumerate((a, b)):
                out[r].append(head + b"\n" + seq[:keep[r]] + b"\n+\n" + qual[:keep[r]] + b"\n")
        texts[f], texts[f2] = b"".join(out[0]), b"".join(out[1])
    return (texts, table) if trim is None else (texts, table, first)
