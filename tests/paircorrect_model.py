"""The overlap base correction of read pairs in plain Python: the rule the device stage (quade_amd/csrc/quade_paircorrect.hip) and the
pair correct report are tested against, built on tests/pairtrim_model.py (include/quade_hip.h and quade_paircorrect.h state it in
the same words).

The rule.  The stage runs directly behind the overlap trimming stage and in front of post-trimming, over every pair for which that
stage found an insert length I* (I* >= M and I* < M alike), whatever its destination, the write flags and later filtering.  It uses
the record tables the overlap stage RECEIVED: sequences s1, s2 and quality lines q1, q2 of lengths L1, L2, starting at the tables'
seq / qual (a 5' clip is respected).
  definitions : u(b) = b & 0xDF; valid(b) iff u(b) is one of A C G T; comp maps A<->T and C<->G; the phred of a quality byte c is
                (int)c - 33, so a byte below 33 is negative and therefore "bad" (as in quade_pairtrim.h)
  positions   : i with max(0, I* - L2) <= i < min(L1, I*), with partner j = I* - 1 - i; every such i, j lies inside what the overlap
                stage keeps of both reads (<= Lp <= Lout)
  mismatch    : a position mismatches iff not (valid(s1[i]) and u(s2[j]) == comp(u(s1[i]))): the overlap stage's definition exactly
  at a mismatching position, with G = good_quality and B = bad_quality (B < G, so at most one of the first two cases holds):
    1. if valid(s1[i]) and phred(q1[i]) >= G and phred(q2[j]) <= B: s2[j] = comp(u(s1[i])) and q2[j] = q1[i] -- R2 is corrected
    2. else if valid(s2[j]) and phred(q2[j]) >= G and phred(q1[i]) <= B: s1[i] = comp(u(s2[j])) and q1[i] = q2[j] -- R1 is corrected
    3. else nothing is written: the position is unresolved
  The written base is upper case.  The doubtful byte may be anything (N, lower case, any other byte); the trusted one must be a letter.
  properties  : nothing else in the text changes; no length changes and no pair is dropped; names, index reads and the :IDX[:MOL]
                tag never change; a position's outcome depends on its own four bytes only; applying the rule twice equals applying it
                once, because a corrected position matches afterwards
"""
import os

from tests import pairtrim_model as PM
from tests.trim_model import read_fastq, read_of

COUNTERS = ("r1_corrected_reads", "r1_corrected_bases", "r2_corrected_reads", "r2_corrected_bases", "pairs", "overlapped_pairs",
            "overlap_bases", "mismatches", "unresolved", "corrected_pairs")
VALUES = len(COUNTERS)
R1_READS, R1_BASES, R2_READS, R2_BASES, PAIRS, OVERLAPPED, OVERLAP_BASES, MISMATCHES, UNRESOLVED, CORRECTED_PAIRS = range(10)


class Params(object):
    def __init__(self, good_quality=30, bad_quality=14):
        self.good_quality = good_quality
        self.bad_quality = bad_quality

    def keywords(self):
        return dict(good_quality=self.good_quality, bad_quality=self.bad_quality)


def valid(b):
    return (b & 0xDF) in PM.COMP


def phred(c):
    return int(c) - 33


def correct_pair(s1, q1, s2, q2, I, P):
    """-> (s1, q1, s2, q2 as the stage leaves them, (bases written into R1, into R2, unresolved positions, positions)); I: the
    pair's insert length, None or 0 = none"""
    s1, q1, s2, q2 = bytearray(s1), bytearray(q1), bytearray(s2), bytearray(q2)
    L1, L2 = len(s1), len(s2)
    assert len(q1) == L1 and len(q2) == L2
    n1 = n2 = unresolved = positions = 0
    if I:
        for i in range(max(0, I - L2), min(L1, I)):
            j = I - 1 - i
            positions += 1
            if PM.matches(s1[i], s2[j]):
                continue
            if valid(s1[i]) and phred(q1[i]) >= P.good_quality and phred(q2[j]) <= P.bad_quality:
                s2[j], q2[j] = PM.COMP[s1[i] & 0xDF], q1[i]
                n2 += 1
            elif valid(s2[j]) and phred(q2[j]) >= P.good_quality and phred(q1[i]) <= P.bad_quality:
                s1[i], q1[i] = PM.COMP[s2[j] & 0xDF], q2[j]
                n1 += 1
            else:
                unresolved += 1
    return bytes(s1), bytes(q1), bytes(s2), bytes(q2), (n1, n2, unresolved, positions)


def new_table():
    return [0] * VALUES


def count(table, s1, q1, s2, q2, I, P):
    """adds one pair to the table (10 values) and returns its four lines as the stage leaves them"""
    s1, q1, s2, q2, (n1, n2, unresolved, positions) = correct_pair(s1, q1, s2, q2, I, P)
    table[R1_READS] += n1 > 0
    table[R1_BASES] += n1
    table[R2_READS] += n2 > 0
    table[R2_BASES] += n2
    table[PAIRS] += 1
    table[OVERLAPPED] += bool(I)
    table[OVERLAP_BASES] += positions
    table[MISMATCHES] += n1 + n2 + unresolved
    table[UNRESOLVED] += unresolved
    table[CORRECTED_PAIRS] += n1 + n2 > 0
    return s1, q1, s2, q2


def corrected_outputs(outdir, P_pair, P_corr, trim=None):
    """{file name: text} for every <dest>_R1 / _R2 fastq.gz of a run made without the options, the two files of a destination zipped
    record by record, corrected and cut by the models, then the overlap trimming table (as without the correction) and the
    correction's table of all of them.  trim: tests/trim_model.py's Params of a 3' trimming that runs first (both stages then see
    what that left); its table is returned as a fourth value."""
    from tests import trim_model as TM
    pair_table, table, first, texts = PM.new_table(), new_table(), TM.new_table(), {}
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
            I = PM.insert_size(a[1], b[1], P_pair)  # of the reads as the overlap stage receives them
            keep = PM.count(pair_table, a[1], b[1], P_pair)
            s1, q1, s2, q2 = count(table, a[1], a[2], b[1], b[2], I, P_corr)
            for r, (head, seq, qual) in enumerate(((a[0], s1, q1), (b[0], s2, q2))):
                out[r].append(head + b"\n" + seq[:keep[r]] + b"\n+\n" + qual[:keep[r]] + b"\n")
        texts[f], texts[f2] = b"".join(out[0]), b"".join(out[1])
    return (texts, pair_table, table) if trim is None else (texts, pair_table, table, first)
