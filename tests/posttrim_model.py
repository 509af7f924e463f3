"""Post-trimming of insert reads in plain Python: trailing N, a poly-X tail and the max_length crop, the definition the device stage
(quade_amd/csrc/quade_posttrim.hip) and the post-trim report are tested against (include/quade_hip.h states it in the same words).

For an insert read r (0 = R1, 1 = R2), take the record the stage receives, that is, what clip, trim and pairtrim left: sequence
bytes s, length L; u(b) = b & 0xDF; P = poly_x_min_length; M_r = max_length[r].  Each of steps 1 to 3 is skipped when not
configured; its output length is then its input length.
  1 trailing N (tail_n): Ln = L - k, where k is the number of consecutive bytes at the 3' end with u(b) == 'N'
  2 poly-X (P 6..100): for each X in A, C, G, T, Lx(X) is the clip stage's step 3 exactly as quade_hip.h states it for poly-G, with
    X in place of 'G', over s[0 .. Ln).  Lp = min over X of Lx(X).  The read's tail base is the X with Lx(X) < Ln.  N and every
    other byte count as a mismatch.  One pass only: a T run behind an A run loses the T run
  3 crop (M_r > 0): Lm = min(Lp, M_r)
  4 floor: Lout = max(Lm, min(min_length, L))
The model does the four plain walks; that at most one of them cuts is a property tests/test_host_posttrim.py asserts, not
something the model relies on.  The stage runs behind tests/pairtrim_model.py's and in front of tests/filter_model.py's."""
import os

from tests.clip_model import write_outputs  # noqa: F401  (the texts as a run's files: what the next model reads)
from tests.trim_model import read_fastq, read_of

COUNTERS = ("reads", "bases_in", "bases_out", "n_tail_reads", "n_tail_bases", "polya_reads", "polya_bases", "polyc_reads", "polyc_bases",
            "polyg_reads", "polyg_bases", "polyt_reads", "polyt_bases", "cropped_reads", "cropped_bases", "floored_reads")
LETTERS = b"ACGT"


class Params(object):
    def __init__(self, tail_n=0, poly_x_min_length=0, max_length=(0, 0), min_length=0):
        self.tail_n = int(bool(tail_n))
        self.poly_x_min_length = poly_x_min_length
        self.max_length = tuple(max_length)
        self.min_length = min_length

    def keywords(self):
        """what Engine.posttrim_set takes, and the post-trim report's parameters"""
        return dict(tail_n=self.tail_n, poly_x_min_length=self.poly_x_min_length, max_length_r1=self.max_length[0],
                    max_length_r2=self.max_length[1], min_length=self.min_length)

    @property
    def on(self):
        return bool(self.tail_n or self.poly_x_min_length or any(self.max_length))


def tail_n(seq):
    """-> Ln: the length without the N (or n) bytes at the 3' end"""
    seq = bytes(seq)
    Ln = len(seq)
    while Ln and seq[Ln - 1] & 0xDF == ord("N"):
        Ln -= 1
    return Ln


def walk(seq, P, X):
    """the clip stage's step 3 with the byte X in place of 'G'; -> Lx(X)"""
    seq = bytes(seq)
    Lw = len(seq)
    b = [None] + [seq[Lw - t] & 0xDF for t in range(1, Lw + 1)]  # b[t], t = 1 .. Lw
    mm, T = 0, Lw + 1
    for t in range(1, Lw + 1):
        mm += b[t] != X
        if mm > 5 or (t >= P and 8 * mm > t):
            T = t
            break
    if T - 1 >= P:
        return Lw - max(t for t in range(1, T) if b[t] == X)
    return Lw


def poly_x(seq, P):
    """seq: the bytes step 1 left; -> (Lp, the tail bases: the X of LETTERS with Lx(X) < len(seq), as a bytes object)"""
    seq = bytes(seq)
    if P <= 0:
        return len(seq), b""
    Lx = [walk(seq, P, X) for X in LETTERS]  # four plain walks
    return min(Lx), bytes(X for X, v in zip(LETTERS, Lx) if v < len(seq))


def posttrim_read(seq, read, P):
    """-> (Ln, Lp, tail bases, Lm, Lout) of one insert read; read = 0 (R1) or 1 (R2)"""
    seq = bytes(seq)
    L = len(seq)
    Ln = tail_n(seq) if P.tail_n else L
    Lp, bases = poly_x(seq[:Ln], P.poly_x_min_length)
    M = P.max_length[read]
    Lm = min(Lp, M) if M > 0 else Lp
    return Ln, Lp, bases, Lm, max(Lm, min(P.min_length, L))


def count(table, seq, read, P):
    """adds one read to table[read] (16 counters, COUNTERS) and returns Lout: the read keeps bytes [0, Lout)"""
    L = len(seq)
    Ln, Lp, bases, Lm, Lout = posttrim_read(seq, read, P)
    t = table[read]
    t[0] += 1
    t[1] += L
    t[2] += Lout
    t[3] += Ln < L
    t[4] += L - Ln
    for X in bases:
        k = 5 + 2 * LETTERS.index(X)
        t[k] += 1
        t[k + 1] += Ln - Lp
    t[13] += Lm < Lp
    t[14] += Lp - Lm
    t[15] += Lout > Lm
    return Lout


def new_table():
    return [[0] * len(COUNTERS), [0] * len(COUNTERS)]


def posttrimmed_text(records, read, P, table=None):
    """the fastq text of the records with the post-trim applied record by record"""
    table = table if table is not None else new_table()
    out = []
    for head, seq, qual in records:
        n = count(table, seq, read, P)
        out.append(head + b"\n" + seq[:n] + b"\n+\n" + qual[:n] + b"\n")
    return b"".join(out)


def posttrimmed_outputs(outdir, P):
    """{file name: post-trimmed text} for every fastq.gz of a run without the stage (or of the models of the stages in front of it,
    written with write_outputs), and the counters of all of them"""
    table, texts = new_table(), {}
    for f in sorted(os.listdir(outdir)):
        r = read_of(f)
        if r is not None:
            texts[f] = posttrimmed_text(read_fastq(os.path.join(outdir, f)), r, P, table)
    return texts, table
