"""End clipping, sliding-window quality trimming and poly-G tail trimming of insert reads in plain Python: the definition the
device stage (quade_amd/csrc/quade_clip.hip) and the clip report are tested against (include/quade_hip.h states it in the same
words).  Four steps in order -- the fixed clip of both ends, the window rule, the poly-G rule and the min_length floor -- give the
bytes a read keeps: [f, f + Lout) of its sequence and quality lines.  The stage runs in front of tests/trim_model.py's."""
import gzip
import os

from tests.trim_model import read_fastq, read_of

COUNTERS = ("reads", "bases_in", "bases_out", "front_clipped_reads", "front_clipped_bases", "tail_clipped_reads", "tail_clipped_bases",
            "window_reads", "window_bases", "polyg_reads", "polyg_bases", "floored_reads")


class Params(object):
    def __init__(self, front_clip=(0, 0), tail_clip=(0, 0), window_size=0, window_quality=0, poly_g_min_length=0, min_length=0):
        self.front_clip = tuple(front_clip)
        self.tail_clip = tuple(tail_clip)
        self.window_size = window_size
        self.window_quality = window_quality
        self.poly_g_min_length = poly_g_min_length
        self.min_length = min_length

    def keywords(self):
        """what Engine.clip_set takes, and the clip report's parameters"""
        return dict(front_clip_r1=self.front_clip[0], front_clip_r2=self.front_clip[1], tail_clip_r1=self.tail_clip[0],
                    tail_clip_r2=self.tail_clip[1], window_size=self.window_size, window_quality=self.window_quality,
                    poly_g_min_length=self.poly_g_min_length, min_length=self.min_length)

    @property
    def on(self):
        return bool(any(self.front_clip) or any(self.tail_clip) or self.window_size or self.poly_g_min_length)


def window_phred(ph, W, Q):
    """ph: Phred values, 5' to 3'; -> Lw: the first start whose W values sum to less than Q * W, all of them when there is none"""
    s = [0]
    for v in ph:
        s.append(s[-1] + v)
    for p in range(len(ph) - W + 1):
        if s[p + W] - s[p] < Q * W:
            return p
    return len(ph)


def window(qual, W, Q):
    """qual: the quality line's bytes (unsigned, Phred+33, bytes below 33 count as 0)"""
    if W <= 0:
        return len(qual)
    return window_phred([max(0, b - 33) for b in bytes(qual)], W, Q)


def poly_g(seq, P):
    """seq: the sequence bytes the earlier steps left; -> Lg"""
    seq = bytes(seq)
    Lw = len(seq)
    if P <= 0:
        return Lw
    b = [None] + [seq[Lw - t] & 0xDF for t in range(1, Lw + 1)]  # b[t], t = 1 .. Lw
    mm, T = 0, Lw + 1
    for t in range(1, Lw + 1):
        mm += b[t] != ord("G")
        if mm > 5 or (t >= P and 8 * mm > t):
            T = t
            break
    if T - 1 >= P:
        return Lw - max(t for t in range(1, T) if b[t] == ord("G"))
    return Lw


def clip_read(seq, qual, read, P):
    """-> (f, Lc, Lw, Lg, Lout) of one insert read; read = 0 (R1) or 1 (R2)"""
    seq, qual = bytes(seq), bytes(qual)
    L = len(seq)
    f = min(P.front_clip[read], L)
    Lc = max(0, L - f - P.tail_clip[read])
    Lw = window(qual[f:f + Lc], P.window_size, P.window_quality)
    Lg = poly_g(seq[f:f + Lw], P.poly_g_min_length)
    return f, Lc, Lw, Lg, max(Lg, min(P.min_length, L - f))


def count(table, seq, qual, read, P):
    """adds one read to table[read] (12 counters, COUNTERS) and returns (f, Lout): the read keeps bytes [f, f + Lout)"""
    L = len(seq)
    f, Lc, Lw, Lg, Lout = clip_read(seq, qual, read, P)
    t = table[read]
    t[0] += 1
    t[1] += L
    t[2] += Lout
    t[3] += f > 0
    t[4] += f
    t[5] += Lc < L - f
    t[6] += L - f - Lc
    t[7] += Lw < Lc
    t[8] += Lc - Lw
    t[9] += Lg < Lw
    t[10] += Lw - Lg
    t[11] += Lout > Lg
    return f, Lout


def new_table():
    return [[0] * len(COUNTERS), [0] * len(COUNTERS)]


def clipped_text(records, read, P, table=None):
    """the fastq text of the records with the clip applied record by record"""
    table = table if table is not None else new_table()
    out = []
    for head, seq, qual in records:
        f, n = count(table, seq, qual, read, P)
        out.append(head + b"\n" + seq[f:f + n] + b"\n+\n" + qual[f:f + n] + b"\n")
    return b"".join(out)


def clipped_outputs(outdir, P):
    """{file name: clipped text} for every fastq.gz of a run without the stage, and the counters of all of them"""
    table, texts = new_table(), {}
    for f in sorted(os.listdir(outdir)):
        r = read_of(f)
        if r is not None:
            texts[f] = clipped_text(read_fastq(os.path.join(outdir, f)), r, P, table)
    return texts, table


def write_outputs(texts, outdir):
    """the texts as the fastq.gz files of a run: what the models of the stages behind this one (trim_model.trimmed_outputs,
    pairtrim_model.trimmed_outputs, filter_model.filtered_outputs) read, so that the models chain"""
    os.makedirs(outdir, exist_ok=True)
    for name, text in texts.items():
        with gzip.open(os.path.join(outdir, name), "wb", compresslevel=1) as fh:
            fh.write(text)
    return outdir
