"""The 3' trimming of insert reads in plain Python: the definition the device stage (quade_amd/csrc/quade_trim.hip) and the trim
report are tested against.  Three steps in order -- quality trim (cutadapt's / BWA's running-sum rule), adapter trim (leftmost
3' match by substitutions only) and the min_length floor -- give the length a read keeps; its sequence and quality lines are cut
to that many bytes."""
import gzip
import os

COUNTERS = ("reads", "bases_in", "bases_out", "quality_trimmed_reads", "quality_trimmed_bases", "adapter_reads", "adapter_bases",
            "floored_reads")


class Params(object):
    def __init__(self, adapter_r1="", adapter_r2="", quality_cutoff=0, min_overlap=3, max_mismatch_pct=10, min_length=0):
        self.adapters = (adapter_r1.upper().encode() if isinstance(adapter_r1, str) else bytes(adapter_r1).upper(),
                         adapter_r2.upper().encode() if isinstance(adapter_r2, str) else bytes(adapter_r2).upper())
        self.quality_cutoff = quality_cutoff
        self.min_overlap = min_overlap
        self.max_mismatch_pct = max_mismatch_pct
        self.min_length = min_length

    @property
    def on(self):
        return bool(self.adapters[0] or self.adapters[1] or self.quality_cutoff > 0)


def quality_trim_phred(ph, cutoff):
    """ph: Phred values, 5' to 3'; -> the length kept"""
    s, best, stop = 0, 0, len(ph)
    for i in range(len(ph) - 1, -1, -1):
        s += cutoff - ph[i]
        if s < 0:
            break
        if s > best:
            best, stop = s, i
    return stop


def quality_trim(qual, cutoff):
    """qual: the quality line's bytes (unsigned, Phred+33, bytes below 33 count as 0)"""
    if cutoff <= 0:
        return len(qual)
    return quality_trim_phred([max(0, b - 33) for b in bytes(qual)], cutoff)


def adapter_trim(seq, length, adapter, min_overlap, max_mismatch_pct):
    """seq[:length] against the adapter: the leftmost p whose overlap of min(A, length - p) bases has few enough mismatches;
    length when there is none.  Lower case matches, N and every other byte is a mismatch."""
    adapter = bytes(adapter)
    if not adapter:
        return length
    seq = bytes(seq)[:length].upper()
    for p in range(length):
        ov = min(len(adapter), length - p)
        if ov < min_overlap:
            break
        budget, mm = ov * max_mismatch_pct // 100, 0
        for i in range(ov):
            if seq[p + i] != adapter[i]:
                mm += 1
                if mm > budget:  # (only saves time: more mismatches cannot bring it back under the budget)
                    break
        if mm <= budget:
            return p
    return length


def trim_read(seq, qual, read, P):
    """-> (Lq, La, Lout) of one insert read; read = 0 (R1) or 1 (R2)"""
    L = len(seq)
    Lq = quality_trim(qual, P.quality_cutoff)
    La = adapter_trim(seq, Lq, P.adapters[read], P.min_overlap, P.max_mismatch_pct)
    return Lq, La, max(La, min(P.min_length, L))


def count(table, seq, qual, read, P):
    """adds one read to table[read] (8 counters, COUNTERS) and returns the length it keeps"""
    L = len(seq)
    Lq, La, Lout = trim_read(seq, qual, read, P)
    t = table[read]
    t[0] += 1
    t[1] += L
    t[2] += Lout
    t[3] += Lq < L
    t[4] += L - Lq
    t[5] += La < Lq
    t[6] += Lq - La
    t[7] += Lout > La
    return Lout


def new_table():
    return [[0] * len(COUNTERS), [0] * len(COUNTERS)]


def read_fastq(path):
    """[(header, seq, qual)] of a .fastq or .fastq.gz, bytes without line ends"""
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as fh:
        lines = fh.read().split(b"\n")
    return [(lines[i], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def trimmed_text(records, read, P, table=None):
    """the fastq text of the records with the trim applied record by record"""
    table = table if table is not None else new_table()
    out = []
    for head, seq, qual in records:
        n = count(table, seq, qual, read, P)
        out.append(head + b"\n" + seq[:n] + b"\n+\n" + qual[:n] + b"\n")
    return b"".join(out)


def read_of(name):
    """0 / 1 for an output file of R1 / R2 (<dest>_R1.fastq.gz), None for anything else"""
    if name.endswith("_R1.fastq.gz"):
        return 0
    if name.endswith("_R2.fastq.gz"):
        return 1
    return None


def trimmed_outputs(outdir, P):
    """{file name: trimmed text} for every fastq.gz of a run without trimming, and the counters of all of them"""
    table, texts = new_table(), {}
    for f in sorted(os.listdir(outdir)):
        r = read_of(f)
        if r is not None:
            texts[f] = trimmed_text(read_fastq(os.path.join(outdir, f)), r, P, table)
    return texts, table
