"""What the read stages' tests share (tests/test_gpu_{quality,cycle,clip,trim,pairtrim,filter,stage_tables}.py and their host
tests): the byte alphabets, fastq texts with their record tables, the dataset scaffolding around a stage's insert reads, the conf
writer, the child-process CLI, the oracle's run and the comparison of a run's files.  An ordinary module: test modules import it,
never each other."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from tests import filter_model as FM
from tests import pairtrim_model as PM
from tests import qstats_model as QM
from tests import trim_model as TM
from tests.run_support import _conf, _gz, _write_fastq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LENS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 151, 300)
# 330: a line of 330 bytes fits its slab of 21 aligned words at offsets 0 .. 6 mod 16 only -- both paths in one launch
LONG_LENS = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 151, 255, 256, 257, 300, 330, 2049)
# every printable quality, bytes below 33 and from 0x80 on (the clamp, the unsigned rule); never '\n' or '\r' (line ends)
QUALS = bytes(range(33, 127)) + bytes([0, 1, 9, 31, 32, 127, 128, 129, 200, 254, 255])
BASES = b"ACGTNnacgtRYKM.*"
RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


def _rc(s):
    return bytes(s).translate(RC)[::-1]


def _read(path):
    with open(path) as fh:
        return fh.read()


def _barcodes(S):
    """S distinct 16-base barcodes"""
    return ["".join("ACGT"[(i >> (2 * k)) & 3] for k in range(16)) for i in range(S)]


def _engine(S, enable=True):
    eng = hb.Engine(0)
    eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
    eng.set_barcodes(_barcodes(S))
    if enable:
        eng.qstats_enable(True)
    return eng


# ---- fastq texts with their record tables ----------------------------------------------------------------------------------------
def _text(rng, n, lens=LENS):
    """A fastq text of n records with its record table (qd_dev_fastq_scan's layout) and the records' (seq, qual) bytes.  Names of
    1 .. 24 bytes move the lines over every offset mod 16; a third of the records end their lines with CRLF; the first records'
    qualities walk through QUALS."""
    parts, recs, pairs, pos, walk = [], np.zeros((n, 6), dtype=np.uint32), [], 0, 0
    for i in range(n):
        L = int(lens[int(rng.integers(0, len(lens)))])
        name = b"r%d" % i + b"x" * int(rng.integers(0, 20))
        nl = b"\r\n" if rng.integers(0, 3) == 0 else b"\n"
        seq = bytes(BASES[int(v)] for v in rng.integers(0, len(BASES), L))
        if walk < len(QUALS):
            qual = bytes(QUALS[(walk + k) % len(QUALS)] for k in range(L))
            walk += L
        else:
            qual = bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L))
        rec = b"@" + name + b" 1:N:0" + nl + seq + nl + b"+" + nl + qual + nl
        seq_at = pos + 1 + len(name) + 6 + len(nl)
        recs[i] = (pos, pos + 1, len(name), seq_at, L, seq_at + L + len(nl) + 1 + len(nl))
        parts.append(rec)
        pairs.append((seq, qual))
        pos += len(rec)
    return b"".join(parts), recs, pairs


def _text_from(rng, cases):
    """A fastq text of the cases' records (name of the case, seq, qual) with its record table, built as _text builds it: names of
    1 .. 24 bytes move the lines over every offset mod 16, a third of the records end their lines with CRLF."""
    parts, recs, pos = [], np.zeros((len(cases), 6), dtype=np.uint32), 0
    for i, (_, seq, qual) in enumerate(cases):
        L = len(seq)
        name = b"r%d" % i + b"x" * int(rng.integers(0, 20))
        nl = b"\r\n" if rng.integers(0, 3) == 0 else b"\n"
        rec = b"@" + name + b" 1:N:0" + nl + seq + nl + b"+" + nl + qual + nl
        seq_at = pos + 1 + len(name) + 6 + len(nl)
        recs[i] = (pos, pos + 1, len(name), seq_at, L, seq_at + L + len(nl) + 1 + len(nl))
        parts.append(rec)
        pos += len(rec)
    return b"".join(parts), recs


class Stage(object):
    """n pairs: R1 and R2 texts drawn apart (a pair's two reads differ in length), tables, records; the quality counters' stage"""

    def __init__(self, seed, n, lens=LENS):
        rng = np.random.default_rng(seed)
        self.n = n
        self.t1, self.r1, self.p1 = _text(rng, n, lens)
        self.t2, self.r2, self.p2 = _text(rng, n, lens)

    def model(self, S, codes):
        return QM.table(S, [(int(c), a, b) for c, a, b in zip(codes, self.p1, self.p2)])

    def run(self, eng, codes):
        eng.dev_qstats(self.t1, self.r1, self.t2, self.r2, np.asarray(codes, dtype=np.uint16))


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
N_SAMPLES = 6
AD1, AD2 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
# [trim] with adapters, a cutoff and pair_overlap, and [filter]: the sections of the runs behind several stages, and what the
# models take for them
TRIMS = "[trim]\nadapter_R1 : %s\nadapter_R2 : %s\nquality_cutoff : 20\nmin_length : 25\npair_overlap : True\npair_max_mismatches : 3\n" % (AD1, AD2)
FILTER = "[filter]\nmin_length : 40\nmax_n : 5\nmax_unqualified_pct : 40\nmin_mean_quality : 20\nmin_complexity_pct : 30\n"
P_F = FM.Params(min_length=40, max_n=5, max_unqualified_pct=40, min_mean_quality=20, min_complexity_pct=30)
P_PAIR = PM.Params(max_mismatches=3, min_length=25)
P_TRIM = TM.Params(AD1, AD2, quality_cutoff=20, min_length=25)
TRIM_KW = dict(adapter_r1=AD1, adapter_r2=AD2, quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=25)
POLY_G = 0  # the sample all of whose insert reads are poly-G in _filter_inserts' datasets


def _cli(conf, work, ranks=0, timeout=180):
    """bin/Quade.py (or the launcher with `ranks` processes on GPU 0) in a child process under its own time limit"""
    os.makedirs(work, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", str(conf)]
    if ranks:
        env.update(QUADE_DIST_TRANSPORT="files", QUADE_DEVICE="0")
        cmd = [sys.executable, "-m", "quade_amd.launch", "-n", str(ranks), "-c", str(conf)]
    r = subprocess.run(cmd, cwd=str(work), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r


def MM_far_barcodes():
    """8 + 8 base barcodes no two of which collide under the budgets (1, 1)"""
    from quade_amd import synth
    return [(b[:8], b[8:]) for b in synth.make_far_barcodes(N_SAMPLES, 8, 8, 1, 1, seed=3)]


class Draw(object):
    """what an insert-read generator draws from: the dataset's rng, rnd(L, alphabet) a random sequence, q(L, lo, hi) random
    qualities lo .. hi - 1"""

    def __init__(self, rng):
        self.rng = rng

    def rnd(self, L, alphabet="ACGT"):
        return "".join(self.rng.choice(list(alphabet), L))

    def q(self, L, lo, hi):
        return "".join(chr(33 + int(v)) for v in self.rng.integers(lo, hi, L))


def _dataset(d, seed, n_chunks, n, bgzf, inserts, malformed, sample_first=False, one_off=False):
    """n_chunks x n pairs as four fastq.gz files per chunk (BGZF when bgzf), dual 8 + 8 index over a sheet of N_SAMPLES far
    barcodes -> (files, samples).  inserts(draw, i, sample, kind) -> [(seq, qual) of R1, of R2] makes pair i's insert reads;
    sample_first: the pair's sample and kind (0: a random index, 2 and 3: low index qualities) are drawn in front of them and
    passed, else behind them (None is passed).  malformed(n) -> {stream: records whose quality line gets one byte too many}:
    dropped inside their own stream, which shifts the streams against each other as in the reference.  one_off: a tenth of the index
    reads one substitution from a sample's barcode (the mismatch rescue's food)."""
    rng = np.random.default_rng(seed)
    draw = Draw(rng)
    bcs = sorted(set(MM_far_barcodes()))[:N_SAMPLES]
    os.makedirs(d, exist_ok=True)
    files = {"seq_R1": [], "seq_R2": [], "index_R1": [], "index_R2": []}
    for c in range(n_chunks):
        names = ["SIM:1:FC:%d:%d:%d" % (c, i, i * 7) + "x" * (i % 5) for i in range(n)]
        streams = {k: ([], []) for k in files}
        for i in range(n):
            sample = kind = None
            if sample_first:
                sample, kind = int(rng.integers(0, len(bcs))), int(rng.integers(0, 10))
            for key, (s, qual) in zip(("seq_R1", "seq_R2"), inserts(draw, i, sample, kind)):
                streams[key][0].append(s)
                streams[key][1].append(qual)
            if not sample_first:
                sample, kind = int(rng.integers(0, len(bcs))), int(rng.integers(0, 10))
            for k, key in enumerate(("index_R1", "index_R2")):
                s = bcs[sample][k]
                if kind == 0:
                    s = draw.rnd(8)
                elif kind == 1 and one_off:
                    p = int(rng.integers(0, 8))
                    s = s[:p] + ("A" if s[p] != "A" else "C") + s[p + 1:]
                streams[key][0].append(s)
                streams[key][1].append(draw.q(8, 15 if kind in (2, 3) else 30, 41))
        for key, where in malformed(n).items():
            for i in where:
                streams[key][1][i] += "I"
        for key, (ss, qs) in streams.items():
            p = os.path.join(d, "C%d_%s.fastq.gz" % (c, key))
            _write_fastq(p, names, ss, qs)
            if bgzf:
                text = _gz(p)
                assert hb.load_library().qd_write_gzip_file(p.encode(), hb._ptr(np.frombuffer(text, dtype=np.uint8)), len(text), 1, -1) == 0
            files[key].append(p)
    return files, [("S%d" % i, b1, b2) for i, (b1, b2) in enumerate(bcs)]


def _early_places(n):
    """a few malformed records of R1 and one of index read 2"""
    return {"seq_R1": (3, n // 2, n - 2), "index_R2": (7,)}


def _plain_inserts(g, i, sample, kind):
    """insert reads of 30 .. 151 bases with N and a wide quality range"""
    out = []
    for _ in range(2):
        L = int(g.rng.integers(30, 152))
        out.append((g.rnd(L, "ACGTACGTACGTN" if i % 3 else "ACGTn"), g.q(L, 2, 42)))
    return out


def _plain_dataset(d, seed, n_chunks, n, bgzf, one_off=False):
    return _dataset(d, seed, n_chunks, n, bgzf, _plain_inserts, _early_places, one_off=one_off)


def _same_places(n):
    """malformed records at the same places of all four streams: each stream drops its own, and the pairs stay together"""
    return {key: (n // 2, n - 2) for key in ("seq_R1", "seq_R2", "index_R1", "index_R2")}


def _fragment_reads(g, i, Lr, ad, src):
    """a read of Lr bases off a fragment (src, then the adapter read through, then random bases), a fifth unrelated and rich in N;
    every other pair with up to three substitutions, N or lower case"""
    s = list((src + ad + g.rnd(151))[:Lr]) if i % 5 else list(g.rnd(Lr, "ACGTN"))
    for _ in range(int(g.rng.integers(0, 4)) if i % 2 else 0):
        s[int(g.rng.integers(0, Lr))] = "ACGTNn"[int(g.rng.integers(0, 6))]
    return "".join(s)


def _filter_inserts(g, i, sample, kind):
    """insert reads of a fragment of 15 .. 330 bases with food for every rule of the filter: a ninth of the pairs has reads of
    30 .. 44 bases and the others of 60 .. 151, every insert read of sample POLY_G is poly-G, a thirteenth of the pairs has
    qualified but low qualities (15 .. 19) and another thirteenth unqualified ones, both in front of 8 good bases at the 3' end,
    which keep a quality cutoff from trimming them away; the others half with a low-quality 3' tail"""
    rng, out = g.rng, []
    I = int(rng.integers(15, 151)) if rng.integers(0, 2) else int(rng.integers(151, 331))
    frag = g.rnd(I)
    for ad, src in ((AD1, frag), (AD2, _rc(frag.encode()).decode())):
        Lr = int(rng.integers(30, 45)) if i % 9 == 3 else int(rng.integers(60, 152))
        s = _fragment_reads(g, i, Lr, ad, src)
        if sample == POLY_G and kind != 0:
            s = "G" * Lr
        tail = int(rng.integers(0, min(Lr, 60) // 2)) if rng.integers(0, 2) else 0
        out.append((s.lower() if i % 11 == 0 else s,
                    g.q(Lr - 8, 15, 20) + g.q(8, 38, 42) if i % 13 == 1 else g.q(Lr - 8, 2, 24) + g.q(8, 38, 42) if i % 13 == 2
                    else g.q(Lr - tail, 22, 42) + g.q(tail, 2, 24)))
    return out


def _filter_dataset(d, seed, n_chunks, n, bgzf):
    return _dataset(d, seed, n_chunks, n, bgzf, _filter_inserts, _same_places, sample_first=True)


def _write_conf(path, files, samples, flags=(True, True, True), gpu="", quality=False, index_extra="", chunks=None, extra=""):
    """dual 8 + 8 index, minimal_qual 25, batch_pairs 1000; quality: quality_report on; index_extra: lines for [index]; chunks:
    these chunks only; extra: sections appended ([trim], [filter])"""
    if chunks is not None:
        files = {k: [v[c] for c in chunks] for k, v in files.items()}
    _conf(str(path), files, True, ((1, 8), (1, 8), None, None), 25, samples, flags, "[gpu]\nbatch_pairs : 1000\n" + gpu)
    text = _read(path)
    if quality:
        text = text.replace("[output]\n", "[output]\nquality_report : True\n", 1)
    if index_extra:
        text = text.replace("index2_end : 8\n", "index2_end : 8\n" + index_extra, 1)
    open(path, "w").write(text + extra)


def _oracle_run(conf, ref_dir):
    """the oracle's run of the conf (it knows none of the stages' sections) into ref_dir -> its sample set"""
    os.makedirs(ref_dir, exist_ok=True)
    return qo.run_quade(str(conf), outdir=str(ref_dir))[0]


def _check_files(mine, texts, only=None, at_least=3):
    """the run's fastq.gz files are texts' ({file: text}; only(file): those it was to write), byte for byte"""
    want = sorted(f for f in texts if only is None or only(f))
    assert sorted(f for f in os.listdir(str(mine)) if f.endswith(".fastq.gz")) == want and len(want) >= at_least
    for f in want:
        assert _gz(os.path.join(str(mine), f)) == texts[f], f


def _check_main_report(mine, ref, only=None):
    """Quade_report.csv is the oracle's behind the dated first line: the stages leave the assignments alone"""
    a, b = (_read(os.path.join(str(d), "Quade_report.csv")).split("\n") for d in (mine, ref))
    assert a[0].startswith("Program Quade 0.3.2\tDate ") and (only is not None or a[1:] == b[1:])


def _check_report(mine, module, *args):
    """a stage's report file is report_lines(*args) of its module; args[0] None: the file is not there"""
    path = os.path.join(str(mine), module.REPORT_NAME)
    if args[0] is None:
        assert not os.path.exists(path)
    else:
        assert _read(path) == "\n".join(module.report_lines(*args)) + "\n"


def _one_sample_conf(tmp_path, extra="", gpu=""):
    """a conf over one empty fastq file and one sample, for the host tests of QuadeConf: extra = the sections under test"""
    f = tmp_path / "reads.fastq"
    f.write_text("")
    txt = "[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}\nseq_R2 : {0}\nindex_R1 : {0}\nindex_R2 : {0}\n".format(f)
    txt += "[index]\nindex2 : True\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\nindex1_end : 8\nindex2_start : 1\nindex2_end : 8\n"
    txt += "[output]\nwrite_pass : True\nwrite_fail : True\nwrite_undetermined : True\n" + extra + gpu
    txt += "[sample1]\nname : S1\nindex1_seq : ACAGACAG\nindex2_seq : CTTGCTTG\n"
    p = tmp_path / "conf.txt"
    p.write_text(txt)
    return str(p)
