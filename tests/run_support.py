"""What several test modules share to run whole datasets and single kernels: generated fastq datasets and their conf files, the
CLI driver in process, the comparison of two output directories, the record tables of the routing tests, the forged DEFLATE corpus as files
and the C99 client's build.  An ordinary module: no test module imports another one."""
import gzip
import os

import numpy as np

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from tests import deflate_forge as F
from tests import route_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gz(path):
    with gzip.open(path, "rb") as fh:
        return fh.read()


_LAST_PIPE_STATS = {}


def _run_cli(conf, workdir):
    from quade_amd.quade import Quade
    old = os.getcwd()
    os.chdir(workdir)
    try:
        q = Quade(conf_file=conf)
        assert q() == 0
        _LAST_PIPE_STATS["stats"] = getattr(q, "pipe_stats", None)
    finally:
        os.chdir(old)


def _compare_dirs(mine, ref):
    fm = sorted(f for f in os.listdir(mine) if f.endswith(".fastq.gz"))
    fr = sorted(f for f in os.listdir(ref) if f.endswith(".fastq.gz"))
    assert fm == fr
    for f in fr:
        assert _gz(os.path.join(mine, f)) == _gz(os.path.join(ref, f)), f
    with open(os.path.join(mine, "Quade_report.csv")) as fh:
        a = fh.read().split("\n")
    with open(os.path.join(ref, "Quade_report.csv")) as fh:
        b = fh.read().split("\n")
    assert a[0].startswith("Program Quade 0.3.2\tDate ")
    assert a[1:] == b[1:]


def _write_fastq(path, names, seqs, quals, plus="+"):
    with gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb") as fh:
        for n, s, q in zip(names, seqs, quals):
            fh.write(("@%s\n%s\n%s\n%s\n" % (n, s, plus, q)).encode("latin-1"))


def _make_dataset(d, rng, n_chunks, n, dual, idx_len, barcodes, trunc=False, malformed=False, plain=False, bgzf=False):
    """barcodes: list of (b1, b2) expected at the start of index read 1 / 2.  bgzf: the .gz files in bgzip's block layout (what the
    device inflates) instead of one gzip member."""
    ext = ".fastq" if plain else ".fastq.gz"
    files = {"seq_R1": [], "seq_R2": [], "index_R1": [], "index_R2": []}
    for c in range(n_chunks):
        names = ["SIM:1:FC:%d:%d:%d %d:N:0:" % (c, i, i * 7, 1) for i in range(n)]
        def rnd(L):
            return "".join(rng.choice(list("ACGT"), L))
        def q(L, lo=30):
            return "".join(chr(33 + int(v)) for v in rng.integers(lo, 41, L))
        r1 = [rnd(30) for _ in range(n)]
        r2 = [rnd(30) for _ in range(n)]
        i1, i2, q1, q2 = [], [], [], []
        for i in range(n):
            b = barcodes[int(rng.integers(0, len(barcodes)))]
            kind = int(rng.integers(0, 10))
            parts = []
            for k in range(2 if dual else 1):
                s = b[k] + rnd(idx_len - len(b[k]))
                if kind == 0:
                    p = int(rng.integers(0, len(b[k])))
                    s = s[:p] + "N" + s[p + 1:]
                elif kind == 1:
                    s = s.lower()
                elif kind == 2:
                    s = rnd(idx_len)
                if trunc and rng.integers(0, 4) == 0:
                    s = s[:int(rng.integers(0, idx_len))]
                qq = q(len(s), lo=20 if rng.integers(0, 3) == 0 else 30)
                parts.append((s, qq))
            i1.append(parts[0][0]); q1.append(parts[0][1])
            if dual:
                i2.append(parts[1][0]); q2.append(parts[1][1])
        qr1 = [q(30) for _ in range(n)]
        qr2 = [q(30) for _ in range(n)]
        if malformed and n > 5:
            qr1[3] = qr1[3] + "I"        # R1 record 3 dropped -> R1 shifts against the others
            q1[n // 2] = q1[n // 2][:-1] if q1[n // 2] else "I"  # an index record dropped
        for key, (nm, ss, qs) in {"seq_R1": (names, r1, qr1), "seq_R2": (names, r2, qr2),
                                  "index_R1": (names, i1, q1), "index_R2": (names, i2, q2)}.items():
            if key == "index_R2" and not dual:
                continue
            p = os.path.join(d, "C%d_%s%s" % (c, key, ext))
            _write_fastq(p, nm, ss, qs, plus="+" if c % 2 == 0 else "+" + "x")
            if bgzf and not plain:
                from quade_amd import hip_backend as hb
                text = _gz(p)
                buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
                assert hb.load_library().qd_write_gzip_file(p.encode(), hb._ptr(buf), len(text), 1, -1) == 0
            files[key].append(p)
    return files


def _conf(path, files, dual, pos, minq, samples, flags=(True, True, True), gpu=""):
    i1, i2, m1, m2 = pos
    txt = "[quality]\nminimal_qual : %d\n[fastq]\n" % minq
    for k in ("seq_R1", "seq_R2", "index_R1") + (("index_R2",) if dual else ()):
        txt += "%s : %s\n" % (k, "  ".join(files[k]))
    txt += "[index]\nindex2 : %s\nmolecular1 : %s\nmolecular2 : %s\n" % (dual, bool(m1), bool(m2))
    txt += "index1_start : %d\nindex1_end : %d\n" % i1
    if dual:
        txt += "index2_start : %d\nindex2_end : %d\n" % i2
    if m1:
        txt += "molecular1_start : %d\nmolecular1_end : %d\n" % m1
    if m2:
        txt += "molecular2_start : %d\nmolecular2_end : %d\n" % m2
    txt += "[output]\nwrite_pass : %s\nwrite_fail : %s\nwrite_undetermined : %s\n" % flags
    txt += gpu
    for i, (name, b1, b2) in enumerate(samples):
        txt += "[sample%d]\nname : %s\nindex1_seq : %s\n" % (i + 1, name, b1)
        if dual:
            txt += "index2_seq : %s\n" % b2
    with open(path, "w") as fh:
        fh.write(txt)


SCENARIOS = {
    # name: dual, idx_len, positions (1-based incl.), min_qual, flags, trunc, malformed, plain, gpu section
    "single_plain": dict(dual=False, idx_len=8, pos=((1, 8), None, None, None), minq=0, plain=True),
    "single_mol_ext": dict(dual=False, idx_len=12, pos=((1, 6), None, (7, 12), None), minq=25),
    "dual_mol_fail": dict(dual=True, idx_len=14, pos=((1, 8), (1, 8), (9, 14), (9, 14)), minq=25,
                          gpu="[gpu]\nbatch_pairs : 37\nslots : 2\n"),
    "dual_offset_windows": dict(dual=True, idx_len=10, pos=((2, 7), (3, 9), (1, 3), None), minq=30),
    "flags_off": dict(dual=True, idx_len=8, pos=((1, 8), (1, 8), None, None), minq=25, flags=(True, False, False)),
    "truncated_generic": dict(dual=True, idx_len=8, pos=((1, 8), (1, 8), (5, 8), None), minq=20, trunc=True,
                              gpu="[gpu]\nbatch_pairs : 50\n"),
    "malformed_desync": dict(dual=True, idx_len=8, pos=((1, 8), (1, 8), None, None), minq=25, malformed=True,
                             gpu="[gpu]\nbatch_pairs : 16\nslots : 3\n"),
    # two contexts (both on GPU 0 here): batches fed round-robin over pinned slots / a pipeline each with the chunks dealt out --
    # output order must still equal input order
    "two_engines_round_robin": dict(dual=True, idx_len=8, pos=((1, 8), (1, 8), None, None), minq=25,
                                    gpu="[gpu]\ndevices : 0 0\nbatch_pairs : 23\nslots : 2\n"),
    # three host threads take chunks from a queue; per-chunk parts merged in chunk order
    "chunk_workers_threads": dict(dual=True, idx_len=14, pos=((1, 8), (1, 8), (9, 14), None), minq=25, malformed=True,
                                  gpu="[gpu]\nchunk_workers : 3\nbatch_pairs : 31\nslots : 2\n"),
    # "all": every device the library sees (one on this box)
    "devices_all": dict(dual=False, idx_len=8, pos=((1, 8), None, None, None), minq=20, gpu="[gpu]\ndevices : all\n"),
    # dual 10 bp indexes (fused barcode of 20 bytes): the wide form of the fast kernel, incl. truncated reads
    # (listed exceptions redone by the fixup kernel) and a molecular index behind the second barcode
    "dual_10bp_wide_fast": dict(dual=True, idx_len=12, pos=((1, 10), (1, 10), None, None), minq=25),
    "dual_10bp_umi_truncated": dict(dual=True, idx_len=16, pos=((1, 10), (2, 11), None, (12, 16)), minq=20, trunc=True,
                                    gpu="[gpu]\nbatch_pairs : 64\n"),
    # a molecular index of 11 bases behind the barcode of BOTH index reads (rows of 20 bytes in both streams, 22 molecular bytes per
    # pair: the fast kernel's RowsU2 shape, r05), whole reads and truncated ones (the listed exceptions redone by the fixup kernel)
    "dual_umi_in_both_reads": dict(dual=True, idx_len=19, pos=((1, 8), (1, 8), (9, 19), (9, 19)), minq=25),
    "dual_umi_in_both_reads_truncated": dict(dual=True, idx_len=17, pos=((1, 8), (1, 8), (9, 17), (9, 17)), minq=20, trunc=True,
                                             gpu="[gpu]\nbatch_pairs : 64\n"),
    "wide_window_generic": dict(dual=False, idx_len=24, pos=((1, 20), None, (21, 24), None), minq=10),
    # truncated reads on a plan the fast kernel does not take: the generic kernel needs every read's length
    "wide_window_truncated": dict(dual=False, idx_len=24, pos=((1, 20), None, (21, 24), None), minq=10, trunc=True,
                                  gpu="[gpu]\nbatch_pairs : 64\n"),
}


def _scan(text, at_eof=True, names=True, need=0, line_cap=None):
    from quade_amd import hip_backend as hb
    lib = hb.load_library()
    buf = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, np.uint8)
    cap = line_cap if line_cap is not None else (text.count(b"\n") + 8)
    recs = np.zeros((cap // 4 + 2, 6), dtype=np.uint32)
    res = np.zeros(8, dtype=np.uint32)
    n = lib.qd_dev_fastq_scan(0, hb._ptr(buf), len(text), int(at_eof), int(names), int(need), max(cap, 4), hb._ptr(recs), recs.shape[0], hb._ptr(res))
    assert n >= 0, n
    return int(n), recs[:min(n, recs.shape[0])], res


def _bgzip(path, data):
    from quade_amd import hip_backend as hb
    buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, np.uint8)
    assert hb.load_library().qd_write_gzip_file(str(path).encode(), hb._ptr(buf), len(data), 1, -1) == 0


def _dataset(d, rng, n_chunks, n, S, malformed=(), fmt="bgzf", read_len=60, trunc=False):
    """Dual 8 + 8 bp index with a 6-base molecular index behind the first barcode; returns (files, samples)."""
    bcs = set()
    while len(bcs) < S:
        bcs.add(("".join(rng.choice(list("ACGT"), 8)), "".join(rng.choice(list("ACGT"), 8))))
    bcs = sorted(bcs)
    files = {"seq_R1": [], "seq_R2": [], "index_R1": [], "index_R2": []}
    A = np.frombuffer(b"ACGT", dtype=np.uint8)
    for c in range(n_chunks):
        pick = rng.integers(0, S, n)
        kind = rng.integers(0, 12, n)
        recs = {k: [] for k in files}
        r1 = A[rng.integers(0, 4, (n, read_len))]
        r2 = A[rng.integers(0, 4, (n, read_len))]
        q1 = rng.integers(33 + 30, 33 + 41, (n, read_len)).astype(np.uint8)
        q2 = rng.integers(33 + 30, 33 + 41, (n, read_len)).astype(np.uint8)
        for i in range(n):
            name = "SIM:1:FC:%d:%d:%d" % (c, i, i * 7)
            b1, b2 = bcs[pick[i]]
            i1 = b1 + "".join(rng.choice(list("ACGT"), 6))
            i2 = b2
            if kind[i] == 0:
                i1 = "N" + i1[1:]
            elif kind[i] == 1:
                i1, i2 = i1.lower(), i2.lower()
            elif kind[i] == 2:
                i2 = "".join(rng.choice(list("ACGT"), 8))
            if trunc and kind[i] == 3:
                i1 = i1[:int(rng.integers(0, 14))]
            qi1 = "".join(chr(33 + int(v)) for v in rng.integers(20 if kind[i] == 4 else 30, 41, len(i1)))
            qi2 = "".join(chr(33 + int(v)) for v in rng.integers(30, 41, len(i2)))
            rows = {"seq_R1": (r1[i].tobytes().decode(), q1[i].tobytes().decode(), "1"), "seq_R2": (r2[i].tobytes().decode(), q2[i].tobytes().decode(), "2"),
                    "index_R1": (i1, qi1, "1"), "index_R2": (i2, qi2, "2")}
            for k, (s, q, rd) in rows.items():
                if (c, k, i) in malformed:
                    q = q + "I"
                recs[k].append("@%s %s:N:0:\n%s\n+\n%s\n" % (name, rd, s, q))
        for k in files:
            data = "".join(recs[k]).encode()
            if fmt == "bgzf":
                path = os.path.join(d, "C%d_%s.fastq.gz" % (c, k))
                _bgzip(path, data)
            elif fmt == "gz":
                path = os.path.join(d, "C%d_%s.fastq.gz" % (c, k))
                with gzip.open(path, "wb", compresslevel=1) as fh:
                    fh.write(data)
            else:
                path = os.path.join(d, "C%d_%s.fastq" % (c, k))
                with open(path, "wb") as fh:
                    fh.write(data)
            files[k].append(path)
    return files, [("S%d" % i, b1, b2) for i, (b1, b2) in enumerate(bcs)]


def _run_and_compare(tmp_path, files, samples, gpu, flags=(True, True, True), expect_stats=None):
    conf = tmp_path / "conf.txt"
    _conf(str(conf), files, True, ((1, 8), (1, 8), (9, 14), None), 25, samples, flags, gpu)
    ref_dir, my_dir = tmp_path / "ref", tmp_path / "mine"
    ref_dir.mkdir()
    my_dir.mkdir()
    sset, _ = qo.run_quade(str(conf), outdir=str(ref_dir))
    from quade_amd.quade import Quade
    old = os.getcwd()
    os.chdir(my_dir)
    try:
        q = Quade(conf_file=str(conf))
        assert q() == 0
    finally:
        os.chdir(old)
    from quade_amd.sample import Sample
    assert Sample.COUNTS() == sset.counts()
    _compare_dirs(str(my_dir), str(ref_dir))
    assert q.use_pipe
    return q.pipe_stats


# the plans of the oracle comparison (single with extension, dual with offset windows, molecular part in both reads, truncated) and
# the two more that the GPU sweep adds (dual 10 bp, the 20 + 4 wide window)
ORACLE_PLANS = ("single_mol_ext", "dual_offset_windows", "dual_umi_in_both_reads_truncated")


PLANS = ORACLE_PLANS + ("dual_10bp_wide_fast", "wide_window_generic")


NAME_BYTES = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_-/#"


def make_plan(name):
    sc = SCENARIOS[name]
    z = [(p[0] - 1, p[1]) if p else (0, 0) for p in sc["pos"]]  # (1-based inclusive) -> (0-based start, end): src/Quade.py:105-116
    return hb.make_plan(sc["dual"], sc["minq"], z[0], z[1], z[2], z[3])


def rand_bytes(rng, L, alphabet):
    return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))


def build_fastq(reads, styles):
    """[(name, seq, qual)] -> (fastq text, its record table uint32[n, 6] in qd_dev_fastq_scan's layout).  style bits: 1 = CRLF line
    ends, 2 = text behind the '+', 4 = a comment behind the name (blanks behind the '@' of an empty name)."""
    parts, table, pos = [], np.zeros((len(reads), 6), dtype=np.uint32), 0
    for i, ((name, seq, qual), style) in enumerate(zip(reads, styles)):
        nl = b"\r\n" if style & 1 else b"\n"
        comment = (b" 1:N:0:" if name else b" \t") if style & 4 else b""
        head = b"@" + name + comment
        plus = b"+" + name if style & 2 else b"+"
        rec = head + nl + seq + nl + plus + nl + qual + nl
        seq_at = pos + len(head) + len(nl)
        # (an empty name is found behind every blank of the header line, the '\r' included: where its '\n' is)
        table[i] = (pos, pos + 1 if name else seq_at - 1, len(name), seq_at, len(seq), seq_at + len(seq) + len(nl) + len(plus) + len(nl))
        parts.append(rec)
        pos += len(rec)
    return b"".join(parts), table


def reads_of(text, table):
    return [RM.read_of(text, r) for r in table]


def ragged_index_reads(rng, n, start, width, barcodes, k):
    """index reads of stream k: a sample's barcode at the window's start (or random bases), then as read, lower case, with an N,
    truncated, or over-long; qualities on both sides of every threshold in use"""
    out = []
    for i in range(n):
        b = barcodes[int(rng.integers(0, len(barcodes)))][k]
        s = b"A" * start + b + rand_bytes(rng, int(rng.integers(0, 12)), b"ACGT")
        kind = i % 10
        if kind == 0:
            s = s.lower()
        elif kind == 1 and width:
            p = start + int(rng.integers(0, width))
            s = s[:p] + b"N" + s[p + 1:]
        elif kind == 2:
            s = rand_bytes(rng, len(s), b"ACGTacgtN")
        elif kind == 3:
            s = s[:(i // 10) % (len(s) + 1)]
        elif kind == 4:
            s = s + rand_bytes(rng, (255, 256, 300)[i % 3] - len(s), b"ACGTn")
        out.append((b"idx%d" % i, s, rand_bytes(rng, len(s), bytes(range(33 + (18 if i % 3 == 0 else 31), 33 + 41)))))
    return out


def write_corpus(d):
    """the corpus as files for tests/native/inflate3_lane_test.cpp: cNN.deflate + cNN.txt | cNN.illegal + cNN.tags (name, tags)"""
    for i, (name, raw, text, tags) in enumerate(F.corpus()):
        stem = os.path.join(str(d), "c%02d" % i)
        open(stem + ".deflate", "wb").write(raw)
        open(stem + (".illegal" if text is None else ".txt"), "wb").write(text or b"")
        open(stem + ".tags", "w").write(name + "\n" + " ".join("%s=%s" % (k, int(v)) for k, v in sorted(tags.items())) + "\n")


def _build_abi_client(tmp_path):
    import subprocess
    exe = str(tmp_path / "abi_client")
    lib_dir = os.path.join(ROOT, "quade_amd", "lib")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "abi_client.c"), "-L", lib_dir, "-lquade_hip", "-Wl,-rpath," + lib_dir,
           "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe
