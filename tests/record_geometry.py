"""Inputs whose records are not all one size, for the tests of the chunk loop (run_chunk in quade_amd/csrc/quade_pipe.cpp), which steers
by one learned number per stream, the bytes per record: profile(name, seed) -> Profile, and write(profile, dir, fmt) -> the conf's
file lists.  An ordinary module: no test module imports another one.

A Profile holds the four streams of every chunk as byte strings, the sample sheet, batch_pairs and facts counted from the texts
(never from the generator's bookkeeping).  The conf that goes with it is the one of run_support._run_and_compare: dual 8 + 8 bp index,
molecular index at 9-14 of index read 1, minimal_qual 25, five samples; barcodes, lower case, an N, random index reads and low index
qualities are mixed in as in run_support._dataset, so pass, fail and Undetermined occur in every profile.

Pair j of a chunk is kept record j of every stream and the chunk ends with its shortest stream (src/Quade.py:210-224):
a dropped record shifts its stream against the others, it does not remove a pair.

Out of scope: a record larger than one output member (1 MiB of text); `giant` stays below it (a read of 200 000 bases is a record
of about 400 KB)."""
import functools
import gzip
import os

import numpy as np

STREAMS = ("seq_R1", "seq_R2", "index_R1", "index_R2")
FORMATS = ("bgzf", "gz", "plain")
POSITIONS = ((1, 8), (1, 8), (9, 14), None)  # 1-based inclusive, as run_support._conf takes them
MIN_QUAL = 25
N_SAMPLES = 5
NAMES = ("ragged", "regimes", "chunk_regimes", "ends", "dropped_runs", "giant", "sparse")
UPLOAD_TEXT = 8 << 20  # a plain file reaches its window in reads of 8 MiB (READ_BYTES in quade_io.cpp): the least a top-up adds

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NAME = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_-/#", dtype=np.uint8)
MINIMAL_RECORD = b"@\n\n+\n\n"  # an empty name, an empty read: a whole record of 6 bytes


class Profile(object):
    __slots__ = ("name", "seed", "batch_pairs", "chunks", "samples", "facts")

    def __init__(self, name, seed, batch_pairs, chunks, samples):
        self.name, self.seed, self.batch_pairs, self.chunks, self.samples = name, seed, batch_pairs, chunks, samples
        self.facts = {}

    @property
    def n_chunks(self):
        return len(self.chunks)


# ---- what a text holds, by the reader's rules (oracle.FastqReader) -------------------------------------------------------------
def lines_of(text):
    """the lines of a text, a last one without newline included, each without its '\\r'"""
    if text and not text.endswith(b"\n"):
        text += b"\n"
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in text.split(b"\n")[:-1]]


def records_of(text):
    """[(first byte, bytes, kept)] of every whole record (four lines) of a text"""
    out, pos, at = [], 0, []
    while True:
        e = text.find(b"\n", pos)
        if e < 0:
            break
        at.append((pos, e))
        pos = e + 1
    if pos < len(text):
        at.append((pos, len(text)))
    for r in range(len(at) // 4):
        (h0, _), (s0, s1), _, (q0, q1) = at[4 * r:4 * r + 4]
        cr = lambda a, b: b - a - (1 if b > a and text[b - 1:b] == b"\r" else 0)
        out.append((h0, min(q1 + 1, len(text)) - h0, cr(s0, s1) == cr(q0, q1)))
    return out


def kept_count(text):
    return sum(1 for _, _, kept in records_of(text) if kept)


def pairs_of(chunk):
    """pairs of a chunk: its shortest stream's kept records"""
    return min(kept_count(chunk[k]) for k in STREAMS)


# ---- pieces -------------------------------------------------------------------------------------------------------------------
def _bases(rng, L):
    return _ACGT[rng.integers(0, 4, L)].tobytes()


def _quals(rng, L, lo=30):
    return rng.integers(33 + lo, 33 + 41, L).astype(np.uint8).tobytes()


def _record(name, read_no, seq, qual, nl=b"\n", plus=b"+"):
    return b"@" + name + b" " + read_no + b":N:0:" + nl + seq + nl + plus + nl + qual + nl


def _sheet(rng):
    bcs = set()
    while len(bcs) < N_SAMPLES:
        bcs.add((_bases(rng, 8).decode(), _bases(rng, 8).decode()))
    return [("S%d" % i, b1, b2) for i, (b1, b2) in enumerate(sorted(bcs))]


def _index_pair(rng, samples):
    """index reads 1 and 2 of a pair with their qualities, mixed as in run_support._dataset: a sample's barcodes and a 6-base
    molecular index, with an N, in lower case, a random second read, low qualities"""
    _, b1, b2 = samples[int(rng.integers(0, len(samples)))]
    kind = int(rng.integers(0, 12))
    i1, i2 = b1.encode() + _bases(rng, 6), b2.encode()
    if kind == 0:
        i1 = b"N" + i1[1:]
    elif kind == 1:
        i1, i2 = i1.lower(), i2.lower()
    elif kind == 2:
        i2 = _bases(rng, 8)
    return i1, _quals(rng, len(i1), 20 if kind == 4 else 30), i2, _quals(rng, len(i2))


def _plain_name(c, i):
    return b"SIM:1:FC:%d:%d:%d" % (c, i, i * 7)


def _chunk(rng, samples, c, n, len1=150, len2=150, counts=None):
    """a chunk of n ordinary pairs; len1 / len2: the insert reads' bases, a number or a function of the record; counts: records per
    stream where they are not n"""
    out = {k: [] for k in STREAMS}
    counts = counts or {}
    L = lambda v, i: v(i) if callable(v) else v
    for i in range(max([n] + list(counts.values()))):
        name = _plain_name(c, i)
        i1, q1, i2, q2 = _index_pair(rng, samples)
        rows = {"seq_R1": (b"1", L(len1, i)), "seq_R2": (b"2", L(len2, i))}
        for k, (rd, ln) in rows.items():
            if i < counts.get(k, n):
                out[k].append(_record(name, rd, _bases(rng, ln), _quals(rng, ln)))
        if i < counts.get("index_R1", n):
            out["index_R1"].append(_record(name, b"1", i1, q1))
        if i < counts.get("index_R2", n):
            out["index_R2"].append(_record(name, b"2", i2, q2))
    return out


def _join(recs):
    return {k: b"".join(v) for k, v in recs.items()}


# ---- the profiles -------------------------------------------------------------------------------------------------------------
def _ragged(rng, samples):
    """reads of 0 to 300 bases, names of 1 to 200 bytes, index reads of 0 to 30 bases; every 400th insert read 16 383, 16 384 or
    16 385 bases long (a scan tile is 16 KiB); seq_R2 in CRLF, '+name' lines in index_R2, no final newline in seq_R1"""
    n = 2500
    out = {k: [] for k in STREAMS}
    for i in range(n):
        name = _NAME[rng.integers(0, len(_NAME), int(rng.integers(1, 201)))].tobytes()
        i1, _, i2, _ = _index_pair(rng, samples)
        lo = 20 if rng.integers(0, 12) == 4 else 30
        i1 = (i1 + _bases(rng, 16))[:int(rng.integers(0, 31))]
        i2 = (i2 + _bases(rng, 22))[:int(rng.integers(0, 31))]
        L1, L2 = int(rng.integers(0, 301)), int(rng.integers(0, 301))
        if i % 400 == 0:
            L1 = (16383, 16384, 16385)[(i // 400) % 3]
        if i % 400 == 200:
            L2 = (16383, 16384, 16385)[(i // 400) % 3]
        out["seq_R1"].append(_record(name, b"1", _bases(rng, L1), _quals(rng, L1)))
        out["seq_R2"].append(_record(name, b"2", _bases(rng, L2), _quals(rng, L2), nl=b"\r\n"))
        out["index_R1"].append(_record(name, b"1", i1, _quals(rng, len(i1), lo)))
        out["index_R2"].append(_record(name, b"2", i2, _quals(rng, len(i2)), plus=b"+" + name))
    chunk = _join(out)
    chunk["seq_R1"] = chunk["seq_R1"][:-1]
    return 97, [chunk]


REGIME_CHANGE = 1500  # regimes: the record at which both insert streams change their read length


def _regimes(rng, samples):
    """seq_R1: 1 500 reads of 20 bases, then 1 500 of 3 000; seq_R2 the other way round"""
    return 97, [_join(_chunk(rng, samples, 0, 3000, len1=lambda i: 20 if i < REGIME_CHANGE else 3000,
                             len2=lambda i: 3000 if i < REGIME_CHANGE else 20))]


def _chunk_regimes(rng, samples):
    """chunk 0 teaches seq_R1 records of 4 KB; chunk 1's seq_R1 is 24 000 records of 6 bytes (96 000 lines in a window whose line
    table was sized for 4 KB records) against 700 records of the other streams; chunk 2 is ordinary"""
    c0 = _join(_chunk(rng, samples, 0, 600, len1=2000))
    c1 = _join(_chunk(rng, samples, 1, 700))
    c1["seq_R1"] = MINIMAL_RECORD * 24000
    c2 = _join(_chunk(rng, samples, 2, 600))
    return 500, [c0, c1, c2]


def _ends(rng, samples):
    """chunks 0-7: one stream, each in its turn, ends one record before, on and one behind a multiple of batch_pairs; chunk 8: index_R1
    ends in three lines of a record; chunk 9: seq_R2 is one header line; chunk 10 is ordinary"""
    B, chunks = 97, []
    for c in range(8):
        chunks.append(_join(_chunk(rng, samples, c, 400, counts={STREAMS[c % 4]: 3 * B - 1 + c % 3})))
    c8 = _join(_chunk(rng, samples, 8, 300, counts={"index_R1": 200}))
    c8["index_R1"] += b"@partial 1:N:0:\nACGTACGTACGTAC\n+\n"
    chunks.append(c8)
    c9 = _join(_chunk(rng, samples, 9, 300))
    c9["seq_R2"] = b"@" + _plain_name(9, 0) + b" 2:N:0:\n"
    chunks.append(c9)
    chunks.append(_join(_chunk(rng, samples, 10, 300)))
    return B, chunks


def _malform(rec):
    return rec[:-1] + b"I\n"  # the quality one byte longer than the read


def _dropped_runs(rng, samples):
    """index_R1: records 1 000 to 1 599 malformed, more than six batches' worth in a row; seq_R2: every second record of 1 800 to
    2 799"""
    recs = _chunk(rng, samples, 0, 3000)
    for i in range(1000, 1600):
        recs["index_R1"][i] = _malform(recs["index_R1"][i])
    for i in range(1800, 2800, 2):
        recs["seq_R2"][i] = _malform(recs["seq_R2"][i])
    return 97, [_join(recs)]


GIANTS = {"seq_R1": (300, 70000), "seq_R2": (900, 200000)}  # stream: (record, bases)


def _giant(rng, samples):
    """one read longer than a coder sub-block (64 KiB) in seq_R1, one longer than three BGZF blocks in seq_R2"""
    return 500, [_join(_chunk(rng, samples, 0, 1200, len1=lambda i: GIANTS["seq_R1"][1] if i == GIANTS["seq_R1"][0] else 150,
                              len2=lambda i: GIANTS["seq_R2"][1] if i == GIANTS["seq_R2"][0] else 150))]


SPARSE = ((250, 25), (90, 50), (500, 0))  # sparse: (kept records, malformed records in front of each) of seq_R2's parts


def _sparse(rng, samples):
    """seq_R2 keeps one record in 26, then one in 51, of records of 4 KB, then every record: a read of 8 MiB of its first 43 MB holds
    fewer kept records than a batch has pairs, so a window that was topped up is still short of records while its stream has more -- the
    one profile with a stream larger than an upload (as plain text; compressed, the filler shrinks it to one upload again)"""
    n = sum(k for k, _ in SPARSE)
    recs = _chunk(rng, samples, 0, n)
    filler = _malform(_record(b"filler", b"2", _bases(rng, 2000), _quals(rng, 2000)))
    out, i = [], 0
    for kept, gap in SPARSE:
        for _ in range(kept):
            out.append(filler * gap + recs["seq_R2"][i])
            i += 1
    recs["seq_R2"] = out
    return 97, [_join(recs)]


_BUILDERS = {"sparse": _sparse, "ragged": _ragged, "regimes": _regimes, "chunk_regimes": _chunk_regimes, "ends": _ends, "dropped_runs": _dropped_runs,
             "giant": _giant}


def _facts(p):
    """counted from the texts"""
    f = {"pairs_per_chunk": [pairs_of(c) for c in p.chunks]}
    f["pairs"] = sum(f["pairs_per_chunk"])
    f["kept"] = [{k: kept_count(c[k]) for k in STREAMS} for c in p.chunks]
    f["records"] = [{k: len(records_of(c[k])) for k in STREAMS} for c in p.chunks]
    B = p.batch_pairs
    if p.name == "regimes":
        f["regime_ratio"] = {}
        for k in ("seq_R1", "seq_R2"):
            recs = records_of(p.chunks[0][k])
            before = sum(n for _, n, _ in recs[:REGIME_CHANGE]) / float(REGIME_CHANGE)
            f["regime_ratio"][k] = sum(n for _, n, _ in recs[REGIME_CHANGE:REGIME_CHANGE + B]) / (B * before)
    if p.name == "chunk_regimes":
        text = p.chunks[1]["seq_R1"]
        f["lines"] = len(lines_of(text))
        f["line_cap_left"] = 5.5 * B + 65536 + 4096
        used = sum(n for _, n, _ in records_of(text)[:f["pairs_per_chunk"][1]])
        f["bytes_used"], f["bytes_left"] = used, len(text) - used
    if p.name == "dropped_runs":
        kept = {k: np.cumsum([r[2] for r in records_of(p.chunks[0][k])]) for k in STREAMS}
        f["max_shift"] = int(max(np.abs(kept[a] - kept[b]).max() for a in STREAMS for b in STREAMS))
    if p.name == "sparse":
        # kept records that start in every whole 8 MiB slice of seq_R2: what one more read brings a window
        recs = records_of(p.chunks[0]["seq_R2"])
        n = len(p.chunks[0]["seq_R2"]) // UPLOAD_TEXT
        f["kept_per_upload"] = [sum(1 for at, _, kept in recs if kept and k * UPLOAD_TEXT <= at < (k + 1) * UPLOAD_TEXT) for k in range(n)]
    return f


@functools.lru_cache(maxsize=None)
def profile(name, seed=0):
    """the profile of that name; the same texts for the same seed (cached: treat them as read-only)"""
    rng = np.random.default_rng([NAMES.index(name), seed])
    samples = _sheet(rng)
    B, chunks = _BUILDERS[name](rng, samples)
    p = Profile(name, seed, B, chunks, samples)
    p.facts = _facts(p)
    return p


# ---- on disk ------------------------------------------------------------------------------------------------------------------
def write_text(path, text, fmt):
    if fmt == "bgzf":  # bgzip's layout by the library's own writer, as run_support._bgzip
        from quade_amd import hip_backend as hb
        buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
        assert hb.load_library().qd_write_gzip_file(str(path).encode(), hb._ptr(buf), len(text), 1, -1) == 0
    elif fmt == "gz":  # one member
        with gzip.open(path, "wb", compresslevel=1) as fh:
            fh.write(text)
    else:
        assert fmt == "plain"
        with open(path, "wb") as fh:
            fh.write(text)


def read_text(path):
    with (gzip.open if str(path).endswith(".gz") else open)(path, "rb") as fh:
        return fh.read()


def write(p, d, fmt):
    """the profile's files under d: {stream: [path of chunk 0, ...]}, what run_support._conf takes"""
    files = {k: [] for k in STREAMS}
    for c, chunk in enumerate(p.chunks):
        for k in STREAMS:
            path = os.path.join(str(d), "C%d_%s.fastq%s" % (c, k, "" if fmt == "plain" else ".gz"))
            write_text(path, chunk[k], fmt)
            files[k].append(path)
    return files


def bgzf_blocks(path):
    """[(first text byte, text bytes)] of every block of a BGZF file, from the blocks' BSIZE and ISIZE fields"""
    with open(path, "rb") as fh:
        raw = fh.read()
    out, at, text_at = [], 0, 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 12:at + 14] == b"BC", at
        size = int.from_bytes(raw[at + 16:at + 18], "little") + 1
        isize = int.from_bytes(raw[at + size - 4:at + size], "little")
        out.append((text_at, isize))
        text_at += isize
        at += size
    return out
