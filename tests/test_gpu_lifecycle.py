"""Create -> use -> destroy, three rounds in one process, of every object of the library that owns device or page-locked memory
(quade_amd/csrc/quade_buf.h): a context with every table it can hold, an inflater, a deflater, qd_dev_gunzip's locals and a pipeline.
Every round gives the bytes of the first -- what a buffer that went back too early, twice or to the wrong place would change --
and the oracle's, zlib's or the input's where there is one.  A stage is set again with other parameters while its context lives, so a
table is released and allocated under a live context too.  Every call returns QD_OK; no error path is provoked."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

from quade_amd import hip_backend as hb
from quade_amd.screen import canonical_words
from tests import clip_model as CM
from tests import deflate_forge as F
from tests import filter_model as FM
from tests import helpers as H
from tests import pairtrim_model as PM
from tests import run_support as RS
from tests.stage_support import _text_from

pytestmark = pytest.mark.gpu

ROUNDS = 3
N = 64
BCS = ("ACGTACGT" + "TTGGCCAA", "GGATCCTA" + "CAGTCAGT")  # the two-barcode sheet, dual 8 + 8
FAR = ("AAAAAAAA", "CCCCCCCC")  # on no sample's side of a budget of one mismatch
CLIP = CM.Params(front_clip=(1, 0), tail_clip=(0, 2), window_size=4, window_quality=20, poly_g_min_length=6, min_length=5)
PAIR = PM.Params(min_overlap=8, max_mismatches=2, max_mismatch_pct=20, min_length=6)
FILTER = FM.Params(min_length=18, max_n=1, min_mean_quality=20, min_complexity_pct=30)
TRIM = dict(adapter_r1="AGATCGGAAG", adapter_r2="AGATCGGAAG", quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=4)
TRIM_OTHER = dict(TRIM, adapter_r1="CTGTCTCTTATACACATCT", quality_cutoff=10)
POST = dict(tail_n=1, poly_x_min_length=6, max_length_r1=0, max_length_r2=0, min_length=0)
PROBES = ("AGATCGGAAGAG", "CTGTCTCTTATA")
SCREEN_K = 15
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


def _blob(x):
    """whatever a call gave back, as bytes"""
    if isinstance(x, dict):
        return b"".join(k.encode() + _blob(v) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return b"".join(_blob(v) for v in x)
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    return np.ascontiguousarray(x).tobytes() if x is not None else b"-"


def _tally(keys, counts):
    """a key tally's entries, which come in no particular order, sorted"""
    return sorted(tuple(int(v) for v in k) + (int(n),) for k, n in zip(keys, counts))


class Batch(object):
    """64 pairs: index reads that carry a sample's barcode (every fifth with a low-quality base), the two samples' parts swapped,
    and bases far from both samples -- none within one mismatch of a sample it does not carry, so the rescue changes no code and
    the unmodified oracle is the reference -- and insert reads of 40 bases with short inserts, adapters, poly-G tails and N."""

    def __init__(self):
        rng = np.random.default_rng(2610)
        self.idx = ([], [], [], [])  # s1, q1, s2, q2
        cases = ([], [])
        for j in range(N):
            kind = j % 8
            b = BCS[j % 2]
            i1, i2 = (b[:8], b[8:]) if kind < 5 else (BCS[0][:8], BCS[1][8:]) if kind < 7 else FAR
            q = [bytearray(33 + int(v) for v in rng.integers(30, 41, 8)) for _ in range(2)]
            if j % 5 == 0:
                q[j % 2][j % 8] = 33 + 12
            for k, v in enumerate((i1, q[0].decode(), i2, q[1].decode())):
                self.idx[k].append(v)
            L = 40
            s1 = bytearray(b"ACGT"[int(v)] for v in rng.integers(0, 4, L))
            s2 = bytearray(b"ACGT"[int(v)] for v in rng.integers(0, 4, L))
            if j % 4 == 1:
                I = 20 + j % 16
                s2[:I] = bytes(s1[:I]).translate(COMP)[::-1]
            if j % 4 == 2:
                s1[L - 12:] = PROBES[0].encode()
            if j % 5 == 3:
                s2[L - 8:] = b"G" * 8
            if j % 6 == 4:
                s1[3:6] = b"NnN"
            if j % 16 == 7:
                s2[:] = s2[:20] * 2  # a duplicate's food: see below
            qq = [bytes(33 + int(v) for v in rng.integers(2 if j % 3 == 0 else 22, 41, L)) for _ in range(2)]
            cases[0].append(("pair %d" % j, bytes(s1), qq[0]))
            cases[1].append(("pair %d" % j, bytes(s2), qq[1]))
        cases[0][9], cases[1][9] = cases[0][8], cases[1][8]  # one duplicated pair
        (self.t1, self.r1), (self.t2, self.r2) = (_text_from(rng, c) for c in cases)
        self.kmers = np.unique(np.concatenate([w[ok] for w, ok in (canonical_words(cases[r][j][1], SCREEN_K) for r, j in ((0, 0), (1, 3), (0, 7)))]))
        self.plan = hb.make_plan(True, 25, (0, 8), (0, 8))
        self.codes, _, _, self.counts = H.oracle_on_reads(list(BCS), self.plan, *self.idx)
        for parts in (FAR, (BCS[0][:8], BCS[1][8:])):  # (what the docstring says of the rescue)
            assert all(sum(a != c for a, c in zip(parts[0], s[:8])) > 1 or sum(a != c for a, c in zip(parts[1], s[8:])) > 1 for s in BCS)
        assert len(set(int(c) for c in self.codes)) >= 4  # pass and fail of a sample, the other sample, Undetermined

    def a(self):
        return self.t1, self.r1, self.t2, self.r2


def _stages_on(eng, batch, trim=TRIM):
    eng.adapters_set(PROBES)
    eng.clip_set(**CLIP.keywords())
    eng.trim_set(**trim)
    eng.pairtrim_set(**PAIR.keywords())
    eng.paircorrect_set(good_quality=30, bad_quality=14)
    eng.posttrim_set(**POST)
    eng.filter_set(**FILTER.keywords())
    eng.screen_set(kmer=SCREEN_K, min_hits=1, action="report", kmers=batch.kmers)
    eng.qstats_enable(True)
    eng.cstats_enable(True)
    eng.dup_set(bases=8, sample=1, slots=1 << 10)


def _run_stages(eng, batch, codes):
    a = batch.a()
    return [eng.dev_adapters(*a, codes), eng.dev_clip(*a), eng.dev_trim(*a), eng.dev_pairtrim(*a), eng.dev_paircorrect(*a), eng.dev_posttrim(*a),
            eng.dev_filter(*a, codes), eng.dev_screen(*a, codes), eng.dev_qstats(*a, codes), eng.dev_cstats(*a, codes), eng.dev_dup(*a, codes)]


def _tables(eng):
    return [eng.adapters_read(), eng.clip_read(), eng.trim_read(), eng.pairtrim_read(), eng.paircorrect_read(), eng.posttrim_read(), eng.filter_read(),
            eng.screen_read(), eng.qstats_read(), eng.cstats_read(), eng.dup_stats(), repr(_tally(*eng.dup_read())).encode(),
            repr(_tally(*eng.unknown_read())).encode(), eng.unknown_stats(), eng.hop_read(), eng.counts()]


def _context_round(torch, batch):
    out = []
    with hb.Engine(0) as eng:
        eng.set_plan(batch.plan)
        eng.set_barcodes(list(BCS))
        eng.set_mismatches(1, 1)
        eng.unknown_enable(1 << 10)
        eng.hop_enable(True)
        _stages_on(eng, batch)
        L = eng.layout
        rows = [hb.pack_index_reads(L, k, [s.encode() for s in batch.idx[2 * k]], [q.encode() for q in batch.idx[2 * k + 1]]) for k in range(2)]
        assert all(r[3] for r in rows)  # (whole reads: no length rows)
        seq = [torch.from_numpy(r[0]).cuda() for r in rows]
        qual = [torch.from_numpy(r[1]).cuda() for r in rows]
        codes, _ = H.hip_on_device(eng, seq, qual, N)
        assert (codes == batch.codes).all() and (eng.counts() == batch.counts).all()
        out += [codes, _run_stages(eng, batch, codes), _tables(eng)]
        # the stages set again with other parameters, a tally with another table size: their tables go and come while the context lives
        _stages_on(eng, batch, trim=TRIM_OTHER)
        eng.dup_set(bases=12, sample=1, slots=1 << 11)
        eng.screen_set(kmer=SCREEN_K, min_hits=2, action="drop", kmers=batch.kmers[::2])
        eng.unknown_enable(1 << 12)
        out += [_run_stages(eng, batch, codes), _tables(eng)]
        _stages_on(eng, batch)
        out += [_run_stages(eng, batch, codes), _tables(eng)]
        # the pinned slots: the same batch through slot 1 of two
        eng.slots_create(2, N)
        v = eng.slot(1)
        for k in range(2):
            v["seq"][k][:N] = rows[k][0]
            v["qual"][k][:N] = rows[k][1]
        eng.submit(1, N)
        eng.wait(1)
        assert (v["codes"][:N] == batch.codes).all()
        out.append(v["codes"][:N].copy())
        eng.slots_destroy()
        out.append(eng.counts())
    return _blob(out)


def test_a_context_with_every_table(torch_cuda):
    batch = Batch()
    rounds = [_context_round(torch_cuda, batch) for _ in range(ROUNDS)]
    assert len(rounds[0]) > 10000 and all(r == rounds[0] for r in rounds[1:])


def _fastq(rng, n):
    return b"".join(b"@r%d 1:N:0:\n%s\n+\n%s\n" % (i, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)), bytes(rng.integers(35, 74, 100).astype(np.uint8)))
                    for i in range(n))


def _raw(text, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(text) + c.flush()


def test_an_inflater_through_its_three_forms(torch_cuda):
    text = _fastq(np.random.default_rng(5), 700)
    parts = (text[:60000], text[60000:100000], text[100000:])
    comp = b"".join(F.bgzf_block(_raw(p, lv), p) for p, lv in zip(parts, (6, 0, 1)))  # three blocks, the second one stored
    for _ in range(ROUNDS):
        with hb.Inflater(0) as inf:
            for form in (1, 2, 3):
                inf.set_form(form)
                assert inf.run(comp, len(text)) == text, form


def test_a_deflater_at_both_levels(torch_cuda):
    lib = hb.load_library()
    text = _fastq(np.random.default_rng(6), 700)
    pieces = [text[:70000], text[70000:140000]]  # two sub-blocks each
    lens = np.array([len(t) for t in pieces], np.int64)
    crc = np.array([zlib.crc32(t) for t in pieces], np.uint32)
    bufs = [np.frombuffer(t, np.uint8) for t in pieces]
    ptrs = (C.c_void_p * 2)(*[b.ctypes.data for b in bufs])
    stride = lib.qd_huffman_member_bound(70000)
    first = None
    for _ in range(ROUNDS):
        d = C.c_void_p()
        assert lib.qd_deflater_create(0, C.byref(d)) == hb.QD_OK
        got = []
        for level in (-1, 1, -1):
            assert lib.qd_deflater_set_level(d, level) == hb.QD_OK
            out, ml = np.zeros(2 * stride, np.uint8), np.zeros(2, np.int64)
            assert lib.qd_deflater_run(d, 2, ptrs, hb._ptr(lens), hb._ptr(crc), 0, hb._ptr(out), stride, hb._ptr(ml)) == hb.QD_OK
            members = [bytes(out[i * stride:i * stride + int(ml[i])]) for i in range(2)]
            assert [gzip.decompress(m) for m in members] == pieces, level
            got.append(members)
        assert lib.qd_deflater_destroy(d) == hb.QD_OK
        assert got[0] == got[2]
        first = first or got
        assert got == first


def test_dev_gunzip_of_two_members(torch_cuda):
    text = _fastq(np.random.default_rng(7), 450)[:100000]
    gz = gzip.compress(text[:55000], 6) + gzip.compress(text[55000:], 1)
    first = None
    for _ in range(ROUNDS):
        got, stats = hb.dev_gunzip(gz, len(text) + 64)
        assert got == text and stats["members"] == 2
        first = first or stats
        assert stats == first


@pytest.mark.parametrize("fmt", ["gz", "bgzf"])
def test_a_pipeline_of_299_pairs(torch_cuda, tmp_path, fmt):
    data = tmp_path / "data"
    data.mkdir()
    files, samples = RS._dataset(str(data), np.random.default_rng(11), 1, 299, 2, fmt=fmt)
    first = None
    for k in range(ROUNDS):
        work = tmp_path / ("round%d" % k)
        work.mkdir()
        stats = RS._run_and_compare(work, files, samples, "[gpu]\nbatch_pairs : 128\n")  # (equal to the oracle's files and report)
        assert stats["pairs"] == 299
        mine = {f: open(os.path.join(str(work), "mine", f), "rb").read() for f in sorted(os.listdir(str(work / "mine"))) if f.endswith(".fastq.gz")}
        first = first or mine
        assert mine == first and len(mine) >= 3
