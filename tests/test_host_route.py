"""The model of the routing and format stages (tests/route_model.py) without a GPU: its per-destination text against the oracle's
whole run of a ragged dataset (variable insert lengths, truncated and over-long index reads, lower case and N, both '+' styles,
CRLF) for plans of tests/test_gpu_e2e.py::SCENARIOS, its rows against the host packer, a batch written out by hand, the member
model, what the three stage entries refuse before they touch a device, and the exported symbols."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import hip_backend as hb
from tests import helpers as H
from tests import route_model as RM
from tests.run_support import (NAME_BYTES, ORACLE_PLANS, PLANS, SCENARIOS, _conf, build_fastq, make_plan, ragged_index_reads, rand_bytes,
                               reads_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ragged_inserts(rng, n, max_len=160):
    reads = []
    for i in range(n):
        L = int(rng.integers(0, max_len + 1)) if i % 9 else (0, 1, 7, 8, 9, 129)[i // 9 % 6]
        name = rand_bytes(rng, int(rng.integers(1, 40)) if i % 17 else 0, NAME_BYTES)
        reads.append((name, rand_bytes(rng, L, b"ACGTNacgtn"), rand_bytes(rng, L, bytes(range(33, 75)))))
    return reads


class Dataset(object):
    """the four texts of n ragged pairs for one plan, their tables, and the oracle's codes"""

    def __init__(self, plan_name, n=150, S=5, seed=1):
        rng = np.random.default_rng(seed)
        self.plan, self.S = make_plan(plan_name), S
        self.sc = SCENARIOS[plan_name]
        w = [(self.plan.idx1_start, self.plan.idx1_end - self.plan.idx1_start), (self.plan.idx2_start, self.plan.idx2_end - self.plan.idx2_start)]
        self.ni = 2 if self.plan.dual else 1
        bcs = set()
        while len(bcs) < S:
            bcs.add(tuple(rand_bytes(rng, w[k][1], b"ACGT") if k < self.ni else b"" for k in range(2)))
        self.barcodes = sorted(bcs)
        reads = [ragged_inserts(rng, n), ragged_inserts(rng, n)] + [ragged_index_reads(rng, n, w[k][0], w[k][1], self.barcodes, k) for k in range(self.ni)]
        self.texts, self.tables = [], []
        for s, r in enumerate(reads):
            text, table = build_fastq(r, [int(v) for v in rng.integers(0, 8, n)])
            assert reads_of(text, table) == r
            self.texts.append(text)
            self.tables.append(table)
        self.reads = reads
        self.n = n

    def index_seqs(self):
        return [[r[1] for r in self.reads[2 + k]] for k in range(self.ni)]

    def oracle_codes(self):
        sq = []
        for k in range(self.ni):
            sq += [[r[1].decode("latin-1") for r in self.reads[2 + k]], [r[2].decode("latin-1") for r in self.reads[2 + k]]]
        codes, _idx, _mol, _counts = H.oracle_on_reads([(b1 + b2).decode() for b1, b2 in self.barcodes], self.plan, *sq)
        return codes


def test_the_builder_writes_what_the_reference_reader_reads():
    """the tables of build_fastq name the bytes that the oracle's reader (tests/helpers.py: kept_records) finds in the text"""
    ds = Dataset("dual_offset_windows", n=120, seed=3)
    for text, table, reads in zip(ds.texts, ds.tables, ds.reads):
        kept = H.kept_records(text)
        assert len(kept) == len(reads) and b"\r\n" in text and b"\n+\n" in text
        assert [int(h) for h in table[:, 0]] == [h for h, _ in kept]
        assert [RM.parse_record(rec) for _, rec in kept] == reads == reads_of(text, table)
    assert any(not r[0] for r in ds.reads[0]) and any(not r[1] for r in ds.reads[0]) and any(len(r[1]) >= 256 for r in ds.reads[2])


@pytest.mark.parametrize("flags", [(True, True, True), (True, False, True), (False, True, False)])
@pytest.mark.parametrize("plan_name", ORACLE_PLANS)
def test_model_text_equals_the_oracles_files(tmp_path, plan_name, flags):
    ds = Dataset(plan_name, seed=len(plan_name))
    files = {}
    for key, text in zip(("seq_R1", "seq_R2", "index_R1", "index_R2"), ds.texts):
        path = tmp_path / (key + ".fastq")
        path.write_bytes(text)
        files[key] = [str(path)]
    samples = [("S%d" % i, b1.decode(), b2.decode()) for i, (b1, b2) in enumerate(ds.barcodes)]
    conf = tmp_path / "conf.txt"
    _conf(str(conf), files, ds.sc["dual"], ds.sc["pos"], ds.sc["minq"], samples, flags)
    out = tmp_path / "ref"
    out.mkdir()
    _sset, run_codes = qo.run_quade(str(conf), outdir=str(out))
    codes = ds.oracle_codes()
    assert [int(c) for c in codes] == run_codes
    kinds = {int(c) & 1 if c != RM.UNDETERMINED else 2 for c in codes}
    assert kinds == {0, 1, 2}  # pass, fail and undetermined pairs all occur
    recs = [[RM.parse_record(rec) for _, rec in H.kept_records(t)] for t in ds.texts]
    m = RM.route(ds.plan, ds.S, flags, recs[0], recs[1], [[r[1] for r in recs[2 + k]] for k in range(ds.ni)], codes)
    names = ["S%d_%s" % (i, q) for i in range(ds.S) for q in ("pass", "fail")] + ["Undetermined"]
    seen = 0
    for d, name in enumerate(names):
        for k in (0, 1):
            path = out / ("%s_R%d.fastq.gz" % (name, k + 1))
            if m["text"][(d, k)]:
                assert gzip.open(path).read() == m["text"][(d, k)], (name, k)
                seen += 1
            else:
                assert not path.exists(), (name, k)
    assert seen >= 2 and len([f for f in os.listdir(out) if f.endswith(".fastq.gz")]) == seen
    if "mol" in plan_name or "umi" in plan_name:  # records with and without the ':MOL' part
        tags = [RM.tag(ds.plan, [s[j] for s in ds.index_seqs()]) for j in range(ds.n)]
        assert any(t.count(b":") == 2 for t in tags) and any(t.count(b":") == 1 for t in tags)


@pytest.mark.parametrize("plan_name", PLANS)
def test_row_model_equals_the_host_packer(plan_name):
    ds = Dataset(plan_name, n=200, seed=7)
    lay = hb.plan_layout(ds.plan)
    streams = [[(r[1], r[2]) for r in ds.reads[2 + k]] for k in range(ds.ni)]
    every_full = True
    for k in range(ds.ni):
        seq_rows, qual_rows, lens = RM.rows(lay, k, streams[k])
        hs, hq, hl, full = hb.pack_index_reads(lay, k, [s for s, _ in streams[k]], [q for _, q in streams[k]])
        assert [bytes(r) for r in hs] == seq_rows and [bytes(r) for r in hq] == qual_rows and [int(v) for v in hl] == lens
        assert 255 in lens and 0 in lens and any(b"\x00" in r for r in seq_rows) and any(b"\xff" in r for r in qual_rows)
        every_full = every_full and full
    short = RM.short_set(lay, streams)
    assert (not short) == every_full and 0 < len(short) < ds.n


def test_a_batch_written_out_by_hand():
    """two samples, five pairs: every table and every byte of the buffer as literals"""
    plan = hb.make_plan(True, 25, (0, 2), (1, 3), (2, 4), (0, 0))
    r1 = [(b"a", b"AC", b"II"), (b"bb", b"", b""), (b"", b"G", b"#"), (b"d", b"TTT", b"123"), (b"e", b"A", b"I")]
    r2 = [(b"a", b"G", b"I"), (b"bb", b"TT", b"JJ"), (b"", b"", b""), (b"d", b"C", b"4"), (b"e", b"CC", b"II")]
    i1 = [b"ACgtT", b"AC", b"A", b"", b"NNNN"]
    i2 = [b"TGCA", b"T", b"tgc", b"GGGG", b""]
    codes = [2, RM.UNDETERMINED, 2, 9, 1]  # sample 1 pass, undetermined, sample 1 pass, beyond 2 * S, sample 0 fail
    m = RM.route(plan, 2, (True, True, True), r1, r2, [i1, i2], codes, drop=[0, 0, 0, 1, 0], out_cap=160)
    assert m["dest"] == [2, 4, 2, 4, 1] and m["perm"] == [4, 0, 2, 1, 3] and m["sdest"] == [1, 2, 2, 4, 4]
    rec1 = [b"@a:ACGC:gt\nAC\n+\nII\n", b"@bb:AC\n\n+\n\n", b"@:Agc\nG\n+\n#\n", b"", b"@e:NN:NN\nA\n+\nI\n"]
    rec2 = [b"@a:ACGC:gt\nG\n+\nI\n", b"@bb:AC\nTT\n+\nJJ\n", b"@:Agc\n\n+\n\n", b"", b"@e:NN:NN\nCC\n+\nII\n"]
    assert m["len1"] == [len(r) for r in rec1] == [19, 11, 12, 0, 15] and m["len2"] == [len(r) for r in rec2] == [17, 15, 10, 0, 17]
    assert m["g1"] == [0, 15, 34, 46, 57, 57] and m["g2"] == [0, 17, 34, 44, 59, 59]
    N = RM.NONE
    assert m["first"] == [N, 0, 1, N, 3] and m["g1_first"] == [N, 0, 15, N, 46] and m["g2_first"] == [N, 0, 17, N, 44]
    G = bytes([RM.GUARD])
    want = (rec1[4] + G + rec1[0] + rec1[2] + G + rec1[1] + G * 5  # R1 of destinations 1, 2 and 4 at 0, 16 and 48
            + rec2[4] + G * 15 + rec2[0] + rec2[2] + G * 5 + rec2[1] + G  # R2 at 64, 96 and 128
            + G * 16)  # behind the end
    assert m["used"] == 144 and m["out"] == want and len(want) == 160
    # destination 0 has no pairs and starts where 1 does; 3 starts where 4 does; every base + G = where the text lies
    assert m["base1"] == [0, 0, 1, 2, 2] and m["base2"] == [64, 64, 79, 84, 84]
    assert m["text"][(2, 0)] == rec1[0] + rec1[2] and m["text"][(0, 0)] == m["text"][(3, 1)] == b"" and m["where"][(4, 1)] == 128
    off = RM.route(plan, 2, (False, False, False), r1, r2, [i1, i2], codes, out_cap=16)
    assert off["used"] == 0 and off["out"] == G * 16 and off["g1"] == [0] * 6 and off["first"] == m["first"] and off["base2"] == [0] * 5


def test_member_model():
    slots = bytes(range(40))
    offsets, packed = RM.pack_members(slots, 10, [3, 0, 10, 1], 16)
    assert offsets == [0, 3, 3, 13, 14] and packed == bytes([0, 1, 2]) + bytes(range(20, 30)) + bytes([30]) + bytes([RM.GUARD]) * 2
    assert RM.pack_members(b"", 7, [], 2) == ([0], bytes([RM.GUARD]) * 2)


def test_entries_refuse_bad_arguments_before_they_touch_a_device():
    """a table that names bytes outside its text, sizes out of range: QD_ERR_INVALID, with no device (the checks come first)"""
    ds = Dataset("dual_offset_windows", n=8, seed=5)
    codes = np.zeros(ds.n, dtype=np.uint16)
    for s, col in ((0, 1), (1, 3), (0, 5), (2, 3), (3, 4)):  # name, sequence and quality ranges; an index read's sequence
        bad = [t.copy() for t in ds.tables]
        bad[s][ds.n - 1, col] = len(ds.texts[s]) + 1
        with pytest.raises(hb.QuadeHipError) as ei:
            hb.dev_route_format(ds.plan, ds.S, (1, 1, 1), ds.texts, bad, codes, out_cap=1 << 16)
        assert ei.value.code == hb.QD_ERR_INVALID
    for kw in (dict(shift=16), dict(shift=-1)):
        with pytest.raises(hb.QuadeHipError) as ei:
            hb.dev_route_format(ds.plan, ds.S, (1, 1, 1), ds.texts, ds.tables, codes, out_cap=1 << 16, **kw)
        assert ei.value.code == hb.QD_ERR_INVALID
    with pytest.raises(hb.QuadeHipError):
        hb.dev_route_format(ds.plan, 0, (1, 1, 1), ds.texts, ds.tables, codes, out_cap=1 << 16)
    lay = hb.plan_layout(ds.plan)
    bad = [t.copy() for t in ds.tables[2:]]
    bad[1][0, 5] = len(ds.texts[3])
    bad[1][0, 4] = 1
    with pytest.raises(hb.QuadeHipError) as ei:
        hb.dev_pack_rows(lay, ds.texts[2:], bad, 8)
    assert ei.value.code == hb.QD_ERR_INVALID
    with pytest.raises(hb.QuadeHipError):
        hb.dev_pack_rows(lay, ds.texts[2:], ds.tables[2:], 8, short_room=7)
    slots = np.zeros(64, dtype=np.uint8)
    for stride, lens, cap in ((16, [17], 64), (16, [16, 16], 31), (0, [0], 8)):
        with pytest.raises(hb.QuadeHipError) as ei:
            hb.dev_pack_members(slots, stride, lens, cap)
        assert ei.value.code == hb.QD_ERR_INVALID


def test_exported_symbols():
    new = {"qd_dev_pack_rows", "qd_dev_route_format", "qd_dev_pack_members"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_dev_fastq_scan", "qd_dev_crc32", "qd_dev_sort_by_dest", "qd_pipe_run"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text
    assert "#define QD_DEV_GUARD_BYTE 0x%02X" % RM.GUARD in text and hb.DEV_GUARD_BYTE == RM.GUARD
    for name in sorted(new):  # each says what it runs, and that it has no reference counterpart
        comment = text.split("int %s(" % name)[0][-1500:]
        assert "no reference counterpart" in comment and "runs " in comment, name
    assert C.sizeof(hb.qd_plan) == 40 and C.sizeof(hb.qd_layout) == 60  # the structures the entries take are as they were
