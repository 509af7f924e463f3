"""The host side of the duplication report (no GPU): the model's code, key and hash against hand-worked values, the window's edges,
the [output] / [gpu] options and the configurations they reject, merge_dup against a Counter, the ranks' exchange format,
Quade_duplication_report.csv on a hand-built table, and the exported symbols."""
import ctypes
import os
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import duplication_report as dr
from quade_amd import hip_backend as hb
from tests import dup_model as DM
from tests.stage_support import _one_sample_conf as _conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "duplication_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"


# ---- the model against hand-worked values ----------------------------------------------------------------------------------------
def test_code_of_every_byte():
    # 'A' 0x41 -> 0x20 & 3 = 0, 'C' 0x43 -> 0x21 & 3 = 1, 'T' 0x54 -> 0x2A & 3 = 2, 'G' 0x47 -> 0x23 & 3 = 3; lower case folds
    assert [DM.code(b) for b in b"ACTGactg"] == [0, 1, 2, 3, 0, 1, 2, 3]
    assert [b for b in range(256) if DM.valid(b)] == sorted(b"ACGTacgt")
    assert not DM.valid(ord("N")) and not DM.valid(ord("n")) and not DM.valid(0) and not DM.valid(ord("A") | 0x80)


def test_words_by_hand():
    # ACGTacgt: codes 0 1 3 2 0 1 3 2 from bit 0 up = 0b10_11_01_00_10_11_01_00 = 0xB4B4; TTTTGGGG: 0xAA, then 0xFF above it
    assert DM.classify(b"ACGTacgt", b"TTTTGGGG", 8) == (0xB4B4, 0xFFAA)
    assert DM.classify(b"ACGTacgtNNNN", b"TTTTGGGGxxxx", 8) == (0xB4B4, 0xFFAA)  # behind the window nothing counts
    assert DM.classify(b"C" * 9, b"A" * 9, 9) == (0x15555, 0)


def test_32_bases_fill_all_64_bits():
    assert DM.classify(b"G" * 32, b"g" * 40, 32) == (DM.M64, DM.M64)
    assert DM.classify(b"A" * 31 + b"G", b"A" * 31 + b"T", 32) == (3 << 62, 2 << 62)
    assert DM.classify(b"A" * 31 + b"G", b"A" * 31 + b"T", 31) == (0, 0)
    assert DM.word(b"ACGT" * 8, 32) == int("10110100" * 8, 2)


def test_hash_by_hand():
    """the values of a separate C program over quade_unknown.h's functions"""
    assert DM.tag((0, 0, 0, 0)) == 0xD94AFAF94C8E0F1D
    assert DM.tag((1, 2, 3, 0)) == 0x64810095AA26CDE2
    assert DM.tag((DM.M64, DM.M64, 12, 0)) == 0xF3601473662F03C8
    assert DM.key_hash((0x1B, 0xE4, 4)) == 0x2DFE3F6E47E1DC60
    assert DM.home(0x64810095AA26CDE2, 16) == 10866 and DM.home(1, 10) == 632
    assert DM.trim(0x100, 8) == 1 and DM.trim(0x1FF, 8) == 0xFF and DM.trim(5) == 5 and DM.trim(0) == 1
    # sampling takes the top log2(sample) bits: 0x2DFE... has two leading zero bits
    h = 0x2DFE3F6E47E1DC60
    assert [DM.sampled(h, s) for s in (1, 2, 4, 8, 1024)] == [True, True, True, False, False]


def test_the_window_ends_at_base_B():
    good = b"ACGT" * 10
    for B in (8, 31, 32):
        ok = DM.classify(good, good, B)
        assert isinstance(ok, tuple)
        for bad in (b"N", b"n", b".", b"R"):
            inside = good[:B - 1] + bad + good[B:]
            outside = good[:B] + bad + good[B + 1:]
            assert DM.classify(inside, good, B) == "with_n" and DM.classify(good, inside, B) == "with_n"
            assert DM.classify(outside, good, B) == ok and DM.classify(good, outside, B) == ok
        assert DM.classify(good[:B - 1], good, B) == "short" and DM.classify(good, good[:B - 1], B) == "short"
        assert DM.classify(good[:B], good[:B], B) == ok
        assert DM.classify(b"N" * (B - 1), good, B) == "short"  # short comes first


def test_tally_of_a_small_input():
    S, P = 2, DM.Params(bases=8, sample=1, slots=1024)
    a, b, c = b"ACGTACGTAA", b"TTTTTTTTTT", b"ACGTNCGTAA"
    pairs = [(0, a, b, 0), (0, a, b, 0), (1, a, b, 0), (0xFFFF, a, b, 0), (0, a, b, 3), (2, a[:7], b, 0), (2, c, b, 0), (3, b, a.lower(), 0)]
    table, stats = DM.tally(S, pairs, P)
    wa, wb = DM.word(a, 8), DM.word(b, 8)
    assert table == Counter({(wa, wb, 0): 2, (wa, wb, 1): 1, (wa, wb, 4): 1, (wb, wa, 3): 1})
    assert stats == [[2, 0, 0, 2, 0], [1, 0, 0, 1, 0], [2, 1, 1, 0, 0], [1, 0, 0, 1, 0], [1, 0, 0, 1, 0]]
    rows, levels = DM.report_rows(table, stats)
    assert rows[0] == [2, 0, 0, 2, 2, 0, 2, 1, 1] and rows[-1] == [7, 1, 1, 5, 5, 0, 5, 4, 1] and levels == {1: (3, 3), 2: (1, 2)}
    # sampling is by key: a sampled key keeps its multiplicity, and the sampled keys are a subset
    t4, s4 = DM.tally(S, pairs, DM.Params(bases=8, sample=4, slots=1024))
    assert all(table[k] == n and DM.key_hash(k) >> 62 == 0 for k, n in t4.items())
    assert sum(r[DM.SAMPLED] for r in s4) == sum(t4.values()) and [r[:3] for r in s4] == [r[:3] for r in stats]


# ---- the configuration -----------------------------------------------------------------------------------------------------------
def test_conf_defaults_and_values(tmp_path):
    for extra in ("", "duplication_report :\n", "duplication_report : False\n", "duplication_bases :\nduplication_sample :\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, extra))
        assert cf.duplication_report is False and cf.duplication_params() == dict(bases=32, sample=16, slots=1 << 24)
    cf = qconf.QuadeConf(_conf(tmp_path, "duplication_report : True\nduplication_bases : 8\nduplication_sample : 1\n", gpu="[gpu]\nduplicate_slots : 1024\n"))
    assert cf.duplication_report is True and cf.duplication_params() == dict(bases=8, sample=1, slots=1024)
    cf = qconf.QuadeConf(_conf(tmp_path, "duplication_report : yes\nduplication_sample : 1024\n", gpu="[gpu]\nduplicate_slots : 268435456\ngzip_level : -1\n"))
    assert cf.duplication_report is True and cf.duplication_params() == dict(bases=32, sample=1024, slots=1 << 28)
    for word in ("duplication_report", "duplication_bases", "duplication_sample", "duplicate_slots", "device_pipeline", dr.REPORT_NAME,
                 "unbiased estimates", "not_tallied", "with_n", "short"):
        assert word in qconf.DUPLICATION_HELP, word


@pytest.mark.parametrize("extra,gpu,message", [
    ("duplication_bases : 7\n", "", "Authorized values for duplication_bases : 8 to 32"),
    ("duplication_bases : 33\n", "", "Authorized values for duplication_bases : 8 to 32"),
    ("duplication_sample : 0\n", "", "Authorized values for duplication_sample : a power of two, 1 to 1024"),
    ("duplication_sample : 3\n", "", "Authorized values for duplication_sample : a power of two, 1 to 1024"),
    ("duplication_sample : 2048\n", "", "Authorized values for duplication_sample : a power of two, 1 to 1024"),
    ("", "[gpu]\nduplicate_slots : 512\n", "[gpu] duplicate_slots : a power of two, 1024 to 268435456"),
    ("", "[gpu]\nduplicate_slots : 3000\n", "[gpu] duplicate_slots : a power of two, 1024 to 268435456"),
    ("", "[gpu]\nduplicate_slots : 536870912\n", "[gpu] duplicate_slots : a power of two, 1024 to 268435456"),
])
def test_conf_bad_values(tmp_path, extra, gpu, message):
    for on in ("", "duplication_report : True\n"):  # checked like every other value, whether the report is on or not
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, on + extra, gpu=gpu))
        assert str(ei.value) == message
    with pytest.raises(ValueError):
        qconf.QuadeConf(_conf(tmp_path, "duplication_bases : many\n"))


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n", "gzip_level : 6\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "duplication_report : True\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == NEEDS == qconf.DUPLICATION_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "duplication_report : False\n", gpu="[gpu]\n" + gpu)).duplication_report is False


def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path):
    conf = _conf(tmp_path, "duplication_report : True\n", gpu="[gpu]\ndevice_pipeline : False\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert NEEDS in r.stdout + r.stderr
    assert not (tmp_path / dr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


# ---- merging and the ranks' exchange ---------------------------------------------------------------------------------------------
def _random_table(rng, n, words=50):
    keys = np.stack([rng.integers(0, words, n).astype(np.uint64) << np.uint64(40), rng.integers(0, 3, n).astype(np.uint64), rng.integers(0, 5, n).astype(np.uint64)], axis=1)
    keys = np.unique(keys, axis=0)  # a context's table holds a key once
    return keys, rng.integers(1, 1000, len(keys)).astype(np.uint64)


def test_merge_dup_against_a_counter():
    rng = np.random.default_rng(5)
    tables = [_random_table(rng, n) for n in (300, 1, 0, 200)]
    want = Counter()
    for k, c in tables:
        for row, x in zip(k, c):
            want[tuple(int(v) for v in row)] += int(x)
    keys, counts = hb.merge_dup(tables)
    assert keys.dtype == np.uint64 and counts.dtype == np.uint64 and keys.shape == (len(want), 3)
    assert DM.table_counter(keys, counts) == want and len(want) < sum(len(c) for _, c in tables)  # keys met in several tables
    big = (np.array([[DM.M64, DM.M64, 4], [DM.M64, 0, 4]], dtype=np.uint64), np.array([1 << 62, 7], dtype=np.uint64))
    keys, counts = hb.merge_dup([big, big, (big[0][:1], np.array([5], dtype=np.uint64))])  # 64-bit words and counts beyond 2^53
    assert DM.table_counter(keys, counts) == Counter({(DM.M64, DM.M64, 4): (1 << 63) + 5, (DM.M64, 0, 4): 14})
    keys, counts = hb.merge_dup([])
    assert keys.shape == (0, 3) and counts.shape == (0,)
    keys, counts = hb.merge_dup([(np.zeros((0, 3), np.uint64), np.zeros(0, np.uint64))])
    assert keys.shape == (0, 3) and counts.shape == (0,)


def test_pack_and_unpack_round_trip_and_truncated_blobs():
    rng = np.random.default_rng(6)
    keys, counts = _random_table(rng, 100)
    keys[0] = (DM.M64, DM.M64, 6)
    counts[0] = (1 << 64) - 1
    stats = rng.integers(0, 1 << 62, (7, 5)).astype(np.uint64)
    blob = hb.pack_dup(keys, counts, stats)
    k2, c2, s2 = hb.unpack_dup(blob)
    assert (k2 == keys).all() and (c2 == counts).all() and (s2 == stats).all() and k2.shape == keys.shape and s2.shape == (7, 5)
    k0, c0, s0 = hb.unpack_dup(hb.pack_dup(np.zeros((0, 3), np.uint64), np.zeros(0, np.uint64), stats))
    assert k0.shape == (0, 3) and c0.shape == (0,) and (s0 == stats).all()
    for cut in (blob[:-1], blob[:-8], blob[:40], blob[:23], b"", blob + b"\0" * 8, b"\0" * 8 + blob[8:]):
        with pytest.raises(ValueError):
            hb.unpack_dup(cut)


# ---- the report ------------------------------------------------------------------------------------------------------------------
def test_report_lines_on_a_hand_built_table():
    samples = ["A", "B"]
    stats = [[10, 1, 2, 7, 0], [0, 0, 0, 0, 0], [100, 0, 0, 50, 4], [3, 3, 0, 0, 0], [5, 0, 1, 4, 0]]
    table = Counter({(1, 1, 0): 4, (2, 1, 0): 3, (1, 1, 2): 1, (5, 5, 2): 32, (6, 5, 2): 13, (9, 9, 4): 2, (9, 8, 4): 2})
    keys, counts = DM.arrays(table)
    lines = dr.report_lines(stats, keys, counts, samples, dict(bases=32, sample=16, slots=1024))
    assert lines == [
        "Program Quade-duplication 0.3.2", "",
        "bases\t32", "sample\t16", "slots\t1024", "",
        "destination\tpairs\tshort\twith_n\tkeyed\tsampled\tnot_tallied\ttallied\tdistinct\tduplicate_pairs\tduplication_pct",
        "A_pass\t10\t1\t2\t7\t7\t0\t7\t2\t5\t71.42",
        "A_fail\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.00",
        "B_pass\t100\t0\t0\t100\t50\t4\t46\t3\t43\t93.47",
        "B_fail\t3\t3\t0\t0\t0\t0\t0\t0\t0\t0.00",
        "Undetermined\t5\t0\t1\t4\t4\t0\t4\t2\t2\t50.00",
        "Total\t118\t4\t3\t111\t61\t4\t57\t7\t50\t87.71", "",
        "duplication_level\tkeys\tpairs",
        "1\t1\t1", "2\t2\t4", "3\t1\t3", "4\t1\t4", "13\t1\t13", ">=32\t1\t32"]
    # the same figures by the model's own arithmetic
    rows, levels = DM.report_rows(table, stats)
    for ln, row in zip(lines[7:13], rows):
        assert [int(x) for x in ln.split("\t")[1:10]] == row
    assert {(32 if ln.startswith(">=") else int(ln.split("\t")[0])): tuple(int(x) for x in ln.split("\t")[1:]) for ln in lines[15:]} == levels
    # 31 and 32 and more: the last bin takes everything from 32 on
    keys, counts = DM.arrays(Counter({(1, 1, 0): 31, (2, 1, 0): 32, (3, 1, 0): 1000}))
    tail = dr.report_lines([[2000, 0, 0, 1063, 0]] + [[0] * 5] * 4, keys, counts, samples, dict(bases=8, sample=1, slots=2048))
    assert tail[-3:] == ["duplication_level\tkeys\tpairs", "31\t1\t31", ">=32\t2\t1032"] and tail[2] == "bases\t8"
    # an empty run: every percentage 0.00, no level line
    empty = dr.report_lines([[0] * 5] * 5, [], [], samples, dict(bases=32, sample=16, slots=1024))
    assert empty[-1] == "duplication_level\tkeys\tpairs" and all(ln.endswith("\t0.00") for ln in empty[7:13])
    with pytest.raises(AssertionError):
        dr.report_lines(stats[:4], keys, counts, samples, dict(bases=32, sample=16, slots=1024))


def test_write_report(tmp_path):
    keys, counts = DM.arrays(Counter({(1, 1, 0): 2}))
    args = ([[2, 0, 0, 2, 0], [0] * 5, [0] * 5], keys, counts, ["S"], dict(bases=32, sample=1, slots=1024))
    dr.write_report(str(tmp_path / dr.REPORT_NAME), *args)
    assert (tmp_path / dr.REPORT_NAME).read_text() == "\n".join(dr.report_lines(*args)) + "\n" and dr.REPORT_NAME == "Quade_duplication_report.csv"


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_exported_symbols():
    new = {"qd_dup_set", "qd_dup_get", "qd_dup_stats", "qd_dup_read", "qd_dev_dup"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_dup_active", "qd_dup_device"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text and "#define QD_DUP_VALUES 5" in text
    assert "no reference counterpart" in text.split("int qd_dup_set")[0][-6000:]
    assert "no reference counterpart" in text.split("int qd_dev_dup")[0][-1000:]
    assert ctypes.sizeof(hb.qd_dup_params) == 16 and [f[0] for f in hb.qd_dup_params._fields_] == ["bases", "sample", "slots"]
    assert hb.DUP_COUNTERS == DM.COUNTERS == dr.COUNTERS and len(hb.DUP_COUNTERS) == 5
    assert '"dup_tag_bits"' in text
