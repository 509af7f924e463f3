"""Paired-end overlap trimming off the GPU: the plain Python model against a brute force and its own symmetry, the report writer
against hand-written text, the pair_* options of the [trim] section and the configurations they reject, the exchange format of the
ranks, and the exported symbols."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import pair_trim_report as pr
from tests import pairtrim_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "pair_overlap needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _rc(s):
    return bytes(s).translate(RC)[::-1]


def _brute(s1, s2, P):
    """the definition read once more, from the pairs of positions: every (i, j) with i + j == I - 1"""
    L1, L2, ok = len(s1), len(s2), []
    for I in range(1, L1 + L2 + 1):
        pairs = [(i, j) for i in range(L1) for j in range(L2) if i + j == I - 1]
        assert len(pairs) == PM.overlap(I, L1, L2)
        mm = sum(not (chr(s1[i]).upper() in "ACGT" and chr(s2[j]).upper() == "TGCA"["ACGT".index(chr(s1[i]).upper())]) for i, j in pairs)
        assert mm == PM.mismatches(s1, s2, I)
        if len(pairs) >= P.min_overlap and mm <= min(P.max_mismatches, len(pairs) * P.max_mismatch_pct // 100):
            ok.append(I)
    M = max(L1, L2)
    up, down = [I for I in ok if I >= M], [I for I in ok if I < M]
    return min(up) if up else max(down) if down else None


def _random_pairs(seed, n, lo=0, hi=40):
    """short pairs: unrelated, overlapping by construction at every kind of insert, with N, lower case, other bytes and repeats"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        L1, L2 = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        alphabet = b"ACGT" if k % 3 else b"AC"  # two letters: many accepted inserts
        frag = bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), int(rng.integers(1, 2 * hi))))
        pad = bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, 2 * hi))
        s1, s2 = bytearray((frag + pad)[:L1]), bytearray((_rc(frag) + pad[::-1])[:L2])
        if k % 4 == 0:
            s1, s2 = bytearray(pad[:L1]), bytearray(pad[hi:hi + L2])
        for s in (s1, s2):
            for i in rng.permutation(len(s))[:int(rng.integers(0, 4))]:
                s[i] = b"NnacgtX.\x00 "[int(rng.integers(0, 10))] if rng.integers(0, 2) else b"ACGT"[int(rng.integers(0, 4))]
        yield bytes(s1), bytes(s2)


@pytest.mark.parametrize("kw", [dict(min_overlap=8, max_mismatches=5, max_mismatch_pct=20), dict(min_overlap=8, max_mismatches=0, max_mismatch_pct=50),
                                dict(min_overlap=12, max_mismatches=64, max_mismatch_pct=50), dict(min_overlap=8, max_mismatches=2, max_mismatch_pct=0)])
def test_model_equals_a_brute_force_on_short_random_pairs(kw):
    P, seen = PM.Params(**kw), set()
    for s1, s2 in _random_pairs(11, 300):
        want = _brute(s1, s2, P)
        assert PM.insert_size(s1, s2, P) == want, (s1, s2)
        seen.add(None if want is None else want < max(len(s1), len(s2)))
    assert seen == {None, True, False}


def test_model_equals_its_plain_form_on_full_length_reads():
    """the model the device is held against works on translated copies and stops a candidate at its budget; here it meets the
    definition counted in full, at the read lengths and with the defaults the device tests use"""
    rng = np.random.default_rng(13)
    rs = lambda n: bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, n))  # noqa: E731
    P, seen = PM.Params(), set()
    for k, I in enumerate((29, 30, 31, 60, 100, 149, 150, 151, 152, 200, 271, 272, 273, 0, 0)):
        frag = rs(I)
        s1, s2 = bytearray((frag + rs(151))[:151]), bytearray((_rc(frag) + rs(151))[:151 if k % 3 else 120])
        for s in (s1, s2):  # up to 6 changed bases: on both sides of the budget of 5
            for i in rng.permutation(min(len(s), max(I, 1)))[:int(rng.integers(0, 4))]:
                s[i] = b"NnacgtX. T"[int(rng.integers(0, 10))]
        want = PM.insert_size_plain(s1, s2, P)
        assert PM.insert_size(s1, s2, P) == want, (I, bytes(s1), bytes(s2))
        seen.add(None if want is None else want < 151)
    assert seen == {None, True, False}
    unit = b"ACGGTCATTG"
    s1, s2 = (unit * 20)[:151], _rc(unit * 20)[:151]  # a tandem repeat: many accepted inserts on both sides of M
    assert PM.insert_size(s1, s2, P) == PM.insert_size_plain(s1, s2, P) == 160
    assert PM.insert_size(b"A" * 151, b"T" * 151, P) == PM.insert_size_plain(b"A" * 151, b"T" * 151, P) == 151


def test_model_symmetry_swapping_the_reads_gives_the_same_insert():
    P, hits = PM.Params(min_overlap=8), 0
    for s1, s2 in _random_pairs(12, 400, hi=60):
        a = PM.insert_size(s1, s2, P)
        assert a == PM.insert_size(s2, s1, P), (s1, s2)
        hits += a is not None
    assert hits > 50  # (of the generator: enough pairs that do have an insert)


def test_model_vectors_cut_floor_and_counters():
    frag = b"ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATTGACCA"  # 41 bases
    P = PM.Params(min_overlap=8, min_length=38)
    ad1, ad2 = b"GGGGGGGGGG", b"TTTTTTTTTT"
    s1, s2 = frag[:36] + ad1[:4], _rc(frag[:36]) + ad2[:4]  # an insert of 36 under reads of 40
    assert PM.trim_pair(s1, s2, P) == (36, (36, 36), (38, 38))
    assert PM.trim_pair(s1, s2, PM.Params(min_overlap=8)) == (36, (36, 36), (36, 36))
    assert PM.trim_pair(frag, _rc(frag), P) == (41, (41, 41), (41, 41))  # I == L: nothing is cut
    assert PM.trim_pair(frag[:30], _rc(frag)[:30], P) == (41, (30, 30), (30, 30))  # an insert that spans the reads
    assert PM.trim_pair(frag[:30], _rc(frag)[:30], PM.Params(min_overlap=20))[0] is None  # 19 bases overlap
    assert PM.trim_pair(frag.lower(), _rc(frag), P)[0] == 41
    assert PM.trim_pair(b"N" * 41, b"N" * 41, P)[0] is None and PM.trim_pair(b"", b"", P) == (None, (0, 0), (0, 0))
    assert PM.trim_pair(b"A" * 20, b"T" * 20, P)[0] == 20  # every I from 8 to 32 is accepted: the smallest I >= M
    assert PM.trim_pair(s1[:36], s2[:20], P) == (36, (36, 20), (36, 20)) and PM.trim_pair(s1, s2[:20], P) == (36, (36, 20), (38, 20))
    t = PM.new_table()
    assert PM.count(t, s1, s2, P) == (38, 38) and PM.count(t, frag, b"ACGT", P) == (41, 4)
    assert t[:15] == [2, 81, 79, 1, 4, 1, 2, 44, 42, 1, 4, 1, 2, 1, 1] and t[15 + 36] == 1 and sum(t[15:]) == 1
    big = PM.new_table()
    PM.count(big, b"ACGT" * 300, _rc(b"ACGT" * 300), PM.Params())
    assert big[-1] == 1 and sum(big[15:]) == 1  # I* = 1200: the last bin
    assert PM.VALUES == 1040 == len(t)


PARAMS = dict(min_overlap=30, max_mismatches=5, max_mismatch_pct=20, min_length=25)


def _tiny():
    t = [0] * 1040
    t[:6] = [4, 40, 34, 1, 7, 1]
    t[6:12] = [4, 30, 27, 1, 3, 0]
    t[12:15] = [4, 3, 1]
    t[15 + 33], t[15 + 150], t[-1] = 1, 1, 1
    return t


def test_report_lines_against_hand_written_text(tmp_path):
    t = _tiny()
    want = [
        "Program Quade-pair-trim 0.3.2",
        "",
        "pair_overlap\tTrue",
        "pair_min_overlap\t30",
        "pair_max_mismatches\t5",
        "pair_max_mismatch_pct\t20",
        "min_length\t25",
        "",
        "read\treads\tbases_in\tbases_out\toverlap_trimmed_reads\toverlap_trimmed_bases\tfloored_reads\t"
        "percent_overlap_trimmed_reads\tpercent_bases_trimmed",
        "R1\t4\t40\t34\t1\t7\t1\t25.00\t15.00",
        "R2\t4\t30\t27\t1\t3\t0\t25.00\t10.00",
        "Total\t8\t70\t61\t2\t10\t1\t25.00\t12.85",
        "",
        "pairs\t4\t100.00",
        "overlapped_pairs\t3\t75.00",
        "short_insert_pairs\t1\t25.00",
        "",
        "insert_size\tpairs",
        "33\t1",
        "150\t1",
        ">=1024\t1",
        "not_overlapped\t1",
    ]
    assert pr.report_lines(t, PARAMS) == want
    assert pr.report_lines(np.array(t, dtype=np.uint64), PARAMS) == want
    assert pr.REPORT_NAME == "Quade_pair_trim_report.csv" and "Date" not in "\n".join(want)
    assert pr.report_lines([0] * 1040, PARAMS)[-4:] == ["", "insert_size\tpairs", ">=1024\t0", "not_overlapped\t0"]
    with pytest.raises(AssertionError):
        pr.report_lines([0] * 16, PARAMS)
    p = tmp_path / pr.REPORT_NAME
    pr.write_report(str(p), t, PARAMS)
    assert p.read_text() == "\n".join(want) + "\n"
    assert pr.COUNTERS == hb.PAIRTRIM_COUNTERS == PM.COUNTERS and pr.PAIR_COUNTERS == hb.PAIRTRIM_PAIR_COUNTERS == PM.PAIR_COUNTERS
    assert pr.VALUES == hb.PAIRTRIM_VALUES == PM.VALUES == 1040


def test_report_lines_beyond_53_bits():
    t = np.zeros(1040, dtype=np.uint64)
    t[:6] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 62) + 5, (1 << 61) + 1, 7, 1]
    t[6:12] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 63) + 3, 0, 0, 0]
    t[12:15] = [(1 << 63) + 7, (1 << 63) + 6, 1]
    t[15 + 7] = (1 << 63) + 6
    lines = pr.report_lines(t, PARAMS)
    r1 = lines[9].split("\t")
    assert r1[1:7] == [str(int(x)) for x in t[:6]] and r1[7] == "50.00"
    v = (((1 << 63) + 3) - ((1 << 62) + 5)) * 10000 // ((1 << 63) + 3)
    assert r1[8] == "%d.%02d" % (v // 100, v % 100) == "49.99"  # exact integers: a float would round to 50.00
    total = lines[11].split("\t")
    assert total[1] == str((1 << 63) + 2) and total[2] == str((1 << 64) + 6)  # the sum of two rows passes 64 bits and stays exact
    assert lines[-3:] == ["7\t%d" % ((1 << 63) + 6), ">=1024\t0", "not_overlapped\t1"]


def _conf(tmp_path, trim="", gpu=""):
    f = tmp_path / "reads.fastq"
    f.write_text("")
    txt = "[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}\nseq_R2 : {0}\nindex_R1 : {0}\nindex_R2 : {0}\n".format(f)
    txt += "[index]\nindex2 : True\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\nindex1_end : 8\nindex2_start : 1\nindex2_end : 8\n"
    txt += "[output]\nwrite_pass : True\nwrite_fail : True\nwrite_undetermined : True\n" + trim + gpu
    txt += "[sample1]\nname : S1\nindex1_seq : ACAGACAG\nindex2_seq : CTTGCTTG\n"
    p = tmp_path / "conf.txt"
    p.write_text(txt)
    return str(p)


def test_conf_defaults_and_when_the_stage_is_on(tmp_path):
    for trim in ("", "[trim]\n", "[trim]\npair_overlap :\npair_min_overlap :\npair_max_mismatches :\npair_max_mismatch_pct :\n",
                 "[trim]\npair_overlap : False\npair_min_overlap : 12\n", "[trim]\nquality_cutoff : 20\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, trim))
        assert cf.pair_trim is False and (cf.pair_max_mismatches, cf.pair_max_mismatch_pct) == (5, 20)
    cf = qconf.QuadeConf(_conf(tmp_path, ""))
    assert cf.pair_trim_params() == dict(min_overlap=30, max_mismatches=5, max_mismatch_pct=20, min_length=0)
    assert cf.trim is False and cf.trim_params()["min_overlap"] == 3  # the 3' trimming's own options are apart
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\nmin_length : 25\npair_min_overlap : 12\npair_max_mismatches : 3\n"
                                         "pair_max_mismatch_pct : 10\n"))
    assert cf.pair_trim is True and cf.trim is False
    assert cf.pair_trim_params() == dict(min_overlap=12, max_mismatches=3, max_mismatch_pct=10, min_length=25)
    for word in ("true", "1", "yes", "on", "TRUE"):
        assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : %s\n" % word)).pair_trim is True
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\nquality_cutoff : 20\n"))
    assert cf.pair_trim is True and cf.trim is True
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\n", gpu="[gpu]\n" + ok)).pair_trim is True
    for word in ("pair_overlap", "pair_min_overlap", "pair_max_mismatches", "pair_max_mismatch_pct", "min_length", "device_pipeline"):
        assert word in qconf.PAIR_HELP


@pytest.mark.parametrize("trim", ["pair_min_overlap : 8\n", "pair_min_overlap : 1000\n", "pair_max_mismatches : 0\n", "pair_max_mismatches : 64\n",
                                  "pair_max_mismatch_pct : 0\n", "pair_max_mismatch_pct : 50\n"])
def test_conf_values_at_the_edges_are_accepted(tmp_path, trim):
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\n" + trim)).pair_trim is True


@pytest.mark.parametrize("trim,message", [
    ("pair_min_overlap : 7\n", "Authorized values for pair_min_overlap : 8 to 1000"),
    ("pair_min_overlap : 1001\n", "Authorized values for pair_min_overlap : 8 to 1000"),
    ("pair_max_mismatches : -1\n", "Authorized values for pair_max_mismatches : 0 to 64"),
    ("pair_max_mismatches : 65\n", "Authorized values for pair_max_mismatches : 0 to 64"),
    ("pair_max_mismatch_pct : -1\n", "Authorized values for pair_max_mismatch_pct : 0 to 50"),
    ("pair_max_mismatch_pct : 51\n", "Authorized values for pair_max_mismatch_pct : 0 to 50")])
def test_conf_values_beyond_the_edges_are_rejected(tmp_path, trim, message):
    for on in ("pair_overlap : True\n", ""):  # checked like every other value, whether the stage is on or not
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + on + trim))
        assert str(ei.value) == message
    assert message in (qconf.PAIR_OVERLAP, qconf.PAIR_MISMATCHES, qconf.PAIR_MISMATCH_PCT)


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == NEEDS == qconf.PAIR_NEEDS
    with pytest.raises(AssertionError) as ei:  # both stages asked for: the existing message comes first, as before
        qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\nquality_cutoff : 20\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == qconf.TRIM_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_min_overlap : 20\n", gpu="[gpu]\n" + gpu)).pair_trim is False  # off: as before


@pytest.mark.parametrize("trim,gpu,message", [("pair_overlap : True\n", "[gpu]\ndevice_pipeline : False\n", NEEDS),
                                              ("pair_overlap : True\npair_min_overlap : 7\n", "", "Authorized values for pair_min_overlap : 8 to 1000")])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, trim, gpu, message):
    conf = _conf(tmp_path, "[trim]\n" + trim, gpu=gpu)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / pr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_reference_conf_parses_with_the_stage_off(bundled_dir, tmp_path, monkeypatch):
    import shutil
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        golden = fh.read()
    assert qconf.template_bytes() == golden and b"pair_" not in golden
    work = tmp_path / "result"
    work.mkdir()
    (work / "Quade_conf_file.txt").write_bytes(golden)
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    monkeypatch.chdir(work)  # the template names its files relative to the run's folder
    cf = qconf.QuadeConf("Quade_conf_file.txt")
    assert cf.pair_trim is False and cf.trim is False and cf.pair_min_overlap == 30


def test_exported_symbols():
    new = {"qd_pairtrim_set", "qd_pairtrim_get", "qd_pairtrim_read", "qd_pairtrim_add", "qd_dev_pairtrim"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text and "#define QD_PAIRTRIM_VALUES 1040" in text
    assert "no reference counterpart" in text.split("int qd_pairtrim_set")[0][-5000:]
    assert "no reference counterpart" in text.split("int qd_dev_pairtrim")[0][-1000:]
    assert ctypes.sizeof(hb.qd_pairtrim_params) == 16
    assert ctypes.sizeof(hb.qd_trim_params) == 64 + 64 + 6 * 4  # the 3' trimming's struct is as it was


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, 1040, dtype=np.uint64)
    b = rng.integers(0, 1 << 62, 1040, dtype=np.uint64)
    a[14], b[14], a[1039], b[1039] = (1 << 63) - 1, 1 << 62, (1 << 63) + 5, 7
    blob = hb.pack_table("pairtrim", a)
    assert isinstance(blob, bytes) and len(blob) == 1040 * 8
    a2 = hb.unpack_table("pairtrim", blob)
    assert a2.dtype == np.uint64 and a2.shape == (1040,) and (a2 == a).all()
    a2 += hb.unpack_table("pairtrim", hb.pack_table("pairtrim", b.reshape(2, 520)))  # (any shape of 1040 packs alike; unpacked tables are writable copies)
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2, a, b))
    assert int(a2[14]) == (1 << 63) - 1 + (1 << 62) and int(a2[1039]) == (1 << 63) + 12  # sums stay integers beyond 2^63
    with pytest.raises(AssertionError):
        hb.unpack_table("pairtrim", blob[:-8])
    reads, pairs, hist = hb.split_pairtrim(a2)
    assert [len(reads[0]), len(reads[1]), len(pairs), len(hist)] == [6, 6, 3, 1025] and pairs[2] == int(a2[14]) and hist[-1] == int(a2[1039])
    assert hb.PAIRTRIM_COUNTERS == ("reads", "bases_in", "bases_out", "overlap_trimmed_reads", "overlap_trimmed_bases", "floored_reads")
    assert hb.PAIRTRIM_PAIR_COUNTERS == ("pairs", "overlapped_pairs", "short_insert_pairs")
