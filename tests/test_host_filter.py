"""The read filter without a GPU: the plain Python rule on hand-made reads (both sides of every threshold, precedence, the shortest
reads, case folding), the [filter] section of the configuration file, the report's lines, the table's packing and the exported
symbols."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from tests import filter_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "[filter] needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
GOOD = (b"ACGT" * 8, b"~" * 32)


def _q(*phred):
    return bytes(33 + p for p in phred)


@pytest.mark.parametrize("params,read,fails", [
    (dict(min_length=5), (b"ACGT", b"IIII"), [1]),
    (dict(min_length=5), (b"ACGTA", b"IIIII"), []),
    (dict(min_length=1), (b"", b""), [1]),
    (dict(max_n=1), (b"ANGT", b"IIII"), []),
    (dict(max_n=1), (b"ANGn", b"IIII"), [2]),
    (dict(max_n=0), (b"ACGT", b"IIII"), []),
    (dict(max_n=0), (b"ACnT", b"IIII"), [2]),
    # 2 of 5 unqualified = 40 %: not above 40; 3 of 5 is
    (dict(max_unqualified_pct=40), (b"ACGTA", _q(14, 14, 15, 15, 40)), []),
    (dict(max_unqualified_pct=40), (b"ACGTA", _q(14, 14, 14, 15, 40)), [3]),
    (dict(max_unqualified_pct=0), (b"ACGTA", _q(15, 15, 15, 15, 15)), []),
    (dict(max_unqualified_pct=0), (b"ACGTA", _q(15, 15, 14, 15, 15)), [3]),
    (dict(max_unqualified_pct=100), (b"ACGTA", _q(0, 0, 0, 0, 0)), []),
    (dict(max_unqualified_pct=0, qualified_quality=30), (b"AC", _q(30, 29)), [3]),
    (dict(max_unqualified_pct=0, qualified_quality=30), (b"AC", _q(30, 30)), []),
    # the mean is compared as qsum against min_mean_quality * L
    (dict(min_mean_quality=20), (b"ACGT", _q(20, 20, 20, 20)), []),
    (dict(min_mean_quality=20), (b"ACGT", _q(20, 20, 20, 19)), [4]),
    (dict(min_mean_quality=20), (b"ACGT", _q(0, 0, 40, 40)), []),
    (dict(min_mean_quality=20), (b"ACGT", b"\x00\x20" + _q(40, 39)), [4]),  # bytes below 33 count as 0
    (dict(min_mean_quality=93), (b"AC", b"\xff\x21"), []),  # bytes are unsigned: 255 - 33 = 222
    # 3 of 10 neighbour pairs differ = 30 %: not below 30; 2 of 10 is
    (dict(min_complexity_pct=30), (b"AAACCCGGGGT", b"I" * 11), []),
    (dict(min_complexity_pct=30), (b"AAACCCGGGGG", b"I" * 11), [5]),
    (dict(min_complexity_pct=100), (b"ACACACA", b"I" * 7), []),
    (dict(min_complexity_pct=100), (b"ACACCAC", b"I" * 7), [5]),
    (dict(min_complexity_pct=1), (b"G" * 150, b"I" * 150), [5]),
    (dict(min_complexity_pct=1), (b"G" * 100 + b"A", b"I" * 101), []),  # 1 of 100
    (dict(min_complexity_pct=1), (b"G" * 101 + b"A", b"I" * 102), [5]),  # 1 of 101: 100 < 101
])
def test_a_read_just_inside_and_just_outside_every_rule(params, read, fails):
    P = FM.Params(**params)
    assert FM.read_fails(read[0], read[1], P) == fails
    assert FM.reason(read, GOOD, P) == FM.reason(GOOD, read, P) == (fails[0] if fails else 0)  # either read is enough


def test_counts_and_case_folding():
    P = FM.Params()
    assert FM.read_counts(b"aAaA", b"IIII", P) == (4, 0, 0, 160, 0)
    assert FM.read_counts(b"aCAc", b"IIII", P)[4] == 3 and FM.read_counts(b"NnNn", _q(14, 15, 0, 93), P) == (4, 4, 2, 14 + 15 + 93, 0)
    assert FM.read_counts(b"@`", b"II", P)[4] == 0 and FM.read_counts(b"A!", b"II", P)[4] == 1  # bit 5 alone is folded away
    assert FM.read_counts(b"AC", b"\x0a\xff", P) == (2, 0, 1, 222, 1)


def test_the_shortest_reads():
    """L = 0 fails only rule 1; L = 1 has no neighbour pair and passes the complexity rule at 100 %; L = 2 has one"""
    every = dict(min_length=1, max_n=0, max_unqualified_pct=0, min_mean_quality=93, min_complexity_pct=100)
    assert FM.read_fails(b"", b"", FM.Params(**every)) == [1]
    assert FM.read_fails(b"", b"", FM.Params(**dict(every, min_length=None))) == []
    P = FM.Params(min_complexity_pct=100)
    assert FM.read_fails(b"G", b"I", P) == [] and FM.read_fails(b"GG", b"II", P) == [5] and FM.read_fails(b"Gg", b"II", P) == [5]
    assert FM.read_fails(b"GA", b"II", P) == []
    assert FM.read_fails(b"N", b"!", FM.Params(**every)) == [2, 3, 4] and FM.read_fails(b"A", _q(93), FM.Params(**every)) == []


def test_precedence_and_the_pair_rule():
    P = FM.Params(min_length=4, max_n=0, max_unqualified_pct=40, min_mean_quality=20, min_complexity_pct=30)
    both = (b"NNNNNNNN", b"I" * 8)  # fails rules 2 and 5
    assert FM.read_fails(*both, P) == [2, 5] and FM.reason(both, GOOD, P) == 2 and FM.reason(GOOD, both, P) == 2
    poly = (b"G" * 8, b"I" * 8)
    assert FM.reason(poly, both, P) == 2 and FM.reason(both, poly, P) == 2  # the lowest rule of either read, whichever read it is
    assert FM.reason(poly, (b"ACG", b"III"), P) == 1 and FM.reason(GOOD, poly, P) == 5 and FM.reason(GOOD, GOOD, P) == 0
    lowq = (GOOD[0], _q(*([2] * 32)))  # fails rules 3 and 4
    assert FM.read_fails(*lowq, P) == [3, 4] and FM.reason(lowq, poly, P) == 3
    assert FM.reason(lowq, poly, FM.Params(min_mean_quality=20, min_complexity_pct=30)) == 4  # rules that are off are skipped
    assert FM.reason(both, lowq, FM.Params()) == 0 and not FM.Params().on and FM.Params(max_n=0).on and not FM.Params(qualified_quality=20).on


def test_table_and_addition():
    P = FM.Params(min_length=4, max_n=0)
    t = FM.new_table(2)
    assert FM.count(t, 0, GOOD, GOOD, P) == 0 and FM.count(t, 3, (b"AC", b"II"), GOOD, P) == 1
    assert FM.count(t, FM.UNDETERMINED, GOOD, (b"ACGN", b"IIII"), P) == 2 and FM.count(t, 3, GOOD, GOOD, P) == 0
    assert t == [[1, 0, 0, 0, 0, 0, 64, 0], [0] * 8, [0] * 8, [2, 1, 0, 0, 0, 0, 98, 34], [1, 0, 1, 0, 0, 0, 36, 36]]
    assert FM.add_tables(t, t)[3] == [4, 2, 0, 0, 0, 0, 196, 68]


def test_report_lines_against_hand_written_text():
    t = np.zeros((5, 8), dtype=np.uint64)
    t[0] = [10, 1, 2, 0, 0, 1, 3000, 1200]
    t[3] = [3, 0, 0, 1, 1, 1, 900, 900]
    t[4] = [7, 0, 0, 0, 0, 0, 2100, 0]
    params = dict(min_length=30, max_n=0, max_unqualified_pct=None, qualified_quality=15, min_mean_quality=None, min_complexity_pct=30)
    assert fr.report_lines(t, ["A", "B"], params) == [
        "Program Quade-filter 0.3.2", "",
        "min_length\t30", "max_n\t0", "max_unqualified_pct\t", "qualified_quality\t15", "min_mean_quality\t", "min_complexity_pct\t30", "",
        "destination\tpairs_in\tpairs_kept\ttoo_short\ttoo_many_n\tlow_quality\tlow_mean_quality\tlow_complexity\tbases_in\tbases_kept\t"
        "percent_pairs_kept\tpercent_bases_kept",
        "A_pass\t10\t6\t1\t2\t0\t0\t1\t3000\t1800\t60.00\t60.00",
        "A_fail\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.00\t0.00",
        "B_pass\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.00\t0.00",
        "B_fail\t3\t0\t0\t0\t1\t1\t1\t900\t0\t0.00\t0.00",
        "Undetermined\t7\t7\t0\t0\t0\t0\t0\t2100\t2100\t100.00\t100.00",
        "Total\t20\t13\t1\t2\t1\t1\t2\t6000\t3900\t65.00\t65.00"]
    assert fr.COUNTERS == hb.FILTER_COUNTERS == FM.COUNTERS and fr.PARAMS == hb.FILTER_KEYS == FM.KEYS and fr.REASONS == hb.FILTER_REASONS
    with pytest.raises(AssertionError):
        fr.report_lines(t, ["A"], params)


def test_report_lines_beyond_53_bits(tmp_path):
    t = np.zeros((3, 8), dtype=np.uint64)
    t[0] = [(1 << 63) + 3, (1 << 62) + 5, 0, 0, 0, 0, (1 << 63) + 3, (1 << 62) + 5]
    t[2] = [(1 << 63) + 1, 0, 0, 0, 0, 1, (1 << 63) + 1, 7]
    lines = fr.report_lines(t, ["A"], {})
    row = lines[10].split("\t")
    v = (((1 << 63) + 3) - ((1 << 62) + 5)) * 10000 // ((1 << 63) + 3)
    assert row[1] == str((1 << 63) + 3) and row[2] == str((1 << 62) - 2) and row[10] == "%d.%02d" % (v // 100, v % 100) == "49.99"
    total = lines[13].split("\t")
    assert total[0] == "Total" and total[1] == str((1 << 64) + 4) and total[8] == str((1 << 64) + 4)  # sums pass 64 bits and stay exact
    fr.write_report(str(tmp_path / fr.REPORT_NAME), t, ["A"], {})
    assert (tmp_path / fr.REPORT_NAME).read_text() == "\n".join(lines) + "\n" and fr.REPORT_NAME == "Quade_filter_report.csv"


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, (13, 8), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, (13, 8), dtype=np.uint64)
    a[12, 7], b[12, 7] = (1 << 63) + 5, 7
    blob = hb.pack_table("filter", a)
    assert isinstance(blob, bytes) and len(blob) == 8 + 13 * 8 * 8
    a2 = hb.unpack_table("filter", blob)
    assert a2.dtype == np.uint64 and a2.shape == (13, 8) and (a2 == a).all()
    a2 += hb.unpack_table("filter", hb.pack_table("filter", b.reshape(-1)))  # (a flat table packs alike; unpacked tables are writable copies)
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2.ravel(), a.ravel(), b.ravel())) and int(a2[12, 7]) == (1 << 63) + 12
    with pytest.raises(AssertionError):
        hb.unpack_table("filter", blob[:-8])


def _conf(tmp_path, extra="", gpu=""):
    f = tmp_path / "reads.fastq"
    f.write_text("")
    txt = "[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}\nseq_R2 : {0}\nindex_R1 : {0}\nindex_R2 : {0}\n".format(f)
    txt += "[index]\nindex2 : True\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\nindex1_end : 8\nindex2_start : 1\nindex2_end : 8\n"
    txt += "[output]\nwrite_pass : True\nwrite_fail : True\nwrite_undetermined : True\n" + extra + gpu
    txt += "[sample1]\nname : S1\nindex1_seq : ACAGACAG\nindex2_seq : CTTGCTTG\n"
    p = tmp_path / "conf.txt"
    p.write_text(txt)
    return str(p)


OFF = dict(min_length=None, max_n=None, max_unqualified_pct=None, qualified_quality=15, min_mean_quality=None, min_complexity_pct=None)


def test_conf_defaults_and_when_the_stage_is_on(tmp_path):
    empty = "[filter]\n" + "".join("%s :\n" % k for k in FM.KEYS)
    for extra in ("", "[filter]\n", empty, "[filter]\nqualified_quality : 20\n", "[trim]\nmin_length : 30\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, extra))
        assert cf.filter is False and cf.filter_params() == dict(OFF, qualified_quality=20 if "20" in extra else 15)
    cf = qconf.QuadeConf(_conf(tmp_path, "[filter]\nmax_n : 0\n"))  # 0 is a setting, not "off"
    assert cf.filter is True and cf.filter_params() == dict(OFF, max_n=0)
    cf = qconf.QuadeConf(_conf(tmp_path, "[filter]\nmin_length : 30\nmax_n : 5\nmax_unqualified_pct : 40\nqualified_quality : 20\n"
                                         "min_mean_quality : 25\nmin_complexity_pct : 30\n[trim]\nmin_length : 10\n"))
    assert cf.filter is True and cf.trim is False and cf.pair_trim is False and cf.min_length == 10  # [trim] min_length is apart
    assert cf.filter_params() == dict(min_length=30, max_n=5, max_unqualified_pct=40, qualified_quality=20, min_mean_quality=25, min_complexity_pct=30)
    for k in FM.KEYS:
        if k != "qualified_quality":
            assert qconf.QuadeConf(_conf(tmp_path, "[filter]\n%s : 1\n" % k)).filter is True
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, "[filter]\nmax_n : 1\n", gpu="[gpu]\n" + ok)).filter is True
    for word in FM.KEYS + FM.REASONS + ("device_pipeline", "Quade_filter_report.csv", "Undetermined"):
        assert word in qconf.FILTER_HELP


@pytest.mark.parametrize("name,lo,hi", [("min_length", 1, 100000), ("max_n", 0, 100000), ("max_unqualified_pct", 0, 100), ("qualified_quality", 1, 93),
                                        ("min_mean_quality", 1, 93), ("min_complexity_pct", 1, 100)])
def test_conf_ranges(tmp_path, name, lo, hi):
    for v in (lo, hi):
        cf = qconf.QuadeConf(_conf(tmp_path, "[filter]\n%s : %d\n" % (name, v)))
        assert cf.filter_params()[name] == v and cf.filter is (name != "qualified_quality")
    message = "Authorized values for [filter] %s : %d to %d" % (name, lo, hi)
    for v in (lo - 1, hi + 1, -1):
        for more in ("", "max_n : 2\n"):  # checked like every other value, whether the stage is on or not
            with pytest.raises(AssertionError) as ei:
                qconf.QuadeConf(_conf(tmp_path, "[filter]\n%s : %d\n" % (name, v) + (more if name != "max_n" else "")))
            assert str(ei.value) == message == qconf.filter_range_message(name)
    with pytest.raises(ValueError):
        qconf.QuadeConf(_conf(tmp_path, "[filter]\n%s : many\n" % name))


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[filter]\nmax_n : 0\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == NEEDS == qconf.FILTER_NEEDS
    with pytest.raises(AssertionError) as ei:  # with the trimming asked for too, its message comes first, as before
        qconf.QuadeConf(_conf(tmp_path, "[trim]\nquality_cutoff : 20\n[filter]\nmax_n : 0\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == qconf.TRIM_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "[filter]\nqualified_quality : 20\nmax_n :\n", gpu="[gpu]\n" + gpu)).filter is False  # off: as before


@pytest.mark.parametrize("extra,gpu,message", [("max_n : 0\n", "[gpu]\ndevice_pipeline : False\n", NEEDS),
                                               ("min_complexity_pct : 101\n", "", "Authorized values for [filter] min_complexity_pct : 1 to 100")])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, extra, gpu, message):
    conf = _conf(tmp_path, "[filter]\n" + extra, gpu=gpu)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / fr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_a_conf_without_the_section_is_untouched(bundled_dir, tmp_path, monkeypatch):
    import shutil
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        golden = fh.read()
    assert qconf.template_bytes() == golden and b"[filter]" not in golden
    work = tmp_path / "result"
    work.mkdir()
    (work / "Quade_conf_file.txt").write_bytes(golden)
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    monkeypatch.chdir(work)  # the template names its files relative to the run's folder
    cf = qconf.QuadeConf("Quade_conf_file.txt")
    assert cf.filter is False and cf.trim is False and cf.pair_trim is False and cf.quality_report is False and cf.filter_params() == OFF


def test_exported_symbols():
    new = {"qd_filter_set", "qd_filter_get", "qd_filter_read", "qd_filter_add", "qd_filter_kind", "qd_dev_filter"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_filter_active", "qd_filter_device"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text and "#define QD_FILTER_VALUES 8" in text
    assert "no reference counterpart" in text.split("int qd_filter_set")[0][-6000:]
    assert "no reference counterpart" in text.split("int qd_dev_filter")[0][-1000:]
    assert ctypes.sizeof(hb.qd_filter_params) == 24 and [f[0] for f in hb.qd_filter_params._fields_] == list(FM.KEYS)
    assert ctypes.sizeof(hb.qd_pairtrim_params) == 16 and ctypes.sizeof(hb.qd_trim_params) == 64 + 64 + 6 * 4  # the other stages' are as they were
