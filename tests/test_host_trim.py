"""3' trimming off the GPU: the plain Python model against hand-checked vectors, the report writer against hand-written text, the
[trim] section and the configurations it rejects, the exchange format of the ranks, and the exported symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import trim_report as tr
from tests import trim_model as TM
from tests.stage_support import _one_sample_conf as _conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "[trim] needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"


@pytest.mark.parametrize("ph,want", [([42, 40, 26, 27, 8, 7, 11, 4, 2, 3], 4), ([30, 5, 30], 3), ([30, 5, 5], 1), ([2, 2, 2], 0),
                                     ([10, 10], 2), ([9, 10], 0), ([40, 9, 10, 9], 1)])
def test_model_quality_trim_vectors(ph, want):
    assert TM.quality_trim_phred(ph, 10) == want
    assert TM.quality_trim(bytes(33 + v for v in ph), 10) == want
    assert TM.quality_trim(bytes(33 + v for v in ph), 0) == len(ph)  # off


def test_model_quality_bytes_are_unsigned_and_clamped():
    assert TM.quality_trim(bytes([255, 200, 0, 32, 33]), 10) == 2  # 222, 167 kept; three bytes of Phred 0 cut
    assert TM.quality_trim(b"", 10) == 0


@pytest.mark.parametrize("read,want", [("ACGTACGTAGATCGGAAGAGCTT", 8), ("ACGTACGTAGA", 8), ("ACGTACGTAG", 10),
                                       ("ACGTACGTAGATCGGTAGAGCTT", 8), ("ACGTACGTAGATCGGTAGTGCTT", 23),
                                       ("acgtacgtagatcggaagagc", 8), ("ACGTACGTAGATNGGAAGAGC", 8), ("ACGTACGTAGATNGGAAGAG", 8),
                                       ("AGATCGGAAGAGCACGT", 0), ("ACGAGTTTTTAGATCGGAAGAGC", 10), ("AGA", 0), ("TTAG", 4)])
def test_model_adapter_trim_vectors(read, want):
    assert TM.adapter_trim(read.encode(), len(read), b"AGATCGGAAGAGC", 3, 10) == want


def test_model_steps_in_order_and_the_floor():
    P = TM.Params("AGATCGGAAGAGC", "", quality_cutoff=10, min_length=9)
    seq, qual = b"ACGTACGTAGATCGGAAGAGCTT", bytes([33 + 40] * 20 + [33 + 2] * 3)
    assert TM.trim_read(seq, qual, 0, P) == (20, 8, 9)  # quality first, the adapter in what is left, then the floor
    assert TM.trim_read(seq, qual, 1, P) == (20, 20, 20)  # R2 has no adapter
    assert TM.trim_read(b"AGA", b"III", 0, P) == (3, 0, 3)  # the floor never exceeds the read
    t = TM.new_table()
    assert TM.count(t, seq, qual, 0, P) == 9 and TM.count(t, seq, qual, 1, P) == 20
    assert t == [[1, 23, 9, 1, 3, 1, 12, 1], [1, 23, 20, 1, 3, 0, 0, 0]]
    assert P.on and not TM.Params(min_length=5).on and TM.Params(quality_cutoff=1).on and TM.Params("", "a").adapters[1] == b"A"


PARAMS = dict(adapter_r1="AGATCGGAAGAGC", adapter_r2="", quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=0)


def test_report_lines_against_hand_written_text(tmp_path):
    t = [[3, 10, 7, 1, 2, 1, 1, 0], [3, 3, 3, 0, 0, 0, 0, 0]]
    want = [
        "Program Quade-trim 0.3.2",
        "",
        "adapter_r1\tAGATCGGAAGAGC",
        "adapter_r2\t",
        "quality_cutoff\t20",
        "min_overlap\t3",
        "max_mismatch_pct\t10",
        "min_length\t0",
        "",
        "read\treads\tbases_in\tbases_out\tquality_trimmed_reads\tquality_trimmed_bases\tadapter_reads\tadapter_bases\tfloored_reads\t"
        "percent_quality_trimmed_reads\tpercent_adapter_reads\tpercent_bases_trimmed",
        "R1\t3\t10\t7\t1\t2\t1\t1\t0\t33.33\t33.33\t30.00",
        "R2\t3\t3\t3\t0\t0\t0\t0\t0\t0.00\t0.00\t0.00",
        "Total\t6\t13\t10\t1\t2\t1\t1\t0\t16.66\t16.66\t23.07",
    ]
    assert tr.report_lines(t, PARAMS) == want
    assert tr.report_lines(np.array(t, dtype=np.uint64), PARAMS) == want
    assert tr.REPORT_NAME == "Quade_trim_report.csv" and "Date" not in "\n".join(want)
    assert tr.report_lines([[0] * 8, [0] * 8], PARAMS)[-1] == "Total\t0\t0\t0\t0\t0\t0\t0\t0\t0.00\t0.00\t0.00"
    with pytest.raises(AssertionError):
        tr.report_lines([[0] * 8], PARAMS)
    p = tmp_path / tr.REPORT_NAME
    tr.write_report(str(p), t, PARAMS)
    assert p.read_text() == "\n".join(want) + "\n"
    assert tr.COUNTERS == hb.TRIM_COUNTERS == TM.COUNTERS


def test_report_lines_beyond_53_bits():
    t = np.zeros((2, 8), dtype=np.uint64)
    t[0] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 62) + 5, (1 << 61) + 1, 7, 1 << 60, 9, 1]
    t[1] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 63) + 3, 0, 0, 0, 0, 0]
    lines = tr.report_lines(t, PARAMS)
    r1 = lines[-3].split("\t")
    assert r1[1:9] == [str(int(x)) for x in t[0]]
    v = ((1 << 61) + 1) * 10000 // ((1 << 62) + 1)
    assert r1[9] == "%d.%02d" % (v // 100, v % 100) == "50.00"
    v = (((1 << 63) + 3) - ((1 << 62) + 5)) * 10000 // ((1 << 63) + 3)
    assert r1[11] == "%d.%02d" % (v // 100, v % 100) == "49.99"  # exact integers: a float would round to 50.00
    total = lines[-1].split("\t")
    assert total[1] == str((1 << 63) + 2) and total[2] == str((1 << 64) + 6)  # the sum of two rows passes 64 bits and stays exact


def test_conf_defaults_and_when_trimming_is_on(tmp_path):
    for trim in ("", "[trim]\n", "[trim]\nadapter_R1 :\nadapter_R2 :\nquality_cutoff :\nmin_overlap :\nmax_mismatch_pct :\nmin_length :\n",
                 "[trim]\nquality_cutoff : 0\nmin_length : 30\nmin_overlap : 5\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, trim))
        assert cf.trim is False and (cf.adapter_R1, cf.adapter_R2, cf.quality_cutoff, cf.max_mismatch_pct) == ("", "", 0, 10)
    cf = qconf.QuadeConf(_conf(tmp_path, ""))
    assert cf.trim_params() == dict(adapter_r1="", adapter_r2="", quality_cutoff=0, min_overlap=3, max_mismatch_pct=10, min_length=0)
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\nadapter_R1 : agatcggaagagc\n"))
    assert cf.trim is True and cf.adapter_R1 == "AGATCGGAAGAGC" and cf.adapter_R2 == ""  # upper-cased on reading
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\nadapter_R2 : A\nmin_overlap : 1\n")).trim is True
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\nquality_cutoff : 1\n")).trim is True
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, "[trim]\nquality_cutoff : 20\n", gpu="[gpu]\n" + ok)).trim is True


A64 = "ACGT" * 16


@pytest.mark.parametrize("trim", [
    "adapter_R1 : A\nmin_overlap : 1\n", "adapter_R1 : %s\n" % A64, "adapter_R2 : %s\nmin_overlap : 64\n" % A64,
    "quality_cutoff : 0\nadapter_R1 : ACG\n", "quality_cutoff : 93\n", "quality_cutoff : 1\nmin_overlap : 1\n",
    "quality_cutoff : 1\nmin_overlap : 64\n", "quality_cutoff : 1\nmax_mismatch_pct : 0\n", "quality_cutoff : 1\nmax_mismatch_pct : 50\n",
    "quality_cutoff : 1\nmin_length : 0\n", "quality_cutoff : 1\nmin_length : 65535\n", "adapter_R1 : ACG\nadapter_R2 : ACGTT\nmin_overlap : 3\n"])
def test_conf_values_at_the_edges_are_accepted(tmp_path, trim):
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + trim)).trim is True


@pytest.mark.parametrize("trim,message", [
    ("adapter_R1 : %sA\n" % A64, qconf.TRIM_ADAPTER), ("adapter_R2 : ACGN\n", qconf.TRIM_ADAPTER), ("adapter_R1 : AC-GT\n", qconf.TRIM_ADAPTER),
    ("quality_cutoff : -1\n", qconf.TRIM_CUTOFF), ("quality_cutoff : 94\n", qconf.TRIM_CUTOFF),
    ("quality_cutoff : 1\nmin_overlap : 0\n", qconf.TRIM_OVERLAP), ("quality_cutoff : 1\nmin_overlap : 65\n", qconf.TRIM_OVERLAP),
    ("adapter_R1 : AC\n", qconf.TRIM_OVERLAP), ("adapter_R1 : ACGTACGT\nadapter_R2 : ACG\nmin_overlap : 4\n", qconf.TRIM_OVERLAP),
    ("quality_cutoff : 1\nmax_mismatch_pct : -1\n", qconf.TRIM_MISMATCH), ("quality_cutoff : 1\nmax_mismatch_pct : 51\n", qconf.TRIM_MISMATCH),
    ("quality_cutoff : 1\nmin_length : -1\n", qconf.TRIM_LENGTH), ("quality_cutoff : 1\nmin_length : 65536\n", qconf.TRIM_LENGTH)])
def test_conf_values_beyond_the_edges_are_rejected(tmp_path, trim, message):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + trim))
    assert str(ei.value) == message and message.startswith("Authorized values for ")


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    for trim in ("[trim]\nquality_cutoff : 20\n", "[trim]\nadapter_R2 : AGATCGGAAGAGC\n"):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, trim, gpu="[gpu]\n" + gpu))
        assert str(ei.value) == NEEDS == qconf.TRIM_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\nmin_length : 20\n", gpu="[gpu]\n" + gpu)).trim is False  # off: as before
    assert qconf.QuadeConf(_conf(tmp_path, "", gpu="[gpu]\n" + gpu)).trim is False


@pytest.mark.parametrize("trim,gpu,message", [("quality_cutoff : 20\n", "[gpu]\ndevice_pipeline : False\n", NEEDS),
                                              ("quality_cutoff : 94\n", "", qconf.TRIM_CUTOFF)])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, trim, gpu, message):
    conf = _conf(tmp_path, "[trim]\n" + trim, gpu=gpu)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / tr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_reference_conf_parses_with_trimming_off(bundled_dir, tmp_path, monkeypatch):
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        golden = fh.read()
    assert qconf.template_bytes() == golden and b"[trim]" not in golden and b"adapter" not in golden
    work = tmp_path / "result"
    work.mkdir()
    (work / "Quade_conf_file.txt").write_bytes(golden)
    import shutil
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    monkeypatch.chdir(work)  # the template names its files relative to the run's folder
    cf = qconf.QuadeConf("Quade_conf_file.txt")
    assert cf.trim is False and cf.quality_report is False and (cf.min_overlap, cf.max_mismatch_pct, cf.min_length) == (3, 10, 0)
    assert [n for n, _ in cf.samples] == ["S1", "S2"] and cf.minimal_qual == 25 and cf.device_pipeline
    for word in ("adapter_R1", "adapter_R2", "quality_cutoff", "min_overlap", "max_mismatch_pct", "min_length", "device_pipeline"):
        assert word in qconf.TRIM_HELP


def test_exported_symbols():
    new = {"qd_trim_set", "qd_trim_get", "qd_trim_read", "qd_trim_add", "qd_dev_trim"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text
    assert "no reference counterpart" in text.split("int qd_trim_set")[0][-4000:]
    assert "no reference counterpart" in text.split("int qd_dev_trim")[0][-1000:]
    import ctypes
    assert ctypes.sizeof(hb.qd_trim_params) == 64 + 64 + 6 * 4


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, (2, 8), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, (2, 8), dtype=np.uint64)
    a[1, 2], b[1, 2] = (1 << 63) - 1, 1 << 62
    blob = hb.pack_table("trim", a)
    assert isinstance(blob, bytes) and len(blob) == 128
    a2 = hb.unpack_table("trim", blob)
    assert a2.dtype == np.uint64 and a2.shape == (2, 8) and (a2 == a).all()
    a2 += hb.unpack_table("trim", hb.pack_table("trim", b.reshape(-1)))  # (a flat table packs alike; unpacked tables are writable copies)
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2.reshape(-1), a.reshape(-1), b.reshape(-1)))
    assert int(a2[1, 2]) == (1 << 63) - 1 + (1 << 62)  # sums stay integers beyond 2^63
    with pytest.raises(AssertionError):
        hb.unpack_table("trim", blob[:-8])
    assert hb.TRIM_COUNTERS == ("reads", "bases_in", "bases_out", "quality_trimmed_reads", "quality_trimmed_bases", "adapter_reads",
                                "adapter_bases", "floored_reads")
