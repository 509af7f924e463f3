"""The quality report off the GPU: the writer against hand-written text, the conf option and the configurations it rejects, the
exchange format of the ranks, and the exported symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import quality_report as qr
from tests import qstats_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "quality_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"


def test_report_lines_against_hand_written_text():
    t = np.zeros((5, 2, 6), dtype=np.uint64)
    #            records bases qual_sum q20 q30 n
    t[0, 0] = [3, 10, 305, 2, 1, 3]     # A_pass R1: mean length 3.33, 20.00 %, 10.00 %, mean quality 30.50, 30.00 % N
    t[0, 1] = [3, 3, 2, 2, 0, 2]        # A_pass R2: 2 / 3 -> 66.66 (rounded down), mean quality 0.66
    t[1, 0] = [2, 0, 0, 0, 0, 0]        # A_fail: reads without bases -> every ratio's denominator is 0
    t[1, 1] = [2, 7, 280, 7, 7, 0]
    #                                     B (t[2], t[3]): a sample without reads
    t[4, 0] = [1, 151, 5587, 150, 149, 1]
    t[4, 1] = [1, 1, 93, 1, 1, 1]       # mean quality 93.00: the largest Phred+33 value of a printable byte
    want = [
        "Program Quade-quality 0.3.2",
        "",
        "destination\tread\treads\tbases\tmean_length\tq20_bases\tq30_bases\tpercent_q20\tpercent_q30\tmean_quality\tn_bases\tpercent_n",
        "A_pass\tR1\t3\t10\t3.33\t2\t1\t20.00\t10.00\t30.50\t3\t30.00",
        "A_pass\tR2\t3\t3\t1.00\t2\t0\t66.66\t0.00\t0.66\t2\t66.66",
        "A_fail\tR1\t2\t0\t0.00\t0\t0\t0.00\t0.00\t0.00\t0\t0.00",
        "A_fail\tR2\t2\t7\t3.50\t7\t7\t100.00\t100.00\t40.00\t0\t0.00",
        "B_pass\tR1\t0\t0\t0.00\t0\t0\t0.00\t0.00\t0.00\t0\t0.00",
        "B_pass\tR2\t0\t0\t0.00\t0\t0\t0.00\t0.00\t0.00\t0\t0.00",
        "B_fail\tR1\t0\t0\t0.00\t0\t0\t0.00\t0.00\t0.00\t0\t0.00",
        "B_fail\tR2\t0\t0\t0.00\t0\t0\t0.00\t0.00\t0.00\t0\t0.00",
        "Undetermined\tR1\t1\t151\t151.00\t150\t149\t99.33\t98.67\t37.00\t1\t0.66",
        "Undetermined\tR2\t1\t1\t1.00\t1\t1\t100.00\t100.00\t93.00\t1\t100.00",
        "Total\tR1\t6\t161\t26.83\t152\t150\t94.40\t93.16\t36.59\t4\t2.48",
        "Total\tR2\t6\t11\t1.83\t10\t8\t90.90\t72.72\t34.09\t3\t27.27",
    ]
    assert qr.report_lines(t, ["A", "B"]) == want
    assert qr.REPORT_NAME == "Quade_quality_report.csv"
    assert "Date" not in "\n".join(want)
    with pytest.raises(AssertionError):
        qr.report_lines(t, ["A"])  # a table of another sample count


def test_report_lines_beyond_32_and_53_bits(tmp_path):
    t = np.zeros((1, 2, 6), dtype=np.uint64)
    t[0, 0] = [1 << 40, (1 << 62) + 1, (1 << 63) - 5, 1 << 61, 3, 1]
    lines = qr.report_lines(t, [])
    v = ((1 << 63) - 5) * 100 // ((1 << 62) + 1)
    assert lines[3].split("\t")[9] == "%d.%02d" % (v // 100, v % 100) == "1.99"  # exact integers, no float rounding up to 2.00
    assert lines[3] == lines[5].replace("Total", "Undetermined")
    p = tmp_path / qr.REPORT_NAME
    qr.write_report(str(p), t, [])
    assert p.read_text() == "\n".join(lines) + "\n"


def test_model_definitions():
    q = bytes([0, 32, 33, 34, 52, 53, 62, 63, 126, 127, 128, 255])
    assert QM.read_stats(b"NnACGTXnN...", q) == [1, 12, 1 + 19 + 20 + 29 + 30 + 93 + 94 + 95 + 222, 7, 5, 4]
    t = QM.table(1, [(0, (b"N", b"I"), (b"", b"")), (QM.UNDETERMINED, (b"AC", b"5>"), (b"n", b"!")), (1, (b"", b""), (b"G", b"?"))])
    assert t.shape == (3, 2, 6)
    assert t[0].tolist() == [[1, 1, 40, 1, 1, 1], [1, 0, 0, 0, 0, 0]]
    assert t[2].tolist() == [[1, 2, 49, 2, 0, 0], [1, 1, 0, 0, 0, 1]]
    assert t[1].tolist() == [[1, 0, 0, 0, 0, 0], [1, 1, 30, 1, 1, 0]]


def _conf(tmp_path, output_extra="", gpu=""):
    f = tmp_path / "reads.fastq"
    f.write_text("")
    txt = "[quality]\nminimal_qual : 25\n[fastq]\nseq_R1 : {0}\nseq_R2 : {0}\nindex_R1 : {0}\nindex_R2 : {0}\n".format(f)
    txt += "[index]\nindex2 : True\nmolecular1 : False\nmolecular2 : False\nindex1_start : 1\nindex1_end : 8\nindex2_start : 1\nindex2_end : 8\n"
    txt += "[output]\nwrite_pass : True\nwrite_fail : True\nwrite_undetermined : True\n" + output_extra + gpu
    txt += "[sample1]\nname : S1\nindex1_seq : ACAGACAG\nindex2_seq : CTTGCTTG\n"
    p = tmp_path / "conf.txt"
    p.write_text(txt)
    return str(p)


@pytest.mark.parametrize("extra,want", [("", False), ("quality_report :\n", False), ("quality_report : False\n", False),
                                        ("quality_report : True\n", True), ("quality_report : yes\n", True),
                                        ("quality_report : on\n", True), ("quality_report : 1\n", True),
                                        ("quality_report : 0\n", False), ("quality_report : no\n", False)])
def test_conf_option(tmp_path, extra, want):
    cf = qconf.QuadeConf(_conf(tmp_path, extra))
    assert cf.quality_report is want
    assert cf.top_unknown_barcodes == 0 and cf.device_pipeline
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, extra, gpu="[gpu]\n" + ok)).quality_report is want


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "quality_report : True\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "quality_report : False\n", gpu="[gpu]\n" + gpu)).quality_report is False  # off: as before
    assert qconf.QuadeConf(_conf(tmp_path, "", gpu="[gpu]\n" + gpu)).quality_report is False


def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path):
    conf = _conf(tmp_path, "quality_report : True\n", gpu="[gpu]\ndevice_pipeline : False\n")
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert NEEDS in r.stdout + r.stderr
    assert not (tmp_path / qr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_reference_conf_parses_as_before(bundled_dir, tmp_path, monkeypatch):
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        golden = fh.read()
    assert qconf.template_bytes() == golden and b"quality_report" not in golden
    work = tmp_path / "result"
    work.mkdir()
    (work / "Quade_conf_file.txt").write_bytes(golden)
    import shutil
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    monkeypatch.chdir(work)  # the template names its files relative to the run's folder
    cf = qconf.QuadeConf("Quade_conf_file.txt")
    assert cf.quality_report is False and cf.top_unknown_barcodes == 0 and (cf.idx1_mismatches, cf.idx2_mismatches) == (0, 0)
    assert [n for n, _ in cf.samples] == ["S1", "S2"] and cf.minimal_qual == 25 and cf.device_pipeline
    assert "quality_report" in qconf.QUALITY_HELP and "device_pipeline" in qconf.QUALITY_HELP


def test_exported_symbols():
    new = {"qd_qstats_enable", "qd_qstats_read", "qd_qstats_add", "qd_dev_qstats"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        header = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_qstats_kind"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6
    assert "no reference counterpart" in open(os.path.join(ROOT, "include", "quade_hip.h")).read().split("qd_qstats_enable")[0][-3000:]


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, (2 * 7 + 1, 2, 6), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, (2 * 7 + 1, 2, 6), dtype=np.uint64)
    a[3, 1, 2] = (1 << 63) - 1
    b[3, 1, 2] = 1 << 62
    blob = hb.pack_table("quality", a)
    assert isinstance(blob, bytes)
    a2 = hb.unpack_table("quality", blob)
    assert a2.dtype == np.uint64 and a2.shape == a.shape and (a2 == a).all()
    a2 += hb.unpack_table("quality", hb.pack_table("quality", b.reshape(-1)))  # (a flat table packs alike; unpacked tables are writable copies)
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2.reshape(-1), a.reshape(-1), b.reshape(-1)))
    assert int(a2[3, 1, 2]) == (1 << 63) - 1 + (1 << 62)  # sums stay integers beyond 2^63
    one = hb.unpack_table("quality", hb.pack_table("quality", np.zeros((1, 2, 6), np.uint64)))
    assert one.shape == (1, 2, 6)
    with pytest.raises(AssertionError):
        hb.unpack_table("quality", blob[:-8])
    assert hb.QSTATS_COUNTERS == ("records", "bases", "qual_sum", "q20_bases", "q30_bases", "n_bases")
