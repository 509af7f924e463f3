"""The per-cycle report off the GPU: the writer against hand-written text, the conf option and the configurations it rejects, the
exchange format of the ranks, the exported symbols, and the model's own cross-checks against tests/qstats_model.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import cycle_report as cr
from quade_amd import hip_backend as hb
from tests import cycle_model as CM
from tests import qstats_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = "cycle_report needs the device pipeline (device_pipeline, device_inflate, device_deflate : True and gzip_level 1 or -1)"
HEAD = "group\tread\tcycle\treads\tA\tC\tG\tT\tN\tother\tpercent_gc\tmean_quality\tq20\tq30\tpercent_q20\tpercent_q30"


def test_report_lines_against_hand_written_text():
    t = CM.empty()
    # pass R1: three reads of lengths 1, 2, 2 -> reads(cycle 1) = 3, reads(cycle 2) = 2, nothing listed behind cycle 2
    t["len"][0, 0, 1], t["len"][0, 0, 2] = 1, 2
    t["cycle"][0, 0, 0] = [1, 0, 1, 0, 0, 100, 2, 1]   # A, G and one other letter: other = 3 - 2 = 1
    t["cycle"][0, 0, 1] = [0, 1, 0, 0, 1, 61, 1, 1]    # C and N
    t["meanq"][0, 0, 30], t["meanq"][0, 0, 40] = 2, 1
    t["gc"][0, 0, 0], t["gc"][0, 0, 50], t["gc"][0, 0, 100] = 1, 1, 1
    # pass R2: three empty reads -> no cycle rows, a length bin 0, no per-read bins
    t["len"][0, 1, 0] = 3
    # Undetermined R1: one read of 1024 bases or more, T with quality 35 at every cycle
    t["len"][2, 0, 1024] = 1
    t["cycle"][2, 0, :, 3] = 1
    t["cycle"][2, 0, :, 5] = 35
    t["cycle"][2, 0, :, 6] = 1
    t["meanq"][2, 0, 93] = 1
    t["gc"][2, 0, 0] = 1
    lines = cr.report_lines(t)
    assert lines[:5] == ["Program Quade-cycle 0.3.2", "",
                         "Reads of 1024 bases or more\t1\t(cycles from 1025 on are not counted per cycle)", "", HEAD]
    per_cycle = lines[5:lines.index("Read lengths") - 1]
    assert per_cycle[:2] == ["pass\tR1\t1\t3\t1\t0\t1\t0\t0\t1\t33.33\t33.33\t2\t1\t66.66\t33.33",
                             "pass\tR1\t2\t2\t0\t1\t0\t0\t1\t0\t50.00\t30.50\t1\t1\t50.00\t50.00"]
    und = ["Undetermined\tR1\t%d\t1\t0\t0\t0\t1\t0\t0\t0.00\t35.00\t1\t0\t100.00\t0.00" % c for c in range(1, 1025)]
    assert per_cycle[2:1026] == und
    # Total = the sum of the groups: cycles 1 and 2 hold both groups' reads, the later ones the long read alone
    assert per_cycle[1026:1028] == ["Total\tR1\t1\t4\t1\t0\t1\t1\t0\t1\t25.00\t33.75\t3\t1\t75.00\t25.00",
                                    "Total\tR1\t2\t3\t0\t1\t0\t1\t1\t0\t33.33\t32.00\t2\t1\t66.66\t33.33"]
    assert per_cycle[1028:] == [ln.replace("Undetermined", "Total") for ln in und[2:]]
    rest = lines[lines.index("Read lengths") - 1:]
    assert rest == [
        "", "Read lengths", "group\tread\tlength\treads",
        "pass\tR1\t1\t1", "pass\tR1\t2\t2", "pass\tR2\t0\t3", "Undetermined\tR1\t>=1024\t1",
        "Total\tR1\t1\t1", "Total\tR1\t2\t2", "Total\tR1\t>=1024\t1", "Total\tR2\t0\t3",
        "", "Per-read mean quality", "group\tread\tmean_quality\treads",
        "pass\tR1\t30\t2", "pass\tR1\t40\t1", "Undetermined\tR1\t93\t1", "Total\tR1\t30\t2", "Total\tR1\t40\t1", "Total\tR1\t93\t1",
        "", "Per-read GC percent", "group\tread\tpercent_gc\treads",
        "pass\tR1\t0\t1", "pass\tR1\t50\t1", "pass\tR1\t100\t1", "Undetermined\tR1\t0\t1",
        "Total\tR1\t0\t2", "Total\tR1\t50\t1", "Total\tR1\t100\t1"]
    assert cr.REPORT_NAME == "Quade_cycle_report.csv" and "Date" not in "\n".join(lines)
    assert not [ln for ln in lines if ln.startswith("fail")]  # an empty group has no rows


def test_report_without_long_reads_and_beyond_63_bits(tmp_path):
    t = CM.empty()
    t["len"][1, 1, 1] = (1 << 63) + 5
    t["len"][2, 1, 1] = 1 << 63
    t["cycle"][1, 1, 0] = [1 << 62, 0, 0, 0, 0, (1 << 63) - 5, 3, 1]
    lines = cr.report_lines(t)
    assert lines[:3] == ["Program Quade-cycle 0.3.2", "", HEAD]  # no note: no read of 1024 bases or more
    reads = (1 << 63) + 5
    v = ((1 << 63) - 5) * 100 // reads
    assert lines[3].split("\t")[:4] == ["fail", "R2", "1", str(reads)] and lines[3].split("\t")[9] == str(reads - (1 << 62))
    assert lines[3].split("\t")[11] == "%d.%02d" % (v // 100, v % 100) == "0.99"  # exact integers, no float rounding up to 1.00
    assert lines[5].split("\t")[:4] == ["Total", "R2", "1", str((1 << 64) + 5)]  # sums stay integers beyond 2^64
    p = tmp_path / cr.REPORT_NAME
    cr.write_report(str(p), t)
    assert p.read_text() == "\n".join(lines) + "\n"


def test_model_definitions_and_cross_checks_against_the_qstats_model():
    q = bytes([0, 32, 33, 34, 52, 53, 62, 63, 126, 127, 128, 255])
    pairs = [(0, 0, (b"NnACGTXnN...", q), (b"", b"")),
             (4, 0, (b"gc", b"5>"), (b"aCgTn*", b"!!IIII")),
             (1, 0, (b"", b""), (b"G", b"?")),
             (7, 3, (b"AAAA", b"IIII"), (b"CCCC", b"IIII")),  # dropped: adds nothing anywhere
             (CM.UNDETERMINED, 0, (b"AC", b"5>"), (b"n", b"!"))]
    t = CM.table(pairs)
    assert t["cycle"].shape == (3, 2, 1024, 8) and t["len"].shape == (3, 2, 1025) and t["meanq"].shape == (3, 2, 94) and t["gc"].shape == (3, 2, 101)
    assert t["cycle"][0, 0, 0].tolist() == [0, 0, 1, 0, 1, 20, 1, 0]   # 'N' (q 0) of the first pair and 'g' (q 20) of the second
    assert t["cycle"][0, 0, 1].tolist() == [0, 1, 0, 0, 1, 29, 1, 0]   # 'n' and 'c' (q 29)
    assert t["cycle"][0, 0, 2].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]    # 'A' with q byte 33
    assert t["cycle"][0, 0, 6].tolist() == [0, 0, 0, 0, 0, 29, 1, 0]   # 'X' is none of the letters: other
    assert t["cycle"][0, 0, 11].tolist() == [0, 0, 0, 0, 0, 222, 1, 1]  # quality byte 255
    assert t["len"][0, 0, 12] == 1 and t["len"][0, 0, 2] == 1 and t["len"][0, 1, 0] == 1 and t["len"][0, 1, 6] == 1
    assert t["meanq"][0, 0, (1 + 19 + 20 + 29 + 30 + 93 + 94 + 95 + 222) // 12] == 1 and t["meanq"][0, 0, 24] == 1
    assert t["gc"][0, 0, 100 * 2 // 12] == 1 and t["gc"][0, 0, 100] == 1 and t["gc"][0, 1, 33] == 1
    assert t["meanq"][0, 1].sum() == 1  # the empty read has no per-read bins
    assert t["len"][1].sum() == 2 and t["cycle"][1, 1, 0].tolist() == [0, 0, 1, 0, 0, 30, 1, 1] and not t["cycle"][1, 0].any()
    assert t["len"][2, 0, 2] == 1 and t["cycle"][2, 1, 0, 4] == 1
    assert sum(int(t[k].sum()) for k in ("len",)) == 8  # the dropped pair is nowhere
    # a mean above 93 lands in the last bin
    hi = CM.table([(0, 0, (b"A", bytes([255])), (b"A", bytes([126])))])
    assert hi["meanq"][0, 0, 93] == 1 and hi["meanq"][0, 1, 93] == 1
    # cross-checks: N, qual_sum, q20, q30 and bases against the qstats model over the same (kept) pairs
    S = 4
    qs = QM.table(S, [(c, a, b) for c, d, a, b in pairs if not d])
    want = [[int(qs[:, r, k].sum()) for k in range(6)] for r in range(2)]
    assert CM.qstats_columns(t) == want
    assert CM.equal(CM.add(t, hi), CM.table(pairs + [(0, 0, (b"A", bytes([255])), (b"A", bytes([126])))]))


def test_reads_beyond_1024_cycles_count_per_read_only():
    seq, qual = b"G" * 1500, b"I" * 1500
    t = CM.table([(1, 0, (seq, qual), (seq[:1024], qual[:1024]))])
    assert t["len"][1, :, 1024].tolist() == [1, 1] and t["cycle"][1, :, :, 2].sum() == 2048 and t["cycle"][1, 0, 1023, 5] == 40
    assert t["gc"][1, 0, 100] == 1 and t["meanq"][1, 0, 40] == 1


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


@pytest.mark.parametrize("extra,want", [("", False), ("cycle_report :\n", False), ("cycle_report : False\n", False),
                                        ("cycle_report : True\n", True), ("cycle_report : yes\n", True),
                                        ("cycle_report : on\n", True), ("cycle_report : 1\n", True),
                                        ("cycle_report : 0\n", False), ("cycle_report : no\n", False)])
def test_conf_option(tmp_path, extra, want):
    cf = qconf.QuadeConf(_conf(tmp_path, extra))
    assert cf.cycle_report is want
    assert cf.quality_report is False and cf.device_pipeline
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, extra, gpu="[gpu]\n" + ok)).cycle_report is want


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "cycle_report : True\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == NEEDS == qconf.CYCLE_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "cycle_report : False\n", gpu="[gpu]\n" + gpu)).cycle_report is False  # off: as before
    assert qconf.QuadeConf(_conf(tmp_path, "", gpu="[gpu]\n" + gpu)).cycle_report is False


def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path):
    conf = _conf(tmp_path, "cycle_report : True\n", gpu="[gpu]\ndevice_pipeline : False\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert NEEDS in r.stdout + r.stderr
    assert not (tmp_path / cr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_reference_conf_parses_as_before(bundled_dir, tmp_path, monkeypatch):
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt"), "rb") as fh:
        golden = fh.read()
    assert qconf.template_bytes() == golden and b"cycle_report" not in golden
    work = tmp_path / "result"
    work.mkdir()
    (work / "Quade_conf_file.txt").write_bytes(golden)
    import shutil
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    monkeypatch.chdir(work)  # the template names its files relative to the run's folder
    cf = qconf.QuadeConf("Quade_conf_file.txt")
    assert cf.cycle_report is False and cf.quality_report is False
    assert [n for n, _ in cf.samples] == ["S1", "S2"] and cf.minimal_qual == 25 and cf.device_pipeline
    assert "cycle_report" in qconf.CYCLE_HELP and "device_pipeline" in qconf.CYCLE_HELP


def test_exported_symbols_and_layout_constants():
    new = {"qd_cstats_enable", "qd_cstats_read", "qd_cstats_add", "qd_cstats_lds_cycles", "qd_dev_cstats"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_cstats_device"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6
    assert "no reference counterpart" in text.split("int qd_cstats_enable")[0][-6000:]
    consts = {k: int(v) for k, v in re.findall(r"\b(QD_CS_[A-Z_0-9]+) = (\d+)", header)}
    assert (consts["QD_CS_CYCLES"], consts["QD_CS_LEN_BINS"], consts["QD_CS_MEANQ_BINS"], consts["QD_CS_GC_BINS"]) == \
        (hb.CSTATS_CYCLES, hb.CSTATS_LEN_BINS, hb.CSTATS_MEANQ_BINS, hb.CSTATS_GC_BINS) == (CM.CYCLES, CM.LEN_BINS, CM.MEANQ_BINS, CM.GC_BINS)
    assert consts["QD_CS_GR_VALUES"] == hb.CSTATS_GR_VALUES == 9412 and consts["QD_CS_VALUES"] == hb.CSTATS_VALUES == 56472
    assert [consts["QD_CS_" + n.upper()] for n in hb.CSTATS_COUNTERS] == list(range(8)) and consts["QD_CS_COUNTERS"] == 8
    lds = hb.load_library().qd_cstats_lds_cycles()
    assert 0 < lds <= 1024 and lds % 16 == 0


def test_views_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, hb.CSTATS_VALUES, dtype=np.uint64)
    b = rng.integers(0, 1 << 62, hb.CSTATS_VALUES, dtype=np.uint64)
    va = hb.cstats_views(a)
    assert {k: v.shape for k, v in va.items()} == {"cycle": (3, 2, 1024, 8), "len": (3, 2, 1025), "meanq": (3, 2, 94), "gc": (3, 2, 101)}
    # the layout: group-major, then read; cycle, len, meanq, gc
    at = (1 * 2 + 1) * 9412
    assert va["cycle"][1, 1, 7, 5] == a[at + 7 * 8 + 5] and va["len"][1, 1, 1024] == a[at + 8192 + 1024]
    assert va["meanq"][1, 1, 93] == a[at + 8192 + 1025 + 93] and va["gc"][2, 1, 100] == a[-1] and va["cycle"][0, 0, 0, 0] == a[0]
    assert (hb.cstats_flat(va) == a).all() and (hb.cstats_flat(a) == a).all()
    va["gc"][2, 1, 100] = (1 << 63) - 1  # a view: the flat table changes
    assert int(a[-1]) == (1 << 63) - 1
    b[-1] = 1 << 62
    blob = hb.pack_table("cycle", va)
    assert isinstance(blob, bytes) and blob == hb.pack_table("cycle", a)
    a2 = hb.unpack_table("cycle", blob)
    assert all(a2[k].dtype == np.uint64 and (a2[k] == va[k]).all() for k in va)
    total = hb.cstats_flat(a2) + hb.cstats_flat(hb.unpack_table("cycle", hb.pack_table("cycle", b)))
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(total[::97], a[::97], b[::97]))
    assert int(total[-1]) == (1 << 63) - 1 + (1 << 62)  # sums stay integers beyond 2^63
    with pytest.raises(AssertionError):
        hb.unpack_table("cycle", blob[:-8])
    with pytest.raises(AssertionError):
        hb.cstats_views(a[:-1])
    assert hb.CSTATS_GROUPS == ("pass", "fail", "Undetermined") == cr.GROUPS
    assert hb.CSTATS_COUNTERS == ("A", "C", "G", "T", "N", "qual_sum", "q20", "q30")
    # the model's dict is the backend's dict
    m = CM.table([(0, 0, (b"AC", b"II"), (b"G", b"5"))])
    assert CM.equal(hb.cstats_views(hb.cstats_flat(m)), m)
