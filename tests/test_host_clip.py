"""End clipping, window and poly-G trimming without a GPU: the model's rules (tests/clip_model.py) on hand-checked vectors and against a
second, independent form of each rule, the [trim] section's new options, the clip report's arithmetic and the exported symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import clip_report as cr
from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from tests import clip_model as CM
from tests.stage_support import _one_sample_conf as _conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(front_clip_r1=2, front_clip_r2=0, tail_clip_r1=1, tail_clip_r2=0, window_size=4, window_quality=20, poly_g_min_length=10,
              min_length=0)


@pytest.mark.parametrize("read,want", [
    (b"ACGTACGTAC" + b"G" * 10, 10),
    (b"ACGTACGTAC" + b"G" * 9, 10),  # the C counts as the one allowed mismatch
    (b"ACGTACGTCAGTGGGGGGGGGGGG", 10),
    (b"ACGTACGTACGTAGGGGGGGGA", 22),
    (b"G" * 12, 0),
    (b"TTTTGAGAGAGAGAGGGGGGGGGG", 12),
    (b"ACGTGGGAGGGGGGGGGGGGAGGGGGGG", 2)])
def test_model_poly_g_vectors(read, want):
    assert CM.poly_g(read, 10) == want
    assert CM.poly_g(read.lower(), 10) == want  # g counts as G
    assert CM.poly_g(read, 0) == len(read)  # off


@pytest.mark.parametrize("ph,W,Q,want", [
    ([30] * 10 + [2] * 5, 4, 20, 8),
    ([30, 30, 30, 10, 30, 30, 30, 30], 4, 25, 8),  # sum 100 is not below 100
    ([30] * 6 + [19] * 4, 4, 20, 6),
    ([30, 30, 20, 20, 20, 10, 30], 4, 20, 2),
    ([10, 10, 10], 4, 20, 3)])
def test_model_window_vectors(ph, W, Q, want):
    assert CM.window_phred(ph, W, Q) == want
    assert CM.window(bytes(33 + v for v in ph), W, Q) == want
    assert CM.window(bytes(33 + v for v in ph), 0, 0) == len(ph)  # off


def test_model_quality_bytes_are_unsigned_and_clamped():
    assert CM.window(bytes([0, 10, 32, 33]), 4, 1) == 0  # below 33: Phred 0
    assert CM.window(bytes([255] * 4), 4, 93) == 4  # 222 each
    assert CM.window(bytes([33 + 93] * 3 + [32]), 4, 70) == 0 and CM.window(bytes([33 + 93] * 3 + [32]), 4, 69) == 4


def _poly_g_loop(seq, P):
    """fastp's trimPolyG as a loop over the read's 3' end (one mismatch per 8 bases, at most 5), on upper-cased bases"""
    data = bytes(seq).upper()
    rlen = len(data)
    mismatch, first_g, i = 0, rlen - 1, 0
    while i < rlen:
        if data[rlen - i - 1] != ord("G"):
            mismatch += 1
        else:
            first_g = rlen - i - 1
        if mismatch > 5 or (mismatch > (i + 1) // 8 and i >= P - 1):
            break
        i += 1
    return first_g if i >= P else rlen


def _window_brute(ph, W, Q):
    for p in range(len(ph) - W + 1):
        if sum(ph[p:p + W]) < Q * W:
            return p
    return len(ph)


def test_model_agrees_with_the_second_forms_on_random_reads():
    rng = np.random.default_rng(77)
    cut_g = cut_w = 0
    for k in range(4000):
        L = int(rng.integers(0, 41))
        alphabet = (b"G" * 12 + b"ACTNg", b"GGGA", b"ACGT")[k % 3]
        seq = bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))
        P = int(rng.integers(6, 16))
        got = CM.poly_g(seq, P)
        assert got == _poly_g_loop(seq, P), (seq, P)
        cut_g += got < L
        W, Q = int(rng.integers(1, 12)), int(rng.integers(1, 41))
        ph = [int(v) for v in rng.integers(0, 42, L)]
        got = CM.window_phred(ph, W, Q)
        assert got == _window_brute(ph, W, Q), (ph, W, Q)
        cut_w += got < L
    assert cut_g > 300 and cut_w > 500  # both rules cut often enough for the comparison to mean something


def test_model_steps_in_order_and_the_floor():
    seq = b"TTACATACATACAT" + b"G" * 12 + b"AC"
    qual = bytes([33 + 35] * 26 + [33 + 2] * 2)
    P = CM.Params(front_clip=(2, 0), tail_clip=(0, 1), window_size=2, window_quality=20, poly_g_min_length=10)
    # R1: 2 off the front; the first window with a bad base starts one base in front of it, which uncovers the G tail; 11 G go
    assert CM.clip_read(seq, qual, 0, P) == (2, 26, 23, 12, 12)
    # R2: 1 off the tail; the window with the bad base that is left; the G tail
    assert CM.clip_read(seq, qual, 1, P) == (0, 27, 25, 14, 14)
    P.min_length = 20
    assert CM.clip_read(seq, qual, 0, P)[4] == 20 and CM.clip_read(seq, qual, 1, P)[4] == 20
    P.min_length = 1000  # above L - f: everything cut from the 3' end comes back, the front clip does not
    assert CM.clip_read(seq, qual, 0, P)[4] == 26 and CM.clip_read(seq, qual, 1, P)[4] == 28
    P = CM.Params(front_clip=(1000, 27), tail_clip=(5, 5))
    assert CM.clip_read(seq, qual, 0, P) == (28, 0, 0, 0, 0) and CM.clip_read(seq, qual, 1, P) == (27, 0, 0, 0, 0)
    table = CM.new_table()
    assert CM.count(table, seq, qual, 1, P) == (27, 0) and table[1] == [1, 28, 0, 1, 27, 1, 1, 0, 0, 0, 0, 0]
    text = CM.clipped_text([(b"@r", seq, qual)], 0, CM.Params(front_clip=(2, 0), tail_clip=(3, 0)))
    assert text == b"@r\n" + seq[2:25] + b"\n+\n" + qual[2:25] + b"\n"


def test_report_lines_against_hand_written_text(tmp_path):
    t = [[3, 30, 20, 3, 6, 2, 2, 1, 1, 1, 1, 0], [3, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    want = [
        "Program Quade-clip 0.3.2",
        "",
        "front_clip_r1\t2",
        "front_clip_r2\t0",
        "tail_clip_r1\t1",
        "tail_clip_r2\t0",
        "window_size\t4",
        "window_quality\t20",
        "poly_g_min_length\t10",
        "min_length\t0",
        "",
        "read\treads\tbases_in\tbases_out\tfront_clipped_reads\tfront_clipped_bases\ttail_clipped_reads\ttail_clipped_bases\twindow_reads\t"
        "window_bases\tpolyg_reads\tpolyg_bases\tfloored_reads\tpercent_window_reads\tpercent_polyg_reads\tpercent_bases_clipped",
        "R1\t3\t30\t20\t3\t6\t2\t2\t1\t1\t1\t1\t0\t33.33\t33.33\t33.33",
        "R2\t3\t3\t3\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0.00\t0.00\t0.00",
        "Total\t6\t33\t23\t3\t6\t2\t2\t1\t1\t1\t1\t0\t16.66\t16.66\t30.30",
    ]
    assert cr.report_lines(t, PARAMS) == want
    assert cr.report_lines(np.array(t, dtype=np.uint64), PARAMS) == want
    assert cr.REPORT_NAME == "Quade_clip_report.csv" and "Date" not in "\n".join(want)
    assert cr.report_lines([[0] * 12, [0] * 12], PARAMS)[-1] == "Total" + "\t0" * 12 + "\t0.00\t0.00\t0.00"
    with pytest.raises(AssertionError):
        cr.report_lines([[0] * 8, [0] * 8], PARAMS)
    p, p2 = tmp_path / cr.REPORT_NAME, tmp_path / "again.csv"
    cr.write_report(str(p), t, PARAMS)
    cr.write_report(str(p2), np.array(t, dtype=np.uint64), dict(PARAMS))
    assert p.read_bytes() == p2.read_bytes() == ("\n".join(want) + "\n").encode()  # two writes of one table: byte-identical
    assert cr.COUNTERS == hb.CLIP_COUNTERS == CM.COUNTERS
    assert set(cr.PARAMS) == set(CM.Params().keywords())


def test_report_lines_beyond_53_bits():
    t = np.zeros((2, 12), dtype=np.uint64)
    t[0, :3] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 62) + 5]
    t[1, :3] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 63) + 3]
    lines = cr.report_lines(t, PARAMS)
    v = (((1 << 63) + 3) - ((1 << 62) + 5)) * 10000 // ((1 << 63) + 3)
    assert lines[-3].split("\t")[15] == "%d.%02d" % (v // 100, v % 100) == "49.99"  # exact integers: a float would round to 50.00
    total = lines[-1].split("\t")
    assert total[1] == str((1 << 63) + 2) and total[2] == str((1 << 64) + 6)  # the sum of two rows passes 64 bits and stays exact


OFF = dict(front_clip_r1=0, front_clip_r2=0, tail_clip_r1=0, tail_clip_r2=0, window_size=0, window_quality=0, poly_g_min_length=0, min_length=0)


def test_conf_defaults_and_when_the_stage_is_on(tmp_path):
    for trim in ("", "[trim]\n", "[trim]\nfront_clip_R1 :\nfront_clip_R2 :\ntail_clip_R1 :\ntail_clip_R2 :\nwindow_size :\nwindow_quality :\npoly_g :\n"
                 "poly_g_min_length :\n", "[trim]\nfront_clip_R1 : 0\ntail_clip_R2 : 0\npoly_g : False\npoly_g_min_length : 20\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, trim))
        assert cf.clip is False and cf.trim is False and cf.clip_params() == OFF
        assert (cf.front_clip, cf.tail_clip, cf.window_size, cf.window_quality, cf.poly_g) == ((0, 0), (0, 0), None, None, False)
    assert qconf.QuadeConf(_conf(tmp_path, "")).poly_g_min_length == 10
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\nfront_clip_R2 : 7\ntail_clip_R1 : 1\nwindow_size : 4\nwindow_quality : 20\npoly_g : True\n"
                                         "min_length : 25\n"))
    assert cf.clip is True and cf.trim is False  # these options alone do not turn the 3' trimming on
    assert cf.clip_params() == dict(front_clip_r1=0, front_clip_r2=7, tail_clip_r1=1, tail_clip_r2=0, window_size=4, window_quality=20,
                                    poly_g_min_length=10, min_length=25)
    for one in ("front_clip_R1 : 1\n", "front_clip_R2 : 1\n", "tail_clip_R1 : 1\n", "tail_clip_R2 : 1\n", "window_size : 1\nwindow_quality : 1\n",
                "poly_g : True\n", "poly_g : yes\npoly_g_min_length : 6\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + one))
        assert cf.clip is True and cf.trim is False and cf.pair_trim is False, one
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\npoly_g_min_length : 30\n"))
    assert cf.clip is False and cf.clip_params()["poly_g_min_length"] == 0  # the length alone turns nothing on
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\nquality_cutoff : 20\npoly_g : True\n"))
    assert cf.clip is True and cf.trim is True
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npoly_g : True\n", gpu="[gpu]\n" + ok)).clip is True
    for word in ("front_clip_R1", "front_clip_R2", "tail_clip_R1", "tail_clip_R2", "window_size", "window_quality", "poly_g ", "poly_g_min_length",
                 "min_length", "device_pipeline", "Quade_clip_report.csv", "insert sizes"):
        assert word in qconf.CLIP_HELP, word


@pytest.mark.parametrize("trim", [
    "front_clip_R1 : 1000\n", "front_clip_R2 : 1000\n", "tail_clip_R1 : 1000\n", "tail_clip_R2 : 1000\n", "front_clip_R1 : 0\npoly_g : True\n",
    "window_size : 1\nwindow_quality : 1\n", "window_size : 100\nwindow_quality : 93\n", "poly_g : True\npoly_g_min_length : 6\n",
    "poly_g : True\npoly_g_min_length : 100\n", "poly_g : True\nmin_length : 65535\n"])
def test_conf_values_at_the_edges_are_accepted(tmp_path, trim):
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + trim))
    assert cf.clip is True and cf.trim is False


@pytest.mark.parametrize("trim,message", [
    ("front_clip_R1 : 1001\n", qconf.CLIP_FIXED), ("front_clip_R2 : -1\n", qconf.CLIP_FIXED), ("tail_clip_R1 : -1\n", qconf.CLIP_FIXED),
    ("tail_clip_R2 : 1001\n", qconf.CLIP_FIXED), ("front_clip_R2 : 1001\n", qconf.CLIP_FIXED), ("tail_clip_R1 : 1001\n", qconf.CLIP_FIXED),
    ("window_size : 0\nwindow_quality : 20\n", qconf.CLIP_WINDOW_SIZE), ("window_size : 101\nwindow_quality : 20\n", qconf.CLIP_WINDOW_SIZE),
    ("window_size : 4\nwindow_quality : 0\n", qconf.CLIP_WINDOW_QUALITY), ("window_size : 4\nwindow_quality : 94\n", qconf.CLIP_WINDOW_QUALITY),
    ("poly_g : True\npoly_g_min_length : 5\n", qconf.CLIP_POLY_G), ("poly_g : True\npoly_g_min_length : 101\n", qconf.CLIP_POLY_G),
    ("poly_g_min_length : 5\n", qconf.CLIP_POLY_G),
    ("poly_g : True\nmin_length : 65536\n", qconf.TRIM_LENGTH), ("poly_g : True\nmin_length : -1\n", qconf.TRIM_LENGTH)])
def test_conf_values_beyond_the_edges_are_rejected(tmp_path, trim, message):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + trim))
    assert str(ei.value) == message and message.startswith("Authorized values for ")


@pytest.mark.parametrize("trim", ["window_size : 4\n", "window_quality : 20\n", "window_size : 4\nwindow_quality :\n"])
def test_conf_window_options_go_together(tmp_path, trim):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + trim))
    assert str(ei.value) == qconf.CLIP_WINDOW_BOTH


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    for trim in ("[trim]\npoly_g : True\n", "[trim]\ntail_clip_R1 : 1\n", "[trim]\nwindow_size : 4\nwindow_quality : 20\n", "[trim]\nfront_clip_R2 : 3\n"):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, trim, gpu="[gpu]\n" + gpu))
        assert str(ei.value) == qconf.CLIP_NEEDS and "needs the device pipeline" in qconf.CLIP_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npoly_g_min_length : 20\n", gpu="[gpu]\n" + gpu)).clip is False  # off: as before
    assert qconf.QuadeConf(_conf(tmp_path, "", gpu="[gpu]\n" + gpu)).clip is False


@pytest.mark.parametrize("trim,gpu,message", [("poly_g : True\n", "[gpu]\ndevice_pipeline : False\n", qconf.CLIP_NEEDS),
                                              ("front_clip_R1 : 1001\n", "", qconf.CLIP_FIXED)])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, trim, gpu, message):
    conf = _conf(tmp_path, "[trim]\n" + trim, gpu=gpu)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / cr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_exported_symbols():
    new = {"qd_clip_set", "qd_clip_get", "qd_clip_read", "qd_clip_add", "qd_dev_clip"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_clip_active", "qd_clip_device"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text  # additive: the version stays
    assert "no reference counterpart" in text.split("int qd_clip_set")[0][-6000:]
    assert "no reference counterpart" in text.split("int qd_dev_clip")[0][-1000:]
    import ctypes
    assert ctypes.sizeof(hb.qd_clip_params) == 8 * 4 and "#define QD_CLIP_VALUES 24" in text


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, (2, 12), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, (2, 12), dtype=np.uint64)
    a[1, 2], b[1, 2] = (1 << 63) - 1, 1 << 62
    blob = hb.pack_table("clip", a)
    assert isinstance(blob, bytes) and len(blob) == 192
    a2 = hb.unpack_table("clip", blob)
    assert a2.dtype == np.uint64 and a2.shape == (2, 12) and (a2 == a).all()
    a2 += hb.unpack_table("clip", hb.pack_table("clip", b.reshape(-1)))  # (a flat table packs alike; unpacked tables are writable copies)
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2.reshape(-1), a.reshape(-1), b.reshape(-1)))
    with pytest.raises(AssertionError):
        hb.unpack_table("clip", blob[:-8])
