"""Post-trimming (trailing N, poly-X, max_length) without a GPU: the model's rule (tests/posttrim_model.py) on worked examples, the
property the kernel's shortcut rests on (at most one base cuts, and it is the one that is frequent among the last P bytes),
exhaustively, the [trim] section's new options, the report's arithmetic, the table's bytes in the ranks' exchange and the
exported symbols."""
import ctypes
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import posttrim_report as xr
from tests import clip_model as CM
from tests import posttrim_model as XM
from tests.stage_support import _one_sample_conf as _conf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = dict(tail_n=1, poly_x_min_length=10, max_length_r1=100, max_length_r2=0, min_length=20)
INSERT = b"ACGTACGTAC"


def _lout(seq, read=0, **kw):
    return XM.posttrim_read(seq, read, XM.Params(**kw))[4]


def test_worked_examples():
    P = dict(poly_x_min_length=10)
    # one pass only: the T run goes, the A run in front of it stays
    assert XM.posttrim_read(INSERT + b"A" * 10 + b"T" * 10, 0, XM.Params(**P))[:3] == (30, 20, b"T")
    # N count as mismatches: four of them in the first ten bases end every walk before t = P
    seq = INSERT + b"A" * 12 + b"NNNN"
    assert _lout(seq, **P) == 26
    # ... with tail_n the A walk starts behind them.  It forgives the insert's last C (one mismatch in 13 bases), takes the A in
    # front of it and stops at the T (two in 15): by the rule 8 bases stay, the leftmost A reached being the cut
    assert XM.posttrim_read(seq, 0, XM.Params(tail_n=1, **P))[:3] == (22, 8, b"A")
    # an insert whose end cannot be taken for part of the tail keeps its 10 bases
    assert XM.posttrim_read(b"ACGTACGTCC" + b"A" * 12 + b"NNNN", 0, XM.Params(tail_n=1, **P))[:3] == (22, 10, b"A")
    assert XM.posttrim_read(b"ACGTACGTCC" + b"A" * 12 + b"NNNN", 0, XM.Params(tail_n=1))[:3] == (22, 22, b"")
    # a tail one base short of P: a read of P - 1 bases is never cut, and at P = 6 neither are 5 A behind another base (8 x 1 > 6);
    # at P = 10 the base in front of 9 A is the one mismatch the rule forgives, as the clip stage's poly-G rule does
    assert _lout(b"A" * 9, **P) == 9 and _lout(b"A" * 10, **P) == 0
    assert _lout(b"CGCGCG" + b"A" * 5, poly_x_min_length=6) == 11 and _lout(b"CGCGCG" + b"A" * 6, poly_x_min_length=6) == 6
    assert _lout(b"CGCGCG" + b"A" * 9, **P) == 6 == CM.poly_g(b"CACACA" + b"G" * 9, 10)
    assert _lout(b"CGCGCG" + b"A" * 8, **P) == 14
    # an all-A read is cut to nothing, and the floor gives bases back -- never more than the read had
    assert _lout(b"A" * 40, **P) == 0 and _lout(b"A" * 40, min_length=25, **P) == 25 and _lout(b"A" * 12, min_length=25, **P) == 12
    # crop, per read; the floor wins over it
    seq = b"ACGT" * 10
    assert [_lout(seq, r, max_length=(16, 0)) for r in (0, 1)] == [16, 40]
    assert [_lout(seq, r, max_length=(40, 41)) for r in (0, 1)] == [40, 40]
    assert _lout(seq, 0, max_length=(16, 0), min_length=30) == 30
    assert _lout(seq[:30] + b"T" * 10, 1, max_length=(0, 35), poly_x_min_length=10) == 30  # the crop of what the poly-X rule left
    # lower case matches, for N and for the bases
    seq = INSERT + b"t" * 12 + b"nNn"
    assert XM.posttrim_read(seq, 0, XM.Params(tail_n=1, **P))[:3] == (22, 10, b"T")
    assert XM.posttrim_read(seq.upper(), 0, XM.Params(tail_n=1, **P))[:3] == (22, 10, b"T")
    assert XM.tail_n(b"NNNN") == 0 and XM.tail_n(b"") == 0 and XM.tail_n(b"ACNGN.") == 6 and XM.tail_n(b"NA") == 2
    # every step off: the stage would be off
    assert XM.posttrim_read(seq, 0, XM.Params(min_length=5)) == (25, 25, b"", 25, 25) and not XM.Params(min_length=5).on


def test_the_walk_is_the_clip_stage_poly_g_rule_with_another_base():
    rng = np.random.default_rng(11)
    swap = bytes.maketrans(b"GAgaCTct", b"AGagTCtc")
    for k in range(1500):
        L = int(rng.integers(0, 60))
        alphabet = (b"G" * 12 + b"ACTNg", b"GGGA", b"ACGT")[k % 3]
        seq = bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))
        P = int(rng.integers(6, 16))
        assert XM.walk(seq, P, ord("G")) == CM.poly_g(seq, P)
        assert XM.walk(seq.translate(swap), P, ord("A")) == CM.poly_g(seq, P)


def test_counters_and_text():
    P = XM.Params(tail_n=1, poly_x_min_length=10, max_length=(12, 0), min_length=3)
    table = XM.new_table()
    assert XM.count(table, b"CGCGCGCGCGCGCGCG" + b"A" * 12 + b"NN", 0, P) == 12
    assert table[0] == [1, 30, 12, 1, 2, 1, 12, 0, 0, 0, 0, 0, 0, 1, 4, 0]
    assert XM.count(table, b"t" * 11, 1, P) == 3 and table[1] == [1, 11, 3, 0, 0, 0, 0, 0, 0, 0, 0, 1, 11, 0, 0, 1]
    for X, k in ((b"C", 7), (b"G", 9)):
        t = XM.new_table()
        XM.count(t, b"ATATATAT" + X * 10, 1, P)
        assert t[1][k:k + 2] == [1, 10] and sum(t[1][5:13]) == 11
    text = XM.posttrimmed_text([(b"@r", b"CGCGCGCG" + b"A" * 12, b"I" * 20)], 1, P)
    assert text == b"@r\nCGCGCGCG\n+\nIIIIIIII\n"
    assert XM.COUNTERS == hb.POSTTRIM_COUNTERS == xr.COUNTERS and len(XM.COUNTERS) == 16


@pytest.mark.parametrize("P", [6, 8, 10])
def test_at_most_one_base_cuts_and_the_last_p_bytes_name_it(P):
    """every string over {A, C, G, N} of up to 9 bytes: what quade_posttrim.hip's shortcut rests on, shown by the four plain walks"""
    lim = min(5, P // 8)
    cuts = 0
    for L in range(10):
        for tup in itertools.product(b"ACGN", repeat=L):
            seq = bytes(tup)
            Lx = [XM.walk(seq, P, X) for X in XM.LETTERS]
            cut = [X for X, v in zip(XM.LETTERS, Lx) if v < L]
            assert len(cut) <= 1, seq
            if cut:
                rare = [X for X in XM.LETTERS if sum(b != X for b in seq[L - P:]) <= lim]
                assert L >= P and rare == cut, seq
                cuts += 1
    # a string is cut exactly when one of A, C, G is that frequent among its last P bytes: at P = 6 they are all X (3 bases, and
    # 4 ** (L - 6) strings in front), at P = 8 one of the 8 may be one of 3 other bytes (25 tails); no string of 9 bytes has 10
    assert cuts == {6: 3 * (1 + 4 + 16 + 64), 8: 3 * 25 * (1 + 4), 10: 0}[P]


def test_the_property_on_random_reads_with_planted_tails():
    rng = np.random.default_rng(13)
    cuts = 0
    for k in range(3000):
        P = int(rng.integers(6, 101))
        body = bytes(b"ACGTN"[int(v)] for v in rng.integers(0, 5, int(rng.integers(0, 40))))
        X = b"ACGT"[k % 4]
        tail = bytearray([X]) * int(rng.integers(0, 2 * P))
        for _ in range(int(rng.integers(0, 7))):
            if tail:
                tail[int(rng.integers(0, len(tail)))] = b"ACGTN"[int(rng.integers(0, 5))]
        seq = body + bytes(tail) if k % 5 else (body + bytes(tail)).lower()
        Lp, bases = XM.poly_x(seq, P)
        assert len(bases) <= 1
        if bases:
            rare = [Y for Y in XM.LETTERS if sum(b & 0xDF != Y for b in seq[len(seq) - P:]) <= min(5, P // 8)]
            assert bytes(rare) == bases == bytes([X]) and Lp == XM.walk(seq, P, X)
            cuts += 1
    assert cuts > 500


# ---- the configuration file ----------------------------------------------------------------------------------------------------------
OFF = dict(tail_n=0, poly_x_min_length=0, max_length_r1=0, max_length_r2=0, min_length=0)
CLIP_OFF = dict(front_clip_r1=0, front_clip_r2=0, tail_clip_r1=0, tail_clip_r2=0, window_size=0, window_quality=0, poly_g_min_length=0, min_length=0)
TRIM_OFF = dict(adapter_r1="", adapter_r2="", quality_cutoff=0, min_overlap=3, max_mismatch_pct=10, min_length=0)
PAIR_OFF = dict(min_overlap=30, max_mismatches=5, max_mismatch_pct=20, min_length=0)
FILTER_OFF = dict(min_length=None, max_n=None, max_unqualified_pct=None, qualified_quality=15, min_mean_quality=None, min_complexity_pct=None)


def test_conf_every_option_is_parsed(tmp_path):
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\ntail_n : True\npoly_x : True\npoly_x_min_length : 12\nmax_length_R1 : 100\nmax_length_R2 : 75\n"
                                         "min_length : 25\n"))
    assert (cf.tail_n, cf.poly_x, cf.poly_x_min_length, cf.max_length) == (True, True, 12, (100, 75))
    assert cf.posttrim is True and cf.posttrim_params() == dict(tail_n=1, poly_x_min_length=12, max_length_r1=100, max_length_r2=75, min_length=25)
    assert set(cf.posttrim_params()) == set(xr.PARAMS) == set(XM.Params().keywords())
    assert qconf.QuadeConf(_conf(tmp_path, "")).poly_x_min_length == 10
    for word in ("tail_n ", "poly_x ", "poly_x_min_length", "max_length_R1", "max_length_R2", "min_length", "device_pipeline",
                 "Quade_post_trim_report.csv", "u(b) = b & 0xDF", "Lout = max(Lm, min(min_length, L))", "One pass only"):
        assert word in qconf.POSTTRIM_HELP, word


def test_conf_when_the_stage_is_on(tmp_path):
    for trim in ("", "[trim]\n", "[trim]\ntail_n :\npoly_x :\npoly_x_min_length :\nmax_length_R1 :\nmax_length_R2 :\n",
                 "[trim]\ntail_n : False\npoly_x : False\npoly_x_min_length : 20\nmax_length_R1 : 0\nmax_length_R2 : 0\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, trim))
        assert cf.posttrim is False and cf.posttrim_params() == OFF, trim
        assert (cf.tail_n, cf.poly_x, cf.max_length) == (False, False, (0, 0))
        # ... and the other stages' parameters are what they were without these options
        assert (cf.clip, cf.trim, cf.pair_trim, cf.filter) == (False, False, False, False)
        assert cf.clip_params() == CLIP_OFF and cf.trim_params() == TRIM_OFF and cf.pair_trim_params() == PAIR_OFF
        assert cf.filter_params() == FILTER_OFF
    for tn, px, m1, m2 in itertools.product((False, True), (False, True), (0, 50), (0, 60)):
        text = "[trim]\ntail_n : %s\npoly_x : %s\nmax_length_R1 : %d\nmax_length_R2 : %d\n" % (tn, px, m1, m2)
        cf = qconf.QuadeConf(_conf(tmp_path, text))
        assert cf.posttrim is bool(tn or px or m1 or m2), text
        assert (cf.clip, cf.trim, cf.pair_trim, cf.filter) == (False, False, False, False)  # the stage turns nothing else on
        assert cf.posttrim_params() == dict(tail_n=int(tn), poly_x_min_length=10 if px else 0, max_length_r1=m1, max_length_r2=m2, min_length=0)
        assert cf.clip_params() == CLIP_OFF and cf.trim_params() == TRIM_OFF
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\npoly_x_min_length : 30\n"))
    assert cf.posttrim is False and cf.posttrim_params()["poly_x_min_length"] == 0  # the length alone turns nothing on
    cf = qconf.QuadeConf(_conf(tmp_path, "[trim]\npoly_g : True\nadapter_R1 : ACGTACGT\npair_overlap : True\ntail_n : yes\n"))
    assert (cf.clip, cf.trim, cf.pair_trim, cf.posttrim) == (True, True, True, True)
    assert [s.name for s in hb.RUN_STAGES if s.on(cf)] == ["clip", "trim", "pairtrim", "posttrim"]
    for ok in ("tail_n : True\nmin_length : 65535\n", "poly_x : True\npoly_x_min_length : 6\n", "poly_x : True\npoly_x_min_length : 100\n",
               "max_length_R1 : 1\n", "max_length_R2 : 65535\nmin_length : 65535\n", "max_length_R1 : 30\nmax_length_R2 : 0\nmin_length : 30\n"):
        assert qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + ok)).posttrim is True, ok


REJECTED = [
    ("poly_x : True\npoly_x_min_length : 5\n", qconf.POSTTRIM_POLY_X), ("poly_x : True\npoly_x_min_length : 101\n", qconf.POSTTRIM_POLY_X),
    ("poly_x_min_length : 5\n", qconf.POSTTRIM_POLY_X),
    ("max_length_R1 : -1\n", qconf.POSTTRIM_MAX_LENGTH), ("max_length_R2 : 65536\n", qconf.POSTTRIM_MAX_LENGTH),
    ("max_length_R1 : 65536\n", qconf.POSTTRIM_MAX_LENGTH), ("max_length_R2 : -1\n", qconf.POSTTRIM_MAX_LENGTH),
    ("max_length_R1 : 30\nmin_length : 31\n", qconf.POSTTRIM_FLOOR), ("max_length_R1 : 100\nmax_length_R2 : 30\nmin_length : 31\n", qconf.POSTTRIM_FLOOR)]


@pytest.mark.parametrize("trim,message", REJECTED)
def test_conf_values_beyond_the_edges_are_rejected(tmp_path, trim, message):
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[trim]\n" + trim))
    assert str(ei.value) == message
    assert len({qconf.POSTTRIM_POLY_X, qconf.POSTTRIM_MAX_LENGTH, qconf.POSTTRIM_FLOOR, qconf.POSTTRIM_NEEDS}) == 4


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n",
                                 "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    for trim in ("[trim]\ntail_n : True\n", "[trim]\npoly_x : True\n", "[trim]\nmax_length_R1 : 100\n", "[trim]\nmax_length_R2 : 100\n"):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, trim, gpu="[gpu]\n" + gpu))
        assert str(ei.value) == qconf.POSTTRIM_NEEDS and "needs the device pipeline" in qconf.POSTTRIM_NEEDS
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npoly_x_min_length : 20\n", gpu="[gpu]\n" + gpu)).posttrim is False  # off: as before
    assert qconf.POSTTRIM_NEEDS.split(" needs ")[1] == qconf.CLIP_NEEDS.split(" needs ")[1]


@pytest.mark.parametrize("trim,gpu,message", [("tail_n : True\n", "[gpu]\ndevice_pipeline : False\n", qconf.POSTTRIM_NEEDS),
                                              ("max_length_R1 : 30\nmin_length : 31\n", "", qconf.POSTTRIM_FLOOR)])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, trim, gpu, message):
    conf = _conf(tmp_path, "[trim]\n" + trim, gpu=gpu)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / xr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


# ---- the report ------------------------------------------------------------------------------------------------------------------------
def test_report_lines_against_hand_written_text(tmp_path):
    t = [[4, 400, 300, 2, 8, 1, 30, 0, 0, 1, 12, 0, 0, 2, 50, 0], [3, 90, 90, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]]
    want = [
        "Program Quade-post-trim 0.3.2",
        "",
        "tail_n\t1",
        "poly_x_min_length\t10",
        "max_length_r1\t100",
        "max_length_r2\t0",
        "min_length\t20",
        "",
        "read\treads\tbases_in\tbases_out\tn_tail_reads\tn_tail_bases\tpolya_reads\tpolya_bases\tpolyc_reads\tpolyc_bases\tpolyg_reads\t"
        "polyg_bases\tpolyt_reads\tpolyt_bases\tcropped_reads\tcropped_bases\tfloored_reads\tpercent_n_tail_reads\tpercent_polyx_reads\t"
        "percent_cropped_reads\tpercent_bases_trimmed",
        "R1\t4\t400\t300\t2\t8\t1\t30\t0\t0\t1\t12\t0\t0\t2\t50\t0\t50.00\t50.00\t50.00\t25.00",
        "R2\t3\t90\t90\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t1\t0.00\t0.00\t0.00\t0.00",
        "Total\t7\t490\t390\t2\t8\t1\t30\t0\t0\t1\t12\t0\t0\t2\t50\t1\t28.57\t28.57\t28.57\t20.40",
    ]
    assert xr.report_lines(t, PARAMS) == want
    assert xr.report_lines(np.array(t, dtype=np.uint64), PARAMS) == want
    assert xr.REPORT_NAME == "Quade_post_trim_report.csv" and "Date" not in "\n".join(want)
    assert xr.report_lines([[0] * 16, [0] * 16], PARAMS)[-1] == "Total" + "\t0" * 16 + "\t0.00" * 4
    with pytest.raises(AssertionError):
        xr.report_lines([[0] * 12, [0] * 12], PARAMS)
    p, p2 = tmp_path / xr.REPORT_NAME, tmp_path / "again.csv"
    xr.write_report(str(p), t, PARAMS)
    hb.RUN_STAGE["posttrim"].write_report(str(tmp_path), np.array(t, dtype=np.uint64), params=dict(PARAMS))
    xr.write_report(str(p2), np.array(t, dtype=np.uint64), dict(PARAMS))
    assert p.read_bytes() == p2.read_bytes() == ("\n".join(want) + "\n").encode()  # byte-identical, whoever writes it


def test_report_lines_beyond_53_bits():
    t = np.zeros((2, 16), dtype=np.uint64)
    t[0, :3] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 62) + 5]
    t[1, :3] = [(1 << 62) + 1, (1 << 63) + 3, (1 << 63) + 3]
    lines = xr.report_lines(t, PARAMS)
    assert lines[-3].split("\t")[-1] == "49.99"  # exact integers: a float would round to 50.00
    total = lines[-1].split("\t")
    assert total[1] == str((1 << 63) + 2) and total[2] == str((1 << 64) + 6)  # the sum of two rows passes 64 bits and stays exact


# ---- the stage table, the exchange and the library --------------------------------------------------------------------------------
def test_the_run_walks_seven_stages_and_the_pinned_table_keeps_six():
    assert [s.name for s in hb.RUN_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter"]
    assert [s.name for s in hb.STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "filter"] and "posttrim" not in hb.STAGE
    assert all(hb.RUN_STAGE[s.name] is s for s in hb.RUN_STAGES) and all(hb.RUN_STAGE[s.name] is s for s in hb.STAGES)
    st = hb.RUN_STAGE["posttrim"]
    assert st is hb.POSTTRIM and (st.engine, st.conf, st.params, st.shape, st.count, st.report) == \
        ("posttrim", "posttrim", "posttrim_params", (2, 16), None, "posttrim_report")
    assert st.report_module() is xr
    for name in ("posttrim_set", "posttrim_get", "posttrim_read", "posttrim_add", "posttrim_active", "dev_posttrim"):
        assert callable(getattr(hb.Engine, name)), name


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, (2, 16), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, (2, 16), dtype=np.uint64)
    a[1, 2], b[1, 2] = (1 << 63) - 1, 1 << 62
    blob = hb.pack_table("posttrim", a)
    assert isinstance(blob, bytes) and len(blob) == 256 and blob == a.astype("<u8").tobytes()  # no head word
    assert blob == hb.pack_table(hb.POSTTRIM, a.reshape(-1))  # by object or by name, flat or shaped
    a2 = hb.unpack_table("posttrim", blob)
    assert a2.dtype == np.uint64 and a2.shape == (2, 16) and (a2 == a).all() and a2.flags.writeable
    a2 += hb.unpack_table(hb.POSTTRIM, hb.pack_table("posttrim", b))
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2.reshape(-1), a.reshape(-1), b.reshape(-1)))
    for bad in (blob[:-8], blob + bytes(8), blob[:192]):
        with pytest.raises(AssertionError, match="of the wrong size"):
            hb.unpack_table("posttrim", bad)
    assert len(hb.pack_table("clip", np.zeros((2, 12), np.uint64))) == 192  # the pinned stages resolve as before


def test_exported_symbols():
    new = {"qd_posttrim_set", "qd_posttrim_get", "qd_posttrim_read", "qd_posttrim_add", "qd_dev_posttrim"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_posttrim_active", "qd_posttrim_device"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text  # additive: the version stays
    assert "no reference counterpart" in text.split("int qd_posttrim_set")[0][-6000:]
    assert "no reference counterpart" in text.split("int qd_dev_posttrim")[0][-1000:]
    assert ctypes.sizeof(hb.qd_posttrim_params) == 20 and "#define QD_POSTTRIM_VALUES 32" in text
    # the rule stands in the header, the model and the help in the same words
    norm = lambda s: re.sub(r"(\n \*|\s)+", " ", s)  # noqa: E731  (line breaks and the comment's margin apart)
    for words in ("u(b) = b & 0xDF", "what clip, trim and pairtrim left", "One pass only: a T run behind an A run loses the T run",
                  "Lout = max(Lm, min(min_length, L))", "with u(b) == 'N'", "N and every other byte count as a mismatch",
                  "Each of steps 1 to 3 is skipped when not configured; its output length is then its input length"):
        assert words in norm(text) and words in norm(XM.__doc__) and words in norm(qconf.POSTTRIM_HELP), words
