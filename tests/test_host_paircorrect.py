"""Overlap base correction off the GPU: the plain Python model against a second, independent form (R2 reverse-complemented as a
string and compared column by column), its properties (idempotent, only overlap positions change, I* stays accepted, the counter
identity), the threshold edges, the pair_correct options of the [trim] section and the configurations they reject, the report
writer against hand-written text, the exchange format of the ranks, the pinned stage tuples and the exported symbols."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import pair_correct_report as cr
from quade_amd import stages
from tests import paircorrect_model as CM
from tests import pairtrim_model as PM
from tests.stage_support import _one_sample_conf, _rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _columns(s1, q1, s2, q2, I, P):
    """The rule read once more: RC2 = the reverse complement of R2 as a string ('*' for a byte that is no letter) laid under R1 so
    that RC2's column x sits under R1's column x + I - L2; every column that holds both is a position.  Works on strings and maps
    back to R2's own order at the end."""
    a, qa = [chr(b) for b in s1], list(q1)
    rc = [COMP.get(chr(b).upper(), "*") for b in reversed(s2)]
    raw = [chr(b) for b in reversed(s2)]
    qr = list(reversed(q2))
    L1, L2 = len(a), len(rc)
    n1 = n2 = unresolved = columns = 0
    shift = I - L2  # column of R1 under which RC2[0] sits
    for x in range(L2):
        i = x + shift
        if not (0 <= i < L1) or not I:
            continue
        columns += 1
        letter = a[i].upper() if a[i].upper() in COMP else None
        if letter is not None and rc[x] == letter:
            continue
        if letter is not None and qa[i] - 33 >= P.good_quality and qr[x] - 33 <= P.bad_quality:
            rc[x], raw[x], qr[x] = letter, COMP[letter], qa[i]
            n2 += 1
        elif rc[x] != "*" and qr[x] - 33 >= P.good_quality and qa[i] - 33 <= P.bad_quality:
            a[i], qa[i] = rc[x], qr[x]
            n1 += 1
        else:
            unresolved += 1
    return (bytes(ord(c) for c in a), bytes(qa), bytes(ord(c) for c in reversed(raw)), bytes(reversed(qr)), (n1, n2, unresolved, columns))


QUALS = bytes([33 + 30, 33 + 29, 33 + 14, 33 + 15, 33 + 40, 33 + 2, 33, 32, 0, 10, 126, 127, 200, 255, 33 + 93])


def _random_pairs(seed, n, hi=60):
    """pairs off a fragment with substitutions, N, lower case and other bytes in either read, qualities from QUALS -> (s1, q1, s2, q2)"""
    rng = np.random.default_rng(seed)
    for k in range(n):
        L1, L2 = int(rng.integers(0, hi)), int(rng.integers(0, hi))
        frag = bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, int(rng.integers(1, 2 * hi))))
        pad = bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, 2 * hi))
        s1, s2 = bytearray((frag + pad)[:L1]), bytearray((_rc(frag) + pad[::-1])[:L2])
        for s in (s1, s2):
            for i in rng.permutation(len(s))[:int(rng.integers(0, 6))]:
                s[i] = b"NnacgtX.\x00 ACGT"[int(rng.integers(0, 14))]
        q1 = bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L1))
        q2 = bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L2))
        yield bytes(s1), q1, bytes(s2), q2, len(frag)


@pytest.mark.parametrize("kw", [dict(), dict(good_quality=15, bad_quality=14), dict(good_quality=93, bad_quality=0), dict(good_quality=1, bad_quality=0)])
def test_model_equals_the_column_form(kw):
    P, seen = CM.Params(**kw), [0, 0, 0]
    for s1, q1, s2, q2, frag in _random_pairs(31, 600):
        for I in {min(frag, len(s1) + len(s2)), 0, 1, len(s1) + len(s2), int(frag * 7 % (len(s1) + len(s2) + 1))}:  # 0 <= I <= L1 + L2
            got = CM.correct_pair(s1, q1, s2, q2, I, P)
            assert got == _columns(s1, q1, s2, q2, I, P), (s1, q1, s2, q2, I)
            assert got[4][3] == (PM.overlap(I, len(s1), len(s2)) if I else 0)
            for k in range(3):
                seen[k] += got[4][k]
    assert all(v > 50 for v in seen) or kw.get("good_quality") == 93


def test_properties_idempotent_local_and_still_accepted():
    P, Pp = CM.Params(), PM.Params(min_overlap=8, max_mismatches=5, max_mismatch_pct=20)
    with_insert = corrected = 0
    for s1, q1, s2, q2, _ in _random_pairs(32, 1600):
        I = PM.insert_size(s1, s2, Pp)
        once = CM.correct_pair(s1, q1, s2, q2, I, P)
        n1, n2, unresolved, positions = once[4]
        assert CM.correct_pair(once[0], once[1], once[2], once[3], I, P)[:4] == once[:4]  # twice == once
        assert CM.correct_pair(once[0], once[1], once[2], once[3], I, P)[4] == (0, 0, unresolved, positions)
        assert [len(x) for x in once[:4]] == [len(s1), len(s1), len(s2), len(s2)]  # lengths never change
        if I is None:
            assert once[:4] == (s1, q1, s2, q2) and once[4] == (0, 0, 0, 0)
            continue
        with_insert += 1
        corrected += n1 + n2
        lo, hi = max(0, I - len(s2)), min(len(s1), I)
        changed1 = [i for i in range(len(s1)) if (s1[i], q1[i]) != (once[0][i], once[1][i])]
        changed2 = [j for j in range(len(s2)) if (s2[j], q2[j]) != (once[2][j], once[3][j])]
        assert all(lo <= i < hi for i in changed1) and all(lo <= I - 1 - j < hi for j in changed2)  # only overlap positions change
        assert len(changed1) <= n1 and len(changed2) <= n2  # (a written quality may equal the one it replaces)
        # the identity, against the overlap stage's own count of the candidate
        assert n1 + n2 + unresolved == PM.mismatches(s1, s2, I) and PM.mismatches(once[0], once[2], I) == unresolved
        assert PM.accepted(once[0].translate(PM.FOLD1), once[2].translate(PM.COMP2), I, Pp)  # I* is still accepted
        assert all(chr(once[0][i]) in "ACGT" for i in changed1 if s1[i] != once[0][i])  # the written base is upper case
    assert with_insert > 200 and corrected > 100


def _one(b1, c1, b2, c2, P=CM.Params()):
    """one position: R1 = b1 with quality byte c1 opposite R2 = b2 with c2 -> (R1 byte, its quality, R2 byte, its quality, counts)"""
    s1, q1, s2, q2, c = CM.correct_pair(bytes([b1]), bytes([c1]), bytes([b2]), bytes([c2]), 1, P)
    return s1[0], q1[0], s2[0], q2[0], c[:3]


def test_threshold_edges_and_bytes():
    A, C, G, T, N = (ord(x) for x in "ACGTN")
    g, b = 33 + 30, 33 + 14
    assert _one(A, g, T, b) == (A, g, T, b, (0, 0, 0))  # a match: nothing, whatever the qualities
    assert _one(A, g, C, b) == (A, g, T, g, (0, 1, 0))  # phred exactly G and exactly B: R2 corrected
    assert _one(A, g - 1, C, b) == (A, g - 1, C, b, (0, 0, 1))  # G - 1
    assert _one(A, g, C, b + 1) == (A, g, C, b + 1, (0, 0, 1))  # B + 1
    assert _one(A, b, C, g) == (G, g, C, g, (1, 0, 0))  # the other way round: R1 corrected
    assert _one(A, b + 1, C, g) == (A, b + 1, C, g, (0, 0, 1)) and _one(A, b, C, g - 1) == (A, b, C, g - 1, (0, 0, 1))
    assert _one(A, g, C, g)[4] == (0, 0, 1) and _one(A, b, C, b)[4] == (0, 0, 1)  # both good, both bad
    for low in (32, 10, 0):  # a byte below 33 has a negative phred: bad
        assert _one(A, g, C, low) == (A, g, T, g, (0, 1, 0)) and _one(A, low, C, g) == (G, g, C, g, (1, 0, 0))
        assert _one(A, low, C, low)[4] == (0, 0, 1)
    for high in (126, 127, 200, 255):  # unsigned bytes: good
        assert _one(A, high, C, b) == (A, high, T, high, (0, 1, 0))
    for doubtful in (N, ord("n"), ord("c"), ord("."), 0, 0xE1):  # the doubtful byte may be anything
        assert _one(A, g, doubtful, b) == (A, g, T, g, (0, 1, 0)) and _one(doubtful, b, C, g) == (G, g, C, g, (1, 0, 0))
    assert _one(A, g, ord("t"), b) == (A, g, ord("t"), b, (0, 0, 0))  # lower case matches
    for trusted in (N, ord("n"), ord("."), 0, 0xC1):  # the trusted one must be a letter
        assert _one(trusted, g, C, b) == (trusted, g, C, b, (0, 0, 1)) and _one(A, b, trusted, g) == (A, b, trusted, g, (0, 0, 1))
    assert _one(ord("a"), g, C, b) == (ord("a"), g, T, g, (0, 1, 0))  # trusted lower case: written upper case
    assert _one(A, b, ord("c"), g) == (G, g, ord("c"), g, (1, 0, 0))
    assert _one(N, g, N, b)[4] == (0, 0, 1) and _one(N, b, N, g)[4] == (0, 0, 1)
    P = CM.Params(good_quality=1, bad_quality=0)
    assert _one(A, 34, C, 33, P) == (A, 34, T, 34, (0, 1, 0)) and _one(A, 34, C, 34, P)[4] == (0, 0, 1)


def test_count_and_positions_by_hand():
    frag = b"ACGTTGCAAGGCTTAACCGG"  # 20 bases
    s1, s2 = bytearray(frag + b"TTTT"), bytearray(_rc(frag) + b"GGGG")  # reads of 24 over an insert of 20
    q1, q2 = bytearray(b"I" * 24), bytearray(b"I" * 24)
    s1[0], q1[0] = ord("C"), ord("#")  # i = 0 <-> j = 19: R1 doubtful -> corrected to A
    s2[0], q2[0] = ord("N"), ord("!")  # j = 0 <-> i = 19: R2 doubtful -> comp(G) = C
    s1[5], s2[14] = ord("A"), ord("A")  # i = 5 <-> j = 14: both good -> unresolved
    s1[22], q1[22] = ord("N"), ord("#")  # outside the overlap: untouched
    t = CM.new_table()
    o1, p1, o2, p2 = CM.count(t, s1, q1, s2, q2, 20, CM.Params())
    assert o1 == b"A" + bytes(s1[1:]) and p1 == b"I" + bytes(q1[1:]) and o2 == b"C" + bytes(s2[1:]) and p2 == b"I" * 24 and p1[22] == ord("#")
    assert t == [1, 1, 1, 1, 1, 1, 20, 3, 1, 1]
    CM.count(t, s1, q1, s2, q2, None, CM.Params())
    CM.count(t, b"ACGT", b"IIII", b"ACGT", b"IIII", 8, CM.Params())  # I = L1 + L2: no positions
    CM.count(t, frag, b"I" * 20, _rc(frag), b"I" * 20, 30, CM.Params())  # I > M: positions 10 .. 19, and they do not agree
    assert t[:7] == [1, 1, 1, 1, 4, 3, 30] and t[7] == t[1] + t[3] + t[8] and t[9] == 1
    assert CM.VALUES == 10 == len(t) and CM.COUNTERS == hb.PAIRCORRECT_COUNTERS


PARAMS = dict(good_quality=30, bad_quality=14)


def test_report_lines_against_hand_written_text(tmp_path):
    t = [3, 5, 2, 4, 10, 8, 1000, 12, 3, 4]
    want = [
        "Program Quade-pair-correct 0.3.2",
        "",
        "pair_correct\tTrue",
        "pair_correct_good_quality\t30",
        "pair_correct_bad_quality\t14",
        "",
        "read\treads\tcorrected_reads\tcorrected_bases\toverlap_bases\tpercent_corrected_reads\tpercent_corrected_bases",
        "R1\t10\t3\t5\t1000\t30.00\t0.50",
        "R2\t10\t2\t4\t1000\t20.00\t0.40",
        "Total\t20\t5\t9\t2000\t25.00\t0.45",
        "",
        "pairs\t10",
        "overlapped_pairs\t8\t80.00",
        "overlap_bases\t1000",
        "mismatches\t12",
        "corrected\t9\t75.00",
        "unresolved\t3\t25.00",
        "corrected_pairs\t4\t50.00",
        "mismatches_per_100000_overlap_bases_before\t1200.00",
        "mismatches_per_100000_overlap_bases_after\t300.00",
    ]
    assert cr.report_lines(t, PARAMS) == want
    assert cr.report_lines(np.array(t, dtype=np.uint64), PARAMS) == want
    assert cr.REPORT_NAME == "Quade_pair_correct_report.csv" and "Date" not in "\n".join(want)
    assert cr.report_lines([0] * 10, PARAMS)[-2:] == ["mismatches_per_100000_overlap_bases_before\t0.00", "mismatches_per_100000_overlap_bases_after\t0.00"]
    with pytest.raises(AssertionError):
        cr.report_lines([0] * 16, PARAMS)
    p = tmp_path / cr.REPORT_NAME
    cr.write_report(str(p), t, PARAMS)
    assert p.read_text() == "\n".join(want) + "\n"
    big = np.array([1, (1 << 63) + 1, 1, (1 << 63) + 1, 1 << 62, 1 << 62, (1 << 63) + 9, (1 << 63) + 5, 3, 1], dtype=np.uint64)
    lines = cr.report_lines(big, PARAMS)
    assert lines[9].split("\t")[3] == str((1 << 64) + 2) and lines[15].startswith("corrected\t%d\t" % ((1 << 64) + 2))  # exact beyond 64 bits
    assert cr.COUNTERS == hb.PAIRCORRECT_COUNTERS == CM.COUNTERS and cr.VALUES == hb.PAIRCORRECT_VALUES == CM.VALUES == 10


def _conf(tmp_path, trim="", gpu=""):
    return _one_sample_conf(tmp_path, trim, gpu)


ON = "[trim]\npair_overlap : True\npair_correct : True\n"


def test_conf_defaults_and_when_the_stage_is_on(tmp_path):
    for trim in ("", "[trim]\n", "[trim]\npair_correct :\npair_correct_good_quality :\npair_correct_bad_quality :\n",
                 "[trim]\npair_correct : False\npair_correct_good_quality : 20\n", "[trim]\npair_overlap : True\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, trim))
        assert cf.pair_correction is False and cf.pair_correct_bad_quality == 14 and not hb.PAIRCORRECT.on(cf)
    cf = qconf.QuadeConf(_conf(tmp_path, ""))
    assert cf.pair_correct_params() == dict(good_quality=30, bad_quality=14)
    cf = qconf.QuadeConf(_conf(tmp_path, ON + "pair_correct_good_quality : 25\npair_correct_bad_quality : 10\n"))
    assert cf.pair_correction is True and cf.pair_trim is True and hb.PAIRCORRECT.on(cf)
    assert cf.pair_correct_params() == hb.PAIRCORRECT.conf_params(cf) == dict(good_quality=25, bad_quality=10)
    for word in ("true", "1", "yes", "on", "TRUE"):
        assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_overlap : True\npair_correct : %s\n" % word)).pair_correction is True
    for edge in ("pair_correct_good_quality : 93\n", "pair_correct_good_quality : 1\npair_correct_bad_quality : 0\n",
                 "pair_correct_bad_quality : 29\n", "pair_correct_bad_quality : 0\n"):
        assert qconf.QuadeConf(_conf(tmp_path, ON + edge)).pair_correction is True
    for ok in ("gzip_level : 1\n", "gzip_level : -1\n"):
        assert qconf.QuadeConf(_conf(tmp_path, ON, gpu="[gpu]\n" + ok)).pair_correction is True
    for word in ("pair_correct", "pair_correct_good_quality", "pair_correct_bad_quality", "pair_overlap", "device pipeline", "unresolved"):
        assert word in qconf.CORRECT_HELP
    assert "pair_correct" not in qconf.PAIR_HELP  # left as it is


@pytest.mark.parametrize("trim,message", [
    ("pair_correct_good_quality : 0\n", qconf.CORRECT_GOOD), ("pair_correct_good_quality : 94\n", qconf.CORRECT_GOOD),
    ("pair_correct_good_quality : -3\n", qconf.CORRECT_GOOD), ("pair_correct_bad_quality : -1\n", qconf.CORRECT_BAD),
    ("pair_correct_bad_quality : 30\n", qconf.CORRECT_BAD), ("pair_correct_good_quality : 10\n", qconf.CORRECT_BAD),
    ("pair_correct_good_quality : 20\npair_correct_bad_quality : 20\n", qconf.CORRECT_BAD)])
def test_conf_values_out_of_range_are_rejected(tmp_path, trim, message):
    for on in (ON, "[trim]\n"):  # checked like every other value, whether the stage is on or not
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, on + trim))
        assert str(ei.value) == message
    assert message in ("Authorized values for pair_correct_good_quality : 1 to 93",
                       "Authorized values for pair_correct_bad_quality : 0 to pair_correct_good_quality - 1")


def test_conf_rejected_without_pair_overlap(tmp_path):
    for trim in ("[trim]\npair_correct : True\n", "[trim]\npair_correct : True\npair_overlap : False\n", "[trim]\npair_correct : True\nquality_cutoff : 20\n"):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, trim))
        assert str(ei.value) == qconf.CORRECT_NEEDS_OVERLAP == "pair_correct needs pair_overlap : True"


@pytest.mark.parametrize("gpu", ["device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n", "gzip_level : 6\n", "gzip_level : 0\n"])
def test_conf_rejected_without_the_device_pipeline(tmp_path, gpu):
    with pytest.raises(AssertionError) as ei:  # pair_overlap asks for the pipeline too, and its message comes first, as before
        qconf.QuadeConf(_conf(tmp_path, ON, gpu="[gpu]\n" + gpu))
    assert str(ei.value) == qconf.PAIR_NEEDS
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_correct : True\n", gpu="[gpu]\n" + gpu))
    assert str(ei.value) == qconf.CORRECT_NEEDS == qconf.PAIR_NEEDS.replace("pair_overlap", "pair_correct")  # the same message form
    assert qconf.QuadeConf(_conf(tmp_path, "[trim]\npair_correct_good_quality : 20\n", gpu="[gpu]\n" + gpu)).pair_correction is False


@pytest.mark.parametrize("trim,gpu,message", [
    ("pair_correct : True\n", "", "pair_correct needs pair_overlap : True"),
    ("pair_correct : True\n", "[gpu]\ndevice_pipeline : False\n", "pair_correct needs the device pipeline"),
    ("pair_overlap : True\npair_correct : True\npair_correct_bad_quality : 30\n", "", "Authorized values for pair_correct_bad_quality")])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, trim, gpu, message):
    conf = _conf(tmp_path, "[trim]\n" + trim, gpu=gpu)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / cr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 1 << 62, 10, dtype=np.uint64)
    b = rng.integers(0, 1 << 62, 10, dtype=np.uint64)
    a[9], b[9] = (1 << 63) + 5, 7
    for stage in (hb.PAIRCORRECT, stages.PAIRCORRECT):  # a Stage outside the name table: passed as itself
        blob = hb.pack_table(stage, a)
        assert isinstance(blob, bytes) and len(blob) == 80  # no count in front
        a2 = hb.unpack_table(stage, blob)
        assert a2.dtype == np.uint64 and a2.shape == (10,) and (a2 == a).all()
        a2 += hb.unpack_table(stage, hb.pack_table(stage, b.reshape(2, 5)))
        assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2, a, b)) and int(a2[9]) == (1 << 63) + 12
        with pytest.raises(AssertionError):
            hb.unpack_table(stage, blob[:-8])
    with pytest.raises(KeyError):
        hb.pack_table("paircorrect", a)  # not a name of READ_STAGE: the pinned table stays as it is


def test_the_pinned_tuples_are_unchanged_and_the_stage_stands_outside():
    names = ("quality", "cycle", "clip", "trim", "pairtrim", "filter")
    assert tuple(s.name for s in hb.STAGES) == names
    assert tuple(s.name for s in hb.RUN_STAGES) == ("quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter")
    assert tuple(s.name for s in hb.PIPE_STAGES) == ("quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter", "screen")
    assert tuple(s.name for s in hb.READ_STAGES) == ("adapters",) + tuple(s.name for s in hb.PIPE_STAGES)
    S = hb.PAIRCORRECT
    assert S not in hb.READ_STAGES and S.name not in hb.READ_STAGE and S.name == S.engine == "paircorrect"
    assert S.shape == (10,) and S.count is None and S.flat is None and S.view is None and S.report_args == ("params",)
    assert S.report_module() is cr
    with open(os.path.join(ROOT, "quade_amd", "quade.py")) as fh:
        text = fh.read()
    assert text.count("hb.READ_STAGES") == 2 and text.count("hb.PAIRCORRECT.on(cf)") == 2  # enabled and collected beside the two walks


def test_exported_symbols_and_the_rule_in_the_same_words():
    new = {"qd_paircorrect_set", "qd_paircorrect_get", "qd_paircorrect_read", "qd_paircorrect_add", "qd_dev_paircorrect"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_paircorrect_active", "qd_paircorrect_device", "qd_pairtrim_device_inserts"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_PAIRCORRECT_VALUES 10" in text
    assert "no reference counterpart" in text.split("int qd_paircorrect_set")[0][-6000:]
    assert "no reference counterpart" in text.split("int qd_dev_paircorrect")[0][-1200:]
    assert ctypes.sizeof(hb.qd_paircorrect_params) == 8 and ctypes.sizeof(hb.qd_pairtrim_params) == 16
    # the rule stands in the same words in the public header, the kernel's header and the model
    with open(os.path.join(ROOT, "quade_amd", "csrc", "quade_paircorrect.h")) as fh:
        kernel = fh.read()
    words = lambda s: " ".join(re.sub(r"^\s*(//|\*)", "", ln) for ln in s.splitlines()).split()  # noqa: E731
    cut = lambda s: " ".join(words(s)).split("It uses the record tables", 1)[1].split("because a corrected position matches afterwards")[0]  # noqa: E731
    assert cut(text) == cut(kernel) == cut(CM.__doc__) and len(cut(text)) > 1200
