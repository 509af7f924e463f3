"""The k-mer screen without a GPU: the model's rule (tests/screen_model.py) against a second, independent form (string reverse
complement and substring search), the canonical-word arithmetic at the edges of k, the numpy builder of the reference set
(quade_amd/screen.py) against the model on awkward FASTA, the [screen] section and every message that rejects one, the report's
arithmetic, the table's bytes in the ranks' exchange, the stage tuples and the exported symbols."""
import ctypes
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from quade_amd import conf as qconf
from quade_amd import hip_backend as hb
from quade_amd import screen as qscreen
from quade_amd import screen_report as sr
from tests import screen_model as SM
from tests.stage_support import _one_sample_conf as _conf
from tests.stage_support import _rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"A": 0, "C": 1, "T": 2, "G": 3}
REFERENCE = dict(name="phix.fa", records=1, bases=5386, kmers=5356)
PARAMS = dict(kmer=31, min_hits=1, action="report", reference=REFERENCE)


def _rs(rng, L, alphabet=b"ACGT"):
    return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))


def _word(s):
    """a string of bases as a base-4 number, the first base the most significant"""
    w = 0
    for ch in s.upper():
        w = w * 4 + CODE[ch]
    return w


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def test_the_model_against_reverse_complement_and_substring_search():
    """a second form of the rule: the k-mer at p hits when its text, or the text of its reverse complement, occurs in a record of
    the reference (upper case both), and exists when it is made of bases alone"""
    rng = np.random.default_rng(1)
    for k in (15, 16, 21):
        recs = [_rs(rng, 90), _rs(rng, 40, b"ACGTacgtN"), _rs(rng, k - 1), b"G" * 20]
        fasta = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(recs))
        R = SM.kmers_of(fasta, k)
        upper = [r.upper() for r in recs]
        for _ in range(60):
            a = int(rng.integers(0, 60))
            read = [recs[0][a:a + 30], _rc(recs[0])[a:a + 30], recs[1][:30] + _rs(rng, 8), _rs(rng, 40, b"ACGTn"), b"c" * 25, _rs(rng, k - 1)][int(rng.integers(0, 6))]
            n_hits = n_kmers = 0
            for p in range(len(read) - k + 1):
                w = read[p:p + k].upper()
                if w.strip(b"ACGT"):
                    continue
                n_kmers += 1
                n_hits += any(w in r or _rc(w) in r for r in upper)
            assert SM.scan(read, k, R) == (n_hits, n_kmers) and SM.hits(read, k, R) == n_hits
            assert [SM.canonical(read, p, k) for p in range(len(read) - k + 1)].count(None) == max(0, len(read) - k + 1) - n_kmers
    assert SM.scan(b"ACGT" * 3, 15, {0}) == (0, 0)  # shorter than k: no hits and no k-mers


@pytest.mark.parametrize("k", [15, 16, 31, 32])
def test_canonical_word_arithmetic(k):
    rng = np.random.default_rng(k)
    for _ in range(50):
        s = _rs(rng, k).decode()
        w, rc = _word(s), _word(_rc(s.encode()).decode())
        assert SM.canonical(s.encode(), 0, k) == min(w, rc) == SM.canonical(_rc(s.encode()), 0, k) == SM.canonical(s.lower().encode(), 0, k)
        assert SM.canonical(b"N" + s.encode(), 1, k) == min(w, rc) and SM.canonical(b"N" + s.encode(), 0, k) is None
        words, exists = qscreen.canonical_words(s.encode(), k)
        assert exists.tolist() == [True] and int(words[0]) == min(w, rc)
    ones = (1 << (2 * k)) - 1
    assert _word("G" * k) == ones and SM.canonical(b"G" * k, 0, k) == SM.canonical(b"C" * k, 0, k) == ones // 3  # poly-C: 0101...
    assert SM.canonical(b"A" * k, 0, k) == SM.canonical(b"T" * k, 0, k) == 0
    if k == 32:  # no canonical word is the table's empty slot
        assert ones == 0xFFFFFFFFFFFFFFFF and SM.canonical(b"G" * 32, 0, 32) == 0x5555555555555555
    if k % 2 == 0:  # a palindrome is its own reverse complement: w == rc
        half = _rs(rng, k // 2)
        pal = half + _rc(half)
        assert _rc(pal) == pal and SM.canonical(pal, 0, k) == _word(pal.decode())
        assert int(qscreen.canonical_words(pal, k)[0][0]) == _word(pal.decode())
        assert len(SM.kmers_of(b">p\n" + pal + b"\n>q\n" + _rc(pal) + b"\n", k)) == 1


# ---- the reference set ---------------------------------------------------------------------------------------------------------------
def _awkward_fasta(rng, k):
    a, b, c = _rs(rng, 200), _rs(rng, 300, b"ACGTacgt" * 8 + b"NRYKMSW"), _rs(rng, 3 * k)
    lines = lambda s, w, nl: b"".join(s[i:i + w] + nl for i in range(0, len(s), w))  # noqa: E731
    return (b">one a plain record\n" + lines(a, 60, b"\n") + b">two lower case, N and IUPAC letters, CRLF\r\n" + lines(b, 70, b"\r\n") +
            b">three shorter than k\n" + a[:k - 1] + b"\n>four empty\n>five a k-mer split across every line break\n" + lines(c, 7, b"\n") +
            b">six the first record again, reverse-complemented\n" + lines(_rc(a), 50, b"\n") + b"\n\n>seven blank lines inside\n" +
            a[:k] + b"\n\n" + a[k:2 * k] + b"\n"), (a, b, c)


@pytest.mark.parametrize("k", [15, 16, 31, 32])
def test_the_numpy_builder_against_the_model(tmp_path, k):
    rng = np.random.default_rng(100 + k)
    fasta, (a, b, c) = _awkward_fasta(rng, k)
    R = SM.kmers_of(fasta, k)
    ref = qscreen.reference_kmers(fasta, k)
    assert ref.kmers.dtype == np.uint64 and ref.kmers.tolist() == sorted(R) and (np.diff(ref.kmers.astype(object)) > 0).all()
    assert ref.records == 7 and ref.bases == 200 + 300 + k - 1 + 0 + 3 * k + 200 + 2 * k
    assert SM.records_of(fasta) == qscreen.records_of(fasta) and SM.records_of(fasta)[3] == b"" and SM.records_of(fasta)[4] == c
    # record six adds nothing (canonical words), record three nothing (no k-mer), five all of its 2 k + 1
    assert len(R) == len(SM.kmers_of(b">x\n" + a + b"\n>y\n" + b + b"\n>z\n" + c + b"\n", k))
    assert all(SM.canonical(c, p, k) in R for p in range(2 * k + 1))
    assert SM.canonical(a[:k - 1] + a[:1], 0, k) not in R or a[k - 1:k] == a[:1]  # k-mers do not span records
    assert 0 < len(SM.kmers_of(b">b\n" + b, k)) < 300 - k + 1  # the other letters break k-mers; lower case counts
    assert SM.kmers_of(b">b\n" + b, k) == SM.kmers_of(b">b\n" + b.upper().replace(b"R", b"N"), k)
    # gzip input, by its magic number; sequence in front of the first header is a record
    plain, packed = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    plain.write_bytes(fasta)
    packed.write_bytes(gzip.compress(fasta))
    assert qscreen.read_fasta(str(plain)) == qscreen.read_fasta(str(packed)) == fasta
    head = qscreen.reference_kmers(a + b"\n>two\n" + c, k)
    assert head.records == 2 and head.kmers.tolist() == sorted(SM.kmers_of(b">one\n" + a + b"\n>two\n" + c, k))
    assert qscreen.reference_kmers(b">none\nACGTNACGT\n", k).kmers.size == 0 and qscreen.reference_kmers(b"", k).records == 0


# ---- the [screen] section --------------------------------------------------------------------------------------------------------------
def _ref_file(tmp_path, name="spike.fa", seq=None):
    path = tmp_path / name
    seq = seq if seq is not None else _rs(np.random.default_rng(7), 300)
    data = b">spike\n" + seq + b"\n"
    path.write_bytes(gzip.compress(data) if name.endswith(".gz") else data)
    return path, seq


def test_conf_section(tmp_path):
    path, seq = _ref_file(tmp_path)
    cf = qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference : %s\n" % path))
    assert cf.screen is True and (cf.screen_kmer, cf.screen_min_hits, cf.screen_action) == (31, 1, "report")
    p = cf.screen_params()
    assert sorted(p) == ["action", "kmer", "kmers", "min_hits", "reference"] and (p["kmer"], p["min_hits"], p["action"]) == (31, 1, "report")
    assert p["kmers"].dtype == np.uint64 and p["kmers"].tolist() == sorted(SM.kmers_of(b">s\n" + seq, 31))
    assert p["reference"] == dict(name="spike.fa", records=1, bases=300, kmers=270)
    assert hb.SCREEN.on(cf) and hb.SCREEN.conf_params(cf)["kmers"] is p["kmers"]  # what stage.enable hands screen_set
    gz, _ = _ref_file(tmp_path, "spike.fa.gz", seq)
    cf = qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference : %s\nkmer : 15\nmin_hits : 65535\naction : Drop\n" % gz))
    p2 = cf.screen_params()
    assert (p2["kmer"], p2["min_hits"], p2["action"]) == (15, 65535, "drop") and p2["reference"]["name"] == "spike.fa.gz"
    assert p2["kmers"].tolist() == sorted(SM.kmers_of(b">s\n" + seq, 15))
    for k in (15, 32):
        assert qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference : %s\nkmer : %d\n" % (path, k))).screen_params()["kmer"] == k


def test_conf_without_the_section_or_with_an_empty_reference(tmp_path):
    for extra in ("", "[screen]\n", "[screen]\nreference :\n", "[screen]\nreference :\nkmer : 99\nmin_hits : 0\naction : burn\n"):
        cf = qconf.QuadeConf(_conf(tmp_path, extra))
        assert cf.screen is False and not hb.SCREEN.on(cf) and cf.screen_reference == ""
    # off, the section needs no device pipeline either
    assert qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference :\n", gpu="[gpu]\ndevice_pipeline : False\n")).screen is False


def test_conf_rejections(tmp_path):
    path, _ = _ref_file(tmp_path)
    sec = "[screen]\nreference : %s\n" % path

    def message(extra, gpu=""):
        with pytest.raises(AssertionError) as ei:
            qconf.QuadeConf(_conf(tmp_path, extra, gpu=gpu))
        return str(ei.value)

    for k in (14, 33, 0, -1):
        assert message(sec + "kmer : %d\n" % k) == qconf.SCREEN_KMER == "Authorized values for [screen] kmer : 15 to 32"
    for m in (0, 65536, -5):
        assert message(sec + "min_hits : %d\n" % m) == qconf.SCREEN_MIN_HITS == "Authorized values for [screen] min_hits : 1 to 65535"
    for a in ("keep", "1", "report drop"):
        assert message(sec + "action : %s\n" % a) == qconf.SCREEN_ACTION == "Authorized values for [screen] action : report or drop"
    for gpu in ("device_pipeline : False\n", "device_inflate : False\n", "device_deflate : False\n", "gzip_level : 6\n"):
        assert message(sec, gpu="[gpu]\n" + gpu) == qconf.SCREEN_NEEDS
    assert qconf.SCREEN_NEEDS.split(" needs ")[1] == qconf.FILTER_NEEDS.split(" needs ")[1]
    # the reference: missing, a directory, a damaged gzip file; no k-mer; too many k-mers
    assert message("[screen]\nreference : %s\n" % (tmp_path / "nothing.fa")) == qconf.SCREEN_REFERENCE
    assert message("[screen]\nreference : %s\n" % tmp_path) == qconf.SCREEN_REFERENCE
    (tmp_path / "cut.fa.gz").write_bytes(gzip.compress(b">x\n" + b"ACGT" * 500)[:-20])
    assert message("[screen]\nreference : %s\n" % (tmp_path / "cut.fa.gz")) == qconf.SCREEN_REFERENCE
    short, _ = _ref_file(tmp_path, "short.fa", b"ACGTACGTACGTACGTACGTACGTACGTAC")  # 30 bases
    assert message("[screen]\nreference : %s\n" % short) == qconf.SCREEN_NO_KMER
    assert qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference : %s\nkmer : 30\n" % short)).screen_params()["kmers"].size == 1
    broken, _ = _ref_file(tmp_path, "broken.fa", b"ACGTACGTACGTACGTNACGTACGTACGTACGTN" * 20)
    assert message("[screen]\nreference : %s\nkmer : 17\n" % broken) == qconf.SCREEN_NO_KMER
    assert "4194304" in qconf.SCREEN_TOO_MANY and qscreen.MAX_KMERS == 1 << 22 and qscreen.LDS_MAX_KMERS == 6144
    for text in (qconf.SCREEN_NEEDS, qconf.SCREEN_REFERENCE, qconf.SCREEN_NO_KMER, qconf.SCREEN_TOO_MANY, qconf.SCREEN_KMER,
                 qconf.SCREEN_MIN_HITS, qconf.SCREEN_ACTION):
        assert "\n" not in text and "[screen]" in text  # one line each


def test_conf_rejects_more_than_the_cap_of_kmers(tmp_path, monkeypatch):
    """the cap itself, on a small scale: the check compares the distinct k-mers with screen.MAX_KMERS"""
    path, _ = _ref_file(tmp_path)  # 270 distinct 31-mers
    monkeypatch.setattr(qscreen, "MAX_KMERS", 269)
    with pytest.raises(AssertionError) as ei:
        qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference : %s\n" % path))
    assert str(ei.value) == qconf.SCREEN_TOO_MANY
    monkeypatch.setattr(qscreen, "MAX_KMERS", 270)
    assert qconf.QuadeConf(_conf(tmp_path, "[screen]\nreference : %s\n" % path)).screen


@pytest.mark.parametrize("extra,message", [("kmer : 40\n", qconf.SCREEN_KMER), ("action : erase\n", qconf.SCREEN_ACTION)])
def test_rejected_configuration_ends_the_command_line_with_status_1(tmp_path, extra, message):
    path, _ = _ref_file(tmp_path)
    conf = _conf(tmp_path, "[screen]\nreference : %s\n" % path + extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", conf], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert message in r.stdout + r.stderr
    assert not (tmp_path / sr.REPORT_NAME).exists() and not (tmp_path / "Quade_report.csv").exists()


# ---- the report ------------------------------------------------------------------------------------------------------------------------
def test_report_lines_against_hand_written_text(tmp_path):
    t = [[10, 4, 3, 2, 2000, 300, 3000, 1200], [0] * 8, [5, 5, 5, 5, 100, 100, 1500, 1500]]
    head = ["Program Quade-screen 0.3.2", "", "reference\tphix.fa", "reference_records\t1", "reference_bases\t5386", "reference_kmers\t5356",
            "kmer\t31", "min_hits\t1"]
    cols = ("destination\tpairs\tmatched_pairs\tr1_hit_reads\tr2_hit_reads\tkmers\thit_kmers\tbases_in\tbases_matched\tmatched_pct\t"
            "hit_kmer_pct\tdropped_pairs")
    rows = ["S1_pass\t10\t4\t3\t2\t2000\t300\t3000\t1200\t40.00\t15.00\t%d", "S1_fail\t0\t0\t0\t0\t0\t0\t0\t0\t0.00\t0.00\t%d",
            "Undetermined\t5\t5\t5\t5\t100\t100\t1500\t1500\t100.00\t100.00\t%d", "Total\t15\t9\t8\t7\t2100\t400\t4500\t2700\t60.00\t19.04\t%d"]
    want = head + ["action\treport", "", cols] + [r % 0 for r in rows]
    assert sr.report_lines(t, ["S1"], PARAMS) == want
    assert sr.report_lines(np.array(t, dtype=np.uint64), ["S1"], PARAMS) == want
    drop = head + ["action\tdrop", "", cols] + [r % n for r, n in zip(rows, (4, 0, 5, 9))]
    assert sr.report_lines(t, ["S1"], dict(PARAMS, action="drop")) == drop
    assert sr.REPORT_NAME == "Quade_screen_report.csv" and "Date" not in "\n".join(want)
    assert sr.COLUMNS[1:9] == hb.SCREEN_COUNTERS == SM.COUNTERS
    with pytest.raises(AssertionError):
        sr.report_lines(t, ["S1", "S2"], PARAMS)
    with pytest.raises(AssertionError):
        sr.report_lines([[0] * 7] * 3, ["S1"], PARAMS)
    p, p2 = tmp_path / sr.REPORT_NAME, tmp_path / "again.csv"
    sr.write_report(str(p), t, ["S1"], PARAMS)
    os.makedirs(tmp_path / "x")
    assert hb.PIPE_STAGE["screen"].write_report(str(tmp_path / "x"), np.array(t, dtype=np.uint64), ["S1"], dict(PARAMS)) == \
        str(tmp_path / "x" / sr.REPORT_NAME)
    sr.write_report(str(p2), np.array(t, dtype=np.uint64), ["S1"], dict(PARAMS))
    assert p.read_bytes() == p2.read_bytes() == (tmp_path / "x" / sr.REPORT_NAME).read_bytes() == ("\n".join(want) + "\n").encode()


def test_report_arithmetic_past_63_bits():
    t = np.zeros((3, 8), dtype=np.uint64)
    t[0] = [(1 << 63) + 3, (1 << 62) + 1, 0, 0, (1 << 63) + 3, (1 << 62) + 1, 1 << 63, 1]
    t[1] = [(1 << 63) + 3, (1 << 63) + 3, 0, 0, 1 << 63, 1 << 63, 1 << 63, 1]
    lines = sr.report_lines(t, ["S"], dict(PARAMS, action="drop"))
    first = lines[-4].split("\t")
    assert first[9] == "49.99" and first[10] == "49.99" and first[11] == str((1 << 62) + 1)  # exact integers: a float would give 50.00
    total = lines[-1].split("\t")
    assert total[1] == str((1 << 64) + 6) and total[2] == str((1 << 63) + (1 << 62) + 4) and total[7] == str(1 << 64)  # past 64 bits, exact
    assert total[9] == "74.99"


# ---- the stage tuples, the exchange and the library ------------------------------------------------------------------------------------
def test_the_pinned_tuples_stay_and_the_pipeline_tuple_ends_in_the_screen():
    assert [s.name for s in hb.STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "filter"]
    assert [s.name for s in hb.RUN_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter"]
    assert [s.name for s in hb.PIPE_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter", "screen"]
    assert "screen" not in hb.STAGE and "screen" not in hb.RUN_STAGE and hb.PIPE_STAGES[:7] == hb.RUN_STAGES
    assert all(hb.PIPE_STAGE[s.name] is s for s in hb.PIPE_STAGES)
    st = hb.PIPE_STAGE["screen"]
    assert st is hb.SCREEN and (st.engine, st.conf, st.params, st.shape, st.count, st.report, st.report_args) == \
        ("screen", "screen", "screen_params", (-1, 8), "rows", "screen_report", ("samples", "params"))
    assert st.report_module() is sr and hb.SCREEN_ACTIONS == ("report", "drop")
    for name in ("screen_set", "screen_get", "screen_read", "screen_add", "screen_active", "screen_kind", "dev_screen"):
        assert callable(getattr(hb.Engine, name)), name


def test_pack_unpack_and_sum():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 62, (7, 8), dtype=np.uint64)
    b = rng.integers(0, 1 << 62, (7, 8), dtype=np.uint64)
    a[1, 2], b[1, 2] = (1 << 63) - 1, 1 << 62
    blob = hb.pack_table("screen", a)
    assert isinstance(blob, bytes) and len(blob) == 8 + 7 * 64 and blob == np.array([7], dtype="<u8").tobytes() + a.astype("<u8").tobytes()
    assert blob == hb.pack_table(hb.SCREEN, a.reshape(-1))  # by object or by name, flat or shaped
    a2 = hb.unpack_table("screen", blob)
    assert a2.dtype == np.uint64 and a2.shape == (7, 8) and (a2 == a).all() and a2.flags.writeable
    a2 += hb.unpack_table(hb.SCREEN, hb.pack_table("screen", b))
    assert all(int(x) == int(y) + int(z) for x, y, z in zip(a2.reshape(-1), a.reshape(-1), b.reshape(-1)))
    for bad in (blob[:-8], blob + bytes(8), blob[8:]):
        with pytest.raises(AssertionError, match="of the wrong size"):
            hb.unpack_table("screen", bad)
    assert len(hb.pack_table("filter", np.zeros((3, 8), np.uint64))) == 8 + 192 and len(hb.pack_table("posttrim", np.zeros((2, 16), np.uint64))) == 256


def test_exported_symbols():
    new = {"qd_screen_set", "qd_screen_get", "qd_screen_read", "qd_screen_add", "qd_screen_kind", "qd_screen_first_slot", "qd_dev_screen"}
    with open(os.path.join(ROOT, "include", "quade_hip.h")) as fh:
        text = fh.read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert new <= set(re.findall(r"\b(qd_[a-z_0-9]+)\s*\(", header))
    lib = os.path.join(ROOT, "quade_amd", "lib", "libquade_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert new | {"qd_screen_active", "qd_screen_device"} <= names
    assert new <= {s[0] for s in hb.SYMBOLS}
    assert hb.load_library().qd_version() == 6 and "#define QD_ABI_VERSION 6" in text  # additive: the version stays
    assert "no reference counterpart" in text.split("int qd_screen_set")[0][-6000:]
    assert "no reference counterpart" in text.split("int qd_dev_screen")[0][-1200:]
    assert ctypes.sizeof(hb.qd_screen_params) == 12 and "#define QD_SCREEN_VALUES 8" in text
    assert "#define QD_SCREEN_MAX_KMERS (1u << 22)" in text and "#define QD_SCREEN_LDS_MAX_KMERS 6144u" in text
    assert "#define QD_SCREEN_DROPPED 0x80u" in text and SM.DROPPED == 0x80
    # the library's hash helper answers without a context, and refuses a count no table is built for
    lib = hb.load_library()
    assert 0 <= lib.qd_screen_first_slot(12345, 100) < 1 << 14 and lib.qd_screen_first_slot(12345, 0) == hb.QD_ERR_INVALID
    assert lib.qd_screen_first_slot(12345, (1 << 22) + 1) == hb.QD_ERR_INVALID and 0 <= lib.qd_screen_first_slot(12345, 1 << 22) < 1 << 23
    # the rule stands in the header, the model and the help in the same words
    norm = lambda s: re.sub(r"(\n \*|\s)+", " ", s)  # noqa: E731  (line breaks and the comment's margin apart)
    for words in ("u(b) = b & 0xDF", "A base is valid when u(b) is one of A, C, G, T", "c(b) = (u(b) >> 1) & 3, which gives A 0, C 1, T 2, G 3",
                  "the complement is c ^ 2", "exists when s[p .. p + k) are all valid", "w = sum c(s[p + i]) << 2 (k - 1 - i)",
                  "rc = sum (c(s[p + k - 1 - i]) ^ 2) << 2 (k - 1 - i)", "canonical word min(w, rc)",
                  "holds the distinct canonical words of every k-mer of every record of the reference FASTA",
                  "so k-mers never span two records; lower case counts; any other letter breaks k-mers",
                  "the number of positions p in [0, L - k] whose k-mer exists and whose canonical word is in R",
                  "A read shorter than k has 0 hits and 0 k-mers", "matched when hits(R1) + hits(R2) >= min_hits"):
        assert words in norm(text) and words in norm(SM.__doc__) and words in norm(qconf.SCREEN_HELP), words
