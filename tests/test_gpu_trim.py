"""3' quality and adapter trimming on the MI355X (qd_trim_*, quade_amd/csrc/quade_trim.hip): the trimmed record tables and the 16
counters equal tests/trim_model.py's plain Python rule, exactly -- for the stage on its own (qd_dev_trim: alignments, lengths on
both sides of the staged-line limit, planted adapters at every position, mismatch budgets, case, N, quality edges, the floor,
accumulation, state and errors) and through the command line (every output file against the oracle's file trimmed by the model,
the trim report, the quality report of the trimmed reads, chunk workers, write flags, ranks, the bundled golden run)."""
import os
import shutil

import numpy as np
import pytest

from quade_amd import hip_backend as hb
from quade_amd import quality_report as qr
from quade_amd import trim_report as tr
from tests import qstats_model as QM
from tests import trim_model as TM
from tests import stage_support as SS
from tests.run_support import _compare_dirs
from tests.stage_support import AD1, AD2, BASES, QUALS, _cli, _text_from, torch_cuda  # noqa: F401
from tests.stage_support import LONG_LENS as LENS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ADAPTER_LENS = (1, 3, 8, 19, 33, 64)


def _adapter(A, seed=0):
    """A letters of ACGT, no two neighbours equal (a shifted copy never matches itself whole)"""
    rng = np.random.default_rng(1000 + 7 * A + seed)
    out = [int(rng.integers(0, 4))]
    while len(out) < A:
        out.append((out[-1] + 1 + int(rng.integers(0, 3))) % 4)
    return bytes(b"ACGT"[v] for v in out)


def _cases(rng, ad, mo, pct, C):
    """[(tag, seq, qual)] for one read stream: adapter ad (may be empty), min_overlap mo, max_mismatch_pct pct, cutoff C (0: the
    quality cases are made for a cutoff of 20 and simply pass)."""
    A, Cq = len(ad), C or 20
    out = []

    def rs(L, alphabet=b"ACGT"):
        return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))

    def good(L):
        return bytes(33 + int(v) for v in rng.integers(Cq + 5, Cq + 20, L))

    def other(b):
        return b"ACGT"[(b"ACGT".index(b) + 1 + int(rng.integers(0, 3))) % 4]

    def spoil(copy, k, with_byte=None):
        copy = bytearray(copy)
        for i in rng.permutation(len(copy))[:k]:
            copy[i] = with_byte if with_byte is not None else other(copy[i])
        return bytes(copy)

    # every length, every kind of base, every quality byte
    walk = 0
    for rep in range(5):
        for L in LENS:
            if L > 1000 and rep > 1:
                continue
            if walk < 2 * len(QUALS):
                qual = bytes(QUALS[(walk + k) % len(QUALS)] for k in range(L))
                walk += L
            else:
                qual = bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L))
            out.append(("random", rs(L, BASES), qual))
    if A:
        budget = A * pct // 100
        for p in range(151):  # the adapter (or what fits of it) from every position of a 151-base read
            out.append(("planted@%d" % p, rs(p) + (ad + rs(151))[:151 - p], good(151)))
        for L in (300, 330, 2049):  # ... and in lines beyond one word per lane, staged or not
            for p in (0, 1, L // 2, L - A, L - mo, L - mo + 1):
                if 0 <= p <= L:
                    out.append(("planted-long", rs(p) + (ad + rs(L))[:L - p], good(L)))
        for L in sorted({mo - 1, mo, A - 1, A, A // 2} & set(range(0, 65))):  # the adapter is longer than the read
            out.append(("short%d" % L, ad[:L], good(L)))
        if 40 + A <= 151:
            tail = 151 - 40 - A
            out.append(("budget", rs(40) + spoil(ad, budget) + rs(tail), good(151)))
            if budget + 1 <= A:
                out.append(("beyond", rs(40) + spoil(ad, budget + 1) + rs(tail), good(151)))
                out.append(("n-beyond", rs(40) + spoil(ad, budget + 1, ord("N")) + rs(tail), good(151)))
            out.append(("n-budget", rs(40) + spoil(ad, budget, ord("N")) + rs(tail), good(151)))
            out.append(("lower", (rs(40) + ad + rs(tail)).lower(), good(151)))
            out.append(("lower-budget", rs(40) + spoil(ad, budget).lower() + rs(tail), good(151)))
        if 20 + 2 * A + 5 <= 151:  # a perfect copy behind an acceptable earlier one: the leftmost wins
            out.append(("leftmost", rs(20) + spoil(ad, budget) + rs(5) + ad + rs(151 - 25 - 2 * A), good(151)))
    # quality: tails at the cutoff's edges, a tail that recovers, whole lines at the edges, noisy lines of every length class
    for v in (Cq - 1, Cq, Cq + 1):
        for run in (1, 5, 30):
            out.append(("run%+d" % (v - Cq), rs(151), good(151 - run) + bytes([33 + v]) * run))
        out.append(("all%+d" % (v - Cq), rs(64), bytes([33 + v]) * 64))
    out.append(("recover", rs(23), good(20) + bytes([33 + Cq + 20, 33 + max(0, Cq - 15), 33 + Cq + 20])))
    out.append(("recover-not", rs(23), good(20) + bytes([33 + max(0, Cq - 15), 33 + Cq + 2, 33 + max(0, Cq - 15)])))
    for k in range(0, 152, 3):  # a bad tail of every length: its end falls into every lane's stretch
        out.append(("tail", rs(151), good(151 - k) + bytes(33 + int(v) for v in rng.integers(0, Cq, k))))
    for L in (17, 151, 151, 151, 257, 300, 330, 2049):
        for _ in range(4):
            out.append(("noisy", rs(L, b"ACGTN"), bytes(33 + int(v) for v in rng.integers(0, 2 * Cq + 2, L))))
    if A:  # an adapter inside a bad tail and in front of one
        for p in (30, 100, 140):
            out.append(("both", rs(p) + (ad + rs(151))[:151 - p], good(120) + bytes([35]) * 31))
    return out


class Stage(object):
    """R1 and R2 drawn apart: each stream has the cases of its own adapter in its own order (a pair's two reads differ), the
    shorter list filled up with random reads."""

    def __init__(self, seed, P, n=None):
        rng = np.random.default_rng(seed)
        self.P = P
        lists = [_cases(rng, P.adapters[r], P.min_overlap, P.max_mismatch_pct, P.quality_cutoff) for r in (0, 1)]
        m = max(len(x) for x in lists)
        for x in lists:
            while len(x) < m:
                L = int(LENS[int(rng.integers(0, len(LENS) - 1))])
                x.append(("fill", bytes(BASES[int(v)] for v in rng.integers(0, len(BASES), L)),
                          bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L))))
        self.cases = [[x[int(i)] for i in rng.permutation(m)] for x in lists]
        if n is not None:
            while len(self.cases[0]) < n:
                self.cases = [c + c for c in self.cases]
            self.cases = [c[:n] for c in self.cases]
        self.n = len(self.cases[0])
        (self.t1, self.r1), (self.t2, self.r2) = (_text_from(rng, c) for c in self.cases)

    def model(self):
        """-> (trimmed tables, counters uint64[2, 8])"""
        table, outs = TM.new_table(), []
        for r, recs in enumerate((self.r1, self.r2)):
            o = recs.copy()
            for j, (_, seq, qual) in enumerate(self.cases[r]):
                o[j, 4] = TM.count(table, seq, qual, r, self.P)
            outs.append(o)
        return outs, np.array(table, dtype=np.uint64)

    def run(self, eng):
        return eng.dev_trim(self.t1, self.r1, self.t2, self.r2)


def _engine(P=None):
    eng = hb.Engine(0)
    if P is not None and P.on:
        eng.trim_set(P.adapters[0], P.adapters[1], P.quality_cutoff, P.min_overlap, P.max_mismatch_pct, P.min_length)
    return eng


def _params(a1=0, a2=0, **kw):
    return TM.Params(_adapter(a1, 1) if a1 else b"", _adapter(a2, 2) if a2 else b"", **kw)


def _check(stage, eng, before=None):
    got = stage.run(eng)
    want, table = stage.model()
    for r in (0, 1):
        assert got[r].shape == want[r].shape and got[r].dtype == np.uint32
        bad = np.argwhere(got[r] != want[r])
        assert not len(bad), [(r, int(j), stage.cases[r][int(j)][0], int(got[r][j, 4]), int(want[r][j, 4])) for j, _ in bad[:6]]
    counters = eng.trim_read()
    assert counters.shape == (2, 8) and counters.dtype == np.uint64
    if before is not None:
        table = table + before
    assert (counters == table).all(), (counters.tolist(), table.tolist())
    return table


# name: (R1 adapter length, R2 adapter length, parameters)
CONFIGS = {
    "both_19_33": (19, 33, dict(quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=0)),
    "quality_only": (0, 0, dict(quality_cutoff=10, min_length=1)),
    "r1_only_8": (8, 0, dict(min_overlap=3, max_mismatch_pct=13, min_length=20)),
    "r2_only_64": (0, 64, dict(min_overlap=5, max_mismatch_pct=10, min_length=0)),
    "both_1_3": (1, 3, dict(quality_cutoff=30, min_overlap=1, max_mismatch_pct=50, min_length=400)),
    "both_33_19_exact": (33, 19, dict(quality_cutoff=2, min_overlap=19, max_mismatch_pct=0, min_length=20)),
    "both_64_8_cutoff_93": (64, 8, dict(quality_cutoff=93, min_overlap=8, max_mismatch_pct=50, min_length=0)),
}


def test_the_generated_inputs_hold_the_cases():
    a1, a2, kw = CONFIGS["both_19_33"]
    P = _params(a1, a2, **kw)
    st = Stage(1, P)
    assert st.n > 300 and {a for a, _, _ in CONFIGS.values()} | {b for _, b, _ in CONFIGS.values()} == set(ADAPTER_LENS) | {0}
    assert {kw.get("min_length", 0) for _, _, kw in CONFIGS.values()} == {0, 1, 20, 400}
    modes = {(bool(a), bool(b), kw.get("quality_cutoff", 0) > 0) for a, b, kw in CONFIGS.values()}
    assert {(False, False, True), (True, False, False), (False, True, False), (True, True, True)} <= modes
    for r, (text, recs) in enumerate(((st.t1, st.r1), (st.t2, st.r2))):
        cases, ad = st.cases[r], P.adapters[r]
        A, budget = len(ad), len(ad) * 10 // 100
        assert budget >= 1
        assert all(text[int(q[3]):int(q[3]) + int(q[4])] == s and text[int(q[5]):int(q[5]) + int(q[4])] == ql for q, (_, s, ql) in zip(recs, cases))
        assert {int(q[3]) % 16 for q in recs if q[4]} == set(range(16)) == {int(q[5]) % 16 for q in recs if q[4]}
        assert b"\r\n" in text and {len(s) for _, s, _ in cases} >= set(LENS)
        assert set(b"".join(q for t, _, q in cases if t == "random")) == set(QUALS)
        # 330 bases: lines on both sides of the staged-line limit (21 aligned words)
        assert {(int(q[3]) % 16 + 330 + 15) // 16 <= 21 for q in recs if q[4] == 330} == {True, False}
        by = {}
        for t, s, ql in cases:
            by.setdefault(t, []).append((s, ql))
        trim = lambda s, ql: TM.trim_read(s, ql, r, P)  # noqa: E731
        for p in range(151):  # planted at every p: found there (or, rarely, further left by chance) while the overlap is long enough
            (s, ql), = by["planted@%d" % p]
            Lq, La, _ = trim(s, ql)
            assert Lq == 151 and (La <= p if p <= 151 - 3 else La <= 151)
        exact = [p for p in range(151) if trim(*by["planted@%d" % p][0])[1] == p]
        assert len(exact) > 140 and {0, 1, 148} <= set(exact)  # 148: an overlap of exactly min_overlap is cut
        assert sum(trim(*by["planted@%d" % p][0])[1] == 151 for p in (149, 150)) >= 1  # one less is left alone
        assert trim(*by["budget"][0])[1] == 40 and trim(*by["beyond"][0])[1] > 40
        assert trim(*by["n-budget"][0])[1] == 40 and trim(*by["n-beyond"][0])[1] > 40 and b"N" in by["n-budget"][0][0]
        assert trim(*by["lower"][0])[1] == 40 and by["lower"][0][0].islower() and trim(*by["lower-budget"][0])[1] == 40
        s, ql = by["leftmost"][0]
        assert trim(s, ql)[1] == 20 and s[25 + A:25 + 2 * A] == ad and s[20:20 + A] != ad
        assert {len(s) for t in by if t.startswith("short") for s, _ in by[t]} >= {2, 3, A - 1}
        assert trim(*by["short3"][0])[1] == 0 and trim(*by["short2"][0])[1] == 2
        assert any(TM.trim_read(s, ql, r, P)[1] < len(s) for s, ql in by["planted-long"] if len(s) == 2049)
        # quality: runs at the edges of the cutoff, a tail that recovers and one that does not
        assert sorted(trim(*x)[0] for x in by["run-1"]) == [121, 146, 150] and [trim(*x)[0] for x in by["run+0"]] == [151] * 3
        assert [trim(*x)[0] for x in by["run+1"]] == [151] * 3
        assert trim(*by["all-1"][0])[0] == 0 and trim(*by["all+0"][0])[0] == 64 and trim(*by["all+1"][0])[0] == 64
        assert trim(*by["recover"][0])[0] == 23 and trim(*by["recover-not"][0])[0] == 20
        assert len({trim(*x)[0] for x in by["tail"]}) > 40 and len({trim(*x)[0] for x in by["noisy"]}) > 10
        assert any(La < Lq < len(s) for s, ql in by["both"] for Lq, La, _ in [trim(s, ql)])
    assert any(len(a[1]) != len(b[1]) for a, b in zip(*st.cases))
    _, table = st.model()
    assert (table[:, 3:7] > 0).all() and (table[:, 0] == st.n).all()
    floor = Stage(1, _params(*CONFIGS["r1_only_8"][:2], **CONFIGS["r1_only_8"][2]))
    assert floor.model()[1][0, 7] > 0  # reads the floor holds back


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_stage_equals_the_model(torch_cuda, name):
    a1, a2, kw = CONFIGS[name]
    P = _params(a1, a2, **kw)
    with _engine(P) as eng:
        got = eng.trim_get()
        assert got["adapter_r1"].encode() == P.adapters[0] and got["adapter_r2"].encode() == P.adapters[1]
        assert got["quality_cutoff"] == P.quality_cutoff and got["min_length"] == P.min_length
        _check(Stage(2, P), eng)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_stage_pair_counts(torch_cuda, n):
    a1, a2, kw = CONFIGS["both_19_33"]
    P = _params(a1, a2, **kw)
    with _engine(P) as eng:
        st = Stage(3, P, n=n)
        assert st.n == n
        table = _check(st, eng)
        assert (table[:, 0] == n).all()


def test_accumulation_reset_and_add(torch_cuda):
    P = _params(19, 33, quality_cutoff=20)
    a, b = Stage(20, P, n=300), Stage(21, P, n=65)
    with _engine(P) as eng, _engine(P) as other:
        ta = _check(a, eng)
        both = _check(b, eng, before=ta)
        eng.reset_counts()
        assert not eng.trim_read().any() and eng.trim_get()["quality_cutoff"] == 20
        tb = _check(b, eng)
        _check(a, other)
        eng.trim_add(other.trim_read())  # a second context's counters fold in
        assert (eng.trim_read() == both).all() and (both == ta + tb).all() and (other.trim_read() == ta).all()
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.trim_add(np.zeros(5, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        eng.trim_set()  # all off: the table is freed
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.trim_read()
        assert ei.value.code == hb.QD_ERR_STATE
        eng.trim_set(quality_cutoff=5)
        assert not eng.trim_read().any()


def test_state_and_errors(torch_cuda):
    P = _params(19, 0, quality_cutoff=20)
    st = Stage(30, P, n=64)
    with hb.Engine(0) as eng:
        for call in (eng.trim_read, lambda: st.run(eng), lambda: eng.trim_add(np.zeros((2, 8), np.uint64))):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        assert eng.trim_get() == dict(adapter_r1="", adapter_r2="", quality_cutoff=0, min_overlap=0, max_mismatch_pct=0, min_length=0)
        assert eng.lib.qd_trim_set(eng._h, None) == 0  # NULL = off
        eng.trim_set(P.adapters[0], b"", 20)
        good = eng.trim_get()
        for bad in (dict(adapter_r1="ACGN"), dict(adapter_r1="AC"), dict(quality_cutoff=94), dict(quality_cutoff=-1, adapter_r1="ACGT"),
                    dict(quality_cutoff=1, min_overlap=0), dict(quality_cutoff=1, min_overlap=65), dict(quality_cutoff=1, max_mismatch_pct=51),
                    dict(quality_cutoff=1, max_mismatch_pct=-1), dict(quality_cutoff=1, min_length=65536), dict(quality_cutoff=1, min_length=-1),
                    dict(adapter_r1="A" * 65), dict(adapter_r1="ACGTACGT", adapter_r2="ACG", min_overlap=4)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.trim_set(**bad)
            assert ei.value.code == hb.QD_ERR_INVALID, bad
            assert eng.trim_get() == good  # a rejected call changes nothing
        for ok in (dict(adapter_r1="a", min_overlap=1), dict(adapter_r2="ACGT" * 16, min_overlap=64), dict(quality_cutoff=93, max_mismatch_pct=50),
                   dict(quality_cutoff=1, max_mismatch_pct=0, min_length=65535)):
            eng.trim_set(**ok)
        assert eng.trim_get()["min_length"] == 65535
        eng.trim_set("a", min_overlap=1)
        assert eng.trim_get()["adapter_r1"] == "A"
        eng.trim_set(P.adapters[0], b"", 20)
        out = np.zeros(7, dtype=np.uint64)
        assert eng.lib.qd_trim_read(eng._h, hb._ptr(out), 7) == hb.QD_ERR_INVALID
        want = _check(st, eng)
        # a bad table never becomes an address: refused on the host, nothing launched, the counters as they were
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_trim(st.t1, bad, st.t2, st.r2)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_trim(st.t1, st.r1, st.t2, bad)
        assert ei.value.code == hb.QD_ERR_INVALID
        assert (eng.trim_read() == want).all()
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))  # plan and barcodes leave the trimming alone
        eng.set_barcodes(["ACGTACGTACGTACGT"])
        assert eng.trim_get() == good and (eng.trim_read() == want).all()


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
TRIM = "[trim]\nadapter_R1 : %s\nadapter_R2 : %s\nquality_cutoff : 20\nmin_length : 25\n" % (AD1, AD2.lower())
P_CLI = TM.Params(AD1, AD2, quality_cutoff=20, min_length=25)
PARAMS_CLI = dict(adapter_r1=AD1, adapter_r2=AD2, quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=25)


def _inserts(g, i, sample, kind):
    """what a trimmer is for: insert reads of 30 .. 151 bases, two in five with an insert shorter than the read (the adapter read
    through, sometimes with a substitution or an N), half with a low-quality 3' tail"""
    rng, out = g.rng, []
    for ad in (AD1, AD2):
        L = int(rng.integers(30, 152))
        s = g.rnd(L, "ACGTACGTACGTN" if i % 3 else "ACGTn")
        if rng.integers(0, 5) < 2:
            p = int(rng.integers(0, L))
            a = list(ad)
            if rng.integers(0, 3) == 0:
                a[int(rng.integers(0, len(a)))] = "N" if rng.integers(0, 2) else "a"
            s = (s[:p] + "".join(a) + g.rnd(151))[:L]
        tail = int(rng.integers(0, min(L, 60))) if rng.integers(0, 2) else 0
        out.append((s, g.q(L - tail, 22, 42) + g.q(tail, 2, 24)))
    return out


def _dataset(d, seed, n_chunks, n, bgzf):
    return SS._dataset(d, seed, n_chunks, n, bgzf, _inserts, SS._early_places)


def _write_conf(path, files, samples, trim=TRIM, **kw):
    SS._write_conf(path, files, samples, extra=trim, **kw)


def _oracle(conf, ref_dir, P=P_CLI):
    """the oracle's run of the conf without trimming -> ({file: trimmed text}, the model's counters)"""
    SS._oracle_run(conf, ref_dir)
    return TM.trimmed_outputs(str(ref_dir), P)


def _check_run(mine, ref, texts, table, params=PARAMS_CLI, only=None):
    SS._check_files(mine, texts, only)
    SS._check_main_report(mine, ref, only)  # as without trimming
    SS._check_report(mine, tr, table, params)


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 3 000 pairs in BGZF, run once with trimming and the quality report on; the model over the oracle's outputs"""
    top = tmp_path_factory.mktemp("trim_bgzf")
    files, samples = _dataset(str(top / "data"), 51, 2, 3000, bgzf=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, trim="")
    texts, table = _oracle(plain, top / "ref")
    conf = top / "conf.txt"
    _write_conf(conf, files, samples, quality=True)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, texts=texts, table=table, mine=top / "mine", ref=top / "ref", plain=plain)


def test_cli_outputs_and_reports_equal_the_model_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert t[0][0] == t[1][0] < 6000 and all(t[r][k] > 0 for r in (0, 1) for k in range(8))  # every counter is exercised
    _check_run(run["mine"], run["ref"], run["texts"], t)
    # the quality report counts the trimmed reads: the model over the outputs just compared
    names = [s[0] for s in run["samples"]]
    with open(run["mine"] / qr.REPORT_NAME) as fh:
        got = fh.read()
    assert got == "\n".join(qr.report_lines(QM.table_from_outputs(str(run["mine"]), names), names)) + "\n"
    assert got != "\n".join(qr.report_lines(QM.table_from_outputs(str(run["ref"]), names), names)) + "\n"


def test_cli_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 52, 2, 3000, bgzf=False)
    _write_conf(tmp_path / "plain.txt", files, samples, trim="")
    texts, table = _oracle(tmp_path / "plain.txt", tmp_path / "ref")
    _write_conf(tmp_path / "conf.txt", files, samples)
    _cli(tmp_path / "conf.txt", tmp_path / "mine")
    _check_run(tmp_path / "mine", tmp_path / "ref", texts, table)
    assert not os.path.exists(tmp_path / "mine" / qr.REPORT_NAME)


def test_cli_chunk_workers_and_write_flags(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n")
    _cli(conf, tmp_path / "workers")
    _check_run(tmp_path / "workers", run["ref"], run["texts"], run["table"])
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, False, False))
    _cli(conf, tmp_path / "flags")  # the counters do not depend on what is written; the files are absent
    _check_run(tmp_path / "flags", run["ref"], run["texts"], run["table"], only=lambda f: "_pass_" in f)


def test_cli_two_ranks_sharded_and_whole_chunks(bgzf_run, tmp_path):
    """2 ranks on GPU 0 (counters through the rendezvous files): each a pair range of ONE shared BGZF chunk, then a chunk each"""
    run = bgzf_run
    _write_conf(tmp_path / "plain.txt", run["files"], run["samples"], trim="", chunks=[0])
    texts, table = _oracle(tmp_path / "plain.txt", tmp_path / "ref")
    assert table != run["table"]
    conf = tmp_path / "shared.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : True\n", chunks=[0])
    _cli(conf, tmp_path / "shared", ranks=2)
    _check_run(tmp_path / "shared", tmp_path / "ref", texts, table)
    conf = tmp_path / "two.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n")
    _cli(conf, tmp_path / "two", ranks=2)
    _check_run(tmp_path / "two", run["ref"], run["texts"], run["table"])
    assert not [f for f in os.listdir(tmp_path / "two") if f.startswith(".quade_rdv")]


def test_cli_without_the_section_nothing_changes(bgzf_run, tmp_path):
    run = bgzf_run
    _cli(run["plain"], tmp_path / "off")
    assert not os.path.exists(tmp_path / "off" / tr.REPORT_NAME)
    _compare_dirs(str(tmp_path / "off"), str(run["ref"]))
    assert sorted(os.listdir(tmp_path / "off")) == sorted(f for f in os.listdir(run["mine"]) if f not in (tr.REPORT_NAME, qr.REPORT_NAME))


def test_bundled_golden_run_with_a_quality_cutoff(torch_cuda, tmp_path, bundled_dir):
    """the reference's own 299 pairs with [trim] quality_cutoff : 20: the goldens trimmed by the model, all on the device"""
    from quade_amd.quade import Quade
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    with open(os.path.join(bundled_dir, "result", "Quade_conf_file.txt")) as fh:
        base = fh.read()
    work = tmp_path / "result"
    work.mkdir()
    conf = work / "conf.txt"
    conf.write_text(base + "\n[trim]\nquality_cutoff : 20\n")
    old = os.getcwd()
    os.chdir(str(work))
    try:
        q = Quade(conf_file=str(conf))
        assert q() == 0
    finally:
        os.chdir(old)
    os.remove(conf)
    st = q.pipe_stats
    assert st is not None and st["gzip_fallbacks"] == 0 and st["host_inflated_runs"] == 0, st
    P = TM.Params(quality_cutoff=20)
    texts, table = TM.trimmed_outputs(os.path.join(bundled_dir, "result"), P)
    assert table[0][0] == table[1][0] == 299 and table[0][3] > 0 and table[1][3] > 0
    _check_run(work, os.path.join(bundled_dir, "result"), texts, table,
               params=dict(adapter_r1="", adapter_r2="", quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=0))
