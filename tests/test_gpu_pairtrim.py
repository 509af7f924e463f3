"""Paired-end overlap trimming on the MI355X (qd_pairtrim_*, quade_amd/csrc/quade_pairtrim.hip): the cut record tables and the
1040 values of the table equal tests/pairtrim_model.py's plain Python rule, exactly -- for the stage on its own (qd_dev_pairtrim:
inserts on both sides of every edge of the rule, mismatch budgets, N, case, other bytes, unequal reads, repeats, the floor, both
sides of the staged-line limit, every alignment, accumulation, state and errors) and through the command line (every output file
against the oracle's file cut by the model, both trim reports, the quality report of the cut reads, chunk workers, write flags,
ranks)."""
import os

import numpy as np
import pytest

from quade_amd import hip_backend as hb
from quade_amd import pair_trim_report as pr
from quade_amd import quality_report as qr
from quade_amd import trim_report as tr
from tests import pairtrim_model as PM
from tests import qstats_model as QM
from tests import trim_model as TM
from tests import stage_support as SS
from tests.run_support import _gz
from tests.stage_support import AD1, AD2, _cli, _rc, _text_from, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 151


def _cases(rng, P):
    """[(tag, s1, s2)]: pairs made from a fragment of I bases -- R1 reads it forwards, R2 its reverse complement, each runs on into
    an adapter of its own where the fragment ends -- and changed by hand"""
    mo = P.min_overlap
    out = []

    def rs(n, alphabet=b"ACGT"):
        return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), n))

    def pair(I, L1=L, L2=L, frag=None):
        frag = rs(I) if frag is None else frag
        return (frag + rs(L1))[:L1], (_rc(frag) + rs(L2))[:L2]

    def other(b):
        return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + 1 + int(rng.integers(0, 3))) % 4]

    def spoiled(s1, s2, I, k, n1=0, n2=0, nn=0, byte=ord("N")):
        """k substitutions in R1, then n1 / n2 / nn positions of the overlap with `byte` in R1 / in R2 / in both, all distinct"""
        s1, s2 = bytearray(s1), bytearray(s2)
        pos = [int(i) for i in rng.permutation(np.arange(max(0, I - len(s2)), min(len(s1), I)))[:k + n1 + n2 + nn]]
        assert len(pos) == k + n1 + n2 + nn
        for i in pos[:k]:
            s1[i] = other(s1[i])
        for i in pos[k:k + n1] + pos[k + n1 + n2:]:
            s1[i] = byte
        for i in pos[k + n1:]:
            s2[I - 1 - i] = byte
        return bytes(s1), bytes(s2)

    def budget(I, L1=L, L2=L):
        ov = PM.overlap(I, L1, L2)
        return min(P.max_mismatches, ov * P.max_mismatch_pct // 100)

    for _ in range(6):
        out.append(("none", rs(L), rs(L)))
    out.append(("full", *pair(L)))
    out.append(("between", *pair(200)))
    out.append(("far-edge", *pair(2 * L - mo)))
    out.append(("far-edge+1", *pair(2 * L - mo + 1)))
    out.append(("M-1", *pair(L - 1)))
    out.append(("I=min", *pair(mo)))
    out.append(("I=min-1", *pair(mo - 1)))
    for I in (100, mo + 2, 200, 2 * L - mo):  # 100: the absolute cap binds under the defaults; mo + 2, 2L - mo: the percentage does
        b = budget(I)
        s1, s2 = pair(I)
        out.append(("budget@%d" % I, *spoiled(s1, s2, I, b)))
        out.append(("beyond@%d" % I, *spoiled(s1, s2, I, b + 1)))
        if b:
            out.append(("n1-in@%d" % I, *spoiled(s1, s2, I, b - 1, n1=1)))
            out.append(("n2-in@%d" % I, *spoiled(s1, s2, I, b - 1, n2=1)))
            out.append(("nn-in@%d" % I, *spoiled(s1, s2, I, b - 1, nn=1)))
        out.append(("n1-out@%d" % I, *spoiled(s1, s2, I, b, n1=1)))
        out.append(("n2-out@%d" % I, *spoiled(s1, s2, I, b, n2=1)))
        out.append(("nn-out@%d" % I, *spoiled(s1, s2, I, b, nn=1)))
        for byte in b".\x00 \x01@`\xc1\xe1":  # '@' and '`' differ in bit 5 only; 0xC1 and 0xE1 are 'A' and 'a' with bit 7 set
            out.append(("byte-out@%d" % I, *spoiled(s1, s2, I, b, nn=1, byte=byte)))
            out.append(("byte1-out@%d" % I, *spoiled(s1, s2, I, b, n1=1, byte=byte)))
        out.append(("lower1@%d" % I, s1.lower(), s2))
        out.append(("lower2@%d" % I, s1, s2.lower()))
        x1, x2 = spoiled(s1, s2, I, b)
        out.append(("lower-budget@%d" % I, x1.lower(), x2.lower()))
    out.append(("uneven1", *pair(120, L, 100)))  # I between the lengths, both ways
    out.append(("uneven2", *pair(120, 100, L)))
    out.append(("uneven-long", *pair(140, 76, L)))
    unit = rs(10)
    while len(set(unit)) < 4 or unit[:5] == unit[5:]:
        unit = rs(10)
    out.append(("tandem-both", *pair(200, frag=unit * 20)))  # accepted at 200, 190, .. on both sides of M: nothing is cut
    out.append(("tandem-short", *pair(100, frag=unit * 10)))  # accepted at 100, 90, ..: the larger wins
    out.append(("poly", b"A" * L, b"T" * L))
    out.append(("poly-n", b"N" * L, b"N" * L))
    for L1, L2 in ((0, 0), (0, L), (L, 0), (mo - 1, mo - 1), (mo - 1, L), (L, mo - 1), (mo, mo), (1, 1)):
        s1, s2 = pair(max(L1, L2, 1), L1, L2)
        out.append(("short%d-%d" % (L1, L2), s1, s2))
    for I in (60, 99, 100, 101):  # (under a floor of 100: held back, and not)
        out.append(("floor@%d" % I, *pair(I)))
    out.append(("floor-uneven", *pair(60, L, 80)))
    for I in (300, 399, 400, 500, 800 - mo, 801 - mo):  # lines of 400 bases: the byte path
        out.append(("long@%d" % I, *pair(I, 400, 400)))
    out.append(("long-none", rs(400), rs(400)))
    out.append(("long-mixed1", *pair(120, 400, L)))
    out.append(("long-mixed2", *pair(300, L, 400)))
    s1, s2 = pair(350, 400, 400)
    out.append(("long-budget", *spoiled(s1, s2, 350, budget(350, 400, 400), nn=0)))
    out.append(("long-beyond", *spoiled(s1, s2, 350, budget(350, 400, 400), nn=1)))
    out.append(("long-lower", s1.lower(), s2))
    out.append(("huge@1100", *pair(1100, 600, 600)))  # I* >= 1024: the last bin
    out.append(("huge@1023", *pair(1023, 600, 600)))
    out.append(("huge@1024", *pair(1024, 600, 600)))
    for L1 in (300, 321, 330, 336):  # both sides of the staged-line limit of 21 words, by alignment
        for I in (200, L1 - 1, L1 + 40) + ((90, 250, 329, 330, 331, 400, 600) if L1 == 330 else ()):
            out.append(("limit%d" % L1, *pair(I, L1, L1)))
    for I in range(mo - 3, 2 * L - mo + 4, 5):  # inserts all along, a few substitutions
        s1, s2 = pair(I)
        out.append(("sweep", *(spoiled(s1, s2, I, int(rng.integers(0, 3))) if I > 8 else (s1, s2))))
    for _ in range(40):  # reads of any length
        L1, L2 = int(rng.integers(1, 260)), int(rng.integers(1, 260))
        out.append(("any", *pair(int(rng.integers(1, 400)), L1, L2)))
    return out


class Stage(object):
    def __init__(self, seed, P, n=None):
        rng = np.random.default_rng(seed)
        self.P = P
        cases = _cases(rng, P)
        cases = [cases[int(i)] for i in rng.permutation(len(cases))]
        if n is not None:
            while len(cases) < n:
                cases = cases + cases
            cases = cases[:n]
        self.cases, self.n = cases, len(cases)
        qual = lambda s: b"I" * len(s)  # noqa: E731
        self.t1, self.r1 = _text_from(rng, [(t, a, qual(a)) for t, a, _ in cases])
        self.t2, self.r2 = _text_from(rng, [(t, b, qual(b)) for t, _, b in cases])
        self._model = None

    def shortened(self, seed):
        """the same text under tables whose seq_len a 3' trimming has cut already"""
        rng = np.random.default_rng(seed)
        st = Stage.__new__(Stage)
        st.__dict__.update(self.__dict__)
        st.r1, st.r2, st._model = self.r1.copy(), self.r2.copy(), None
        for recs in (st.r1, st.r2):
            for j in range(st.n):
                if rng.integers(0, 2):
                    recs[j, 4] = int(rng.integers(0, int(recs[j, 4]) + 1))
        st.cases = [(t, a[:int(q1[4])], b[:int(q2[4])]) for (t, a, b), q1, q2 in zip(self.cases, st.r1, st.r2)]
        return st

    def model(self):
        """-> (the two tables as the stage leaves them, the 1040 values); computed once"""
        if self._model is None:
            table, o1, o2 = PM.new_table(), self.r1.copy(), self.r2.copy()
            for j, (_, a, b) in enumerate(self.cases):
                o1[j, 4], o2[j, 4] = PM.count(table, a, b, self.P)
            self._model = ((o1, o2), np.array(table, dtype=np.uint64))
        return self._model

    def run(self, eng):
        return eng.dev_pairtrim(self.t1, self.r1, self.t2, self.r2)


def _engine(P=None):
    eng = hb.Engine(0)
    if P is not None:
        eng.pairtrim_set(**P.keywords())
    return eng


def _check(stage, eng, before=None):
    got = stage.run(eng)
    want, table = stage.model()
    for r in (0, 1):
        assert got[r].shape == want[r].shape and got[r].dtype == np.uint32
        bad = np.argwhere(got[r] != want[r])
        assert not len(bad), [(r, int(j), stage.cases[int(j)][0], int(got[r][j, 4]), int(want[r][j, 4])) for j, _ in bad[:8]]
    values = eng.pairtrim_read()
    assert values.shape == (1040,) and values.dtype == np.uint64
    if before is not None:
        table = table + before
    bad = np.flatnonzero(values != table)
    assert not len(bad), [(int(i), int(values[i]), int(table[i])) for i in bad[:8]]
    return table


CONFIGS = {
    "defaults": dict(),
    "low_overlap": dict(min_overlap=8),  # short overlaps: the percentage binds
    "floor_100": dict(min_length=100),
    "exact": dict(min_overlap=20, max_mismatches=0, max_mismatch_pct=50),
    "loose": dict(min_overlap=40, max_mismatches=64, max_mismatch_pct=50, min_length=30),
    "pct_0": dict(min_overlap=120, max_mismatches=5, max_mismatch_pct=0, min_length=65535),
}


@pytest.fixture(scope="module")
def stages():
    return {name: Stage(2, PM.Params(**kw)) for name, kw in CONFIGS.items() if name in ("defaults", "low_overlap", "floor_100")}


def test_the_generated_inputs_hold_the_cases(stages):
    st = stages["defaults"]
    P = st.P
    assert 200 < st.n < 900
    for text, recs, k in ((st.t1, st.r1, 1), (st.t2, st.r2, 2)):
        assert all(text[int(q[3]):int(q[3]) + int(q[4])] == c[k] for q, c in zip(recs, st.cases))
        assert {int(q[3]) % 16 for q in recs if q[4]} == set(range(16))  # line starts at every residue mod 16
        assert {(int(q[3]) % 16 + 330 + 15) // 16 <= 21 for q in recs if q[4] == 330} == {True, False}
    by = {}
    for t, a, b in st.cases:
        by.setdefault(t, []).append((a, b))
    ins = lambda t, P=P: [PM.trim_pair(a, b, P) for a, b in by[t]]  # noqa: E731
    one = lambda t, P=P: ins(t, P)[0]  # noqa: E731
    assert all(x == (None, (L, L), (L, L)) for x in ins("none"))
    assert one("full") == (L, (L, L), (L, L)) and one("between")[0] == 200 and one("between")[1] == (L, L)
    assert one("far-edge")[0] == 2 * L - 30 and one("far-edge+1")[0] is None  # an overlap of 30 and of 29
    assert one("M-1") == (150, (150, 150), (150, 150))
    assert one("I=min") == (30, (30, 30), (30, 30)) and one("I=min-1")[0] is None
    for I, b in ((100, 5), (32, 5), (200, 5), (272, 5)):  # the absolute cap binds: 20 % of the overlap is 6 or more
        assert PM.overlap(I, L, L) * 20 // 100 > 5
        assert one("budget@%d" % I)[0] == I and one("beyond@%d" % I)[0] != I
        for t in ("n1", "n2", "nn"):
            assert one("%s-in@%d" % (t, I))[0] == I and one("%s-out@%d" % (t, I))[0] != I
        assert b"N" in by["n1-in@%d" % I][0][0] and b"N" not in by["n1-in@%d" % I][0][1] and b"N" in by["n2-in@%d" % I][0][1]
        a, b2 = by["nn-out@%d" % I][0]
        assert any(a[i] == b2[I - 1 - i] == ord("N") for i in range(max(0, I - L), min(L, I)))  # N opposite N
        assert all(x[0] != I for x in ins("byte-out@%d" % I)) and all(x[0] != I for x in ins("byte1-out@%d" % I))
        assert len(by["byte-out@%d" % I]) == 8 and {a[i] for a, _ in by["byte-out@%d" % I] for i in range(len(a))} >= set(b".\x00 \x01@`\xc1\xe1")
        assert one("lower1@%d" % I)[0] == one("lower2@%d" % I)[0] == one("lower-budget@%d" % I)[0] == I
        assert by["lower1@%d" % I][0][0].islower() and by["lower2@%d" % I][0][1].islower()
    low = stages["low_overlap"]
    lby = {}
    for t, a, b in low.cases:
        lby.setdefault(t, []).append((a, b))
    # the percentage binds: overlaps of 10 bases allow 2 mismatches, at I = 10 and at I = 2 L - 8
    for I in (10, 2 * L - 8):
        assert PM.overlap(I, L, L) in (8, 10) and PM.overlap(I, L, L) * 20 // 100 < 5
        assert PM.trim_pair(*lby["budget@%d" % I][0], low.P)[0] == I and PM.trim_pair(*lby["beyond@%d" % I][0], low.P)[0] != I
    assert one("uneven1") == (120, (120, 100), (120, 100)) and one("uneven2") == (120, (100, 120), (100, 120))
    assert one("uneven-long") == (140, (76, 140), (76, 140))
    a, b = by["tandem-both"][0]
    I = one("tandem-both")[0]
    assert L <= I < 200 and one("tandem-both")[1] == (L, L)
    assert any(PM.accepted(a.translate(PM.FOLD1), b.translate(PM.COMP2), x, P) for x in range(30, L))  # a shorter one matches too
    a, b = by["tandem-short"][0]
    assert one("tandem-short")[0] == 100 and PM.accepted(a.translate(PM.FOLD1), b.translate(PM.COMP2), 90, P)
    assert one("poly")[0] == L and one("poly-n")[0] is None
    assert one("short0-0") == (None, (0, 0), (0, 0)) and one("short29-29")[0] is None and one("short29-151")[0] is None
    assert one("short30-30")[0] == 30 and {len(a) for a, _ in by["short0-151"]} == {0}
    fl = stages["floor_100"]
    fby = {t: (a, b) for t, a, b in fl.cases}
    assert PM.trim_pair(*fby["floor@60"], fl.P) == (60, (60, 60), (100, 100)) and PM.trim_pair(*fby["floor@101"], fl.P)[2] == (101, 101)
    assert PM.trim_pair(*fby["floor-uneven"], fl.P) == (60, (60, 60), (100, 80))
    assert fl.model()[1][5] > 0 and fl.model()[1][11] > 0 and st.model()[1][5] == 0
    assert [one("long@%d" % I)[0] for I in (300, 399, 400, 500, 770, 771)] == [300, 399, 400, 500, 770, None]
    assert one("long@300")[1] == (300, 300) and one("long-none")[0] is None and {len(a) for a, _ in by["long@300"]} == {400}
    assert one("long-mixed1")[1] == (120, 120) and one("long-mixed2")[1] == (L, 300)
    assert one("long-budget")[0] == 350 and one("long-beyond")[0] != 350 and one("long-lower")[0] == 350
    assert one("huge@1100")[0] == 1100 and one("huge@1023")[0] == 1023 and one("huge@1024")[0] == 1024
    _, table = st.model()
    assert table[-1] == 2 and table[15 + 1023] == 1 and table[12] == st.n and 0 < table[14] < table[13] < st.n
    assert (table[[0, 6]] == st.n).all() and (table[[3, 4, 9, 10]] > 0).all() and np.count_nonzero(table[15:]) > 60
    assert table[15:].sum() == table[13]


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_stage_equals_the_model(torch_cuda, stages, name):
    st = stages[name] if name in stages else Stage(2, PM.Params(**CONFIGS[name]))
    with _engine(st.P) as eng:
        assert eng.pairtrim_get() == st.P.keywords()
        _check(st, eng)


def test_stage_on_tables_a_trim_has_shortened(torch_cuda, stages):
    st = stages["defaults"].shortened(5)
    assert sum(int(a[4]) < int(b[4]) for a, b in zip(st.r1, stages["defaults"].r1)) > 100
    assert not (st.model()[1] == stages["defaults"].model()[1]).all()
    with _engine(st.P) as eng:
        _check(st, eng)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1025])
def test_stage_pair_counts(torch_cuda, n):
    P = PM.Params()
    with _engine(P) as eng:
        st = Stage(3, P, n=n)
        assert st.n == n
        table = _check(st, eng)
        assert table[12] == n and table[0] == n and table[6] == n


def test_accumulation_reset_and_add(torch_cuda):
    P = PM.Params()
    a, b = Stage(20, P, n=300), Stage(21, P, n=65)
    with _engine(P) as eng, _engine(P) as other:
        ta = _check(a, eng)
        both = _check(b, eng, before=ta)
        eng.reset_counts()
        assert not eng.pairtrim_read().any() and eng.pairtrim_get() == P.keywords()
        tb = _check(b, eng)
        _check(a, other)
        eng.pairtrim_add(other.pairtrim_read())  # a second context's table folds in
        assert (eng.pairtrim_read() == both).all() and (both == ta + tb).all() and (other.pairtrim_read() == ta).all()
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.pairtrim_add(np.zeros(16, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        eng.pairtrim_set(on=False)  # off: the table is freed
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.pairtrim_read()
        assert ei.value.code == hb.QD_ERR_STATE
        eng.pairtrim_set(min_overlap=12)
        assert not eng.pairtrim_read().any()


def test_state_and_errors(torch_cuda):
    P = PM.Params(min_length=20)
    st = Stage(30, P, n=64)
    zero = dict(min_overlap=0, max_mismatches=0, max_mismatch_pct=0, min_length=0)
    with hb.Engine(0) as eng:
        for call in (eng.pairtrim_read, lambda: st.run(eng), lambda: eng.pairtrim_add(np.zeros(1040, np.uint64))):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        assert eng.pairtrim_get() == zero
        assert eng.lib.qd_pairtrim_set(eng._h, None) == 0 and eng.pairtrim_get() == zero  # NULL = off
        eng.pairtrim_set(**P.keywords())
        good = eng.pairtrim_get()
        assert good == P.keywords()
        for bad in (dict(min_overlap=7), dict(min_overlap=1001), dict(min_overlap=-1), dict(max_mismatches=-1), dict(max_mismatches=65),
                    dict(max_mismatch_pct=-1), dict(max_mismatch_pct=51), dict(min_length=-1), dict(min_length=65536)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.pairtrim_set(**bad)
            assert ei.value.code == hb.QD_ERR_INVALID, bad
            assert eng.pairtrim_get() == good  # a rejected call changes nothing
        for ok in (dict(min_overlap=8, max_mismatches=0, max_mismatch_pct=0), dict(min_overlap=1000, max_mismatches=64, max_mismatch_pct=50, min_length=65535)):
            eng.pairtrim_set(**ok)
        assert eng.pairtrim_get()["min_length"] == 65535
        eng.pairtrim_set(**P.keywords())
        for size in (1039, 1041, 16):
            out = np.zeros(size, dtype=np.uint64)
            assert eng.lib.qd_pairtrim_read(eng._h, hb._ptr(out), size) == hb.QD_ERR_INVALID
        want = _check(st, eng)
        # a bad table never becomes an address: refused on the host, nothing launched, the table as it was
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_pairtrim(st.t1, bad, st.t2, st.r2)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_pairtrim(st.t1, st.r1, st.t2, bad)
        assert ei.value.code == hb.QD_ERR_INVALID
        assert (eng.pairtrim_read() == want).all()
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))  # plan, barcodes and the 3' trimming leave the stage alone
        eng.set_barcodes(["ACGTACGTACGTACGT"])
        eng.trim_set(quality_cutoff=20)
        assert eng.pairtrim_get() == good and (eng.pairtrim_read() == want).all() and eng.trim_get()["min_overlap"] == 3


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
PAIR = "[trim]\npair_overlap : True\npair_min_overlap : 20\n"
BOTH = "[trim]\nadapter_R1 : %s\nadapter_R2 : %s\nquality_cutoff : 20\nmin_length : 25\npair_overlap : True\npair_max_mismatches : 3\n" % (AD1, AD2)
P_PAIR = PM.Params(min_overlap=20)
P_BOTH = PM.Params(max_mismatches=3, min_length=25)
T_BOTH = TM.Params(AD1, AD2, quality_cutoff=20, min_length=25)
T_BOTH_KW = dict(adapter_r1=AD1, adapter_r2=AD2, quality_cutoff=20, min_overlap=3, max_mismatch_pct=10, min_length=25)


def _inserts(g, i, sample, kind):
    """pairs that belong together: insert reads of 30 .. 151 bases of a fragment of 15 .. 330 bases (half of them shorter than a
    read: the adapters read through), a fifth unrelated, some with substitutions, N or lower case, half with a low-quality 3' tail"""
    rng, out = g.rng, []
    I = int(rng.integers(15, 151)) if rng.integers(0, 2) else int(rng.integers(151, 331))
    frag = g.rnd(I)
    for ad, src in ((AD1, frag), (AD2, _rc(frag.encode()).decode())):
        Lr = int(rng.integers(30, 152))
        s = SS._fragment_reads(g, i, Lr, ad, src)
        tail = int(rng.integers(0, min(Lr, 60))) if rng.integers(0, 2) else 0
        out.append((s.lower() if i % 11 == 0 else s, g.q(Lr - tail, 22, 42) + g.q(tail, 2, 24)))
    return out


def _dataset(d, seed, n_chunks, n, bgzf):
    """the malformed records shift the streams against each other: pairs that no longer belong together"""
    return SS._dataset(d, seed, n_chunks, n, bgzf, _inserts, lambda n: {"seq_R1": (n // 2, n - 2), "seq_R2": (n // 2 + 40,)})


def _write_conf(path, files, samples, trim=PAIR, **kw):
    SS._write_conf(path, files, samples, extra=trim, **kw)


def _oracle(conf, ref_dir, P=P_PAIR, trim=None):
    """the oracle's run of the conf without any trimming -> trimmed_outputs of the model"""
    SS._oracle_run(conf, ref_dir)
    return PM.trimmed_outputs(str(ref_dir), P, trim)


def _check_run(mine, ref, texts, table, P=P_PAIR, only=None, trim_table=None):
    SS._check_files(mine, texts, only)
    SS._check_main_report(mine, ref, only)  # as without trimming
    SS._check_report(mine, pr, table, P.keywords())
    SS._check_report(mine, tr, trim_table, T_BOTH_KW)


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF, run once with pair_overlap alone; the model over the oracle's outputs"""
    top = tmp_path_factory.mktemp("pairtrim_bgzf")
    files, samples = _dataset(str(top / "data"), 61, 2, 1500, bgzf=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, trim="")
    texts, table = _oracle(plain, top / "ref")
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, texts=texts, table=table, mine=top / "mine", ref=top / "ref", plain=plain)


def test_cli_pair_overlap_alone_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert t[12] == t[0] == t[6] < 3000 and 0 < t[14] < t[13] < t[12] and all(t[k] > 0 for k in (3, 4, 9, 10))
    assert np.count_nonzero(np.array(t[15:])) > 100
    _check_run(run["mine"], run["ref"], run["texts"], t)
    assert not os.path.exists(run["mine"] / qr.REPORT_NAME)


def test_cli_with_quality_cutoff_adapters_and_min_length(bgzf_run, tmp_path):
    run = bgzf_run
    texts, table, first = PM.trimmed_outputs(str(run["ref"]), P_BOTH, T_BOTH)
    assert all(first[r][k] > 0 for r in (0, 1) for k in range(8)) and table[14] > 0 and table[1] == first[0][2]
    conf = tmp_path / "both.txt"
    _write_conf(conf, run["files"], run["samples"], trim=BOTH)
    _cli(conf, tmp_path / "both")
    _check_run(tmp_path / "both", run["ref"], texts, table, P=P_BOTH, trim_table=first)


def test_cli_quality_report_counts_the_final_lengths(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "quality.txt"
    _write_conf(conf, run["files"], run["samples"], quality=True)
    _cli(conf, tmp_path / "quality")
    _check_run(tmp_path / "quality", run["ref"], run["texts"], run["table"])
    names = [s[0] for s in run["samples"]]
    with open(tmp_path / "quality" / qr.REPORT_NAME) as fh:
        got = fh.read()
    assert got == "\n".join(qr.report_lines(QM.table_from_outputs(str(tmp_path / "quality"), names), names)) + "\n"
    assert got != "\n".join(qr.report_lines(QM.table_from_outputs(str(run["ref"]), names), names)) + "\n"


def test_cli_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 62, 2, 1000, bgzf=False)
    _write_conf(tmp_path / "plain.txt", files, samples, trim="")
    texts, table = _oracle(tmp_path / "plain.txt", tmp_path / "ref")
    _write_conf(tmp_path / "conf.txt", files, samples)
    _cli(tmp_path / "conf.txt", tmp_path / "mine")
    _check_run(tmp_path / "mine", tmp_path / "ref", texts, table)


def test_cli_chunk_workers_and_write_flags(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n")
    _cli(conf, tmp_path / "workers")
    _check_run(tmp_path / "workers", run["ref"], run["texts"], run["table"])
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, False, False))
    _cli(conf, tmp_path / "flags")  # the table does not depend on what is written; the files are absent
    _check_run(tmp_path / "flags", run["ref"], run["texts"], run["table"], only=lambda f: "_pass_" in f)


def test_cli_two_ranks_sharded_and_whole_chunks(bgzf_run, tmp_path):
    """2 ranks on GPU 0 (tables through the rendezvous files): each a pair range of ONE shared BGZF chunk, then a chunk each"""
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


def test_cli_without_the_option_nothing_changes(bgzf_run, tmp_path):
    """a conf with a [trim] section, as written before the pair_* options existed, and the same with the options added but off"""
    run = bgzf_run
    before = BOTH.split("pair_overlap")[0]
    assert "pair_" not in before and "quality_cutoff" in before
    runs = {}
    for name, trim in (("before", before), ("off", before + "pair_overlap : False\npair_min_overlap : 12\npair_max_mismatches : 0\n")):
        conf = tmp_path / (name + ".txt")
        _write_conf(conf, run["files"], run["samples"], trim=trim)
        _cli(conf, tmp_path / name)
        assert not os.path.exists(tmp_path / name / pr.REPORT_NAME)
        runs[name] = {f: _gz(str(tmp_path / name / f)) if f.endswith(".gz") else open(tmp_path / name / f, "rb").read()
                      for f in sorted(os.listdir(tmp_path / name)) if f.endswith(".fastq.gz") or f == tr.REPORT_NAME}
    assert runs["before"] == runs["off"] and tr.REPORT_NAME in runs["off"] and len(runs["off"]) > 6  # byte for byte
    texts, table = TM.trimmed_outputs(str(run["ref"]), T_BOTH)  # ... and what the 3' trimming alone has always written
    assert sorted(texts) == sorted(f for f in runs["off"] if f != tr.REPORT_NAME)
    for f in texts:
        assert _gz(str(tmp_path / "off" / f)) == texts[f], f
    assert runs["off"][tr.REPORT_NAME].decode() == "\n".join(tr.report_lines(table, T_BOTH_KW)) + "\n"
