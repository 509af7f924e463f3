"""Overlap base correction on the MI355X (qd_paircorrect_*, quade_amd/csrc/quade_paircorrect.hip): both texts, byte for byte over
the WHOLE text (the bytes between and around the records included: what catches a wide store), and the 10 values of the table equal
tests/paircorrect_model.py's plain Python rule -- for the stage on its own with hand-given insert lengths (qd_dev_paircorrect: every
alignment, lengths on both sides of the staged-line limit, mismatches at the overlap's edges, in one dword and across a 16-byte
boundary, every kind of doubtful and trusted byte, a front-clipped table), for the hand-over of I* from the overlap kernel, for
batch edges, accumulation, state and errors, and through the command line (every output file, the new report and the overlap
trimming report against the models over the oracle's files; BGZF and ordinary gzip, other stages in front, the quality report of
the corrected text, chunk workers, write flags, ranks, and the option absent)."""
import os

import numpy as np
import pytest

from quade_amd import hip_backend as hb
from quade_amd import pair_correct_report as cr
from quade_amd import pair_trim_report as pr
from quade_amd import quality_report as qr
from tests import clip_model as KM
from tests import paircorrect_model as CM
from tests import pairtrim_model as PM
from tests import qstats_model as QM
from tests import stage_support as SS
from tests import trim_model as TM
from tests.run_support import _gz
from tests.stage_support import AD1, AD2, _cli, _rc, _text_from, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 29, 30, 31, 150, 151, 320, 321, 322, 336, 337, 400)  # slab and byte path on both sides of the limit of 21 words
GOOD, BAD = ord("I"), ord("#")  # Q40 and Q2
MO = 30  # the overlap stage's default min_overlap


def _lines(text, rec):
    """(sequence line, quality line) of a record through its table entry"""
    return text[int(rec[3]):int(rec[3]) + int(rec[4])], text[int(rec[5]):int(rec[5]) + int(rec[4])]


def model(t1, r1, t2, r2, inserts, P):
    """-> (text 1, text 2 as the stage leaves them, the 10 values): every pair's lines taken through the tables, corrected by the
    plain Python rule and written back into copies of the whole texts"""
    o1, o2, table = bytearray(t1), bytearray(t2), CM.new_table()
    for a, b, I in zip(r1, r2, inserts):
        (s1, q1), (s2, q2) = _lines(t1, a), _lines(t2, b)
        s1, q1, s2, q2 = CM.count(table, s1, q1, s2, q2, int(I), P)
        for out, rec, s, q in ((o1, a, s1, q1), (o2, b, s2, q2)):
            out[int(rec[3]):int(rec[3]) + len(s)] = s
            out[int(rec[5]):int(rec[5]) + len(q)] = q
    return bytes(o1), bytes(o2), np.array(table, dtype=np.uint64)


def _cases(rng):
    """[(tag, s1, q1, s2, q2, I)]: pairs made from a fragment of I bases (R1 reads it forwards, R2 its reverse complement), good
    qualities everywhere, then spoiled at chosen overlap positions; I is what the test hands to the stage"""
    out = []

    def rs(n):
        return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, n))

    def other(b):
        return b"ACGT"[(b"ACGT".index(bytes([b]).upper()) + 1 + int(rng.integers(0, 3))) % 4]

    def pair(I, L1, L2):
        frag = rs(I)
        return [bytearray((frag + rs(L1))[:L1]), bytearray(b"I" * L1), bytearray((_rc(frag) + rs(L2))[:L2]), bytearray(b"I" * L2)]

    def positions(I, L1, L2):
        return list(range(max(0, I - L2), min(L1, I)))

    KINDS = ("r2", "r1", "both-good", "both-bad", "r2-N", "r1-N", "r2-lower", "r1-lower", "r2-byte", "r1-byte", "trusted-N1", "trusted-N2",
             "trusted-lower1", "trusted-lower2", "match-lower", "bad-match", "edge-quals")

    def spoil(p, I, i, kind):
        """position i of R1 and its partner j of R2 (a matching pair of good calls so far) becomes a case of `kind`"""
        s1, q1, s2, q2 = p
        j = I - 1 - i
        if kind == "r2":  # R2 doubtful, another letter
            s2[j], q2[j] = other(s2[j]), BAD
        elif kind == "r1":
            s1[i], q1[i] = other(s1[i]), BAD
        elif kind == "both-good":  # unresolved
            s1[i] = other(s1[i])
        elif kind == "both-bad":
            s1[i], q1[i], q2[j] = other(s1[i]), BAD, 33 + 14
        elif kind == "r2-N":  # the doubtful byte may be anything
            s2[j], q2[j] = ord("N"), BAD
        elif kind == "r1-N":
            s1[i], q1[i] = ord("n"), 33 + 14
        elif kind == "r2-lower":
            s2[j], q2[j] = ord(chr(other(s2[j])).lower()), 10  # (a quality byte below 33)
        elif kind == "r1-lower":
            s1[i], q1[i] = ord(chr(other(s1[i])).lower()), BAD
        elif kind == "r2-byte":
            s2[j], q2[j] = int(rng.choice(list(b".\x00 @`\xc1\xe1*"))), BAD
        elif kind == "r1-byte":
            s1[i], q1[i] = int(rng.choice(list(b".\x00 @`\xc1\xe1*"))), 0
        elif kind == "trusted-N1":  # the trusted byte is no letter: nothing is written
            s1[i], q2[j] = ord("N"), BAD
        elif kind == "trusted-N2":
            s2[j], q1[i] = ord("N"), BAD
        elif kind == "trusted-lower1":  # trusted lower case: written upper case
            s1[i], s2[j], q2[j] = ord(chr(s1[i]).lower()), other(s2[j]), BAD
        elif kind == "trusted-lower2":
            s2[j], s1[i], q1[i] = ord(chr(s2[j]).lower()), other(s1[i]), BAD
        elif kind == "match-lower":  # lower case matches: nothing, whatever the qualities
            s1[i], q1[i] = ord(chr(s1[i]).lower()), BAD
        elif kind == "bad-match":
            q2[j] = BAD
        elif kind == "edge-quals":  # phred exactly G - 1 against B, or G against B + 1: unresolved
            s2[j] = other(s2[j])
            q1[i], q2[j] = (33 + 29, 33 + 14) if rng.integers(0, 2) else (33 + 30, 33 + 15)

    def add(tag, p, I):
        out.append((tag, bytes(p[0]), bytes(p[1]), bytes(p[2]), bytes(p[3]), I))

    def spoiled(tag, I, L1, L2, given=None):
        """the edges of the overlap, a run of adjacent positions (one dword, and across a 16-byte boundary of either line), a few anywhere"""
        p = pair(I, L1, L2)
        pos = positions(I, L1, L2)
        if pos:
            chosen = {pos[0], pos[-1]}
            at = int(rng.integers(0, len(pos)))
            chosen.update(pos[at:at + 20:1 + int(rng.integers(0, 2))])  # 10 to 20 adjacent bytes: some share a dword, some straddle a 16-byte word
            chosen.update(int(x) for x in rng.choice(pos, min(len(pos), 6), replace=False))
            for n, i in enumerate(sorted(chosen)):
                spoil(p, I, i, KINDS[(n + len(out)) % len(KINDS)])
        add(tag, p, I if given is None else given)

    for L in LENGTHS + (330,):  # equal lengths: I below M, at M, above M, at L1 + L2 - min_overlap
        for I in sorted({max(L // 2, 1), L - 1, L, L + 1, L + L // 2, 2 * L - MO, 2 * L - 1} - {0, -1}):
            if 0 < I <= 2 * L:
                spoiled("L%d@%d" % (L, I), I, L, L)
        spoiled("L%d-none" % L, max(L, 1), L, L, given=0)  # hand-given I without positions: 0 ...
        spoiled("L%d-one" % L, max(L, 1), L, L, given=min(1, 2 * L))  # ... 1 (the first bases only) ...
        spoiled("L%d-sum" % L, max(L, 1), L, L, given=2 * L)  # ... and L1 + L2
    for L1, L2 in ((151, 400), (400, 151), (321, 337), (337, 321), (336, 30), (30, 336), (151, 100), (100, 151), (1, 400), (322, 0), (0, 151), (320, 322)):
        M = max(L1, L2)
        for I in sorted({min(L1, L2), M - 1, M, M + 7, L1 + L2 - MO, (L1 + L2) // 2}):
            if 0 < I <= L1 + L2:
                spoiled("mixed%d-%d@%d" % (L1, L2, I), I, L1, L2)
    for _ in range(30):  # values the search would never return: unrelated reads under any I, every position a mismatch of some kind
        L1, L2 = int(rng.choice(LENGTHS)), int(rng.choice(LENGTHS))
        p = [bytearray(rs(L1)), bytearray(rng.choice([GOOD, BAD, 33 + 14, 33 + 30, 33 + 15, 33 + 29], L1).astype(np.uint8).tobytes()),
             bytearray(rs(L2)), bytearray(rng.choice([GOOD, BAD, 33 + 14, 33 + 30, 10, 200], L2).astype(np.uint8).tobytes())]
        add("never", p, int(rng.integers(0, L1 + L2 + 1)))
    return out


class Stage(object):
    def __init__(self, seed, P=None, n=None, cases=None):
        rng = np.random.default_rng(seed)
        self.P = P if P is not None else CM.Params()
        cases = _cases(rng) if cases is None else cases
        cases = [cases[int(i)] for i in rng.permutation(len(cases))]
        if n is not None:
            while len(cases) < n:
                cases = cases + cases
            cases = cases[:n]
        self.cases, self.n = cases, len(cases)
        self.t1, self.r1 = _text_from(rng, [(t, s1, q1) for t, s1, q1, _, _, _ in cases])
        self.t2, self.r2 = _text_from(rng, [(t, s2, q2) for t, _, _, s2, q2, _ in cases])
        self.inserts = np.array([c[5] for c in cases], dtype=np.uint64)
        self._model = None

    def front_clipped(self, seed):
        """the same texts under tables a 5' clip has moved: seq and qual start later, by up to 9 bases a read"""
        rng = np.random.default_rng(seed)
        st = Stage.__new__(Stage)
        st.__dict__.update(self.__dict__)
        st.r1, st.r2, st._model = self.r1.copy(), self.r2.copy(), None
        for recs in (st.r1, st.r2):
            for j in range(st.n):
                f = min(int(rng.integers(0, 10)), int(recs[j, 4]))
                recs[j, 3] += f
                recs[j, 5] += f
                recs[j, 4] -= f
        st.inserts = np.minimum(self.inserts, (st.r1[:, 4].astype(np.uint64) + st.r2[:, 4].astype(np.uint64)))
        return st

    def model(self):
        if self._model is None:
            self._model = model(self.t1, self.r1, self.t2, self.r2, self.inserts, self.P)
        return self._model

    def run(self, eng, inserts="given"):
        return eng.dev_paircorrect(self.t1, self.r1, self.t2, self.r2, self.inserts if isinstance(inserts, str) else inserts)


def _engine(P=None, pair=None):
    eng = hb.Engine(0)
    if P is not None:
        eng.paircorrect_set(**P.keywords())
    if pair is not None:
        eng.pairtrim_set(**pair.keywords())
    return eng


def _same_text(got, want, what):
    got = np.asarray(got, dtype=np.uint8)
    want = np.frombuffer(want, dtype=np.uint8)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


def _check(stage, eng, before=None, want=None):
    got = stage.run(eng) if want is None else want[0]
    w1, w2, table = stage.model() if want is None else want[1]
    _same_text(got[0], w1, "text 1")
    _same_text(got[1], w2, "text 2")
    values = eng.paircorrect_read()
    assert values.shape == (10,) and values.dtype == np.uint64
    if before is not None:
        table = table + before
    bad = np.flatnonzero(values != table)
    assert not len(bad), [(int(i), int(values[i]), int(table[i])) for i in bad[:8]]
    return table


@pytest.fixture(scope="module")
def stage():
    return Stage(2)


def test_the_generated_inputs_hold_the_cases(stage):
    st = stage
    assert 200 < st.n < 500
    for text, recs in ((st.t1, st.r1), (st.t2, st.r2)):
        assert {int(q[3]) % 16 for q in recs if q[4]} == set(range(16))  # sequence lines start at every residue mod 16
        assert {int(q[4]) for q in recs} >= set(LENGTHS)
        # 330 bytes fit a slab of 21 aligned words at offsets 0 .. 6 mod 16 only: both paths at one length, by alignment
        assert {(int(q[3]) % 16 + 330 + 15) // 16 <= 21 for q in recs if q[4] == 330} == {True, False}
        # packed back to back: the quality line starts within 5 bytes of the sequence line's end and the next header directly behind
        # it, so neighbouring lines share 16-byte words
        assert all(0 < int(q[5]) - int(q[3]) - int(q[4]) <= 5 for q in recs)
        assert all(0 < int(b[0]) - int(a[5]) - int(a[4]) <= 2 for a, b in zip(recs, recs[1:]))
    w1, w2, table = st.model()
    assert w1 != st.t1 and w2 != st.t2 and len(w1) == len(st.t1) and len(w2) == len(st.t2)
    assert table[CM.PAIRS] == st.n and table[CM.MISMATCHES] == table[CM.R1_BASES] + table[CM.R2_BASES] + table[CM.UNRESOLVED]
    assert table[CM.R1_BASES] > 300 and table[CM.R2_BASES] > 300 and table[CM.UNRESOLVED] > 300 and 0 < table[CM.OVERLAPPED] < st.n
    assert 0 < table[CM.R1_READS] < table[CM.CORRECTED_PAIRS] < table[CM.OVERLAPPED]
    Ls = {(int(a[4]), int(b[4]), int(I)) for a, b, I in zip(st.r1, st.r2, st.inserts)}
    for L in (151, 337, 400):  # I below M, at M, above M, at L1 + L2 - min_overlap, 0, 1 and L1 + L2
        assert {(L, L, I) for I in (L - 1, L, L + 1, 2 * L - MO, 0, 1, 2 * L)} <= Ls
    assert (151, 400, 400) in Ls and (400, 151, 151) in Ls and (321, 337, 337) in Ls  # one line staged, one too long
    # mismatches at the first and the last overlap position, in adjacent bytes, across a 16-byte boundary of the sequence line
    first = last = adjacent = boundary = 0
    for a, b, I in zip(st.r1, st.r2, st.inserts):
        (s1, _), (s2, _) = _lines(st.t1, a), _lines(st.t2, b)
        I = int(I)
        pos = [i for i in range(max(0, I - len(s2)), min(len(s1), I)) if not PM.matches(s1[i], s2[I - 1 - i])]
        if pos:
            first += pos[0] == max(0, I - len(s2))
            last += pos[-1] == min(len(s1), I) - 1
            adjacent += any(y == x + 1 for x, y in zip(pos, pos[1:]))
            boundary += any(y == x + 1 and (int(a[3]) + y) % 16 == 0 for x, y in zip(pos, pos[1:]))
    assert min(first, last, adjacent, boundary) > 30


def test_stage_equals_the_model_text_for_text(torch_cuda, stage):
    with _engine(stage.P) as eng:
        assert eng.paircorrect_get() == stage.P.keywords()
        _check(stage, eng)
        once = stage.model()
        again = eng.dev_paircorrect(once[0], stage.r1, once[1], stage.r2, stage.inserts)  # applying it twice equals applying it once
        _same_text(again[0], once[0], "text 1, twice")
        _same_text(again[1], once[1], "text 2, twice")


@pytest.mark.parametrize("kw", [dict(good_quality=15, bad_quality=14), dict(good_quality=93, bad_quality=0), dict(good_quality=31, bad_quality=1)])
def test_other_thresholds(torch_cuda, stage, kw):
    st = Stage.__new__(Stage)
    st.__dict__.update(stage.__dict__)
    st.P, st._model = CM.Params(**kw), None
    assert not (st.model()[2] == stage.model()[2]).all()
    with _engine(st.P) as eng:
        _check(st, eng)


def test_front_clipped_tables(torch_cuda, stage):
    st = stage.front_clipped(7)
    assert sum(int(a[3]) > int(b[3]) for a, b in zip(st.r1, stage.r1)) > 100 and st.model()[0] != stage.model()[0]
    with _engine(st.P) as eng:
        _check(st, eng)


def _handover_cases(rng, P):
    """the overlap tests' mix, with qualities: inserts on both sides of every edge of the search, a few spoiled positions of every
    resolvable and unresolvable kind, unequal reads, a repeat, the byte path and the staged-line limit"""
    out, L, mo = [], 151, P.min_overlap

    def rs(n):
        return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, n))

    def pair(I, L1=L, L2=L, frag=None, k=3):
        frag = rs(I) if frag is None else frag
        s1, s2 = bytearray((frag + rs(L1))[:L1]), bytearray((_rc(frag) + rs(L2))[:L2])
        q1, q2 = bytearray(b"I" * L1), bytearray(b"I" * L2)
        pos = list(range(max(0, I - L2), min(L1, I)))
        for n, i in enumerate(int(x) for x in rng.permutation(pos)[:k]):
            j, kind = I - 1 - i, (n + len(out)) % 4
            if kind == 0:
                s2[j], q2[j] = ord("N"), BAD
            elif kind == 1:
                s1[i], q1[i] = b"ACGT"[(b"ACGT".index(bytes([s1[i]])) + 1) % 4], BAD
            elif kind == 2:
                s1[i] = b"ACGT"[(b"ACGT".index(bytes([s1[i]])) + 2) % 4]
            else:
                s2[j], q2[j] = ord(chr(s2[j]).lower()), BAD  # lower case matches: no mismatch
        out.append(("I%d" % I, bytes(s1), bytes(q1), bytes(s2), bytes(q2), 0))

    for _ in range(6):
        pair(1, k=0)  # unrelated
    for I in (L, 200, 2 * L - mo, 2 * L - mo + 1, L - 1, mo, mo - 1, 100, mo + 2, 60, 99):
        pair(I)
        pair(I, k=6)  # beyond the budget of 5 at most: often no I*
    for L1, L2, I in ((L, 100, 120), (100, L, 120), (76, L, 140), (0, L, 1), (L, 0, 1), (mo, mo, mo), (mo - 1, L, 40), (1, 1, 1)):
        pair(I, L1, L2, k=2)
    unit = rs(10)
    pair(200, frag=unit * 20, k=0)
    pair(100, frag=unit * 10, k=1)
    for I in (300, 399, 400, 500, 800 - mo, 801 - mo):  # lines of 400 bases: the byte path
        pair(I, 400, 400)
    pair(120, 400, L)
    pair(300, L, 400)
    for L1 in (321, 322, 336, 337):  # both sides of the staged-line limit, by alignment
        for I in (200, L1 - 1, L1 + 40):
            pair(I, L1, L1)
            pair(I, L1, L1)
    for I in range(mo - 3, 2 * L - mo + 4, 7):
        pair(I, k=int(rng.integers(0, 4)))
    return out


def test_hand_over_from_the_overlap_kernel(torch_cuda):
    """inserts=None: the overlap kernel runs first and stores every pair's I*, which the model takes from pairtrim_model"""
    Pp = PM.Params()
    st = Stage(4, cases=_handover_cases(np.random.default_rng(40), Pp))
    want = np.array([PM.insert_size(*[_lines(t, q)[0] for t, q in ((st.t1, a), (st.t2, b))], Pp) or 0 for a, b in zip(st.r1, st.r2)], dtype=np.uint64)
    st.inserts = want
    M = np.maximum(st.r1[:, 4], st.r2[:, 4])
    assert sum(want == 0) > 15 and sum((want > 0) & (want < M)) > 30 and sum(want > M) > 30 and sum(want == M) > 3 and sum(want > 336) > 8
    table = st.model()[2]
    assert table[CM.R1_BASES] > 40 and table[CM.R2_BASES] > 40 and table[CM.UNRESOLVED] > 40
    pair_table = PM.new_table()
    for a, b in zip(st.r1, st.r2):
        PM.count(pair_table, _lines(st.t1, a)[0], _lines(st.t2, b)[0], Pp)
    with _engine(st.P, pair=Pp) as eng:
        got = st.run(eng, inserts=None)
        _check(st, eng, want=(got, st.model()))
        assert (eng.pairtrim_read() == np.array(pair_table, dtype=np.uint64)).all()  # that stage counted the pairs as it always does
        recs = eng.dev_pairtrim(st.t1, st.r1, st.t2, st.r2)  # ... and without the hand-over its results are what they were
        assert (eng.pairtrim_read() == 2 * np.array(pair_table, dtype=np.uint64)).all()
        assert all(int(o1[4]) == min(int(a[4]), int(I)) for o1, a, I, m in zip(recs[0], st.r1, want, M) if 0 < I < m)


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 1025])
def test_stage_pair_counts(torch_cuda, stage, n):
    with _engine(stage.P) as eng:
        st = Stage(3, n=n, cases=stage.cases)
        assert st.n == n
        table = _check(st, eng)
        assert table[CM.PAIRS] == n
        if n == 0:  # no pairs: the texts as they came
            got = eng.dev_paircorrect(b"@r\nAC\n+\nII\n", np.zeros((0, 6), np.uint32), b"", np.zeros((0, 6), np.uint32), np.zeros(0, np.uint64))
            assert bytes(got[0]) == b"@r\nAC\n+\nII\n" and got[1].size == 0


def test_accumulation_reset_and_add(torch_cuda, stage):
    a, b = Stage(20, n=300, cases=stage.cases), Stage(21, n=65, cases=stage.cases)
    with _engine(a.P) as eng, _engine(a.P) as other:
        ta = _check(a, eng)
        both = _check(b, eng, before=ta)
        eng.reset_counts()
        assert not eng.paircorrect_read().any() and eng.paircorrect_get() == a.P.keywords()
        tb = _check(b, eng)
        _check(a, other)
        eng.paircorrect_add(other.paircorrect_read())  # a second context's table folds in
        assert (eng.paircorrect_read() == both).all() and (both == ta + tb).all() and (other.paircorrect_read() == ta).all()
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.paircorrect_add(np.zeros(16, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        eng.paircorrect_set(on=False)  # off: the table is freed
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.paircorrect_read()
        assert ei.value.code == hb.QD_ERR_STATE
        eng.paircorrect_set(good_quality=20, bad_quality=3)
        assert not eng.paircorrect_read().any()


def test_state_and_errors(torch_cuda, stage):
    st = Stage(30, n=64, cases=stage.cases)
    zero = dict(good_quality=0, bad_quality=0)
    with hb.Engine(0) as eng:
        for call in (eng.paircorrect_read, lambda: st.run(eng), lambda: eng.paircorrect_add(np.zeros(10, np.uint64))):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        assert eng.paircorrect_get() == zero
        assert eng.lib.qd_paircorrect_set(eng._h, None) == 0 and eng.paircorrect_get() == zero  # NULL = off
        eng.paircorrect_set(**st.P.keywords())  # independent of the overlap stage at set time
        good = eng.paircorrect_get()
        assert good == dict(good_quality=30, bad_quality=14)
        for bad in (dict(good_quality=0, bad_quality=0), dict(good_quality=94), dict(good_quality=-1), dict(bad_quality=-1), dict(bad_quality=30),
                    dict(good_quality=10, bad_quality=10), dict(good_quality=10)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.paircorrect_set(**bad)
            assert ei.value.code == hb.QD_ERR_INVALID, bad
            assert eng.paircorrect_get() == good  # a rejected call changes nothing
        for ok in (dict(good_quality=1, bad_quality=0), dict(good_quality=93, bad_quality=92)):
            eng.paircorrect_set(**ok)
        eng.paircorrect_set(**st.P.keywords())
        for size in (9, 11, 1040):
            out = np.zeros(size, dtype=np.uint64)
            assert eng.lib.qd_paircorrect_read(eng._h, hb._ptr(out), size) == hb.QD_ERR_INVALID
        with pytest.raises(hb.QuadeHipError) as ei:  # the hand-over needs the overlap stage
            st.run(eng, inserts=None)
        assert ei.value.code == hb.QD_ERR_STATE
        want = _check(st, eng)
        # bad inputs never become addresses: refused on the host, nothing launched, the table as it was
        ins = st.inserts.copy()
        ins[7] = int(st.r1[7, 4]) + int(st.r2[7, 4]) + 1  # I > L1 + L2
        with pytest.raises(hb.QuadeHipError) as ei:
            st.run(eng, inserts=ins)
        assert ei.value.code == hb.QD_ERR_INVALID
        ins[7] -= 1
        st.run(eng, inserts=np.zeros_like(ins))  # (I == 0 everywhere is fine: pairs, and nothing else)
        want = want.copy()
        want[CM.PAIRS] += st.n
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_paircorrect(st.t1, bad, st.t2, st.r2, st.inserts)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_paircorrect(st.t1, st.r1, st.t2, bad, st.inserts)
        assert ei.value.code == hb.QD_ERR_INVALID
        with pytest.raises(ValueError):
            eng.dev_paircorrect(st.t1, st.r1, st.t2, st.r2, st.inserts[:-1])
        assert (eng.paircorrect_read() == want).all()
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))  # plan, barcodes and the other stages leave it alone
        eng.set_barcodes(["ACGTACGTACGTACGT"])
        eng.pairtrim_set()
        eng.pairtrim_set(on=False)
        with hb.Pipe(eng) as pipe:
            with pytest.raises(hb.QuadeHipError) as ei:  # the correction without the overlap stage: refused before anything is read
                pipe.run([])
            assert ei.value.code == hb.QD_ERR_STATE and "overlap trimming is off" in str(ei.value)
        assert eng.paircorrect_get() == good and (eng.paircorrect_read() == want).all()


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
PAIR = "[trim]\npair_overlap : True\npair_min_overlap : 20\n"
CORRECT = PAIR + "pair_correct : True\n"
P_PAIR = PM.Params(min_overlap=20)
P_CORR = CM.Params()
FRONT = ("[trim]\nadapter_R1 : %s\nadapter_R2 : %s\nquality_cutoff : 20\nmin_length : 25\nfront_clip_R1 : 3\nfront_clip_R2 : 5\n"
         "pair_overlap : True\npair_max_mismatches : 3\npair_correct : True\npair_correct_good_quality : 32\npair_correct_bad_quality : 10\n" % (AD1, AD2))
K_FRONT = KM.Params(front_clip=(3, 5), min_length=25)
T_FRONT = TM.Params(AD1, AD2, quality_cutoff=20, min_length=25)
PP_FRONT = PM.Params(max_mismatches=3, min_length=25)
PC_FRONT = CM.Params(good_quality=32, bad_quality=10)


def _inserts(g, i, sample, kind):
    """pairs that belong together: insert reads of 30 .. 151 bases of a fragment of 15 .. 330 bases (half of them shorter than a
    read: the adapters read through), a fifth unrelated; up to three overlap positions per pair hold a sequencing error -- the wrong
    call at Q2 against Q37 on the other read (in R1 or in R2), or both calls confident (unresolved), sometimes an N or lower case;
    half the reads with a low-quality 3' tail"""
    rng = g.rng
    I = int(rng.integers(15, 151)) if rng.integers(0, 2) else int(rng.integers(151, 331))
    frag = g.rnd(I)
    reads = []
    for ad, src in ((AD1, frag), (AD2, _rc(frag.encode()).decode())):
        Lr = int(rng.integers(30, 152))
        s = list((src + ad + g.rnd(151))[:Lr]) if i % 5 else list(g.rnd(Lr, "ACGTN"))
        tail = int(rng.integers(0, min(Lr, 60))) if rng.integers(0, 2) else 0
        reads.append([s, list(g.q(Lr - tail, 32, 42) + g.q(tail, 2, 24))])
    (s1, q1), (s2, q2) = reads
    pos = list(range(max(0, I - len(s2)), min(len(s1), I)))
    for p in (rng.permutation(pos)[:int(rng.integers(0, 4))] if i % 5 else []):
        p = int(p)
        j, what = I - 1 - p, int(rng.integers(0, 8))
        wrong = lambda c: "ACGT"[("ACGT".index(c.upper()) + 1 + int(rng.integers(0, 3))) % 4] if c.upper() in "ACGT" else "A"  # noqa: E731
        if what < 3:  # R1 is wrong and says so
            s1[p], q1[p], q2[j] = ("N" if what == 2 else wrong(s1[p])), "#", "F"
        elif what < 6:  # R2 is
            s2[j], q2[j], q1[p] = (wrong(s2[j]).lower() if what == 5 else wrong(s2[j])), "#", "F"
        else:  # both calls confident
            s1[p], q1[p], q2[j] = wrong(s1[p]), "F", "F"
    out = [("".join(s1), "".join(q1)), ("".join(s2), "".join(q2))]
    return [(s.lower(), q) for s, q in out] if i % 11 == 0 else out


def _dataset(d, seed, n_chunks, n, bgzf):
    """the malformed records shift the streams against each other: pairs that no longer belong together"""
    return SS._dataset(d, seed, n_chunks, n, bgzf, _inserts, lambda n: {"seq_R1": (n // 2, n - 2), "seq_R2": (n // 2 + 40,)})


def _write_conf(path, files, samples, trim=CORRECT, **kw):
    SS._write_conf(path, files, samples, extra=trim, **kw)


def _enough(table):
    """what keeps a run from passing vacuously, asserted on the model's own table before anything is compared"""
    assert table[CM.R1_BASES] >= 100 and table[CM.R2_BASES] >= 100 and table[CM.UNRESOLVED] >= 20, table
    assert table[CM.MISMATCHES] == table[CM.R1_BASES] + table[CM.R2_BASES] + table[CM.UNRESOLVED]


def _oracle(conf, ref_dir, P=P_PAIR, C=P_CORR):
    """the oracle's run of the conf without any [trim] -> corrected_outputs of the models"""
    SS._oracle_run(conf, ref_dir)
    texts, pair_table, table = CM.corrected_outputs(str(ref_dir), P, C)
    _enough(table)
    return texts, pair_table, table


def _check_run(mine, ref, texts, pair_table, table, P=P_PAIR, C=P_CORR, only=None):
    SS._check_files(mine, texts, only)
    SS._check_main_report(mine, ref, only)  # as without the stages
    SS._check_report(mine, cr, table, C.keywords())
    SS._check_report(mine, pr, pair_table, P.keywords())  # as without the correction


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF under batches of 1 000 pairs (corrected pairs on both sides of a carry), run once with
    pair_overlap and pair_correct; the models over the oracle's outputs"""
    top = tmp_path_factory.mktemp("paircorrect_bgzf")
    files, samples = _dataset(str(top / "data"), 71, 2, 1500, bgzf=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, trim="")
    texts, pair_table, table = _oracle(plain, top / "ref")
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, texts=texts, pair_table=pair_table, table=table, mine=top / "mine", ref=top / "ref")


def test_cli_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert t[CM.PAIRS] < 3000 and 0 < t[CM.CORRECTED_PAIRS] < t[CM.OVERLAPPED] < t[CM.PAIRS] and t[CM.OVERLAPPED] == run["pair_table"][13]
    plain, plain_table = PM.trimmed_outputs(str(run["ref"]), P_PAIR)
    assert plain_table == run["pair_table"] and plain != run["texts"] and sorted(plain) == sorted(run["texts"])
    assert all(len(plain[f]) == len(run["texts"][f]) for f in plain)  # no length changes, no pair is dropped
    _check_run(run["mine"], run["ref"], run["texts"], run["pair_table"], t)
    assert not os.path.exists(run["mine"] / qr.REPORT_NAME)


def test_cli_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 72, 2, 1100, bgzf=False)
    _write_conf(tmp_path / "plain.txt", files, samples, trim="")
    texts, pair_table, table = _oracle(tmp_path / "plain.txt", tmp_path / "ref")
    _write_conf(tmp_path / "conf.txt", files, samples)
    _cli(tmp_path / "conf.txt", tmp_path / "mine")
    _check_run(tmp_path / "mine", tmp_path / "ref", texts, pair_table, table)


def test_cli_behind_a_front_clip_adapters_and_a_quality_cutoff(bgzf_run, tmp_path):
    run = bgzf_run
    clipped, _ = KM.clipped_outputs(str(run["ref"]), K_FRONT)
    texts, pair_table, table, first = CM.corrected_outputs(KM.write_outputs(clipped, str(tmp_path / "clipped")), PP_FRONT, PC_FRONT, T_FRONT)
    _enough(table)
    assert all(first[r][k] > 0 for r in (0, 1) for k in range(8)) and table != run["table"] and pair_table[14] > 0
    conf = tmp_path / "front.txt"
    _write_conf(conf, run["files"], run["samples"], trim=FRONT)
    _cli(conf, tmp_path / "front")
    _check_run(tmp_path / "front", run["ref"], texts, pair_table, table, P=PP_FRONT, C=PC_FRONT)


def test_cli_quality_report_counts_the_corrected_text(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "quality.txt"
    _write_conf(conf, run["files"], run["samples"], quality=True)
    _cli(conf, tmp_path / "quality")
    _check_run(tmp_path / "quality", run["ref"], run["texts"], run["pair_table"], run["table"])
    names = [s[0] for s in run["samples"]]
    want = QM.table_from_outputs(KM.write_outputs(run["texts"], str(tmp_path / "corrected")), names)
    plain = QM.table_from_outputs(KM.write_outputs(PM.trimmed_outputs(str(run["ref"]), P_PAIR)[0], str(tmp_path / "uncorrected")), names)
    q30 = hb.QSTATS_COUNTERS.index("q30_bases")
    assert int(want[:, :, q30].sum()) > int(plain[:, :, q30].sum())  # every correction turns a doubtful call into a confident one
    with open(tmp_path / "quality" / qr.REPORT_NAME) as fh:
        got = fh.read()
    assert got == "\n".join(qr.report_lines(want, names)) + "\n"
    assert got != "\n".join(qr.report_lines(plain, names)) + "\n"


def test_cli_chunk_workers_and_write_flags(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n", flags=(True, False, True))
    _cli(conf, tmp_path / "workers")  # the tables do not depend on what is written; the files are absent
    _check_run(tmp_path / "workers", run["ref"], run["texts"], run["pair_table"], run["table"], only=lambda f: "_fail_" not in f)


def test_cli_two_ranks(bgzf_run, tmp_path):
    """2 ranks on GPU 0 (tables through the rendezvous files), a chunk each"""
    run = bgzf_run
    conf = tmp_path / "two.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n")
    _cli(conf, tmp_path / "two", ranks=2)
    _check_run(tmp_path / "two", run["ref"], run["texts"], run["pair_table"], run["table"])
    assert not [f for f in os.listdir(tmp_path / "two") if f.startswith(".quade_rdv")]


def test_cli_without_the_option_nothing_changes(bgzf_run, tmp_path):
    """pair_overlap alone, as written before the pair_correct options existed, and the same with the options added but off"""
    run = bgzf_run
    runs = {}
    for name, trim in (("before", PAIR), ("off", PAIR + "pair_correct : False\npair_correct_good_quality : 20\npair_correct_bad_quality : 3\n")):
        conf = tmp_path / (name + ".txt")
        _write_conf(conf, run["files"], run["samples"], trim=trim)
        _cli(conf, tmp_path / name)
        assert not os.path.exists(tmp_path / name / cr.REPORT_NAME)
        runs[name] = {f: _gz(str(tmp_path / name / f)) if f.endswith(".gz") else open(tmp_path / name / f, "rb").read()
                      for f in sorted(os.listdir(tmp_path / name)) if f.endswith(".fastq.gz") or f == pr.REPORT_NAME}
    assert runs["before"] == runs["off"] and pr.REPORT_NAME in runs["off"] and len(runs["off"]) > 6  # byte for byte
    texts, table = PM.trimmed_outputs(str(run["ref"]), P_PAIR)  # ... and what pair_overlap alone has always written
    assert sorted(texts) == sorted(f for f in runs["off"] if f != pr.REPORT_NAME)
    for f in texts:
        assert runs["off"][f] == texts[f], f
    assert runs["off"][pr.REPORT_NAME].decode() == "\n".join(pr.report_lines(table, P_PAIR.keywords())) + "\n"
