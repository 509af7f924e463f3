"""Post-trimming on the MI355X (qd_posttrim_*, quade_amd/csrc/quade_posttrim.hip): the record tables the stage writes and its 32
counters equal tests/posttrim_model.py's plain Python rule, exactly -- for the stage on its own (qd_dev_posttrim: alignments, lengths
on both sides of a round of the walk and of the staged-line limit, tails of every base at the rule's edges, trailing N, the crop and
the floor, accumulation, state and errors, all seven stages in one context) and through the command line (every output file against
the oracle's file passed through the chained models, alone and behind clip, [trim] and pair_overlap and in front of [filter]; chunk
workers, write flags, ranks, and a conf without the options)."""
import os

import numpy as np
import pytest

from quade_amd import clip_report as cr
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from quade_amd import pair_trim_report as pr
from quade_amd import posttrim_report as xr
from quade_amd import quality_report as qr
from quade_amd import trim_report as tr
from tests import clip_model as CM
from tests import filter_model as FM
from tests import pairtrim_model as PM
from tests import posttrim_model as XM
from tests import qstats_model as QM
from tests import trim_model as TM
from tests import stage_support as SS
from tests.run_support import _compare_dirs, _gz
from tests.stage_support import (AD1, AD2, BASES, FILTER, P_F, P_PAIR, P_TRIM, TRIM_KW, TRIMS, _barcodes, _cli, _rc, _read, _text_from,  # noqa: F401
                                 torch_cuda)

pytestmark = pytest.mark.gpu

POLY = (6, 10, 100)
# a round of the walk (64), the slab's bound at every alignment (320 .. 337: 21 words hold 321 bytes at any offset and 336 at
# the best) and the byte path (400, 1000)
FIXED_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 128, 129, 320, 321, 322, 336, 337, 400, 1000)


def _lens(P):
    return tuple(sorted(set(FIXED_LENS + (P - 1, P, P + 1))))


@pytest.fixture(scope="module")
def eng():
    """the one context of this module's stage tests"""
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    with hb.Engine(0) as e:
        yield e


def _rs(rng, L, alphabet=b"ACGT"):
    return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))


def _case(tag, seq):
    return (tag, bytes(seq), b"I" * len(seq))  # the stage never reads the quality line


def _other(X):
    """a body that holds no X (upper or lower), so that a tail ends where it was planted"""
    return bytes(b for b in b"ACGT" if b != (X & 0xDF))


def _length_cases(rng, P):
    """every length: random reads over every kind of byte, reads that end in a tail or in N, and reads of one base throughout"""
    out = []
    for L in _lens(P):
        for rep in range(3 if L < 400 else 1):
            X = b"ACGTacgt"[int(rng.integers(0, 8))]
            t = int(rng.integers(0, L + 1))
            out.append(_case("random", _rs(rng, L, BASES)))
            out.append(_case("tail", _rs(rng, L - t, _other(X)) + bytes([X]) * t))
            out.append(_case("all", bytes([X]) * L))
            k = int(rng.integers(0, min(L, 20) + 1))
            out.append(_case("n-tail", _rs(rng, L - k, b"ACGTN") + _rs(rng, k, b"Nn")))
    return out


def _tail(rng, L, X, G, t_mis=(), with_byte=None):
    """L bases that end in G times X, a body without X in front; t_mis: positions counted from the 3' end that hold another byte"""
    s = bytearray(_rs(rng, L - G, _other(X)) + bytes([X]) * G)
    for t in t_mis:
        s[L - t] = with_byte if with_byte is not None else _other(X)[0]
    return bytes(s)


def _tail_cases(rng, P):
    out = []
    for X in b"ACGTacgt":
        for G in (P - 1, P, P + 1, 63, 64, 65, 130):  # the minimum run, a round of the walk and two of them
            out.append(_case("run%d" % G, _tail(rng, 151, X, G)))
        for L in (P, 64, 151, 330, 400):  # the whole read
            out.append(_case("whole", bytes([X]) * L))
        # mismatches at the 8 mm > t edge of a 60-base tail: one at t = 7, one at t = 8, five inside 40 (all forgiven), the sixth
        out.append(_case("one@7", _tail(rng, 151, X, 60, (7,))))
        out.append(_case("one@8", _tail(rng, 151, X, 60, (8,))))
        out.append(_case("five", _tail(rng, 151, X, 60, (9, 17, 25, 33, 40))))
        out.append(_case("six", _tail(rng, 151, X, 60, (9, 17, 25, 33, 41, 49))))
        for t in (15, 16, 17):
            out.append(_case("two@%d" % t, _tail(rng, 151, X, 60, (8, t))))
        out.append(_case("n-inside", _tail(rng, 151, X, 60, (3, 12, 13), with_byte=ord("N"))))  # N is a mismatch like any other
        out.append(_case("long", _tail(rng, 330, X, 200, (70,))))
        out.append(_case("long", _tail(rng, 1000, X, 700, (70, 300))))
    body = _rs(rng, 100, b"CG")
    out.append(_case("a-behind-t", body + b"T" * 20 + b"A" * 20))  # one pass only: the A run goes, the T run stays
    out.append(_case("t-behind-a", body + b"A" * 20 + b"T" * 20))
    out.append(_case("a-behind-t", body + b"t" * 64 + b"a" * 64))
    return out


def _ntail_cases(rng, P):
    """trailing N of 0, 1, 15, 16, 17, 64 and L bytes, alone and in front of (on the 3' side of) a poly tail"""
    out = []
    for k in (0, 1, 15, 16, 17, 64):
        for L in (k, 151, 330, 400):
            if L >= k:
                out.append(_case("n%d" % k, _rs(rng, L - k, b"ACGT") + _rs(rng, k, b"Nn")))
                if L - k >= 40:
                    X = b"ACGT"[int(rng.integers(0, 4))]
                    out.append(_case("n%d+tail" % k, _tail(rng, L - k, X, 30) + _rs(rng, k, b"Nn")))
    for L in (1, 16, 65, 151, 330, 400, 1000):
        out.append(_case("n-all", b"N" * L))
    out.append(_case("n-inside", _rs(rng, 100, b"ACGT") + b"NNNNACNN"))
    return out


def _noisy_cases(rng, P, n=6):
    """reads with noisy tails of every base and N behind them: every rule cuts, in every length class"""
    out = []
    for L in _lens(P):
        for _ in range(n if L < 400 else 2):
            X = b"ACGT"[int(rng.integers(0, 4))]
            k = int(rng.integers(0, min(L, 6) + 1)) if rng.integers(0, 2) else 0
            G = int(rng.integers(0, min(L - k, 2 * P + 20) + 1))
            tail = _rs(rng, G, bytes([X]) * 14 + bytes([X | 0x20]) + b"N" + _other(X)[:1])
            out.append(_case("noisy", _rs(rng, L - k - G, b"ACGTNa") + tail + _rs(rng, k, b"NNn")))
    return out


class Stage(object):
    """R1 and R2 drawn apart: each stream has its own cases in its own order (a pair's two reads differ), the shorter list filled up
    with random reads."""

    def __init__(self, seed, P, lists, n=None):
        rng = np.random.default_rng(seed)
        self.P = P
        lists = [list(x) for x in lists]
        m = max(len(x) for x in lists)
        for x in lists:
            while len(x) < m:
                x.append(_case("fill", _rs(rng, int(FIXED_LENS[int(rng.integers(0, len(FIXED_LENS) - 2))]), BASES)))
        self.cases = [[x[int(i)] for i in rng.permutation(m)] for x in lists]
        if n is not None:
            while len(self.cases[0]) < n:
                self.cases = [c + c for c in self.cases]
            self.cases = [c[:n] for c in self.cases]
        self.n = len(self.cases[0])
        (self.t1, self.r1), (self.t2, self.r2) = (_text_from(rng, c) for c in self.cases)

    def model(self, P=None):
        """-> (the tables the stage leaves, counters uint64[2, 16])"""
        P = P or self.P
        table, outs = XM.new_table(), []
        for r, recs in enumerate((self.r1, self.r2)):
            o = recs.copy()
            for j, (_, seq, _q) in enumerate(self.cases[r]):
                o[j, 4] = XM.count(table, seq, r, P)
            outs.append(o)
        return outs, np.array(table, dtype=np.uint64)

    def run(self, eng):
        return eng.dev_posttrim(self.t1, self.r1, self.t2, self.r2)


def _check(stage, eng, before=None, P=None):
    got = stage.run(eng)
    want, table = stage.model(P)
    for r in (0, 1):
        assert got[r].shape == want[r].shape and got[r].dtype == np.uint32
        bad = np.argwhere(got[r] != want[r])
        assert not len(bad), [(r, int(j), stage.cases[r][int(j)][0], len(stage.cases[r][int(j)][1]), got[r][j].tolist(), want[r][j].tolist())
                              for j, _ in bad[:6]]
        src = stage.r1 if r == 0 else stage.r2
        assert (np.delete(got[r], 4, axis=1) == np.delete(src, 4, axis=1)).all()  # only seq_len changes
    counters = eng.posttrim_read()
    assert counters.shape == (2, 16) and counters.dtype == np.uint64
    if before is not None:
        table = table + before
    assert (counters == table).all(), (counters.tolist(), table.tolist())
    return table


def _set(eng, P):
    eng.posttrim_set(**P.keywords())
    assert eng.posttrim_get() == P.keywords() and eng.posttrim_active()


def test_the_generated_inputs_hold_the_cases():
    rng = np.random.default_rng(1)
    P = 10
    by = {}
    for tag, s, _ in _tail_cases(rng, P):
        by.setdefault(tag, []).append(s)
    px = lambda s: XM.poly_x(s, P)  # noqa: E731
    assert [px(s)[0] for s in by["run9"]] == [151 - 9] * 8  # the base in front of 9 X is the one mismatch the rule forgives
    assert [px(s)[0] for s in by["run10"]] == [141] * 8 and [px(s)[0] for s in by["run130"]] == [21] * 8
    assert [px(s)[1] for s in by["run64"]] == [bytes([X & 0xDF]) for X in b"ACGTacgt"]  # lower case matches
    assert [px(s)[0] for s in by["one@7"]] == [91] * 8 and [px(s)[0] for s in by["five"]] == [91] * 8
    assert [px(s)[0] for s in by["six"]] == [151 - 48] * 8 and [px(s)[0] for s in by["n-inside"]] == [151 - 11] * 8
    p6 = {}
    for tag, s, _ in _tail_cases(rng, 6):
        p6.setdefault(tag, []).append(s)
    assert [XM.poly_x(s, 6)[0] for s in p6["one@7"]] == [151 - 6] * 8 and [XM.poly_x(s, 6)[0] for s in p6["one@8"]] == [91] * 8  # 8 x 1 > 7
    assert [px(s)[0] for s in by["two@15"]] == [151 - 14] * 8 and [px(s)[0] for s in by["two@16"]] == [91] * 8
    assert [px(s) for s in by["whole"][:5]] == [(0, b"A")] * 5 and {len(s) for s in by["whole"]} == {10, 64, 151, 330, 400}
    assert [px(s) for s in by["a-behind-t"]] == [(120, b"A"), (164, b"A")] and px(by["t-behind-a"][0]) == (120, b"T")
    assert [px(s)[0] for s in by["long"][:2]] == [130, 300]
    nt = {}
    for tag, s, _ in _ntail_cases(rng, P):
        nt.setdefault(tag, []).append(s)
    assert all(XM.tail_n(s) == len(s) - k for k in (0, 1, 15, 16, 17, 64) for s in nt["n%d" % k] + nt["n%d+tail" % k])
    PN = XM.Params(tail_n=1, poly_x_min_length=P)
    assert all(XM.posttrim_read(s, 0, PN)[1] == len(s) - 64 - 30 for s in nt["n64+tail"])  # the tail shows once the N are gone
    assert all(XM.posttrim_read(s, 0, XM.Params(poly_x_min_length=P))[1] == len(s) for s in nt["n64+tail"] + nt["n15+tail"])
    assert [XM.tail_n(s) for s in nt["n-all"]] == [0] * 7 and XM.tail_n(nt["n-inside"][0]) == 106
    Pn = XM.Params(1, P, (100, 60), 20)
    table = XM.new_table()
    noisy = _noisy_cases(rng, P)
    for _, s, _q in noisy:
        XM.count(table, s, 0, Pn)
        XM.count(table, s, 1, Pn)
    assert all(v > 0 for r in (0, 1) for v in table[r])  # every counter is exercised
    st = Stage(5, Pn, (noisy + _length_cases(rng, P), noisy[::-1]))
    for text, recs in ((st.t1, st.r1), (st.t2, st.r2)):
        assert {int(q[3]) % 16 for q in recs if q[4]} == set(range(16))
        # lines on both sides of the staged-line limit (21 aligned words; the upload moves the text by 3 bytes)
        assert {((int(q[3]) + 3) % 16 + int(q[4]) + 15) // 16 <= 21 for q in recs if 321 < q[4] <= 336} == {True, False}
        assert b"\r\n" in text
    assert {len(s) for _, s, _ in st.cases[0]} >= set(_lens(P))


@pytest.mark.parametrize("P", POLY)
def test_lengths_and_tails_equal_the_model(eng, P):
    rng = np.random.default_rng(100 + P)
    Pm = XM.Params(poly_x_min_length=P)
    _set(eng, Pm)
    table = _check(Stage(200 + P, Pm, (_tail_cases(rng, P) + _length_cases(rng, P), _length_cases(rng, P) + _tail_cases(rng, P))), eng)
    assert (table[:, [5, 7, 9, 11]] > 10).all() and (table[:, [3, 4, 13, 14, 15]] == 0).all()


@pytest.mark.parametrize("P", POLY)
def test_trailing_n_alone_and_in_front_of_a_tail_equals_the_model(eng, P):
    rng = np.random.default_rng(300 + P)
    cases = _ntail_cases(rng, P) + _length_cases(rng, P)
    st = Stage(400 + P, None, (cases, cases[::-1] + _noisy_cases(rng, P, 2)))
    for Pm in (XM.Params(tail_n=1), XM.Params(tail_n=1, poly_x_min_length=P), XM.Params(poly_x_min_length=P)):
        _set(eng, Pm)  # (posttrim_set zeroed the table)
        table = _check(st, eng, P=Pm)
        assert (table[:, 3] > 20).all() if Pm.tail_n else (table[:, 3:5] == 0).all()
        assert (table[:, [5, 7, 9, 11]].sum(axis=1) > 10).all() if Pm.poly_x_min_length else (table[:, 5:13] == 0).all()


@pytest.mark.parametrize("min_length", [0, 20, 400])
def test_crop_and_the_floor_equal_the_model(eng, min_length):
    rng = np.random.default_rng(500 + min_length)
    L = 151
    cases = [_case("fixed", _rs(rng, L, BASES)) for _ in range(20)] + _noisy_cases(rng, 10, 2)
    st = Stage(600 + min_length, None, (cases, cases[::-1]))
    for k, M in enumerate((1, 16, 17, L - 1, L, L + 1)):
        other = (0, 65535, 64)[k % 3]
        for Pm in (XM.Params(max_length=(M, other), min_length=min_length),
                   XM.Params(tail_n=1, poly_x_min_length=10, max_length=(other, M), min_length=min_length)):
            _set(eng, Pm)
            table = _check(st, eng, P=Pm)
            r = 0 if Pm.max_length[0] == M else 1
            assert table[r, 13] >= (10 if M < L else 1)  # the 151-base reads are cropped below 151, the longest reads always
            assert table[r, 14] > 0 and (table[1 - r, 13] > 0) == (other == 64)
            if not Pm.tail_n:  # the crop alone: the floor gives back what the crop took exactly where it lies above the crop
                assert (table[r, 15] > 0) == (min_length > M) and (table[:, 3:13] == 0).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_stage_pair_counts(eng, n):
    P = XM.Params(tail_n=1, poly_x_min_length=10, max_length=(120, 0), min_length=5)
    rng = np.random.default_rng(700 + n)
    _set(eng, P)
    st = Stage(800 + n, P, (_noisy_cases(rng, 10, 3), _noisy_cases(rng, 10, 3)), n=n)
    assert st.n == n
    assert (_check(st, eng)[:, 0] == n).all()


def test_accumulation_reset_and_add(eng):
    P = XM.Params(tail_n=1, poly_x_min_length=10, max_length=(0, 100), min_length=10)
    rng = np.random.default_rng(20)
    a = Stage(21, P, (_noisy_cases(rng, 10, 3), _noisy_cases(rng, 10, 3)), n=300)
    b = Stage(22, P, (_noisy_cases(rng, 10, 2), _noisy_cases(rng, 10, 2)), n=65)
    _set(eng, P)
    with hb.Engine(0) as other:
        other.posttrim_set(**P.keywords())
        ta = _check(a, eng)
        both = _check(b, eng, before=ta)
        eng.reset_counts()
        assert not eng.posttrim_read().any() and eng.posttrim_get() == P.keywords()
        tb = _check(b, eng)
        _check(a, other)
        eng.posttrim_add(other.posttrim_read())  # a second context's counters fold in
        assert (eng.posttrim_read() == both).all() and (both == ta + tb).all() and (other.posttrim_read() == ta).all()
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.posttrim_add(np.zeros(24, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
    eng.posttrim_set()  # all off: the table is freed
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.posttrim_read()
    assert ei.value.code == hb.QD_ERR_STATE
    eng.posttrim_set(tail_n=1)
    assert not eng.posttrim_read().any()
    eng.posttrim_set()


def test_state_and_errors(eng):
    P = XM.Params(tail_n=1, poly_x_min_length=10, max_length=(100, 0), min_length=5)
    rng = np.random.default_rng(30)
    st = Stage(31, P, (_noisy_cases(rng, 10, 2), _noisy_cases(rng, 10, 2)), n=64)
    off = XM.Params().keywords()
    eng.posttrim_set()
    assert not eng.posttrim_active() and eng.posttrim_get() == off
    for call in (eng.posttrim_read, lambda: st.run(eng), lambda: eng.posttrim_add(np.zeros((2, 16), np.uint64))):
        with pytest.raises(hb.QuadeHipError) as ei:
            call()
        assert ei.value.code == hb.QD_ERR_STATE
    assert eng.lib.qd_posttrim_set(eng._h, None) == 0 and not eng.posttrim_active()  # NULL = off
    eng.posttrim_set(min_length=30)  # no rule: off, whatever the floor says
    assert not eng.posttrim_active() and eng.posttrim_get() == off
    _set(eng, P)
    good = eng.posttrim_get()
    for bad in (dict(tail_n=2), dict(tail_n=-1), dict(poly_x_min_length=5), dict(poly_x_min_length=101), dict(poly_x_min_length=-1),
                dict(max_length_r1=-1), dict(max_length_r2=65536), dict(max_length_r1=65536), dict(tail_n=1, min_length=65536),
                dict(tail_n=1, min_length=-1)):
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.posttrim_set(**bad)
        assert ei.value.code == hb.QD_ERR_INVALID, bad
        assert eng.posttrim_get() == good and eng.posttrim_active()  # a rejected call changes nothing
    want = _check(st, eng)  # ... and the previous parameters are still in force
    for ok in (dict(tail_n=1), dict(poly_x_min_length=6), dict(poly_x_min_length=100, min_length=65535), dict(max_length_r1=1),
               dict(max_length_r2=65535), dict(max_length_r1=1, min_length=400)):
        eng.posttrim_set(**ok)
        assert eng.posttrim_active()
    assert eng.posttrim_get() == dict(off, max_length_r1=1, min_length=400)
    _set(eng, P)
    out = np.zeros(31, dtype=np.uint64)
    assert eng.lib.qd_posttrim_read(eng._h, hb._ptr(out), 31) == hb.QD_ERR_INVALID
    want = _check(st, eng)
    # a bad table never becomes an address: refused on the host, nothing launched, the counters as they were
    bad = st.r1.copy()
    bad[5, 4] = len(st.t1)  # a sequence range beyond the text
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.dev_posttrim(st.t1, bad, st.t2, st.r2)
    assert ei.value.code == hb.QD_ERR_INVALID
    bad = st.r2.copy()
    bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.dev_posttrim(st.t1, st.r1, st.t2, bad)
    assert ei.value.code == hb.QD_ERR_INVALID
    assert (eng.posttrim_read() == want).all()
    eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))  # plan and barcodes leave the stage alone
    eng.set_barcodes(["ACGTACGTACGTACGT"])
    assert eng.posttrim_get() == good and (eng.posttrim_read() == want).all()
    eng.posttrim_set()


def test_all_seven_stages_in_one_context(torch_cuda):
    """every stage of hb.RUN_STAGES on and run over one small batch: a posttrim_add reaches its own table and no other, and a table
    one value short is refused and changes nothing"""
    rng = np.random.default_rng(40)
    S, n = 2, 17
    cases = [[_case("pair", _rs(rng, 10, b"CGT") + (b"A" * 10 if j % 3 == 0 else _rs(rng, 10)) + (b"N" if j % 4 == 1 else b"")) for j in range(n)]
             for _ in range(2)]
    (t1, r1), (t2, r2) = (_text_from(rng, c) for c in cases)
    codes = np.array([(0, 3, 0xFFFF)[j % 3] for j in range(n)], dtype=np.uint16)
    P = XM.Params(tail_n=1, poly_x_min_length=6, max_length=(18, 0), min_length=4)
    with hb.Engine(0) as e:
        e.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        e.set_barcodes(_barcodes(S))
        e.qstats_enable(True)
        e.cstats_enable(True)
        e.clip_set(tail_clip_r1=1, min_length=5)
        e.trim_set("AGATCGGAAG", "AGATCGGAAG", 20, 3, 10, 4)
        e.pairtrim_set(min_overlap=8, max_mismatches=2, max_mismatch_pct=20, min_length=6)
        e.posttrim_set(**P.keywords())
        e.filter_set(min_length=18, max_n=1)
        assert [s.name for s in hb.RUN_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter"]
        for s in hb.RUN_STAGES:
            args = (t1, r1, t2, r2) + ((codes,) if s.engine in ("qstats", "cstats", "filter") else ())
            getattr(e, "dev_" + s.engine)(*args)
        read_all = lambda: {s.name: np.asarray(s.read(e)).reshape(-1).copy() for s in hb.RUN_STAGES}  # noqa: E731
        t0 = read_all()
        want = XM.new_table()
        for r in (0, 1):
            for _, seq, _q in cases[r]:
                XM.count(want, seq, r, P)
        assert t0["posttrim"].size == 32 and (t0["posttrim"] == np.array(want, dtype=np.uint64).reshape(-1)).all()
        assert all(t.any() for t in t0.values()) and want[0][5] > 0 and want[0][3] > 0 and want[0][13] > 0
        e.posttrim_add(np.full(32, 7, dtype=np.uint64))
        now = read_all()
        assert (now["posttrim"] == t0["posttrim"] + np.uint64(7)).all()
        assert all((now[k] == t0[k]).all() for k in t0 if k != "posttrim")
        short = np.zeros(31, dtype=np.uint64)
        with pytest.raises(hb.QuadeHipError) as ei:
            e._chk(e.lib.qd_posttrim_read(e._h, hb._ptr(short), short.size))
        assert ei.value.code == hb.QD_ERR_INVALID
        with pytest.raises(hb.QuadeHipError) as ei:
            e.posttrim_add(short + np.uint64(1))
        assert ei.value.code == hb.QD_ERR_INVALID
        for name, size in (("clip", 24), ("trim", 16)):  # ... nor does a neighbour's size pass for this stage's
            with pytest.raises(hb.QuadeHipError) as ei:
                e.posttrim_add(np.ones(size, dtype=np.uint64))
            assert ei.value.code == hb.QD_ERR_INVALID
        after = read_all()
        assert all((after[k] == now[k]).all() for k in now)


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
POST = "tail_n : True\npoly_x : True\nmax_length_R1 : 100\nmax_length_R2 : 90\nmin_length : 25\n"
P_POST = XM.Params(tail_n=1, poly_x_min_length=10, max_length=(100, 90), min_length=25)
CLIP = "front_clip_R2 : 5\ntail_clip_R1 : 1\nwindow_size : 4\nwindow_quality : 18\npoly_g : True\n"
P_CLIP = CM.Params(front_clip=(0, 5), tail_clip=(1, 0), window_size=4, window_quality=18, poly_g_min_length=10, min_length=25)


def _inserts(g, i, sample, kind):
    """the filter tests' fragments (stage_support._filter_inserts) with what this stage is for: a quarter of the reads are an insert,
    12 .. 30 A and the adapter read through, a quarter end in 1 .. 20 N (half of those behind a poly-T tail), an eighth end in
    8 .. 40 C; the rest are plain fragments, half of them with a low-quality 3' tail"""
    rng, out = g.rng, []
    I = int(rng.integers(15, 151)) if rng.integers(0, 2) else int(rng.integers(151, 331))
    frag = g.rnd(I)
    for ad, src in ((AD1, frag), (AD2, _rc(frag.encode()).decode())):
        Lr = int(rng.integers(30, 45)) if i % 9 == 3 else int(rng.integers(60, 152))
        s = SS._fragment_reads(g, i, Lr, ad, src)
        qual = g.q(Lr, 22, 42)
        if i % 4 == 1:
            k = int(rng.integers(10, max(11, Lr - 45)))
            s = (src[:k] + g.rnd(max(0, k - len(src))) + "A" * int(rng.integers(12, 31)) + ad + g.rnd(151))[:Lr]
        elif i % 4 == 2:
            k = int(rng.integers(1, 21))
            s = s[:Lr - k] + "N" * k
            if i % 8 == 2:
                T = min(int(rng.integers(10, 25)), Lr - k)
                s = s[:Lr - k - T] + "T" * T + s[Lr - k:]
        elif i % 8 == 3:
            C = int(rng.integers(8, min(Lr, 41)))
            s = s[:Lr - C] + "C" * C
        elif rng.integers(0, 2):
            tail = int(rng.integers(0, min(Lr, 60) // 2))
            qual = g.q(Lr - tail, 22, 42) + g.q(tail, 2, 24)
        assert len(s) == Lr
        out.append((s.lower() if i % 11 == 0 else s, qual))
    return out


def _dataset(d, seed, n_chunks, n, bgzf):
    return SS._dataset(d, seed, n_chunks, n, bgzf, _inserts, SS._same_places, sample_first=True)


def _write_conf(path, files, samples, trim="[trim]\n" + POST, **kw):
    SS._write_conf(path, files, samples, extra=trim, **kw)


def _oracle(conf, ref_dir, P=P_POST):
    """the oracle's run of the conf without the stage -> ({file: post-trimmed text}, the model's counters)"""
    SS._oracle_run(conf, ref_dir)
    return XM.posttrimmed_outputs(str(ref_dir), P)


def _check_run(mine, ref, texts, table, P=P_POST, only=None):
    SS._check_files(mine, texts, only)
    SS._check_main_report(mine, ref, only)  # as without the stage
    SS._check_report(mine, xr, table, P.keywords())
    for other in (cr, tr, pr, fr):  # these options turn nothing else on
        SS._check_report(mine, other, None)


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF, run once with the stage alone; the model over the oracle's outputs"""
    top = tmp_path_factory.mktemp("posttrim_bgzf")
    files, samples = _dataset(str(top / "data"), 71, 2, 1500, bgzf=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, trim="")
    texts, table = _oracle(plain, top / "ref")
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, texts=texts, table=table, mine=top / "mine", ref=top / "ref", plain=plain)


def test_cli_posttrim_alone_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert t[0][0] == t[1][0] < 3000
    assert all(t[r][k] > 20 for r in (0, 1) for k in (3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15))  # N, A, C and T tails, the crop and the floor all act
    _check_run(run["mine"], run["ref"], run["texts"], t)


def test_cli_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 72, 1, 2000, bgzf=False)
    _write_conf(tmp_path / "plain.txt", files, samples, trim="")
    texts, table = _oracle(tmp_path / "plain.txt", tmp_path / "ref")
    _write_conf(tmp_path / "conf.txt", files, samples)
    _cli(tmp_path / "conf.txt", tmp_path / "mine")
    _check_run(tmp_path / "mine", tmp_path / "ref", texts, table)


def test_cli_behind_clip_trim_pair_overlap_and_in_front_of_filter(bgzf_run, tmp_path):
    """every stage on: the files and the reports are the models chained in the pipeline's order -- clip, [trim], pair_overlap,
    post-trim, [filter], then the quality counters over what is written"""
    run = bgzf_run
    names = [s[0] for s in run["samples"]]
    clipped, ctable = CM.clipped_outputs(str(run["ref"]), P_CLIP)
    paired, second, first = PM.trimmed_outputs(CM.write_outputs(clipped, str(tmp_path / "clipped")), P_PAIR, trim=P_TRIM)
    post, xtable = XM.posttrimmed_outputs(XM.write_outputs(paired, str(tmp_path / "paired")), P_POST)
    texts, table, _, _ = FM.filtered_outputs(XM.write_outputs(post, str(tmp_path / "post")), names, P_F)
    without = FM.filtered_outputs(str(tmp_path / "paired"), names, P_F)
    assert texts != without[0] and table != without[1]  # the filter sees other reads than without the stage
    assert xtable[0][1] == second[2] and xtable[1][1] == second[len(PM.COUNTERS) + 2]  # bases_in: what the overlap trimming left
    assert all(xtable[r][k] > 0 for r in (0, 1) for k in (3, 5, 13)) and sum(row[1] for row in table) > 0
    conf = tmp_path / "all.txt"
    _write_conf(conf, run["files"], run["samples"], trim=TRIMS + CLIP + POST.replace("min_length : 25\n", "") + FILTER, quality=True)
    mine = tmp_path / "all"
    _cli(conf, mine)
    assert sorted(f for f in os.listdir(mine) if f.endswith(".fastq.gz")) == sorted(texts)
    for f in texts:
        assert _gz(os.path.join(str(mine), f)) == texts[f], f
    assert _read(mine / cr.REPORT_NAME) == "\n".join(cr.report_lines(ctable, P_CLIP.keywords())) + "\n"
    assert _read(mine / tr.REPORT_NAME) == "\n".join(tr.report_lines(first, TRIM_KW)) + "\n"
    assert _read(mine / pr.REPORT_NAME) == "\n".join(pr.report_lines(second, P_PAIR.keywords())) + "\n"
    assert _read(mine / xr.REPORT_NAME) == "\n".join(xr.report_lines(xtable, P_POST.keywords())) + "\n"
    assert _read(mine / fr.REPORT_NAME) == "\n".join(fr.report_lines(table, names, P_F.keywords())) + "\n"
    # the quality counters see what is written: the model over the files just compared
    assert _read(mine / qr.REPORT_NAME) == "\n".join(qr.report_lines(QM.table_from_outputs(str(mine), names), names)) + "\n"


def test_cli_the_poly_a_tail_between_insert_and_adapter(bgzf_run, tmp_path):
    """the read the stage exists for, insert + 12 A + adapter, one chunk: adapter_R1 alone cuts the adapter and leaves the A; with
    poly_x : True they go"""
    run = bgzf_run
    ADS = "[trim]\nadapter_R1 : %s\nadapter_R2 : %s\n" % (AD1, AD2)
    PT = TM.Params(AD1, AD2)
    PX = XM.Params(poly_x_min_length=10)
    _write_conf(tmp_path / "plain.txt", run["files"], run["samples"], trim="", chunks=[0])
    SS._oracle_run(tmp_path / "plain.txt", tmp_path / "ref")
    alone, ttable = TM.trimmed_outputs(str(tmp_path / "ref"), PT)
    both, xtable = XM.posttrimmed_outputs(XM.write_outputs(alone, str(tmp_path / "trimmed")), PX)
    ends = lambda texts: sum(ln.upper().endswith(b"A" * 12) for text in texts.values() for ln in text.split(b"\n")[1::4])  # noqa: E731
    assert ends(alone) > 100 and ends(both) == 0 and xtable[0][5] > 100 and xtable[1][5] > 100
    for name, trim, texts in (("alone", ADS, alone), ("both", ADS + "poly_x : True\n", both)):
        conf = tmp_path / (name + ".txt")
        _write_conf(conf, run["files"], run["samples"], trim=trim, chunks=[0])
        _cli(conf, tmp_path / name)
        for f in texts:
            assert _gz(os.path.join(str(tmp_path / name), f)) == texts[f], (name, f)
    assert not os.path.exists(tmp_path / "alone" / xr.REPORT_NAME)
    assert _read(tmp_path / "both" / xr.REPORT_NAME) == "\n".join(xr.report_lines(xtable, PX.keywords())) + "\n"
    kw = dict(adapter_r1=AD1, adapter_r2=AD2, quality_cutoff=0, min_overlap=3, max_mismatch_pct=10, min_length=0)
    for name in ("alone", "both"):  # the 3' trimming saw the same reads in both runs
        assert _read(tmp_path / name / tr.REPORT_NAME) == "\n".join(tr.report_lines(ttable, kw)) + "\n"


def test_cli_chunk_workers_and_write_flags(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, False, False), gpu="chunk_workers : 2\n")
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


def test_cli_without_the_options_nothing_changes(bgzf_run, tmp_path):
    run = bgzf_run
    _cli(run["plain"], tmp_path / "off")
    _cli(run["plain"], tmp_path / "again")  # a second run of the same conf: the same files
    assert not os.path.exists(tmp_path / "off" / xr.REPORT_NAME)
    _compare_dirs(str(tmp_path / "off"), str(run["ref"]))
    for f in sorted(os.listdir(tmp_path / "off")):
        if f.endswith(".fastq.gz"):
            assert open(tmp_path / "off" / f, "rb").read() == open(tmp_path / "again" / f, "rb").read(), f
    assert sorted(os.listdir(tmp_path / "off")) == sorted(os.listdir(tmp_path / "again")) == \
        sorted(f for f in os.listdir(run["mine"]) if f != xr.REPORT_NAME)
    with hb.Engine(0) as e:
        assert not e.posttrim_active()  # nothing allocated, nothing to launch
