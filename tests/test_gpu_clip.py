"""End clipping, sliding-window and poly-G trimming on the MI355X (qd_clip_*, quade_amd/csrc/quade_clip.hip): the record tables the
stage writes and its 24 counters equal tests/clip_model.py's plain Python rule, exactly -- for the stage on its own (qd_dev_clip:
alignments, lengths on both sides of the staged-line limit, every front clip, failing windows planted at every start, poly-G tails
at the rule's edges, the floor, accumulation, state and errors) and through the command line (every output file against the
oracle's file passed through the model, alone and in front of [trim], pair_overlap, [filter] and the two reports; chunk workers,
write flags, ranks, the bundled golden run)."""
import os
import shutil

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import clip_report as cr
from quade_amd import cycle_report as cyr
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from quade_amd import pair_trim_report as pr
from quade_amd import quality_report as qr
from quade_amd import trim_report as tr
from tests import clip_model as CM
from tests import cycle_model as CYM
from tests import filter_model as FM
from tests import pairtrim_model as PM
from tests import qstats_model as QM
from tests import trim_model as TM
from tests import stage_support as SS
from tests.run_support import _compare_dirs, _gz
from tests.stage_support import (AD1, AD2, BASES, FILTER, P_F, P_PAIR, P_TRIM, QUALS, TRIM_KW, TRIMS, _cli, _rc, _read, _text_from,  # noqa: F401
                                 torch_cuda)
from tests.stage_support import LONG_LENS as LENS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WINDOWS = (1, 4, 16, 17, 64, 100)
POLY = (6, 10, 100)


@pytest.fixture(scope="module")
def eng():
    """the one context of this module's stage tests"""
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    with hb.Engine(0) as e:
        yield e


def _rs(rng, L, alphabet=b"ACGT"):
    return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))


def _random_cases(rng, reps=4):
    """every length, every kind of base, every quality byte (below 33 and above 126 among them)"""
    out, walk = [], 0
    for rep in range(reps):
        for L in LENS:
            if L > 1000 and rep > 1:
                continue
            if walk < 2 * len(QUALS):
                qual = bytes(QUALS[(walk + k) % len(QUALS)] for k in range(L))
                walk += L
            else:
                qual = bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L))
            out.append(("random", _rs(rng, L, BASES), qual))
    return out


def _planted_window(rng, L, p, W, Q, fail=True):
    """qualities of L bases whose first failing window starts at p exactly: W - 1 values of Q and one of Q - 1 at its end (the sum
    is Q W - 1), everything else above Q.  fail=False: Q at the end too -- the sum is Q W and nothing fails."""
    q = bytearray(33 + int(v) for v in rng.integers(Q + 1, Q + 30, L))
    q[p:p + W] = bytes([33 + Q]) * W
    if fail:
        q[p + W - 1] = 33 + Q - 1
    return bytes(q)


def _window_cases(rng, W, Q, clip):
    """clip: the larger F + T of the two reads -- the lengths around the window are made for Lc, not for L"""
    out = []
    for p in range(151 - W + 1):  # the first failing window at every start: it falls into every lane's stretch and across their borders
        out.append(("win@%d" % p, _rs(rng, 151), _planted_window(rng, 151, p, W, Q)))
    out.append(("win-exact", _rs(rng, 151), _planted_window(rng, 151, 40, W, Q, fail=False)))
    for L in (330, 2049):  # ... and in lines beyond one word per lane, staged or not
        for p in sorted({0, 1, 150, 320, L // 2, L - W - 1, L - W}):
            for _ in range(3 if L == 330 else 1):
                out.append(("win-long", _rs(rng, L), _planted_window(rng, L, p, W, Q)))
    for extra in (0, clip):
        for Lc in (W - 1, W, W + 1):  # a read shorter than the window is left alone, whatever its qualities
            out.append(("win-short", _rs(rng, Lc + extra), bytes([33]) * (Lc + extra)))
    # the kernel adds up a window's bytes when W <= 2 ceil(Lc / 16) and takes prefix sums otherwise: lines on both sides of that
    for Lt in sorted({16 * (W // 2), 16 * (W // 2) + 1, 16 * ((W + 1) // 2), 16 * ((W + 1) // 2) + 1}):
        for extra in (0, 2, clip):
            L = Lt + extra
            if L > W + clip:
                for p in sorted({extra, L // 3, L - W}):
                    out.append(("win-edge", _rs(rng, L), _planted_window(rng, L, p, W, Q)))
                out.append(("win-edge", _rs(rng, L), bytes(33 + int(v) for v in rng.integers(max(0, Q - 12), Q + 14, L))))
    for L in (17, 151, 151, 257, 330, 2049):
        out.append(("win-noisy", _rs(rng, L, b"ACGTN"), bytes(33 + int(v) for v in rng.integers(max(0, Q - 12), Q + 14, L))))
    return out


def _polyg_cases(rng, P):
    out = []
    hi = lambda L: bytes(33 + int(v) for v in rng.integers(30, 42, L))  # noqa: E731  (a dark cluster reads as high-quality G)
    body = lambda L: _rs(rng, L, b"ACT")  # noqa: E731

    def tail(L, t_mis=(), G=60, with_byte=b"A"):
        s = bytearray(body(L - G) + b"G" * G)
        for t in t_mis:
            s[L - t:L - t + 1] = with_byte
        return bytes(s)
    for run in (P - 1, P, P + 1):  # the minimum run
        out.append(("run%+d" % (run - P), body(151 - run) + b"G" * run, hi(151)))
    for t in range(1, 41):  # one mismatch at every t of a 60-G tail
        out.append(("one@%d" % t, tail(151, (t,)), hi(151)))
    out.append(("five", tail(151, (9, 17, 25, 33, 41)), hi(151)))  # one per 8 bases: all five are forgiven
    out.append(("six", tail(151, (9, 17, 25, 33, 41, 49)), hi(151)))  # the sixth ends the walk
    for t in (7, 8, 9):  # the 1-in-8 edge
        out.append(("edge1@%d" % t, tail(151, (t,)), hi(151)))
    for t in (15, 16, 17):
        out.append(("edge2@%d" % t, tail(151, (8, t)), hi(151)))
    out.append(("lower", tail(151).lower(), hi(151)))  # g counts as G
    out.append(("n-tail", tail(151, (3, 12, 13), with_byte=b"N"), hi(151)))  # N does not
    out.append(("n-all", body(91) + b"N" * 60, hi(151)))
    for L in (151, 330, 330, 330, 2049):  # G throughout: nothing is left
        out.append(("all-g", b"G" * L, hi(L)))
    for G in range(0, 71):  # a tail of every length: its 5' end falls into every lane's four bases and across the rounds of 64
        out.append(("tail%d" % G, tail(151, G=G) if G else body(151), hi(151)))
    for L, G in ((330, 200), (330, 64), (2049, 1500), (2049, 65), (300, 128)):
        out.append(("tail-long", tail(L, (70,), G=G), hi(L)))
    return out


def _noisy_cases(rng, n=12):
    """reads rich in G with G tails and qualities around any cutoff: all rules cut, in every length class"""
    out = []
    for L in LENS:
        for _ in range(n if L < 1000 else 2):
            G = int(rng.integers(0, min(L, 80) + 1))
            s = bytearray(_rs(rng, L - G, b"ACGTNg") + _rs(rng, G, b"GGGGGGGGGGGGGGGgAN"))
            good = int(rng.integers(0, L + 1))
            q = bytes(33 + int(v) for v in rng.integers(15, 42, good)) + bytes(33 + int(v) for v in rng.integers(0, 30, L - good))
            out.append(("noisy", bytes(s), q))
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
                L = int(LENS[int(rng.integers(0, len(LENS) - 1))])
                x.append(("fill", _rs(rng, L, BASES), bytes(QUALS[int(v)] for v in rng.integers(0, len(QUALS), L))))
        self.cases = [[x[int(i)] for i in rng.permutation(m)] for x in lists]
        if n is not None:
            while len(self.cases[0]) < n:
                self.cases = [c + c for c in self.cases]
            self.cases = [c[:n] for c in self.cases]
        self.n = len(self.cases[0])
        (self.t1, self.r1), (self.t2, self.r2) = (_text_from(rng, c) for c in self.cases)

    def model(self, P=None):
        """-> (the tables the stage leaves, counters uint64[2, 12])"""
        P = P or self.P
        table, outs = CM.new_table(), []
        for r, recs in enumerate((self.r1, self.r2)):
            o = recs.copy()
            for j, (_, seq, qual) in enumerate(self.cases[r]):
                f, n = CM.count(table, seq, qual, r, P)
                o[j, 3] += f
                o[j, 5] += f
                o[j, 4] = n
            outs.append(o)
        return outs, np.array(table, dtype=np.uint64)

    def run(self, eng):
        return eng.dev_clip(self.t1, self.r1, self.t2, self.r2)


def _check(stage, eng, before=None, P=None):
    got = stage.run(eng)
    want, table = stage.model(P)
    for r in (0, 1):
        assert got[r].shape == want[r].shape and got[r].dtype == np.uint32
        bad = np.argwhere(got[r] != want[r])
        assert not len(bad), [(r, int(j), stage.cases[r][int(j)][0], got[r][j].tolist(), want[r][j].tolist()) for j, _ in bad[:6]]
        # head, name_off and name_len are untouched; seq and qual moved by the same f
        assert (got[r][:, :3] == stage.r1[:, :3] if r == 0 else got[r][:, :3] == stage.r2[:, :3]).all()
        src = stage.r1 if r == 0 else stage.r2
        assert ((got[r][:, 3] - src[:, 3]) == (got[r][:, 5] - src[:, 5])).all()
    counters = eng.clip_read()
    assert counters.shape == (2, 12) and counters.dtype == np.uint64
    if before is not None:
        table = table + before
    assert (counters == table).all(), (counters.tolist(), table.tolist())
    return table


def _set(eng, P):
    eng.clip_set(**P.keywords())
    assert eng.clip_get() == P.keywords() and eng.clip_active()


def test_the_generated_inputs_hold_the_cases():
    rng = np.random.default_rng(1)
    W, Q = 16, 20
    wc = {}
    for t, s, q in _window_cases(rng, W, Q, 7):
        wc.setdefault(t, []).append((s, q))
    for p in range(151 - W + 1):  # planted at p exactly, with a sum of Q W - 1
        (s, q), = wc["win@%d" % p]
        assert CM.window(q, W, Q) == p and sum(b - 33 for b in q[p:p + W]) == Q * W - 1
    (s, q), = wc["win-exact"]
    assert CM.window(q, W, Q) == 151 and sum(b - 33 for b in q[40:40 + W]) == Q * W
    assert {len(s) for s, _ in wc["win-short"]} == {W - 1, W, W + 1, W + 6, W + 7, W + 8}
    assert [CM.window(q, W, Q) for s, q in wc["win-short"][:3]] == [W - 1, 0, 0]
    assert max(CM.window(q, W, Q) for s, q in wc["win-long"] if len(s) == 2049) == 2049 - W > 336
    P = 10
    pc = {}
    for t, s, q in _polyg_cases(rng, P):
        pc.setdefault(t, []).append(s)
    g = lambda tag: CM.poly_g(pc[tag][0], P)  # noqa: E731
    assert (g("run-1"), g("run+0"), g("run+1")) == (142, 141, 140)  # 9 G: the base in front of them is the one forgiven
    assert g("one@1") == 91 and g("one@20") == 91 and g("one@40") == 91 and g("five") == 91 and g("six") == 151 - 48
    assert (g("edge1@7"), g("edge1@8"), g("edge1@9")) == (91, 91, 91)  # one mismatch in front of P = 10 is never too many
    p6 = {t: s for t, s, q in _polyg_cases(rng, 6)}
    assert [CM.poly_g(p6["edge1@%d" % t], 6) for t in (7, 8, 9)] == [151 - 6, 91, 91]  # 8 x 1 > 7: the walk ends there
    assert (g("edge2@15"), g("edge2@16"), g("edge2@17")) == (151 - 14, 91, 91)
    assert g("lower") == 91 and pc["lower"][0].islower() and g("n-tail") == 151 - 11 and g("n-all") == 151
    assert [CM.poly_g(s, P) for s in pc["all-g"]] == [0] * 5 and {len(s) for s in pc["all-g"]} == {151, 330, 2049}
    assert [g("tail%d" % G) for G in (0, 9, 10, 11, 63, 64, 65, 70)] == [151, 142, 141, 140, 88, 87, 86, 81]
    assert all(CM.poly_g(s, P) == len(s) - G for s, G in zip(pc["tail-long"], (200, 64, 1500, 65, 128)))
    noisy = _noisy_cases(rng)
    Pn = CM.Params((3, 0), (0, 2), 4, 20, 10, 20)
    table = CM.new_table()
    for _, s, q in noisy:
        CM.count(table, s, q, 0, Pn)
        CM.count(table, s, q, 1, Pn)
    # every counter is exercised (R1 has no tail clip and R2 no front clip)
    assert all(v > 0 for r in (0, 1) for k, v in enumerate(table[r]) if (r, k) not in ((0, 5), (0, 6), (1, 3), (1, 4)))
    st = Stage(5, Pn, (noisy + _random_cases(rng), noisy[::-1]))
    for text, recs in ((st.t1, st.r1), (st.t2, st.r2)):
        assert {int(q[3]) % 16 for q in recs if q[4]} == set(range(16)) == {int(q[5]) % 16 for q in recs if q[4]}
        # 330 bases: lines on both sides of the staged-line limit (21 aligned words; the upload moves the text by 3 bytes)
        assert {((int(q[3]) + 3) % 16 + 330 + 15) // 16 <= 21 for q in recs if q[4] == 330} == {True, False}
    assert {len(s) for _, s, _ in st.cases[0]} >= set(LENS) and set(b"".join(q for t, _, q in st.cases[0] if t == "random")) == set(QUALS)


@pytest.mark.parametrize("W", WINDOWS)
def test_window_equals_the_model(eng, W):
    Q = {1: 20, 4: 20, 16: 2, 17: 15, 64: 93 - 30, 100: 30}[W]
    P = CM.Params(front_clip=(0, 5), tail_clip=(2, 0), window_size=W, window_quality=Q, min_length=W % 3 * 10)
    rng = np.random.default_rng(100 + W)
    _set(eng, P)
    table = _check(Stage(200 + W, P, (_window_cases(rng, W, Q, 5) + _random_cases(rng, 2), _window_cases(rng, W, Q, 5))), eng)
    assert (table[:, 7] > 100).all() if W < 100 else (table[:, 7] > 40).all()


@pytest.mark.parametrize("G", POLY)
def test_poly_g_equals_the_model(eng, G):
    P = CM.Params(front_clip=(1, 0), tail_clip=(0, 0), poly_g_min_length=G)
    rng = np.random.default_rng(300 + G)
    _set(eng, P)
    table = _check(Stage(400 + G, P, (_polyg_cases(rng, G), _polyg_cases(rng, G) + _random_cases(rng, 2))), eng)
    assert (table[:, 9] > (60 if G < 100 else 5)).all() and (table[:, 7:9] == 0).all()


# F + T on both sides of the 64- and 151-base reads; R1 and R2 always differ
FRONTS = list(range(18)) + [62, 63, 64, 65, 66, 150, 151, 152, 1000]


def test_front_and_tail_clip_equal_the_model(eng):
    rng = np.random.default_rng(7)
    cases = _random_cases(rng, 2) + _noisy_cases(rng, 3)
    st = Stage(8, None, (cases, cases[::-1]))
    seen = set()
    for k, F in enumerate(FRONTS):
        P = CM.Params(front_clip=(F, F // 2), tail_clip=(k % 3, 64 - F // 2 + k % 3 - 1 if F // 2 <= 64 else 1000))
        if k % 2:
            P.window_size, P.window_quality, P.poly_g_min_length, P.min_length = 4, 20, 10, (0, 30, 1000)[k % 3]
        _set(eng, P)
        want, _ = st.model(P)
        got = st.run(eng)
        for r in (0, 1):
            assert (got[r] == want[r]).all(), (F, r)
            src = (st.r1, st.r2)[r]
            f = got[r][:, 3] - src[:, 3]
            assert (f == np.minimum(src[:, 4], P.front_clip[r])).all() and (got[r][:, 5] - src[:, 5] == f).all()
            assert (got[r][:, :3] == src[:, :3]).all()
            seen |= {(int(a) + int(b)) - int(L) for a, b, L in zip(f, np.full(len(f), P.tail_clip[r]), src[:, 4]) if L in (64, 151)}
        assert (eng.clip_read() == st.model(P)[1]).all(), F  # (clip_set zeroed the table)
    assert {-1, 0, 1} <= seen  # f + T one below, at and one above L


@pytest.mark.parametrize("min_length", [0, 20, 400])
def test_all_rules_and_the_floor_equal_the_model(eng, min_length):
    P = CM.Params(front_clip=(3, 0), tail_clip=(0, 2), window_size=4, window_quality=20, poly_g_min_length=10, min_length=min_length)
    rng = np.random.default_rng(500 + min_length)
    _set(eng, P)
    table = _check(Stage(600 + min_length, P, (_noisy_cases(rng), _noisy_cases(rng) + _random_cases(rng, 2))), eng)
    assert (table[:, 7:11] > 0).all() and (table[0, 3:5] > 0).all() and (table[1, 5:7] > 0).all()
    assert (table[:, 11] > 0).all() if min_length else (table[:, 11] == 0).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_stage_pair_counts(eng, n):
    P = CM.Params(front_clip=(0, 1), window_size=4, window_quality=20, poly_g_min_length=10)
    rng = np.random.default_rng(700 + n)
    _set(eng, P)
    st = Stage(800 + n, P, (_noisy_cases(rng, 4), _noisy_cases(rng, 4)), n=n)
    assert st.n == n
    assert (_check(st, eng)[:, 0] == n).all()


def test_the_read_the_stage_exists_for(eng):
    """insert + 10 bases of adapter + 8 G: the adapter rule alone leaves it (the G spend its mismatch budget); with the poly-G rule
    in front the tail goes and the adapter prefix with it -- the 5' offset and the new length reach qd_dev_trim through the tables"""
    rng = np.random.default_rng(9)
    cases = [[("dark", _rs(rng, 60, b"ACT") + ad[:10].encode() + b"G" * 8, bytes([33 + 38]) * 78) for _ in range(40)] for ad in (AD1, AD2)]
    PT = TM.Params(AD1, AD2, min_length=20)
    PC = CM.Params(front_clip=(0, 4), poly_g_min_length=10, min_length=20)
    st = Stage(10, PC, cases)
    eng.trim_set(AD1, AD2, 0, 3, 10, 20)
    try:
        eng.clip_set()  # off
        alone = eng.dev_trim(st.t1, st.r1, st.t2, st.r2)
        assert (alone[0][:, 4] == 78).all() and (alone[1][:, 4] == 78).all()
        assert all(TM.trim_read(s, q, r, PT)[2] == 78 for r in (0, 1) for _, s, q in st.cases[r])
        _set(eng, PC)
        clipped = st.run(eng)
        assert (clipped[0][:, 4] == 69).all() and (clipped[1][:, 4] == 65).all()
        both = eng.dev_trim(st.t1, clipped[0], st.t2, clipped[1])
        for r, f in ((0, 0), (1, 4)):
            src = (st.r1, st.r2)[r]
            assert (both[r][:, 4] == 60 - f).all() and (both[r][:, 3] == src[:, 3] + f).all() and (both[r][:, 5] == src[:, 5] + f).all()
            for _, s, q in st.cases[r]:
                f_, n = CM.count(CM.new_table(), s, q, r, PC)
                assert (f_, TM.trim_read(s[f_:f_ + n], q[f_:f_ + n], r, PT)[2]) == (f, 60 - f)
    finally:
        eng.trim_set()
        eng.clip_set()


def test_accumulation_reset_and_add(eng):
    P = CM.Params(front_clip=(2, 0), tail_clip=(0, 1), window_size=4, window_quality=20, poly_g_min_length=10)
    rng = np.random.default_rng(20)
    a, b = Stage(21, P, (_noisy_cases(rng, 3), _noisy_cases(rng, 3)), n=300), Stage(22, P, (_noisy_cases(rng, 2), _noisy_cases(rng, 2)), n=65)
    _set(eng, P)
    with hb.Engine(0) as other:
        other.clip_set(**P.keywords())
        ta = _check(a, eng)
        both = _check(b, eng, before=ta)
        eng.reset_counts()
        assert not eng.clip_read().any() and eng.clip_get() == P.keywords()
        tb = _check(b, eng)
        _check(a, other)
        eng.clip_add(other.clip_read())  # a second context's counters fold in
        assert (eng.clip_read() == both).all() and (both == ta + tb).all() and (other.clip_read() == ta).all()
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.clip_add(np.zeros(16, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
    eng.clip_set()  # all off: the table is freed
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.clip_read()
    assert ei.value.code == hb.QD_ERR_STATE
    eng.clip_set(tail_clip_r1=1)
    assert not eng.clip_read().any()
    eng.clip_set()


def test_state_and_errors(eng):
    P = CM.Params(front_clip=(2, 0), window_size=4, window_quality=20, poly_g_min_length=10, min_length=5)
    rng = np.random.default_rng(30)
    st = Stage(31, P, (_noisy_cases(rng, 2), _noisy_cases(rng, 2)), n=64)
    off = CM.Params().keywords()
    eng.clip_set()
    assert not eng.clip_active() and eng.clip_get() == off
    for call in (eng.clip_read, lambda: st.run(eng), lambda: eng.clip_add(np.zeros((2, 12), np.uint64))):
        with pytest.raises(hb.QuadeHipError) as ei:
            call()
        assert ei.value.code == hb.QD_ERR_STATE
    assert eng.lib.qd_clip_set(eng._h, None) == 0 and not eng.clip_active()  # NULL = off
    eng.clip_set(min_length=30)  # no rule: off, whatever the floor says
    assert not eng.clip_active() and eng.clip_get() == off
    _set(eng, P)
    good = eng.clip_get()
    for bad in (dict(front_clip_r1=1001), dict(front_clip_r2=-1), dict(tail_clip_r1=-1), dict(tail_clip_r2=1001),
                dict(window_size=101, window_quality=20), dict(window_size=-1, window_quality=20), dict(window_size=4), dict(window_quality=20),
                dict(window_size=4, window_quality=94), dict(window_size=4, window_quality=-1), dict(poly_g_min_length=5),
                dict(poly_g_min_length=101), dict(poly_g_min_length=-1), dict(tail_clip_r1=1, min_length=65536), dict(tail_clip_r1=1, min_length=-1)):
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.clip_set(**bad)
        assert ei.value.code == hb.QD_ERR_INVALID, bad
        assert eng.clip_get() == good and eng.clip_active()  # a rejected call changes nothing
    want = _check(st, eng)  # ... and the previous parameters are still in force
    for ok in (dict(front_clip_r1=1000, front_clip_r2=1000, tail_clip_r1=1000, tail_clip_r2=1000), dict(window_size=1, window_quality=1),
               dict(window_size=100, window_quality=93), dict(poly_g_min_length=6), dict(poly_g_min_length=100, min_length=65535)):
        eng.clip_set(**ok)
        assert eng.clip_active()
    assert eng.clip_get()["min_length"] == 65535
    _set(eng, P)
    out = np.zeros(23, dtype=np.uint64)
    assert eng.lib.qd_clip_read(eng._h, hb._ptr(out), 23) == hb.QD_ERR_INVALID
    want = _check(st, eng)
    # a bad table never becomes an address: refused on the host, nothing launched, the counters as they were
    bad = st.r1.copy()
    bad[5, 4] = len(st.t1)  # a sequence range beyond the text
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.dev_clip(st.t1, bad, st.t2, st.r2)
    assert ei.value.code == hb.QD_ERR_INVALID
    bad = st.r2.copy()
    bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.dev_clip(st.t1, st.r1, st.t2, bad)
    assert ei.value.code == hb.QD_ERR_INVALID
    assert (eng.clip_read() == want).all()
    eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))  # plan and barcodes leave the stage alone
    eng.set_barcodes(["ACGTACGTACGTACGT"])
    assert eng.clip_get() == good and (eng.clip_read() == want).all()
    eng.clip_set()


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
CLIP = "front_clip_R2 : 5\ntail_clip_R1 : 1\nwindow_size : 4\nwindow_quality : 18\npoly_g : True\nmin_length : 25\n"
P_CLIP = CM.Params(front_clip=(0, 5), tail_clip=(1, 0), window_size=4, window_quality=18, poly_g_min_length=10, min_length=25)


def _inserts(g, i, sample, kind):
    """the filter tests' fragments (stage_support._filter_inserts) with what this stage is for: a quarter of the reads end in
    8 .. 40 high-quality G (a fifth of those behind the first 10 bases of the adapter), a seventh have a bad stretch in the middle
    that good bases follow"""
    rng, out = g.rng, []
    I = int(rng.integers(15, 151)) if rng.integers(0, 2) else int(rng.integers(151, 331))
    frag = g.rnd(I)
    for ad, src in ((AD1, frag), (AD2, _rc(frag.encode()).decode())):
        Lr = int(rng.integers(30, 45)) if i % 9 == 3 else int(rng.integers(60, 152))
        s = SS._fragment_reads(g, i, Lr, ad, src)
        qual = g.q(Lr, 22, 42)
        if i % 4 == 1:
            G = int(rng.integers(8, min(Lr, 41)))
            s = s[:Lr - G] + "G" * G
            if i % 20 == 1 and Lr - G > 10:
                s = s[:Lr - G - 10] + ad[:10] + "G" * G
        elif rng.integers(0, 2):
            tail = int(rng.integers(0, min(Lr, 60) // 2))
            qual = g.q(Lr - tail, 22, 42) + g.q(tail, 2, 24)
        if i % 7 == 2:
            at = int(rng.integers(10, Lr - 12))
            qual = qual[:at] + g.q(6, 2, 10) + qual[at + 6:]
        out.append((s.lower() if i % 11 == 0 else s, qual))
    return out


def _dataset(d, seed, n_chunks, n, bgzf):
    return SS._dataset(d, seed, n_chunks, n, bgzf, _inserts, SS._same_places, sample_first=True)


def _write_conf(path, files, samples, trim="[trim]\n" + CLIP, **kw):
    SS._write_conf(path, files, samples, extra=trim, **kw)


def _oracle(conf, ref_dir, P=P_CLIP):
    """the oracle's run of the conf without the stage -> ({file: clipped text}, the model's counters)"""
    SS._oracle_run(conf, ref_dir)
    return CM.clipped_outputs(str(ref_dir), P)


def _check_run(mine, ref, texts, table, P=P_CLIP, only=None):
    SS._check_files(mine, texts, only)
    SS._check_main_report(mine, ref, only)  # as without the stage
    SS._check_report(mine, cr, table, P.keywords())
    for other in (tr, pr, fr):  # these options turn nothing else on
        SS._check_report(mine, other, None)


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF, run once with the stage alone; the model over the oracle's outputs"""
    top = tmp_path_factory.mktemp("clip_bgzf")
    files, samples = _dataset(str(top / "data"), 61, 2, 1500, bgzf=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, trim="")
    texts, table = _oracle(plain, top / "ref")
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, texts=texts, table=table, mine=top / "mine", ref=top / "ref", plain=plain)


def test_cli_clip_alone_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    assert t[0][0] == t[1][0] < 3000 and t[0][3] == 0 and t[1][3] == t[1][0] and t[0][5] == t[0][0] and t[1][5] == 0
    assert all(t[r][k] > 20 for r in (0, 1) for k in (7, 8, 9, 10, 11))  # the window, the poly-G rule and the floor all act
    _check_run(run["mine"], run["ref"], run["texts"], t)


def test_cli_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 62, 1, 2000, bgzf=False)
    _write_conf(tmp_path / "plain.txt", files, samples, trim="")
    texts, table = _oracle(tmp_path / "plain.txt", tmp_path / "ref")
    _write_conf(tmp_path / "conf.txt", files, samples)
    _cli(tmp_path / "conf.txt", tmp_path / "mine")
    _check_run(tmp_path / "mine", tmp_path / "ref", texts, table)


def test_cli_in_front_of_trim_pair_overlap_filter_and_both_reports(bgzf_run, tmp_path):
    """every stage on: the files and the reports are the models chained in the pipeline's order -- clip, [trim], pair_overlap,
    [filter], then the two counters over what is written.  The run that proves the 5' offset passes through every later kernel."""
    run = bgzf_run
    names = [s[0] for s in run["samples"]]
    clipped = CM.write_outputs(run["texts"], str(tmp_path / "clipped"))
    texts, table, first, second = FM.filtered_outputs(clipped, names, P_F, P_TRIM, P_PAIR)
    plain = FM.filtered_outputs(str(run["ref"]), names, P_F, P_TRIM, P_PAIR)
    assert texts != plain[0] and first != plain[2] and second != plain[3]  # the stages behind it see other reads
    assert first[0][1] == run["table"][0][2] and first[1][1] == run["table"][1][2]  # the trim report's bases_in: what this stage left
    assert all(first[r][k] > 0 for r in (0, 1) for k in (3, 5)) and second[PM.PAIRS + 2] > 0 and sum(row[1] for row in table) > 0
    conf = tmp_path / "all.txt"
    _write_conf(conf, run["files"], run["samples"], trim=TRIMS + CLIP.replace("min_length : 25\n", "") + FILTER, quality=True)
    text = _read(conf).replace("[output]\n", "[output]\ncycle_report : True\n", 1)
    open(conf, "w").write(text)
    mine = tmp_path / "all"
    _cli(conf, mine)
    assert sorted(f for f in os.listdir(mine) if f.endswith(".fastq.gz")) == sorted(texts)
    for f in texts:
        assert _gz(os.path.join(str(mine), f)) == texts[f], f
    assert _read(mine / cr.REPORT_NAME) == "\n".join(cr.report_lines(run["table"], P_CLIP.keywords())) + "\n"
    assert _read(mine / tr.REPORT_NAME) == "\n".join(tr.report_lines(first, TRIM_KW)) + "\n"
    assert _read(mine / pr.REPORT_NAME) == "\n".join(pr.report_lines(second, P_PAIR.keywords())) + "\n"
    assert _read(mine / fr.REPORT_NAME) == "\n".join(fr.report_lines(table, names, P_F.keywords())) + "\n"
    # the two counters see what is written: the models over the files just compared
    assert _read(mine / qr.REPORT_NAME) == "\n".join(qr.report_lines(QM.table_from_outputs(str(mine), names), names)) + "\n"
    assert _read(mine / cyr.REPORT_NAME) == "\n".join(cyr.report_lines(CYM.table_from_outputs(str(mine), names))) + "\n"


def test_cli_poly_g_uncovers_the_adapter_that_trim_alone_leaves(bgzf_run, tmp_path):
    """reads of insert + 10 bases of adapter + a G tail, one chunk: [trim] alone keeps adapter prefix and tail in most of them, with
    poly_g : True in front both go"""
    run = bgzf_run
    ADS = "[trim]\nadapter_R1 : %s\nadapter_R2 : %s\n" % (AD1, AD2)
    PT = TM.Params(AD1, AD2)
    PG = CM.Params(poly_g_min_length=10)
    _write_conf(tmp_path / "plain.txt", run["files"], run["samples"], trim="", chunks=[0])
    os.makedirs(tmp_path / "ref")
    qo.run_quade(str(tmp_path / "plain.txt"), outdir=str(tmp_path / "ref"))
    alone, _ = TM.trimmed_outputs(str(tmp_path / "ref"), PT)
    clipped, ctable = CM.clipped_outputs(str(tmp_path / "ref"), PG)
    both, ttable = TM.trimmed_outputs(CM.write_outputs(clipped, str(tmp_path / "clipped")), PT)
    tails = [(ad[:10] + "GGGGGGGG").encode() for ad in (AD1, AD2)]
    kept = sum(text.count(tails[TM.read_of(f)]) for f, text in alone.items())
    assert kept > 20 and sum(text.count(tails[TM.read_of(f)]) for f, text in both.items()) == 0
    for name, trim, texts in (("alone", ADS, alone), ("both", ADS + "poly_g : True\n", both)):
        conf = tmp_path / (name + ".txt")
        _write_conf(conf, run["files"], run["samples"], trim=trim, chunks=[0])
        _cli(conf, tmp_path / name)
        for f in texts:
            assert _gz(os.path.join(str(tmp_path / name), f)) == texts[f], (name, f)
    assert not os.path.exists(tmp_path / "alone" / cr.REPORT_NAME)
    assert _read(tmp_path / "both" / cr.REPORT_NAME) == "\n".join(cr.report_lines(ctable, PG.keywords())) + "\n"
    kw = dict(adapter_r1=AD1, adapter_r2=AD2, quality_cutoff=0, min_overlap=3, max_mismatch_pct=10, min_length=0)
    assert _read(tmp_path / "both" / tr.REPORT_NAME) == "\n".join(tr.report_lines(ttable, kw)) + "\n"


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


def test_cli_without_the_options_nothing_changes(bgzf_run, tmp_path):
    run = bgzf_run
    _cli(run["plain"], tmp_path / "off")
    assert not os.path.exists(tmp_path / "off" / cr.REPORT_NAME)
    _compare_dirs(str(tmp_path / "off"), str(run["ref"]))
    assert sorted(os.listdir(tmp_path / "off")) == sorted(f for f in os.listdir(run["mine"]) if f != cr.REPORT_NAME)


def _bundled(tmp_path, bundled_dir, extra):
    from quade_amd.quade import Quade
    shutil.copytree(os.path.join(bundled_dir, "dataset"), tmp_path / "dataset")
    work = tmp_path / "result"
    work.mkdir()
    conf = work / "conf.txt"
    conf.write_text(_read(os.path.join(bundled_dir, "result", "Quade_conf_file.txt")) + extra)
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
    return work


def test_bundled_golden_run_with_the_stage_off(torch_cuda, tmp_path, bundled_dir):
    """the reference's own 299 pairs with a [trim] section that turns nothing on: the goldens, byte for byte"""
    work = _bundled(tmp_path, bundled_dir, "\n[trim]\nfront_clip_R1 : 0\npoly_g : False\npoly_g_min_length : 12\nmin_length : 30\n")
    _compare_dirs(str(work), os.path.join(bundled_dir, "result"))
    assert sorted(os.listdir(work)) == sorted(f for f in os.listdir(os.path.join(bundled_dir, "result")) if f != "Quade_conf_file.txt")


def test_bundled_golden_run_with_a_tail_clip(torch_cuda, tmp_path, bundled_dir):
    """... and with tail_clip_R1 : 1: the goldens through the model, all on the device"""
    work = _bundled(tmp_path, bundled_dir, "\n[trim]\ntail_clip_R1 : 1\n")
    P = CM.Params(tail_clip=(1, 0))
    texts, table = CM.clipped_outputs(os.path.join(bundled_dir, "result"), P)
    assert table[0][0] == table[1][0] == 299 and table[0][5] == 299 and table[0][6] == 299 and table[1][2] == table[1][1]
    _check_run(work, os.path.join(bundled_dir, "result"), texts, table, P=P)
