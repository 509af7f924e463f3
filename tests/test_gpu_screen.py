"""The k-mer screen on the MI355X (qd_screen_*, quade_amd/csrc/quade_screen.hip): the hits per read, the flag bytes and the table
equal tests/screen_model.py's plain Python rule, exactly -- for the stage on its own (qd_dev_screen: every k at the edges of the
word arithmetic, lengths on both sides of k and of the staged-line limit at every alignment, planted k-mers, bytes that break
them, homopolymers, min_hits over both reads, both table placements up to the fullest LDS table, long probe chains, skipped pairs,
accumulation, state and errors, all eight stages in one context) and through the command line (every output file against the
oracle's file passed through the models, alone with either action, behind every other stage, chunk workers, write flags, ranks,
and a conf without the section)."""
import os

import numpy as np
import pytest

from quade_amd import cycle_report as yr
from quade_amd import duplication_report as dr
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from quade_amd import posttrim_report as xr
from quade_amd import quality_report as qr
from quade_amd import screen as qscreen
from quade_amd import screen_report as sr
from tests import cycle_model as YM
from tests import dup_model as DM
from tests import filter_model as FM
from tests import pairtrim_model as PM
from tests import posttrim_model as XM
from tests import qstats_model as QM
from tests import screen_model as SM
from tests import stage_support as SS
from tests.run_support import _compare_dirs, _gz
from tests.stage_support import (BASES, FILTER, P_F, P_PAIR, P_TRIM, TRIMS, _barcodes, _cli, _rc, _read, _text_from,  # noqa: F401
                                 torch_cuda)

pytestmark = pytest.mark.gpu

KS = (15, 16, 17, 31, 32)
UND = 0xFFFF
LDS_MAX = qscreen.LDS_MAX_KMERS
# stage_support's BASES with the bases six times as frequent: one byte in seven breaks a k-mer, so that runs of k valid bases occur
MIXED = b"ACGTacgt" * 6 + BASES[4:6] + BASES[10:]


def _lens(k):
    """both sides of k, of a 64-base step, of the slab's bound at every alignment (320 .. 337: 21 words hold 321 bytes at any
    offset and 336 at the best) and the byte path (400, 1000)"""
    return tuple(sorted({0, k - 1, k, k + 1, 63, 64, 65, 151, 320, 321, 322, 336, 337, 400, 1000}))


@pytest.fixture(scope="module")
def eng():
    """the one context of this module's stage tests"""
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    with hb.Engine(0) as e:
        e.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        e.set_barcodes(_barcodes(3))
        yield e


def _rs(rng, L, alphabet=b"ACGT"):
    return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))


def _case(tag, seq):
    return (tag, bytes(seq), b"I" * len(seq))  # the stage never reads the quality line


def _fasta(records, width=70):
    out = []
    for i, rec in enumerate(records):
        out.append(b">rec%d some text\n" % i + b"".join(rec[a:a + width] + b"\n" for a in range(0, len(rec), width)))
    return b"".join(out)


class Ref(object):
    """a seeded random reference of `bases` bases and a record of 40 G: its text, its set R and the array screen_set takes"""

    def __init__(self, seed, k, bases=600):
        rng = np.random.default_rng(seed)
        self.k = k
        self.seq = _rs(rng, bases)
        self.fasta = _fasta([self.seq, b"G" * 40])
        self.kmers = qscreen.reference_kmers(self.fasta, k).kmers
        self.R = set(int(w) for w in self.kmers)

    def piece(self, rng, L):
        a = int(rng.integers(0, len(self.seq) - L + 1))
        return self.seq[a:a + L]


def _length_cases(rng, ref):
    """every length: random reads over every kind of byte, reads copied whole from the reference (hits = L - k + 1), reads of
    bases alone that hold none of its k-mers"""
    out, k = [], ref.k
    for L in _lens(k):
        for _ in range(18 if 320 <= L <= 337 else 3 if L < 400 else 1):
            out.append(_case("random", _rs(rng, L, MIXED)))
            out.append(_case("copy", ref.piece(rng, L) if L <= len(ref.seq) else ref.seq + _rs(rng, L - len(ref.seq))))
            out.append(_case("bases", _rs(rng, L)))
    return out


def _planted_cases(rng, ref):
    """one k-mer of the reference at the first and at the last position of a random read, forward and reverse-complemented, in
    lower case; a byte that is no base at each of the k positions of a planted k-mer; homopolymers"""
    out, k = [], ref.k
    for L in (k, k + 1, 64, 151, 330, 400):
        for form in range(4):
            x = ref.piece(rng, k + 2)  # the k-mer with its two neighbours: the read goes on with another base, so that one k-mer hits
            x = _rc(x) if form & 1 else x
            w = x[1:k + 1].lower() if form & 2 else x[1:k + 1]
            body = bytearray(_rs(rng, L - k, b"AT"))  # (the reference is random over four letters and poly-G: no 15-mer of A and T)
            if body:
                out.append(_case("first", w + (b"T" if x[k + 1] == ord("A") else b"A") + body[1:]))
                out.append(_case("last", body[1:] + (b"T" if x[0] == ord("A") else b"A") + w))
            else:
                out += [_case("first", w), _case("last", w)]
    for i in range(k):  # 3 k bases of the reference hold 2 k + 1 k-mers; the byte at k + i kills the k that cover it
        s = bytearray(ref.piece(rng, 3 * k))
        s[k + i] = (ord("N"), ord("."), ord("n"), 0x80 | ord("A"))[i % 4]
        out.append(_case("broken", bytes(s)))
    for L in (k, 64, 151, 400):
        out += [_case("homo", b"G" * L), _case("homo", b"c" * L), _case("homo-out", b"A" * L), _case("homo-n", b"N" * L)]
    return out


class Stage(object):
    """R1 and R2 drawn apart: each stream has its own cases in its own order (a pair's two reads differ), the shorter list filled up
    with random reads; codes over S samples with Undetermined among them"""

    def __init__(self, seed, lists, S=3, n=None):
        rng = np.random.default_rng(seed)
        lists = [list(x) for x in lists]
        m = max(len(x) for x in lists)
        for x in lists:
            while len(x) < m:
                x.append(_case("fill", _rs(rng, int(rng.integers(0, 200)), MIXED)))
        self.cases = [[x[int(i)] for i in rng.permutation(m)] for x in lists]
        if n is not None:
            while len(self.cases[0]) < n:
                self.cases = [c + c for c in self.cases]
            self.cases = [c[:n] for c in self.cases]
        self.n = len(self.cases[0])
        (self.t1, self.r1), (self.t2, self.r2) = (_text_from(rng, c) for c in self.cases)
        self.S = S
        codes = rng.integers(0, 2 * S + 1, self.n)
        codes[codes == 2 * S] = UND
        self.codes = codes.astype(np.uint16)

    def model(self, P, R, drop=None):
        """-> (hits uint32[n, 2], flags uint8[n], table uint64[2 S + 1, 8])"""
        table = SM.new_table(self.S)
        hits, flags = np.zeros((self.n, 2), dtype=np.uint32), np.zeros(self.n, dtype=np.uint8)
        for j in range(self.n):
            if drop is not None and drop[j]:
                flags[j] = drop[j]
                continue
            h1, h2, matched = SM.count(table, int(self.codes[j]), self.cases[0][j][1], self.cases[1][j][1], P, R)
            hits[j] = (h1, h2)
            flags[j] = SM.DROPPED if matched and P.action == "drop" else 0
        return hits, flags, np.array(table, dtype=np.uint64)

    def run(self, eng, drop=None):
        return eng.dev_screen(self.t1, self.r1, self.t2, self.r2, self.codes, drop)


def _check(stage, eng, P, R, drop=None, before=None):
    hits, flags = stage.run(eng, drop)
    want_hits, want_flags, table = stage.model(P, R, drop)
    assert hits.shape == (stage.n, 2) and hits.dtype == np.uint32 and flags.shape == (stage.n,) and flags.dtype == np.uint8
    bad = np.argwhere(hits != want_hits)
    assert not len(bad), [(int(j), int(r), stage.cases[int(r)][int(j)][0], len(stage.cases[int(r)][int(j)][1]), int(hits[j, r]), int(want_hits[j, r]))
                          for j, r in bad[:6]]
    assert (flags == want_flags).all(), np.argwhere(flags != want_flags)[:6].tolist()
    got = eng.screen_read()
    assert got.shape == (2 * stage.S + 1, 8) and got.dtype == np.uint64
    if before is not None:
        table = table + before
    assert (got == table).all(), (got.tolist(), table.tolist())
    return table


def _set(eng, P, kmers):
    eng.screen_set(kmers=kmers, **P.keywords())
    assert eng.screen_get() == dict(P.keywords(), n_kmers=len(kmers)) and eng.screen_active()


def test_the_generated_inputs_hold_the_cases():
    rng = np.random.default_rng(1)
    for k in KS:
        ref = Ref(k, k)
        by = {}
        for tag, s, _ in _planted_cases(rng, ref) + _length_cases(rng, ref):
            by.setdefault(tag, []).append(s)
        h = lambda s: SM.scan(s, k, ref.R)  # noqa: E731
        assert all(h(s)[0] == 1 for s in by["first"] + by["last"]) and any(s[:k].islower() for s in by["first"])
        assert all(h(s)[0] == max(0, len(s) - k + 1) == h(s)[1] for s in by["copy"] if len(s) <= len(ref.seq))
        assert len(by["broken"]) == k and all(h(s) == (k + 1, k + 1) for s in by["broken"])  # 2 k + 1 less the k that cover the byte
        assert all(h(s)[0] == len(s) - k + 1 for s in by["homo"]) and all(h(s) == (0, len(s) - k + 1) for s in by["homo-out"])
        assert all(h(s) == (0, 0) for s in by["homo-n"]) and all(h(s)[0] == 0 for s in by["bases"])
        assert any(0 < h(s)[1] < len(s) - k + 1 for s in by["random"])  # k-mers broken by N, IUPAC letters and other bytes
        st = Stage(5, (_planted_cases(rng, ref) + _length_cases(rng, ref), _length_cases(rng, ref)))
        assert {len(s) for _, s, _ in st.cases[0]} >= set(_lens(k))
        for text, recs in ((st.t1, st.r1), (st.t2, st.r2)):
            assert {int(q[3]) % 16 for q in recs if 320 <= q[4] <= 337} == set(range(16))  # at the slab's bound every alignment
            assert {int(q[3]) % 16 for q in recs if q[4]} == set(range(16))
            # lines on both sides of the staged-line limit (21 aligned words)
            assert {((int(q[3]) + 3) % 16 + int(q[4]) + 15) // 16 <= 21 for q in recs if 321 < q[4] <= 336} == {True, False}
            assert b"\r\n" in text
    # the canonical all-ones word cannot be: poly-G at k = 32 reads as poly-C
    assert SM.canonical(b"G" * 32, 0, 32) == 0x5555555555555555 and SM.canonical(b"C" * 32, 0, 32) == 0x5555555555555555


@pytest.mark.parametrize("k", KS)
def test_lengths_alignments_and_planted_kmers_equal_the_model(eng, k):
    rng = np.random.default_rng(100 + k)
    ref = Ref(k, k)
    for action in ("report", "drop"):
        P = SM.Params(k, 1, action)
        _set(eng, P, ref.kmers)
        assert eng.screen_kind() == "lds"
        st = Stage(200 + k, (_planted_cases(rng, ref) + _length_cases(rng, ref), _length_cases(rng, ref) + _planted_cases(rng, ref)))
        table = _check(st, eng, P, ref.R)
        assert (table[:, :6] > 0).all() and (table[:, SM.MATCHED] < table[:, SM.PAIRS]).all()


@pytest.mark.parametrize("min_hits", [1, 2, 5, 65535])
def test_min_hits_counts_both_reads(eng, min_hits):
    """hits in R1 only, in R2 only, and split so that only the pair's sum reaches min_hits"""
    k = 31
    rng = np.random.default_rng(300 + min_hits)
    ref = Ref(31, k)
    split = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 3), (3, 2), (4, 0), (0, 4), (5, 0), (0, 5), (4, 1), (1, 4), (60, 60)]

    def read(h):
        """exactly h hits: k - 1 + h bases of the reference between flanks of A and T that go on with another base than it does"""
        if not h:
            return _rs(rng, 70, b"AT")
        x = ref.piece(rng, k + 1 + h)
        other = lambda b: b"T" if b == ord("A") else b"A"  # noqa: E731
        return _rs(rng, 39, b"AT") + other(x[0]) + x[1:-1] + other(x[-1]) + _rs(rng, 29, b"AT")

    lists = [[_case("h%d" % hs[r], read(hs[r])) for hs in split * 3] for r in (0, 1)]
    st = Stage(0, lists)
    st.cases = lists  # the pairs as listed: Stage shuffles the two streams apart
    (st.t1, st.r1), (st.t2, st.r2) = (_text_from(rng, c) for c in lists)
    for action in ("report", "drop"):
        P = SM.Params(k, min_hits, action)
        _set(eng, P, ref.kmers)
        hits, flags, table = st.model(P, ref.R)
        assert [tuple(x) for x in hits[:len(split)].tolist()] == split
        assert int(table[:, SM.MATCHED].sum()) == 3 * sum(a + b >= min_hits for a, b in split)
        assert flags.any() == (action == "drop" and min_hits < 65535)
        _check(st, eng, P, ref.R)


@pytest.mark.parametrize("n_kmers", [1, 100, LDS_MAX, LDS_MAX + 1, 8192, 8193, 20000])
def test_both_table_placements_equal_the_model(eng, n_kmers):
    """references of 1, 100, exactly the LDS cap (the fullest LDS table), one more (the first in global memory), both sides of a
    power of two of the global table's slots and 20 000"""
    k = 31
    rng = np.random.default_rng(400 + n_kmers % 997)
    src = _rs(rng, 30000)
    words, exists = qscreen.canonical_words(src, k)
    assert exists.all()
    pos = np.sort(rng.choice(len(words), n_kmers, replace=False))
    kmers = np.unique(words[pos])
    assert kmers.size == n_kmers  # (random 31-mers of 30 000 bases do not repeat)
    R = set(int(w) for w in kmers)
    P = SM.Params(k, 1, "report")
    _set(eng, P, kmers)
    assert eng.screen_kind() == ("lds" if n_kmers <= LDS_MAX else "global")
    cases = [[_case("src", src[a:a + L]) for a, L in zip(rng.integers(0, len(src) - 400, 300), rng.choice([31, 64, 151, 330, 400], 300))]
             for _ in (0, 1)]
    cases[0] += [_case("kmer", src[int(p):int(p) + k]) for p in pos[:60]]
    table = _check(Stage(410, cases), eng, P, R)
    assert 0 < int(table[:, SM.HIT_KMERS].sum()) < int(table[:, SM.KMERS].sum())


@pytest.mark.parametrize("n_other", [0, LDS_MAX + 1000])
def test_long_probe_chains(eng, n_other):
    """many words whose probes start in the same few slots (found by search with the library's own hash): half of them in the
    reference, so that members sit deep in a chain and the others walk all of it; in the LDS table and in the global one"""
    k = 31
    rng = np.random.default_rng(500)
    src = _rs(rng, 200000)
    words, _ = qscreen.canonical_words(src, k)
    n_ref = 200 + n_other  # the table's size depends on the count only through the placement and, in global memory, its power of two
    slots = np.array([eng.screen_first_slot(int(w), n_ref) for w in words[:120000]])
    home = int(np.bincount(slots).argmax())
    near = np.flatnonzero((slots >= home) & (slots < home + 16))
    assert 40 <= len(near) < 400
    members, others = near[0::2], near[1::2]
    far = rng.choice(np.arange(120000, len(words)), n_ref - len(members), replace=False)
    kmers = np.unique(words[np.concatenate([members, far])])
    assert kmers.size == n_ref and eng.screen_first_slot(int(words[near[0]]), kmers.size) == slots[near[0]]
    R = set(int(w) for w in kmers)
    P = SM.Params(k, 1, "report")
    _set(eng, P, kmers)
    assert eng.screen_kind() == ("global" if n_other else "lds")
    cases = [[_case("member", src[int(p):int(p) + k + 2]) for p in members], [_case("other", src[int(p):int(p) + k + 2]) for p in others]]
    st = Stage(510, cases)
    table = _check(st, eng, P, R)
    assert int(table[:, SM.HIT_KMERS].sum()) >= len(members)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_stage_pair_counts_and_skipped_pairs(eng, n):
    k = 31
    rng = np.random.default_rng(700 + n)
    ref = Ref(32, k)
    P = SM.Params(k, 2, "drop")
    _set(eng, P, ref.kmers)
    st = Stage(800 + n, (_planted_cases(rng, ref), _length_cases(rng, ref)), n=n)
    assert st.n == n
    table = _check(st, eng, P, ref.R)
    assert int(table[:, 0].sum()) == n
    drop = (rng.integers(0, 3, n) == 0).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)  # a third skipped, any byte
    both = _check(st, eng, P, ref.R, drop=drop, before=table)
    assert int(both[:, 0].sum()) == 2 * n - int((drop != 0).sum())


@pytest.mark.parametrize("S", [1, 1100])
def test_destinations(S):
    """one sample, and more destinations than any table of partials would hold; Undetermined and a code beyond 2 S"""
    k = 31
    rng = np.random.default_rng(900 + S)
    ref = Ref(33, k)
    P = SM.Params(k, 1, "report")
    with hb.Engine(0) as e:
        e.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        e.set_barcodes(_barcodes(S))
        _set(e, P, ref.kmers)
        st = Stage(910, (_planted_cases(rng, ref), _planted_cases(rng, ref)), S=S, n=600)
        st.codes[:4] = (UND, 0, 2 * S - 1, UND)
        st.codes[4:68] = 1  # a wave's four pairs, and more, for one destination
        table = _check(st, e, P, ref.R)
        assert table[2 * S, 0] >= 2 and table[1, 0] >= 64 and (table[:, 0] > 0).sum() >= min(2 * S + 1, 200)
        for code in (2 * S, 0xFFFE):
            c2 = st.codes.copy()
            c2[9] = code
            with pytest.raises(hb.QuadeHipError) as ei:
                e.dev_screen(st.t1, st.r1, st.t2, st.r2, c2)
            assert ei.value.code == hb.QD_ERR_INVALID
        assert (e.screen_read() == table).all()


def test_accumulation_reset_and_add(eng):
    k = 31
    rng = np.random.default_rng(20)
    ref = Ref(34, k)
    P = SM.Params(k, 1, "drop")
    a = Stage(21, (_planted_cases(rng, ref), _planted_cases(rng, ref)), n=300)
    b = Stage(22, (_length_cases(rng, ref), _planted_cases(rng, ref)), n=65)
    _set(eng, P, ref.kmers)
    with hb.Engine(0) as other:
        other.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        other.set_barcodes(_barcodes(3))
        other.screen_set(kmers=ref.kmers, **P.keywords())
        ta = _check(a, eng, P, ref.R)
        both = _check(b, eng, P, ref.R, before=ta)
        eng.reset_counts()
        assert not eng.screen_read().any() and eng.screen_get() == dict(P.keywords(), n_kmers=len(ref.kmers))
        tb = _check(b, eng, P, ref.R)
        _check(a, other, P, ref.R)
        eng.screen_add(other.screen_read())  # a second context's table folds in
        assert (eng.screen_read() == both).all() and (both == ta + tb).all() and (other.screen_read() == ta).all()
        for size in (55, 57, 8):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.screen_add(np.zeros(size, dtype=np.uint64))
            assert ei.value.code == hb.QD_ERR_INVALID
        assert (eng.screen_read() == both).all()
    eng.screen_set(on=False)
    with pytest.raises(hb.QuadeHipError) as ei:
        eng.screen_read()
    assert ei.value.code == hb.QD_ERR_STATE


def test_state_and_errors():
    k = 31
    rng = np.random.default_rng(30)
    ref = Ref(35, k)
    P = SM.Params(k, 2, "drop")
    st = Stage(31, (_planted_cases(rng, ref), _planted_cases(rng, ref)), n=64)
    with hb.Engine(0) as e:
        with pytest.raises(hb.QuadeHipError) as ei:  # plan and barcodes first, as the filter
            e.screen_set(kmers=ref.kmers, **P.keywords())
        assert ei.value.code == hb.QD_ERR_STATE
        e.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        e.set_barcodes(_barcodes(3))
        assert not e.screen_active() and e.screen_get() is None
        for call in (e.screen_read, e.screen_kind, lambda: st.run(e), lambda: e.screen_add(np.zeros((7, 8), np.uint64))):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        assert e.lib.qd_screen_set(e._h, None, None, 0) == 0 and not e.screen_active()  # NULL = off
        e.screen_set(kmers=np.zeros(0, dtype=np.uint64))  # no k-mers = off
        assert not e.screen_active()
        _set(e, P, ref.kmers)
        good = e.screen_get()
        want = _check(st, e, P, ref.R)
        km = ref.kmers
        rcw = lambda w: int("".join("2301"[int(c)] for c in np.base_repr(int(w), 4).zfill(k)[::-1]), 4)  # noqa: E731
        not_canonical = np.array(sorted(max(int(w), rcw(w)) for w in km[:5]), dtype=np.uint64)
        assert all(rcw(w) < int(w) for w in not_canonical)
        lists = dict(unsorted=km[::-1], duplicate=np.concatenate([km[:3], km[2:]]), not_canonical=not_canonical,
                     too_large=np.array([1 << (2 * k)], dtype=np.uint64), too_many=np.arange((1 << 22) + 1, dtype=np.uint64))
        for name, bad in lists.items():
            with pytest.raises(hb.QuadeHipError) as ei:
                e.screen_set(kmers=bad, **P.keywords())
            assert ei.value.code == hb.QD_ERR_INVALID, name
            assert e.screen_get() == good and e.screen_active()  # a rejected call changes nothing
        for bad in (dict(kmer=14), dict(kmer=33), dict(kmer=0), dict(min_hits=0), dict(min_hits=65536), dict(min_hits=-1), dict(action=2),
                    dict(action=-1)):
            with pytest.raises(hb.QuadeHipError) as ei:
                e.screen_set(kmers=km, **dict(P.keywords(), **bad))
            assert ei.value.code == hb.QD_ERR_INVALID, bad
            assert e.screen_get() == good and e.screen_active()
        want = _check(st, e, P, ref.R, before=want)  # ... and the previous state still gives the model's result
        out = np.zeros(55, dtype=np.uint64)
        assert e.lib.qd_screen_read(e._h, hb._ptr(out), 55) == hb.QD_ERR_INVALID
        # a bad table never becomes an address: refused on the host, nothing launched, the table as it was
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            e.dev_screen(st.t1, bad, st.t2, st.r2, st.codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            e.dev_screen(st.t1, st.r1, st.t2, bad, st.codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        assert (e.screen_read() == want).all()
        e.filter_set(max_n=2)  # the other stages leave the screen alone
        e.posttrim_set(tail_n=1)
        assert e.screen_get() == good and (e.screen_read() == want).all()
        e.set_barcodes(_barcodes(4))  # new barcodes turn the stage off, as they do the read filter
        with pytest.raises(hb.QuadeHipError) as ei:
            e.screen_read()
        assert ei.value.code == hb.QD_ERR_STATE and e.screen_get() is None
        _set(e, P, km)
        assert e.screen_read().shape == (9, 8)
        e.set_plan(hb.make_plan(True, 20, (0, 8), (0, 8)))  # and so does a new plan
        assert not e.screen_active()


def test_all_eight_stages_in_one_context(torch_cuda):
    """every stage of hb.PIPE_STAGES on and run over one small batch: a screen_add reaches its own table and no other, and a
    table one value short is refused and changes nothing"""
    rng = np.random.default_rng(40)
    S, n, k = 2, 17, 15
    ref = Ref(36, k)
    cases = [[_case("pair", (ref.piece(rng, 20) if j % 3 == 0 else _rs(rng, 10, b"CGT") + b"A" * 10) + (b"N" if j % 4 == 1 else b"")) for j in range(n)]
             for _ in range(2)]
    (t1, r1), (t2, r2) = (_text_from(rng, c) for c in cases)
    codes = np.array([(0, 3, UND)[j % 3] for j in range(n)], dtype=np.uint16)
    P = SM.Params(k, 1, "report")
    with hb.Engine(0) as e:
        e.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        e.set_barcodes(_barcodes(S))
        e.qstats_enable(True)
        e.cstats_enable(True)
        e.clip_set(tail_clip_r1=1, min_length=5)
        e.trim_set("AGATCGGAAG", "AGATCGGAAG", 20, 3, 10, 4)
        e.pairtrim_set(min_overlap=8, max_mismatches=2, max_mismatch_pct=20, min_length=6)
        e.posttrim_set(tail_n=1, poly_x_min_length=6)
        e.filter_set(min_length=18, max_n=1)
        e.screen_set(kmers=ref.kmers, **P.keywords())
        assert [s.name for s in hb.PIPE_STAGES] == ["quality", "cycle", "clip", "trim", "pairtrim", "posttrim", "filter", "screen"]
        for s in hb.PIPE_STAGES:
            args = (t1, r1, t2, r2) + ((codes,) if s.engine in ("qstats", "cstats", "filter", "screen") else ())
            getattr(e, "dev_" + s.engine)(*args)
        read_all = lambda: {s.name: np.asarray(s.read(e)).reshape(-1).copy() for s in hb.PIPE_STAGES}  # noqa: E731
        t0 = read_all()
        want = SM.new_table(S)
        for j in range(n):
            SM.count(want, int(codes[j]), cases[0][j][1], cases[1][j][1], P, ref.R)
        assert t0["screen"].size == 40 and (t0["screen"] == np.array(want, dtype=np.uint64).reshape(-1)).all()
        assert all(t.any() for t in t0.values()) and want[0][SM.MATCHED] > 0
        e.screen_add(np.full(40, 7, dtype=np.uint64))
        now = read_all()
        assert (now["screen"] == t0["screen"] + np.uint64(7)).all()
        assert all((now[name] == t0[name]).all() for name in t0 if name != "screen")
        with pytest.raises(hb.QuadeHipError) as ei:
            e.screen_add(np.ones(39, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        after = read_all()
        assert all((after[name] == now[name]).all() for name in now)


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
K_CLI = 31
REF_CLI = Ref(77, K_CLI, bases=6000)
N_CHUNK = 1500


def _inserts(g, i, sample, kind):
    """plain fragments, about a fifth of the pairs off the reference instead: most of the pairs with an unknown index (kind 0,
    Undetermined) and a tenth of the others; every other such pair with a substitution or an N or in lower case; and one pair in
    fifty a random pair with a single k-mer of the reference planted in one read"""
    rng = g.rng
    from_ref = rng.integers(0, 10) < (8 if kind == 0 else 1)
    I = int(rng.integers(40, 331))
    if from_ref:
        a = int(rng.integers(0, len(REF_CLI.seq) - I))
        frag = REF_CLI.seq[a:a + I].decode()
    else:
        frag = g.rnd(I)
    out = []
    for r, src in enumerate((frag, _rc(frag.encode()).decode())):
        Lr = int(rng.integers(30, 152))
        s = list((src + g.rnd(151))[:Lr])
        if i % 2:
            for _ in range(int(rng.integers(0, 3))):
                s[int(rng.integers(0, Lr))] = "ACGTNn"[int(rng.integers(0, 6))]
        s = "".join(s)
        if i % 50 == 7 and r == i % 100 // 50 and Lr >= 40:
            a, p = int(rng.integers(0, len(REF_CLI.seq) - K_CLI)), int(rng.integers(0, Lr - K_CLI + 1))
            s = s[:p] + REF_CLI.seq[a:a + K_CLI].decode() + s[p + K_CLI:]
        out.append((s.lower() if i % 11 == 0 else s, g.q(Lr, 2, 42)))
    return out


def _dataset(d, seed, n_chunks, n, bgzf):
    return SS._dataset(d, seed, n_chunks, n, bgzf, _inserts, SS._same_places, sample_first=True)


def _section(top, action="report", min_hits=1):
    path = os.path.join(str(top), "spike.fa")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(REF_CLI.fasta)
    return "[screen]\nreference : %s\nkmer : %d\nmin_hits : %d\naction : %s\n" % (path, K_CLI, min_hits, action)


def _params(P):
    return dict(P.keywords(), reference=dict(name="spike.fa", records=2, bases=len(REF_CLI.seq) + 40, kmers=len(REF_CLI.kmers)))


def _names(samples):
    return [s[0] for s in samples]


def _check_run(mine, ref, texts, table, names, P, only=None):
    SS._check_files(mine, texts, only)
    SS._check_main_report(mine, ref, only)  # as without the stage
    SS._check_report(mine, sr, table, names, _params(P))
    for other in (fr, xr, qr):  # the section turns nothing else on
        SS._check_report(mine, other, None)


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF, run once with action report; the models over the oracle's outputs"""
    top = tmp_path_factory.mktemp("screen_bgzf")
    files, samples = _dataset(str(top / "data"), 91, 2, N_CHUNK, bgzf=True)
    names = _names(samples)
    plain = top / "plain.txt"
    SS._write_conf(plain, files, samples)
    SS._oracle_run(plain, top / "ref")
    P = SM.Params(K_CLI, 1, "report")
    texts, table = SM.screened_outputs(str(top / "ref"), names, P, REF_CLI.R)
    conf = top / "conf.txt"
    SS._write_conf(conf, files, samples, extra=_section(top))
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, names=names, texts=texts, table=table, mine=top / "mine", ref=top / "ref", plain=plain, P=P)


def test_cli_report_bgzf(bgzf_run):
    run = bgzf_run
    t = run["table"]
    S = len(run["names"])
    assert sum(row[0] for row in t) < 2 * N_CHUNK
    by_sample = [[a + b for a, b in zip(t[2 * i], t[2 * i + 1])] for i in range(S)] + [t[2 * S]]
    assert all(0 < row[SM.MATCHED] < row[SM.PAIRS] for row in by_sample)  # every sample and Undetermined: matched and unmatched pairs
    assert all(row[c] > 0 for row in by_sample for c in range(8)) and t[2 * S][SM.MATCHED] * 2 > t[2 * S][SM.PAIRS]
    assert run["texts"] == {f: _gz(os.path.join(str(run["ref"]), f)) for f in run["texts"]}  # action report: the oracle's files
    _check_run(run["mine"], run["ref"], run["texts"], t, run["names"], run["P"])


def test_cli_drop_bgzf(bgzf_run, tmp_path):
    """action drop: the matched pairs are in no file, Quade_report.csv as without the stage; with min_hits 3 the pairs with a single
    planted k-mer stay"""
    run = bgzf_run
    for min_hits in (1, 3):
        P = SM.Params(K_CLI, min_hits, "drop")
        texts, table = SM.screened_outputs(str(run["ref"]), run["names"], P, REF_CLI.R)
        assert texts != run["texts"] and (min_hits == 1) == (table == run["table"])
        conf = tmp_path / ("drop%d.txt" % min_hits)
        SS._write_conf(conf, run["files"], run["samples"], extra=_section(run["top"], "drop", min_hits))
        _cli(conf, tmp_path / ("drop%d" % min_hits))
        _check_run(tmp_path / ("drop%d" % min_hits), run["ref"], texts, table, run["names"], P)


def test_cli_ordinary_gzip_and_a_destination_that_loses_all_its_pairs(torch_cuda, tmp_path):
    """ordinary gzip input, both actions; write_fail off and min_hits 1 on a dataset whose every pair of one destination matches"""
    files, samples = _dataset(str(tmp_path / "data"), 92, 1, 2000, bgzf=False)
    names = _names(samples)
    SS._write_conf(tmp_path / "plain.txt", files, samples)
    SS._oracle_run(tmp_path / "plain.txt", tmp_path / "ref")
    for action in ("report", "drop"):
        P = SM.Params(K_CLI, 1, action)
        texts, table = SM.screened_outputs(str(tmp_path / "ref"), names, P, REF_CLI.R)
        SS._write_conf(tmp_path / (action + ".txt"), files, samples, extra=_section(tmp_path, action))
        _cli(tmp_path / (action + ".txt"), tmp_path / action)
        _check_run(tmp_path / action, tmp_path / "ref", texts, table, names, P)
    # k = 15 over a reference that holds every read of sample 0's pass pairs: that destination has no files
    stem = names[0] + "_pass"
    reads = [seq for r in ("_R1", "_R2") for seq, _ in QM.fastq_records(os.path.join(str(tmp_path / "ref"), stem + r + ".fastq.gz"))]
    with open(tmp_path / "all.fa.gz", "wb") as fh:
        import gzip
        fh.write(gzip.compress(_fasta([s for s in reads if len(s) >= 15], width=60)))
    P = SM.Params(15, 1, "drop")
    R = SM.kmers_of(qscreen.read_fasta(str(tmp_path / "all.fa.gz")), 15)
    texts, table = SM.screened_outputs(str(tmp_path / "ref"), names, P, R)
    assert stem + "_R1.fastq.gz" not in texts and table[0][SM.MATCHED] == table[0][SM.PAIRS] > 0 and len(texts) >= 10
    SS._write_conf(tmp_path / "lose.txt", files, samples, extra="[screen]\nreference : %s\nkmer : 15\naction : drop\n" % (tmp_path / "all.fa.gz"))
    _cli(tmp_path / "lose.txt", tmp_path / "lose")
    SS._check_files(tmp_path / "lose", texts)
    SS._check_main_report(tmp_path / "lose", tmp_path / "ref")
    ref = qscreen.reference_kmers(qscreen.read_fasta(str(tmp_path / "all.fa.gz")), 15)
    assert ref.kmers.size == len(R) > LDS_MAX  # (and this reference is looked up in global memory)
    SS._check_report(tmp_path / "lose", sr, table, names,
                     dict(P.keywords(), reference=dict(name="all.fa.gz", records=ref.records, bases=ref.bases, kmers=len(R))))


def test_cli_every_stage_on(bgzf_run, tmp_path):
    """the models chained in pipeline order -- [trim], pair_overlap, post-trim, [filter], screen with action drop -- then the
    quality, cycle and duplication reports over the files as written; the filter's report is what it is without the screen"""
    run = bgzf_run
    names = run["names"]
    POST = "tail_n : True\npoly_x : True\n"
    P_POST = XM.Params(tail_n=1, poly_x_min_length=10, min_length=25)
    P = SM.Params(K_CLI, 2, "drop")
    paired, second, first = PM.trimmed_outputs(str(run["ref"]), P_PAIR, trim=P_TRIM)
    post, xtable = XM.posttrimmed_outputs(XM.write_outputs(paired, str(tmp_path / "paired")), P_POST)
    kept, ftable, _, _ = FM.filtered_outputs(XM.write_outputs(post, str(tmp_path / "post")), names, P_F)
    texts, table = SM.screened_outputs(SM.write_outputs(kept, str(tmp_path / "kept")), names, P, REF_CLI.R)
    assert texts != kept and sum(row[SM.MATCHED] for row in table) > 50
    assert sum(row[0] for row in table) == sum(row[0] - sum(row[1:6]) for row in ftable)  # only pairs the filter kept
    out = "[output]\nquality_report : True\ncycle_report : True\nduplication_report : True\nduplication_sample : 1\n"
    conf = tmp_path / "all.txt"
    SS._write_conf(conf, run["files"], run["samples"], extra=TRIMS + POST + FILTER + _section(run["top"], "drop", 2))
    text = _read(conf).replace("[output]\n", out, 1)
    open(conf, "w").write(text)
    mine = tmp_path / "all"
    _cli(conf, mine)
    SS._check_files(mine, texts)
    SS._check_main_report(mine, run["ref"])
    SS._check_report(mine, sr, table, names, _params(P))
    SS._check_report(mine, fr, ftable, names, P_F.keywords())  # unchanged by the screen
    SS._check_report(mine, xr, xtable, P_POST.keywords())
    assert _read(mine / qr.REPORT_NAME) == "\n".join(qr.report_lines(QM.table_from_outputs(str(mine), names), names)) + "\n"
    assert _read(mine / yr.REPORT_NAME) == "\n".join(yr.report_lines(YM.table_from_outputs(str(mine), names))) + "\n"
    stems = [n + q for n in names for q in ("_pass", "_fail")] + ["Undetermined"]
    pairs = []
    for d, stem in enumerate(stems):
        p1, p2 = (os.path.join(str(mine), stem + r + ".fastq.gz") for r in ("_R1", "_R2"))
        if os.path.exists(p1):
            pairs += [(UND if d == 2 * len(names) else d, a[0], b[0], 0) for a, b in zip(QM.fastq_records(p1), QM.fastq_records(p2))]
    slots = 1 << 24
    dtable, dstats = DM.tally(len(names), pairs, DM.Params(32, 1, slots))
    keys, counts = DM.arrays(dtable)
    assert _read(mine / dr.REPORT_NAME) == "\n".join(dr.report_lines(dstats, keys, counts, names, dict(bases=32, sample=1, slots=slots))) + "\n"


def test_cli_chunk_workers_and_write_flags(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "flags.txt"
    SS._write_conf(conf, run["files"], run["samples"], flags=(True, False, False), gpu="chunk_workers : 2\n", extra=_section(run["top"]))
    _cli(conf, tmp_path / "flags")  # the counters do not depend on what is written; the files are absent
    _check_run(tmp_path / "flags", run["ref"], run["texts"], run["table"], run["names"], run["P"], only=lambda f: "_pass_" in f)


def test_cli_two_ranks_sharded_and_whole_chunks(bgzf_run, tmp_path):
    """2 ranks on GPU 0 (tables through the rendezvous files): each a pair range of ONE shared BGZF chunk, then a chunk each"""
    run = bgzf_run
    P = SM.Params(K_CLI, 1, "drop")
    SS._write_conf(tmp_path / "plain.txt", run["files"], run["samples"], chunks=[0])
    SS._oracle_run(tmp_path / "plain.txt", tmp_path / "ref")
    texts, table = SM.screened_outputs(str(tmp_path / "ref"), run["names"], P, REF_CLI.R)
    assert table != run["table"]
    conf = tmp_path / "shared.txt"
    SS._write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : True\n", chunks=[0], extra=_section(run["top"], "drop"))
    _cli(conf, tmp_path / "shared", ranks=2)
    _check_run(tmp_path / "shared", tmp_path / "ref", texts, table, run["names"], P)
    conf = tmp_path / "two.txt"
    SS._write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n", extra=_section(run["top"]))
    _cli(conf, tmp_path / "two", ranks=2)
    _check_run(tmp_path / "two", run["ref"], run["texts"], run["table"], run["names"], run["P"])
    assert not [f for f in os.listdir(tmp_path / "two") if f.startswith(".quade_rdv")]


def test_cli_without_the_section_nothing_changes(bgzf_run, tmp_path):
    run = bgzf_run
    _cli(run["plain"], tmp_path / "off")
    empty = tmp_path / "empty.txt"
    open(empty, "w").write(_read(run["plain"]) + "[screen]\nreference :\nkmer : 31\n")  # an empty reference: off
    _cli(empty, tmp_path / "empty")
    assert not os.path.exists(tmp_path / "off" / sr.REPORT_NAME) and not os.path.exists(tmp_path / "empty" / sr.REPORT_NAME)
    _compare_dirs(str(tmp_path / "off"), str(run["ref"]))
    for f in sorted(os.listdir(tmp_path / "off")):
        if f.endswith(".fastq.gz"):
            assert open(tmp_path / "off" / f, "rb").read() == open(tmp_path / "empty" / f, "rb").read(), f
            assert open(tmp_path / "off" / f, "rb").read() == open(run["mine"] / f, "rb").read(), f  # action report writes the same bytes
    assert sorted(os.listdir(tmp_path / "off")) == sorted(os.listdir(tmp_path / "empty")) == \
        sorted(f for f in os.listdir(run["mine"]) if f != sr.REPORT_NAME)
    with hb.Engine(0) as e:
        e.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        e.set_barcodes(_barcodes(2))
        assert not e.screen_active() and e.screen_get() is None
