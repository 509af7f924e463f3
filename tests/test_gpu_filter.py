"""The read filter on the MI355X (qd_filter_*, quade_amd/csrc/quade_filter.hip): the reason bytes and the table equal
tests/filter_model.py's plain Python rule, exactly -- for the stage on its own (qd_dev_filter: every length class at every
alignment, both sides of every rule's threshold, poly-A and alternating reads, neighbour pairs across the kernel's dword, lane
and step boundaries, guard bytes around the lines, quality bytes below 33 and above 127, both accumulation paths, accumulation,
state and errors) and through the command line (every output file against the oracle's file filtered by the model, the reports,
chunk workers, write flags, ranks, every pair dropped, the section absent)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import quade_oracle as qo
from quade_amd import filter_report as fr
from quade_amd import hip_backend as hb
from quade_amd import pair_trim_report as pr
from quade_amd import quality_report as qr
from quade_amd import trim_report as tr
from tests import filter_model as FM
from tests import pairtrim_model as PM
from tests import qstats_model as QM
from tests import stage_support as SS
from tests.run_support import _gz
from tests.stage_support import (BASES, FILTER, P_F, P_PAIR, P_TRIM, POLY_G, QUALS, TRIM_KW, TRIMS, _barcodes, _cli,  # noqa: F401
                                 torch_cuda)
from tests.stage_support import _filter_dataset as _dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UND = FM.UNDETERMINED
LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 150, 151, 255, 256, 257, 300, 2049)
S_STAGE = 3
UPLOAD_SHIFT = 3  # qd_dev_filter uploads a text 3 bytes into an aligned buffer: byte o of the text lies at address o + 3 (mod 16)

# the rule sets: each rule alone, the complexity rule at both ends of its range, max_n at 0, all together
RULES = {
    "min_length": dict(min_length=16),
    "max_n": dict(max_n=3),
    "max_n_0": dict(max_n=0),
    "low_quality": dict(max_unqualified_pct=40),
    "low_quality_q30": dict(max_unqualified_pct=0, qualified_quality=30),
    "mean_quality": dict(min_mean_quality=20),
    "complexity": dict(min_complexity_pct=30),
    "complexity_1": dict(min_complexity_pct=1),
    "complexity_100": dict(min_complexity_pct=100),
    "all": dict(min_length=16, max_n=3, max_unqualified_pct=40, qualified_quality=15, min_mean_quality=20, min_complexity_pct=30),
}


def _with_diffs(rng, L, D):
    """a read of L letters of ACGT in either case whose neighbours differ exactly at the positions i of D (s[i] != s[i + 1])"""
    s, cur = bytearray(L), int(rng.integers(0, 4))
    for i in range(L):
        s[i] = b"ACGT"[cur] | (0x20 if rng.integers(0, 2) else 0)
        if i in D:
            cur = (cur + 1 + int(rng.integers(0, 3))) % 4
    return bytes(s)


def _straddles(s):
    """for a line whose first byte lies at address s (mod 16): the position i whose neighbour pair (i, i + 1) lies across a dword
    boundary inside a lane's 16 bytes, across a lane boundary inside a 256-byte step, and across a step boundary"""
    return {"dword": (3 - s) % 16, "lane": (15 - s) % 16 + 16, "step": 255 - s}


def _cases(rng):
    """[(tag, read1, read2)], a read = dict(seq, qual, align (address of the sequence line mod 16, or None), style)"""
    out = []

    def rs(L, alphabet=b"ACGT"):
        return bytes(alphabet[int(v)] for v in rng.integers(0, len(alphabet), L))

    def read(seq, qual=None, align=None, style=None):
        return dict(seq=seq, qual=b"I" * len(seq) if qual is None else qual, align=align, style=style)

    def good():
        return read(rs(60))

    def both(tag, r):
        out.append((tag + "/1", r, good()))
        out.append((tag + "/2", good(), dict(r)))

    for L in LENS:  # every length class at all 16 alignments, random bytes of every kind
        for a in range(16):
            r = read(rs(L, BASES), rs(L, QUALS), align=a, style=a % 3)
            out.append(("len%d" % L, r, read(rs(int(rng.integers(17, 200)), BASES), None)) if a % 2 else ("len%d" % L, good(), r))
        for a in range(16):  # poly-A in both cases: diff is exactly 0; alternating AC: exactly L - 1 (its mate alternates too)
            out.append(("poly%d" % L, read(bytes(b"Aa"[int(v)] for v in rng.integers(0, 2, L)), align=a, style=a % 3), good()))
            alt = bytes(b"ACac"[(i & 1) + 2 * int(rng.integers(0, 2))] for i in range(L))
            out.append(("alt%d" % L, read(b"GT" * 20), read(alt, align=a, style=(a + 1) % 3)))
    for k in (2, 3, 4, 0, 1):  # max_n : 3 and max_n : 0
        s = bytearray(rs(50))
        for i in rng.permutation(50)[:k]:
            s[int(i)] = b"Nn"[int(rng.integers(0, 2))]
        both("n%d" % k, read(bytes(s)))
    for k in (19, 20, 21):  # max_unqualified_pct : 40 of 50 bases; the unqualified ones one below qualified_quality : 15
        q = bytearray(b"I" * 50)
        pos = [int(i) for i in rng.permutation(50)]
        for i in pos[:k]:
            q[i] = 33 + 14
        for i in pos[k:k + 10]:
            q[i] = 33 + 15
        both("unq%d" % k, read(rs(50), bytes(q)))
    for d in (-1, 0, 1):  # min_mean_quality : 20 of 50 bases: qsum 999, 1000, 1001
        q = bytearray([33 + 20] * 50)
        q[int(rng.integers(0, 50))] += d
        both("mean%+d" % d, read(rs(50), bytes(q)))
    for d in (-1, 0, 1):  # qualified_quality : 30 with max_unqualified_pct : 0: one base at 29, 30, 31
        q = bytearray(b"I" * 50)
        q[int(rng.integers(0, 50))] = 33 + 30 + d
        both("q30%+d" % d, read(rs(50), bytes(q)))
    for k in (14, 15, 16):  # min_complexity_pct : 30 of the 50 neighbour pairs of 51 bases
        both("diff%d" % k, read(_with_diffs(rng, 51, {int(i) for i in rng.permutation(50)[:k]})))
    # min_complexity_pct : 30 of the 300 neighbour pairs of 301 bases, 90 and 89 of them differing, one across each boundary
    for a in range(16):
        for kind, i in _straddles(a).items():
            for k in (90, 89):
                D = {i} | set([int(x) for x in rng.permutation(300) if int(x) != i][:k - 1])
                assert len(D) == k
                out.append(("%s%d" % (kind, k), read(_with_diffs(rng, 301, D), align=a, style=a % 3), good()))
            # ... and the only differing pair of the read
            out.append(("%s1" % kind, good(), read(_with_diffs(rng, 301, {i}), align=a, style=(a + 2) % 3)))
    # lines between bytes that would change every counter if read
    out.append(("guarded", read(b"A" + rs(98) + b"C", bytes([33 + 20] * 100), style=2), read(b"C" + rs(30) + b"G", bytes([33 + 20] * 32), style=2)))
    for _ in range(120):  # reads of any length, any bytes
        L1, L2 = int(rng.integers(0, 330)), int(rng.integers(0, 330))
        out.append(("any", read(rs(L1, BASES), rs(L1, QUALS)), read(rs(L2, BASES), rs(L2, QUALS))))
    for _ in range(60):  # ordinary reads: most of them pass
        L1, L2 = int(rng.integers(10, 160)), int(rng.integers(10, 160))
        out.append(("plain", read(rs(L1, b"ACGTACGTACGTN"), bytes(33 + int(v) for v in rng.integers(10, 42, L1))),
                    read(rs(L2), bytes(33 + int(v) for v in rng.integers(10, 42, L2)))))
    return out


def _build(rng, reads):
    """The text of the reads with its record table (qd_dev_fastq_scan's layout).  style 0: a fastq record with LF, 1: with CRLF,
    2: the sequence line between 'N' and 'n' and the quality line between two bytes 0xFF (the table alone says where a line is).
    align: the name is padded until the sequence line starts at that address mod 16 on the device."""
    parts, recs, pos = [], np.zeros((len(reads), 6), dtype=np.uint32), 0
    for i, r in enumerate(reads):
        seq, qual, L = r["seq"], r["qual"], len(r["seq"])
        style = int(rng.integers(0, 3)) if r["style"] is None else r["style"]
        align = int(rng.integers(0, 16)) if r["align"] is None else r["align"]
        nl = b"\r\n" if style == 1 else b"\n"
        g = (b"N", b"n", b"\xff", b"\xff") if style == 2 else (b"", b"", b"", b"")
        name = b"r%d" % i
        name += b"x" * ((align - (pos + 1 + len(name) + len(nl) + len(g[0]) + UPLOAD_SHIFT)) % 16)
        rec = b"@" + name + nl + g[0] + seq + g[1] + nl + b"+" + nl + g[2] + qual + g[3] + nl
        seq_at = pos + 1 + len(name) + len(nl) + len(g[0])
        recs[i] = (pos, pos + 1, len(name), seq_at, L, seq_at + L + len(g[1]) + 2 * len(nl) + 1 + len(g[2]))
        assert (seq_at + UPLOAD_SHIFT) % 16 == align
        parts.append(rec)
        pos += len(rec)
    return b"".join(parts), recs


class Stage(object):
    def __init__(self, seed, n=None, S=S_STAGE, dests=None):
        rng = np.random.default_rng(seed)
        cases = _cases(rng)
        cases = [cases[int(i)] for i in rng.permutation(len(cases))]
        if n is not None:
            while len(cases) < n:
                cases = cases + cases
            cases = cases[:n]
        self.cases, self.n, self.S = cases, len(cases), S
        self.t1, self.r1 = _build(rng, [a for _, a, _ in cases])
        self.t2, self.r2 = _build(rng, [b for _, _, b in cases])
        lo = 0 if dests is None else 2 * S + 1 - dests
        codes = rng.integers(lo, 2 * S + 1, self.n)
        codes[codes == 2 * S] = UND
        self.codes = codes.astype(np.uint16)
        self._models = {}

    def pairs(self):
        """((seq, qual), (seq, qual)) per pair, by the tables"""
        out = []
        for q1, q2 in zip(self.r1, self.r2):
            out.append(tuple((t[int(q[3]):int(q[3]) + int(q[4])], t[int(q[5]):int(q[5]) + int(q[4])]) for t, q in ((self.t1, q1), (self.t2, q2))))
        return out

    def model(self, name, P=None):
        """-> (reasons uint8[n], table uint64[2S+1, 8]); computed once per rule set"""
        if name not in self._models:
            P = FM.Params(**RULES[name]) if P is None else P
            table = FM.new_table(self.S)
            why = [FM.count(table, int(c), a, b, P) for c, (a, b) in zip(self.codes, self.pairs())]
            self._models[name] = (np.array(why, dtype=np.uint8), np.array(table, dtype=np.uint64))
        return self._models[name]

    def run(self, eng):
        return eng.dev_filter(self.t1, self.r1, self.t2, self.r2, self.codes)


def _engine(S=S_STAGE, **kw):
    eng = hb.Engine(0)
    eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
    eng.set_barcodes(_barcodes(S))
    if kw:
        eng.filter_set(**kw)
    return eng


def _check(stage, eng, name, before=None, P=None):
    got = stage.run(eng)
    want, table = stage.model(name, P)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.flatnonzero(got != want)
    assert not len(bad), [(int(j), stage.cases[int(j)][0], int(got[j]), int(want[j])) for j in bad[:8]]
    values = eng.filter_read()
    assert values.shape == table.shape and values.dtype == np.uint64
    if before is not None:
        table = table + before
    assert (values == table).all(), np.argwhere(values != table)[:8]
    return table


@pytest.fixture(scope="module")
def stage():
    return Stage(2)


def test_the_generated_input_holds_the_cases(stage):
    st = stage
    assert 1000 < st.n < 2048
    by = {}
    for (tag, _, _), pair in zip(st.cases, st.pairs()):
        by.setdefault(tag, []).append(pair)
    for (tag, a, b), (p1, p2) in zip(st.cases, st.pairs()):
        assert p1 == (a["seq"], a["qual"]) and p2 == (b["seq"], b["qual"])  # the tables point at the reads
    P0 = FM.Params()
    counts = lambda r: FM.read_counts(r[0], r[1], P0)  # noqa: E731
    for L in LENS:  # every length at all 16 addresses mod 16, in both streams together; poly-A and alternating reads of every length
        starts = {(int(q[3]) + UPLOAD_SHIFT) % 16 for t, q1, q2 in zip(st.cases, st.r1, st.r2) if t[0] == "len%d" % L for q in (q1, q2) if q[4] == L}
        assert starts == set(range(16)), L
        assert len(by["poly%d" % L]) == 16 and all(counts(p[0])[0] == L and counts(p[0])[4] == 0 for p in by["poly%d" % L])
        assert len(by["alt%d" % L]) == 16 and all(counts(p[1])[0] == L and counts(p[1])[4] == max(L - 1, 0) for p in by["alt%d" % L])
        assert {(int(q[3]) + UPLOAD_SHIFT) % 16 for t, q in zip(st.cases, st.r1) if t[0] == "poly%d" % L} == set(range(16))
    assert any(set(p[0][0]) == {ord("A"), ord("a")} for p in by["poly300"])
    one = lambda name, tag: [FM.reason(*p, FM.Params(**RULES[name])) for p in by[tag]]  # noqa: E731
    # both sides of every threshold, in R1 and in R2
    for side in ("/1", "/2"):
        assert [one("min_length", "len%d" % L).count(1) > 0 for L in (15, 16, 17)] == [True, False, False]
        assert [one("max_n", "n%d%s" % (k, side)) for k in (2, 3, 4)] == [[0], [0], [2]]
        assert [one("max_n_0", "n%d%s" % (k, side)) for k in (0, 1)] == [[0], [2]]
        assert [one("low_quality", "unq%d%s" % (k, side)) for k in (19, 20, 21)] == [[0], [0], [3]]
        assert [one("low_quality_q30", "q30%+d%s" % (d, side)) for d in (-1, 0, 1)] == [[3], [0], [0]]
        assert [one("mean_quality", "mean%+d%s" % (d, side)) for d in (-1, 0, 1)] == [[4], [0], [0]]
        assert [one("complexity", "diff%d%s" % (k, side)) for k in (14, 15, 16)] == [[5], [0], [0]]
        assert [one("all", "diff%d%s" % (k, side)) for k in (14, 15, 16)] == [[5], [0], [0]]
    assert [counts(by["unq%d/1" % k][0][0])[2] for k in (19, 20, 21)] == [19, 20, 21] and 33 + 15 in by["unq20/1"][0][0][1]
    assert [counts(by["mean%+d/2" % d][0][1])[3] for d in (-1, 0, 1)] == [999, 1000, 1001]
    assert all(r == 1 for L in (0, 1, 2, 15) for r in one("all", "poly%d" % L))  # the first rule wins over the complexity of poly-A
    assert set(one("complexity_1", "poly300")) == {5} and set(one("complexity_100", "alt300")) == {0} and set(one("complexity_100", "poly300")) == {5}
    # a differing neighbour pair across a dword, a lane and a step boundary of the kernel's reading, at every alignment
    seen = set()
    for (tag, a, b), q1, q2 in zip(st.cases, st.r1, st.r2):
        for kind in ("dword", "lane", "step"):
            if tag.startswith(kind):
                q, r = (q1, a) if tag[len(kind):] != "1" else (q2, b)
                s = (int(q[3]) + UPLOAD_SHIFT) % 16
                i = _straddles(s)[kind]
                o = s + i  # the byte's place in the aligned words of the line
                assert (r["seq"][i] & 0xDF) != (r["seq"][i + 1] & 0xDF) and int(q[4]) == 301
                assert {"dword": o % 4 == 3 and o % 16 != 15, "lane": o % 16 == 15 and o % 256 != 255, "step": o % 256 == 255}[kind]
                seen.add((kind, s, tag[len(kind):]))
    assert len(seen) == 3 * 16 * 3
    for kind in ("dword", "lane", "step"):
        assert set(one("complexity", kind + "90")) == {0} and set(one("complexity", kind + "89")) == {5}
        assert all(counts(p[1])[4] == 1 for p in by[kind + "1"])
    # guard bytes: read with the line, every counter would change
    (s1, q1), (s2, q2) = by["guarded"][0]
    for s, q in ((s1, q1), (s2, q2)):
        a, b = FM.read_counts(s, q, P0), FM.read_counts(b"N" + s + b"n", b"\xff" + q + b"\xff", P0)
        assert all(a[k] != b[k] for k in (0, 1, 3, 4))  # L, n_count, qsum, diff
        assert FM.read_counts(s, b"\x00" + q[1:], P0)[2] == 1  # ... and a low byte would be unqualified
    i = [t[0] for t in st.cases].index("guarded")
    q = st.r1[i]
    assert st.t1[int(q[3]) - 1:int(q[3])] == b"N" and st.t1[int(q[3]) + int(q[4]):][:1] == b"n"
    assert st.t1[int(q[5]) - 1:int(q[5])] == b"\xff" and st.t1[int(q[5]) + int(q[4]):][:1] == b"\xff"
    assert b"\r\n" in st.t1 and b"\r\n" in st.t2
    allq = b"".join(p[r][1] for p in st.pairs() for r in (0, 1))
    assert set(QUALS) <= set(allq) and min(allq) < 33 and max(allq) > 127
    # every reason and every destination occur under the full rule set
    why, table = st.model("all")
    assert set(int(x) for x in why) == {0, 1, 2, 3, 4, 5} and (table[:, 0] > 0).all() and table.shape == (7, 8)
    assert int(table[:, 0].sum()) == st.n and 0.2 * st.n < int((why == 0).sum()) < 0.9 * st.n
    assert (table[:, 1:6].sum(axis=1) <= table[:, 0]).all() and (table[:, 7] <= table[:, 6]).all() and table[:, 7].sum() > 0


@pytest.mark.parametrize("name", sorted(RULES))
def test_stage_equals_the_model(torch_cuda, stage, name):
    with _engine(**RULES[name]) as eng:
        assert eng.filter_kind() == hb.FILTER_KIND_LDS
        assert eng.filter_get() == FM.Params(**RULES[name]).keywords()
        _check(stage, eng, name)


def test_every_rule_off_is_the_stage_off(torch_cuda, stage):
    with _engine() as eng:
        for kw in (dict(), dict(qualified_quality=20), dict(on=False)):
            eng.filter_set(**kw)
            assert eng.filter_get() == FM.Params().keywords()
            with pytest.raises(hb.QuadeHipError) as ei:
                stage.run(eng)
            assert ei.value.code == hb.QD_ERR_STATE


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 2049])
def test_stage_pair_counts(torch_cuda, n):
    with _engine(**RULES["all"]) as eng:
        st = Stage(3, n=n)
        assert st.n == n
        table = _check(st, eng, "all")
        assert int(table[:, 0].sum()) == n


@pytest.mark.parametrize("S,kind", [(1023, hb.FILTER_KIND_LDS), (1024, hb.FILTER_KIND_GLOBAL)])
def test_stage_both_sides_of_the_lds_limit(torch_cuda, S, kind):
    """the last 41 destinations of the table; on the global path the equal destinations inside a wave are merged"""
    st = Stage(6, n=1500, S=S, dests=41)
    for a in np.random.default_rng(S).integers(0, st.n - 8, 100):
        st.codes[a:a + 5] = st.codes[a]
    with _engine(S, **RULES["all"]) as eng:
        assert eng.filter_kind() == kind
        table = _check(st, eng, "all")
        assert not table[:2 * S - 40].any() and (table[2 * S - 40:, 0] > 0).all()


def test_stage_reads_longer_than_the_lds_partials_take(torch_cuda, stage):
    """reads of more than 2 047 bases go to the 64-bit table directly: the generated input holds 48 of 2 049"""
    assert sum(int(q[4]) == 2049 for q in stage.r1) + sum(int(q[4]) == 2049 for q in stage.r2) == 48
    rules = dict(max_n=200, min_mean_quality=30)  # a random read of 2 049 bases holds some 256 N; poly-A and AC reads hold none
    with _engine(**rules) as eng:
        table = _check(stage, eng, "long", P=FM.Params(**rules))
        assert int(table[:, 6].sum()) > 48 * 2049 and 16 <= int(table[:, 2].sum()) and 0 < int(table[:, 4].sum()) < int(table[:, 0].sum())


def test_stage_on_tables_a_trim_has_shortened(torch_cuda, stage):
    """the 3' trimming's own output tables (qd_dev_trim) fed in: the filter reads the lengths that stage left"""
    st = Stage.__new__(Stage)
    st.__dict__.update(stage.__dict__)
    with _engine(**RULES["all"]) as eng:
        eng.trim_set(quality_cutoff=35, min_length=5)
        st.r1, st.r2 = eng.dev_trim(stage.t1, stage.r1, stage.t2, stage.r2)
        st._models = {}
        cut = sum(int(a[4]) < int(b[4]) for a, b in zip(st.r1, stage.r1))
        assert cut > 50 and (st.r1[:, [0, 1, 2, 3, 5]] == stage.r1[:, [0, 1, 2, 3, 5]]).all()
        _check(st, eng, "all")
        assert not (st.model("all")[0] == stage.model("all")[0]).all()


def test_accumulation_reset_and_add(torch_cuda):
    a, b = Stage(20, n=300), Stage(21, n=65)
    with _engine(**RULES["all"]) as eng, _engine(**RULES["all"]) as other:
        ta = _check(a, eng, "all")
        both = _check(b, eng, "all", before=ta)
        eng.reset_counts()
        assert not eng.filter_read().any() and eng.filter_get() == FM.Params(**RULES["all"]).keywords()
        tb = _check(b, eng, "all")
        _check(a, other, "all")
        eng.filter_add(other.filter_read())  # a second context's table folds in
        assert (eng.filter_read() == both).all() and (both == ta + tb).all() and (other.filter_read() == ta).all()
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.filter_add(np.zeros(16, dtype=np.uint64))
        assert ei.value.code == hb.QD_ERR_INVALID
        eng.filter_set(on=False)  # off: the table is freed
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.filter_read()
        assert ei.value.code == hb.QD_ERR_STATE
        eng.filter_set(max_n=0)
        assert not eng.filter_read().any()


def test_state_and_errors(torch_cuda):
    st = Stage(30, n=64)
    off = FM.Params().keywords()
    with hb.Engine(0) as eng:
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.filter_set(max_n=0)  # no plan, no barcodes: the table has a row per destination
        assert ei.value.code == hb.QD_ERR_STATE
        eng.filter_set()  # nothing to turn on: accepted
        eng.set_plan(hb.make_plan(True, 25, (0, 8), (0, 8)))
        eng.set_barcodes(_barcodes(S_STAGE))
        for call in (eng.filter_read, eng.filter_kind, lambda: st.run(eng), lambda: eng.filter_add(np.zeros((7, 8), np.uint64))):
            with pytest.raises(hb.QuadeHipError) as ei:
                call()
            assert ei.value.code == hb.QD_ERR_STATE
        assert eng.filter_get() == off
        assert eng.lib.qd_filter_set(eng._h, None) == 0 and eng.filter_get() == off  # NULL = off
        eng.filter_set(**RULES["all"])
        good = eng.filter_get()
        assert good == FM.Params(**RULES["all"]).keywords()
        for bad in (dict(min_length=0), dict(min_length=100001), dict(min_length=-1), dict(max_n=-1), dict(max_n=100001), dict(max_unqualified_pct=-1),
                    dict(max_unqualified_pct=101), dict(max_n=1, qualified_quality=0), dict(max_n=1, qualified_quality=94), dict(min_mean_quality=0),
                    dict(min_mean_quality=94), dict(min_complexity_pct=0), dict(min_complexity_pct=101)):
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.filter_set(**bad)
            assert ei.value.code == hb.QD_ERR_INVALID, bad
            assert eng.filter_get() == good  # a rejected call changes nothing
        for ok in (dict(min_length=1, max_n=0, max_unqualified_pct=0, qualified_quality=1, min_mean_quality=1, min_complexity_pct=1),
                   dict(min_length=100000, max_n=100000, max_unqualified_pct=100, qualified_quality=93, min_mean_quality=93, min_complexity_pct=100)):
            eng.filter_set(**ok)
            assert eng.filter_get() == ok
        eng.filter_set(**RULES["all"])
        for size in (55, 57, 8):
            out = np.zeros(size, dtype=np.uint64)
            assert eng.lib.qd_filter_read(eng._h, hb._ptr(out), size) == hb.QD_ERR_INVALID
        want = _check(st, eng, "all")
        # a bad table never becomes an address: refused on the host, nothing launched, the table as it was
        bad = st.r1.copy()
        bad[5, 4] = len(st.t1)  # a sequence range beyond the text
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_filter(st.t1, bad, st.t2, st.r2, st.codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        bad = st.r2.copy()
        bad[63, 5] = len(st.t2) - int(bad[63, 4]) + 1  # a quality range one byte beyond
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.dev_filter(st.t1, st.r1, st.t2, bad, st.codes)
        assert ei.value.code == hb.QD_ERR_INVALID
        for code in (2 * S_STAGE, 0xFFFE):
            c2 = st.codes.copy()
            c2[9] = code
            with pytest.raises(hb.QuadeHipError) as ei:
                eng.dev_filter(st.t1, st.r1, st.t2, st.r2, c2)
            assert ei.value.code == hb.QD_ERR_INVALID
        assert (eng.filter_read() == want).all()
        eng.trim_set(quality_cutoff=20)  # the trimming stages leave the filter alone
        eng.pairtrim_set()
        assert eng.filter_get() == good and (eng.filter_read() == want).all()
        eng.set_barcodes(_barcodes(S_STAGE + 1))  # new barcodes turn the stage off, as they do the quality counters
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.filter_read()
        assert ei.value.code == hb.QD_ERR_STATE and eng.filter_get() == off
        eng.filter_set(max_n=2)
        assert eng.filter_read().shape == (2 * S_STAGE + 3, 8)
        eng.set_plan(hb.make_plan(True, 20, (0, 8), (0, 8)))  # and so does a new plan
        with pytest.raises(hb.QuadeHipError) as ei:
            eng.filter_kind()
        assert ei.value.code == hb.QD_ERR_STATE


# ---- the pipeline through the command line ---------------------------------------------------------------------------------------
def _write_conf(path, files, samples, extra=FILTER, **kw):
    SS._write_conf(path, files, samples, extra=extra, **kw)


def _oracle(conf, ref_dir, samples, P=P_F, trim=None, pair=None):
    """the oracle's run of the conf without the sections -> filtered_outputs of the model"""
    SS._oracle_run(conf, ref_dir)
    return FM.filtered_outputs(str(ref_dir), [s[0] for s in samples], P, trim, pair)


def _input_is_fit(table):
    """the conditions on the input, by the model: every reason takes at least 20 pairs, 40 % to 90 % of the pairs are kept, one
    destination loses all its pairs"""
    t = np.array(table, dtype=np.int64)
    pairs, dropped = int(t[:, 0].sum()), t[:, 1:6].sum(axis=0)
    assert (dropped >= 20).all(), dropped
    assert 0.4 * pairs <= pairs - int(dropped.sum()) <= 0.9 * pairs, (pairs, dropped)
    assert t[2 * POLY_G, 0] > 0 and t[2 * POLY_G, 0] == t[2 * POLY_G, 1:6].sum()


def _report_body(path):
    with open(path) as fh:
        lines = fh.read().split("\n")
    assert lines[0].startswith("Program Quade 0.3.2\tDate ")
    return lines[1:]


def _check_run(mine, ref, samples, texts, table, P=P_F, only=None, trim_table=None, pair_table=None, pair_kw=None):
    SS._check_files(mine, texts, only, at_least=0)
    assert _report_body(os.path.join(str(mine), "Quade_report.csv")) == _report_body(os.path.join(str(ref), "Quade_report.csv"))  # assignments
    SS._check_report(mine, fr, table, [s[0] for s in samples], P.keywords())
    SS._check_report(mine, tr, trim_table, TRIM_KW)
    SS._check_report(mine, pr, pair_table, pair_kw or P_PAIR.keywords())


@pytest.fixture(scope="module")
def bgzf_run(torch_cuda, tmp_path_factory):
    """2 chunks x 1 500 pairs in BGZF, run once with the filter alone; the model over the oracle's outputs"""
    top = tmp_path_factory.mktemp("filter_bgzf")
    files, samples = _dataset(str(top / "data"), 71, 2, 1500, bgzf=True)
    plain = top / "plain.txt"
    _write_conf(plain, files, samples, extra="")
    texts, table, _, _ = _oracle(plain, top / "ref", samples)
    _input_is_fit(table)
    conf = top / "conf.txt"
    _write_conf(conf, files, samples)
    _cli(conf, top / "mine")
    return dict(top=top, files=files, samples=samples, texts=texts, table=table, mine=top / "mine", ref=top / "ref", plain=plain)


def test_cli_filter_alone_bgzf(bgzf_run):
    run = bgzf_run
    _check_run(run["mine"], run["ref"], run["samples"], run["texts"], run["table"])
    assert not os.path.exists(run["mine"] / qr.REPORT_NAME)
    # the destination that lost all its pairs has no files, as one that received none; the oracle, which filters nothing, wrote them
    gone = "S%d_pass_R1.fastq.gz" % POLY_G
    assert gone not in run["texts"] and os.path.exists(run["ref"] / gone) and len(run["texts"]) >= 6


def test_cli_with_quality_cutoff_adapters_and_pair_overlap(bgzf_run, tmp_path):
    run = bgzf_run
    texts, table, first, second = FM.filtered_outputs(str(run["ref"]), [s[0] for s in run["samples"]], P_F, P_TRIM, P_PAIR)
    _input_is_fit(table)
    assert table != run["table"] and int(np.array(table)[:, 1].sum()) > int(np.array(run["table"])[:, 1].sum())
    # an adapter dimer is cut to the floor of 25 bases (here by the adapter match, which runs first) and stays below the filter's 40:
    # dropped as too_short
    assert first[0][7] + first[1][7] > 0 and P_TRIM.min_length < P_F.min_length
    conf = tmp_path / "both.txt"
    _write_conf(conf, run["files"], run["samples"], extra=TRIMS + FILTER)
    _cli(conf, tmp_path / "both")
    _check_run(tmp_path / "both", run["ref"], run["samples"], texts, table, trim_table=first, pair_table=second)
    for f in texts:  # no read of fewer than 40 bases is left
        assert min(len(s) for s, _ in QM.fastq_records(str(tmp_path / "both" / f))) >= 40, f


def test_cli_a_dimer_that_pair_overlap_cuts_to_the_floor_is_dropped(bgzf_run, tmp_path):
    """pair_overlap without adapter sequences: the overlap trimming itself cuts the shortest inserts it can see (30 bases and more:
    pair_min_overlap) to its floor of 35 bases, and the filter's min_length 40 drops them"""
    run = bgzf_run
    P = FM.Params(min_length=40)
    pair = PM.Params(max_mismatches=3, min_length=35)
    texts, table, _, second = FM.filtered_outputs(str(run["ref"]), [s[0] for s in run["samples"]], P, None, pair)
    assert second[5] > 0 and second[11] > 0  # reads the floor held back: every one of them has 35 bases
    plain = FM.filtered_outputs(str(run["ref"]), [s[0] for s in run["samples"]], P)[1]
    assert int(np.array(table)[:, 1].sum()) >= int(np.array(plain)[:, 1].sum()) + second[5] // 2
    conf = tmp_path / "dimer.txt"
    _write_conf(conf, run["files"], run["samples"], extra="[trim]\nmin_length : 35\npair_overlap : True\npair_max_mismatches : 3\n[filter]\nmin_length : 40\n")
    _cli(conf, tmp_path / "dimer")
    _check_run(tmp_path / "dimer", run["ref"], run["samples"], texts, table, P=P, pair_table=second, pair_kw=pair.keywords())


def test_cli_quality_report_counts_the_pairs_that_were_written(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "quality.txt"
    _write_conf(conf, run["files"], run["samples"], quality=True)
    _cli(conf, tmp_path / "quality")
    _check_run(tmp_path / "quality", run["ref"], run["samples"], run["texts"], run["table"])
    names = [s[0] for s in run["samples"]]
    with open(tmp_path / "quality" / qr.REPORT_NAME) as fh:
        got = fh.read()
    assert got == "\n".join(qr.report_lines(QM.table_from_outputs(str(tmp_path / "quality"), names), names)) + "\n"
    assert got != "\n".join(qr.report_lines(QM.table_from_outputs(str(run["ref"]), names), names)) + "\n"


def test_cli_ordinary_gzip(torch_cuda, tmp_path):
    files, samples = _dataset(str(tmp_path / "data"), 72, 2, 1000, bgzf=False)
    _write_conf(tmp_path / "plain.txt", files, samples, extra="")
    texts, table, _, _ = _oracle(tmp_path / "plain.txt", tmp_path / "ref", samples)
    _write_conf(tmp_path / "conf.txt", files, samples)
    _cli(tmp_path / "conf.txt", tmp_path / "mine")
    _check_run(tmp_path / "mine", tmp_path / "ref", samples, texts, table)


def test_cli_chunk_workers_and_write_flags(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "workers.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="chunk_workers : 2\n")
    _cli(conf, tmp_path / "workers")
    _check_run(tmp_path / "workers", run["ref"], run["samples"], run["texts"], run["table"])
    conf = tmp_path / "flags.txt"
    _write_conf(conf, run["files"], run["samples"], flags=(True, False, False))
    _cli(conf, tmp_path / "flags")  # the table does not depend on what is written; the files are absent
    flags_ref = tmp_path / "flags_ref"
    _write_conf(tmp_path / "flags_plain.txt", run["files"], run["samples"], extra="", flags=(True, False, False))
    os.makedirs(flags_ref)
    qo.run_quade(str(tmp_path / "flags_plain.txt"), outdir=str(flags_ref))
    _check_run(tmp_path / "flags", flags_ref, run["samples"], run["texts"], run["table"], only=lambda f: "_pass_" in f)
    assert any("_fail_" in f for f in run["texts"]) and "Undetermined_R1.fastq.gz" in run["texts"]


def test_cli_two_ranks_sharded_and_whole_chunks(bgzf_run, tmp_path):
    """2 ranks on GPU 0 (tables through the rendezvous files): each a pair range of ONE shared BGZF chunk, then a chunk each"""
    run = bgzf_run
    _write_conf(tmp_path / "plain.txt", run["files"], run["samples"], extra="", chunks=[0])
    texts, table, _, _ = _oracle(tmp_path / "plain.txt", tmp_path / "ref", run["samples"])
    assert table != run["table"]
    conf = tmp_path / "shared.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : True\n", chunks=[0])
    _cli(conf, tmp_path / "shared", ranks=2)
    _check_run(tmp_path / "shared", tmp_path / "ref", run["samples"], texts, table)
    conf = tmp_path / "two.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="shard_chunks : False\n")
    _cli(conf, tmp_path / "two", ranks=2)
    _check_run(tmp_path / "two", run["ref"], run["samples"], run["texts"], run["table"])
    assert not [f for f in os.listdir(tmp_path / "two") if f.startswith(".quade_rdv")]


def test_cli_every_pair_dropped(bgzf_run, tmp_path):
    run = bgzf_run
    P = FM.Params(min_length=100000)
    texts, table, _, _ = FM.filtered_outputs(str(run["ref"]), [s[0] for s in run["samples"]], P)
    t = np.array(table)
    assert texts == {} and (t[:, 0] == t[:, 1]).all() and (t[:, 6] == t[:, 7]).all() and t[:, 0].sum() > 2900
    conf = tmp_path / "none.txt"
    _write_conf(conf, run["files"], run["samples"], extra="[filter]\nmin_length : 100000\n", quality=True)
    _cli(conf, tmp_path / "none")
    _check_run(tmp_path / "none", run["ref"], run["samples"], texts, table, P=P)
    names = [s[0] for s in run["samples"]]
    with open(tmp_path / "none" / qr.REPORT_NAME) as fh:  # nothing was written: nothing is counted
        assert fh.read() == "\n".join(qr.report_lines(np.zeros((2 * len(names) + 1, 2, 6), dtype=np.uint64), names)) + "\n"


def test_cli_without_the_section_nothing_changes(bgzf_run, tmp_path):
    """a conf without the section, one with an empty section and one with every option empty: the same bytes"""
    run = bgzf_run
    empty = "[filter]\n" + "".join("%s :\n" % k for k in FM.KEYS)
    runs = {}
    for name, extra in (("absent", ""), ("empty", empty)):
        conf = tmp_path / (name + ".txt")
        _write_conf(conf, run["files"], run["samples"], extra=extra)
        _cli(conf, tmp_path / name)
        assert not os.path.exists(tmp_path / name / fr.REPORT_NAME)
        runs[name] = {f: open(tmp_path / name / f, "rb").read() for f in sorted(os.listdir(tmp_path / name)) if f.endswith(".fastq.gz")}
        runs[name]["Quade_report.csv"] = "\n".join(_report_body(tmp_path / name / "Quade_report.csv")).encode()
        assert sorted(os.listdir(tmp_path / name)) == sorted(f for f in runs[name])  # the file list
    assert runs["absent"] == runs["empty"] and len(runs["empty"]) > 12  # byte for byte, the compressed files included
    ref = sorted(f for f in os.listdir(run["ref"]) if f.endswith(".fastq.gz"))
    assert ref == sorted(f for f in runs["empty"] if f.endswith(".gz"))
    for f in ref:  # ... and what the pipeline has always written
        assert _gz(str(tmp_path / "empty" / f)) == _gz(str(run["ref"] / f)), f


def test_cli_pinned_slots_conf_with_the_section_is_rejected(bgzf_run, tmp_path):
    run = bgzf_run
    conf = tmp_path / "pinned.txt"
    _write_conf(conf, run["files"], run["samples"], gpu="device_pipeline : False\n")
    work = tmp_path / "pinned"
    os.makedirs(work)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "Quade.py"), "-c", str(conf)], cwd=str(work), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.stdout[-1500:], r.stderr[-3000:])
    assert "[filter] needs the device pipeline" in r.stdout + r.stderr and os.listdir(work) == []
