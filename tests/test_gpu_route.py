"""The routing and format stages on the MI355X one by one (quade_amd/csrc/quade_text.hip through qd_dev_pack_rows,
qd_dev_route_format and qd_dev_pack_members) against tests/route_model.py: every returned table and every byte of the output
buffer, guard bytes included.  All comparisons are exact; nothing outside the repository is read.

Which asserted cases reach which branch (from reading the kernels; no pipeline test in the suite reaches them with a reference):
  put()'s second 128-byte step ......... a piece of 136 bytes or more (lane 0 steps from byte 0 to byte 128 when len & ~7 > 128):
                                         test_format_every_length_at_every_shift, reads of 136, 137, 150, 151, 255 .. 2049 bases, names of
                                         200 bytes, at all 16 source alignments; 128, 129 and 135 bytes end inside the first step
  put()'s byte tail, residues 1 .. 7 ... the same test: the scan's tables give len % 8 of 0, 1, 4, 6 and 7, its trimmed copies every
                                         residue (asserted in test_the_sweep_holds_the_cases...), with and without whole steps before
  tag_parts with an empty MOL .......... test_index_read_lengths: index reads of 0, start - 1 and start bases on the plans with a
                                         molecular part (asserted: tags with one ':' and with two), and the sweep's truncated reads
  the two-pass sort feeding sdest ...... test_destinations with S = 128 (257 destinations) and S = 1536; "sparse" is asserted to vary
                                         both radix digits
  the empty-destination walk ........... test_destinations: "first_empty" (destination 0 takes the next one's start), "undetermined_empty"
                                         (the last one takes the total), "only_undetermined", "ends_only" (a run between two populated
                                         ones); test_write_flags_and_drop: populated destinations whose pairs all have length 0
  member_offsets' 1024-member carry .... test_members with n = 1025 and 2049 (1024 members are one trip of the loop: no carry is read)
  member_copy's vector and byte paths .. test_members: 16 bytes and more take the vector path (65535 and more further trips of its loop),
                                         the last len % 16 bytes of a part and members below 16 bytes the byte path; 65536 and more
                                         take a second part of the grid (65537: one byte of it)"""
import numpy as np
import pytest

from quade_amd import hip_backend as hb
from tests import route_model as RM
from tests.run_support import NAME_BYTES, PLANS, build_fastq, make_plan, ragged_index_reads, rand_bytes, reads_of

pytestmark = pytest.mark.gpu

LENS = (0, 1, 7, 8, 9, 15, 16, 17, 120, 127, 128, 129, 135, 136, 137, 150, 151, 255, 256, 257, 300, 2049)
NAME_LENS = (0, 1, 7, 8, 9, 16, 63, 129, 200)
N_PAIRS = (1, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
ALL = (1, 1, 1)
SLACK = 48  # guard bytes asked for behind the text's end
UND = RM.UNDETERMINED


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch


def _scan(text):
    lib = hb.load_library()
    buf = np.frombuffer(text, dtype=np.uint8)
    cap = text.count(b"\n") + 8
    recs = np.zeros((cap // 4 + 2, 6), dtype=np.uint32)
    res = np.zeros(8, dtype=np.uint32)
    n = lib.qd_dev_fastq_scan(0, hb._ptr(buf), len(text), 1, 1, 0, cap, hb._ptr(recs), recs.shape[0], hb._ptr(res))
    assert n >= 0 and res[5] == 0
    return recs[:n]


def _index_window_lengths(plan):
    """0, start - 1, start, start + 1, end - 1, end, end + 1 of every window of the plan, 255, 256 and 300"""
    out = {0, 255, 256, 300}
    for i0, i1, m0, m1 in RM.windows(plan):
        for a, b in ((i0, i1), (m0, m1)):
            if b > a:
                out |= {a - 1, a, a + 1, b - 1, b, b + 1}
    return sorted(v for v in out if v >= 0)


def _index_reads_of_lengths(rng, lengths, barcode, start):
    out = []
    for i, L in enumerate(lengths):
        s = (b"A" * start + barcode + rand_bytes(rng, 300, b"ACGTacgtN"))[:L] if i % 2 else rand_bytes(rng, L, b"ACGTacgtN")
        out.append((b"i%d" % i, s, rand_bytes(rng, L, bytes(range(33 + 20, 33 + 41)))))
    return out


class Batch(object):
    """texts and tables of n pairs (R1, R2, I1[, I2]) with routing codes; models are computed once per (tables, flags, drop)"""

    def __init__(self, plan, S, reads, codes, seed=0):
        rng = np.random.default_rng(seed)
        self.plan, self.S, self.n = plan, S, len(codes)
        self.texts, self.tables = [], []
        for r in reads:
            assert len(r) == self.n
            text, table = build_fastq(r, [int(v) for v in rng.integers(0, 8, self.n)])
            self.texts.append(text)
            self.tables.append(table)
        self.codes = np.asarray(codes, dtype=np.uint16)
        self._models = {}

    def model(self, key, tables=None, n=None, codes=None, flags=ALL, drop=None, S=None):
        if key not in self._models:
            tables = self.tables if tables is None else tables
            n = self.n if n is None else n
            r = [reads_of(t, tb[:n]) for t, tb in zip(self.texts, tables)]
            codes = self.codes[:n] if codes is None else codes
            self._models[key] = RM.route(self.plan, self.S if S is None else S, flags, r[0], r[1], [[x[1] for x in s] for s in r[2:]], codes, drop)
        return self._models[key]

    def run(self, m, tables=None, n=None, codes=None, flags=ALL, drop=None, shift=0, S=None):
        tables = self.tables if tables is None else tables
        n = self.n if n is None else n
        return hb.dev_route_format(self.plan, self.S if S is None else S, flags, self.texts, [tb[:n] for tb in tables],
                                   self.codes[:n] if codes is None else codes, drop=drop, shift=shift, out_cap=m["used"] + SLACK)


def _same(res, m, what=None):
    for k in hb.ROUTE_TABLES:
        want = np.array(m[k], dtype=res[k].dtype)
        assert res[k].shape == want.shape, (what, k)
        bad = np.flatnonzero(res[k] != want)
        assert not len(bad), (what, k, [(int(i), int(res[k][i]), int(want[i])) for i in bad[:6]])
    assert res["used"] == m["used"], what
    got, want = res["out"].tobytes(), m["out"] + bytes([RM.GUARD]) * SLACK
    if got != want:
        at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
        region = max((a, key) for key, a in m["where"].items() if a <= at) if at >= 0 and m["where"] else None
        raise AssertionError((what, "first differing byte", at, "region (start, (dest, read))", region, got[max(at - 24, 0):at + 24], want[max(at - 24, 0):at + 24]))


# ---- read and name lengths at every upload shift ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep():
    """every R1 length with every R2 length (484 pairs), names of every length class, on the plan with a molecular part in both
    index reads; the tables as the scan writes them and as trimmed copies (seq_len reduced, down to 0, offsets kept)"""
    rng = np.random.default_rng(21)
    plan, S = make_plan("dual_umi_in_both_reads_truncated"), 3
    n = len(LENS) ** 2
    r1 = [(rand_bytes(rng, NAME_LENS[j % 9], NAME_BYTES), rand_bytes(rng, LENS[j // len(LENS)], b"ACGTN"), rand_bytes(rng, LENS[j // len(LENS)], bytes(range(33, 75))))
          for j in range(n)]
    r2 = [(rand_bytes(rng, NAME_LENS[(j // 9 + j) % 9], NAME_BYTES), rand_bytes(rng, LENS[j % len(LENS)], b"ACGTN"), rand_bytes(rng, LENS[j % len(LENS)], bytes(range(33, 75))))
          for j in range(n)]
    bcs = [(b"ACGTACGT", b"TTGCAATC"), (b"GGATCCAA", b"CATGCATG"), (b"TTTTACGA", b"AGAGAGTC")]
    idx = [ragged_index_reads(rng, n, 0, 8, bcs, k) for k in range(2)]
    codes = rng.integers(0, 2 * S + 1, n)
    codes[codes == 2 * S] = UND
    b = Batch(plan, S, [r1, r2] + idx, codes, seed=22)
    trimmed = [t.copy() for t in b.tables]
    for s in (0, 1):
        L = trimmed[s][:, 4].astype(np.int64)
        kind = rng.integers(0, 4, n)
        trimmed[s][:, 4] = np.where(kind == 0, 0, np.where(kind == 1, L // 2, np.where(kind == 2, np.maximum(L - 1, 0), rng.integers(0, L + 1))))
    b.trimmed = trimmed
    return b


def test_the_sweep_holds_the_cases_and_the_scan_writes_its_tables(torch_cuda, sweep):
    b = sweep
    for text, table in zip(b.texts, b.tables):  # the tables straight from qd_dev_fastq_scan are the built ones
        assert (_scan(text) == table).all()
    pairs = {(int(a), int(c)) for a, c in zip(b.tables[0][:, 4], b.tables[1][:, 4])}
    assert pairs == {(x, y) for x in LENS for y in LENS}
    for s in (0, 1):
        assert {int(v) for v in b.tables[s][:, 2]} == set(NAME_LENS)
        assert (b.trimmed[s][:, 4] <= b.tables[s][:, 4]).all() and (b.trimmed[s][:, [0, 1, 2, 3, 5]] == b.tables[s][:, [0, 1, 2, 3, 5]]).all()
        kept = b.trimmed[s][:, 4][b.tables[s][:, 4] > 0]
        assert (kept == 0).any() and {int(v) % 8 for v in b.trimmed[s][:, 4]} == set(range(8)) and (b.trimmed[s][:, 4] >= 136).any()
    m = b.model("scan")
    assert all(m["text"][(d, k)] for d in range(2 * b.S + 1) for k in (0, 1)) and b"\r" not in m["out"]
    tags = [RM.tag(b.plan, [RM.read_of(b.texts[2 + k], b.tables[2 + k][j])[1] for k in (0, 1)]) for j in range(b.n)]
    assert any(t.count(b":") == 1 for t in tags) and any(t.count(b":") == 2 for t in tags)


@pytest.mark.parametrize("shift", range(16))
def test_format_every_length_at_every_shift(torch_cuda, sweep, shift):
    b = sweep
    for key, tables in (("scan", b.tables), ("trimmed", b.trimmed)):
        m = b.model(key, tables=tables)
        _same(b.run(m, tables=tables, shift=shift), m, (key, shift))


# ---- index reads of every length around every window ---------------------------------------------------------------------------------
@pytest.mark.parametrize("plan_name", PLANS)
def test_index_read_lengths(torch_cuda, plan_name):
    rng = np.random.default_rng(len(plan_name))
    plan, S = make_plan(plan_name), 2
    lens = _index_window_lengths(plan)
    ni = 2 if plan.dual else 1
    combos = [(a, c) for a in lens for c in (lens if ni == 2 else (0, 1, 2))]
    n = len(combos)
    w = RM.windows(plan)
    bc = [rand_bytes(rng, w[k][1] - w[k][0], b"ACGT") for k in range(ni)]
    idx = [_index_reads_of_lengths(rng, [c[k] for c in combos], bc[k], w[k][0]) for k in range(ni)]
    ins = [[(b"p%d" % j, rand_bytes(rng, int(L), b"ACGT"), rand_bytes(rng, int(L), b"FGHIJ")) for j, L in enumerate(rng.integers(0, 40, n))] for _ in (0, 1)]
    codes = rng.integers(0, 2 * S + 1, n)
    codes[codes == 2 * S] = UND
    b = Batch(plan, S, ins + idx, codes, seed=5)
    m = b.model("all")
    tags = [RM.tag(plan, [s[j][1] for s in idx]) for j in range(n)]
    if plan.mol1_end or plan.mol2_end:
        assert any(t.count(b":") == 1 for t in tags) and any(t.count(b":") == 2 for t in tags)
    assert b":" in tags and max(len(t) for t in tags) == 1 + sum(x[1] - x[0] for x in w) + (1 + sum(x[3] - x[2] for x in w) if plan.mol1_end or plan.mol2_end else 0)
    for shift in (0, 5, 14):
        _same(b.run(m, shift=shift), m, (plan_name, shift))
    for text, table in zip(b.texts[2:], b.tables[2:]):
        assert (_scan(text) == table).all()


# ---- pairs per launch, destinations, flags, drop: one pool of ragged short pairs -----------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """8193 pairs of short ragged reads (0 .. 24 bases, names of 0 .. 12 bytes), ragged index reads, dual plan with offset windows"""
    rng = np.random.default_rng(31)
    plan, n = make_plan("dual_offset_windows"), max(N_PAIRS)
    ins = []
    for _ in (0, 1):
        L, N = rng.integers(0, 25, n), rng.integers(0, 13, n)
        letters = rng.integers(0, 4, (n, 24))
        ins.append([(NAME_BYTES[:int(N[j])], bytes(b"ACGT"[v] for v in letters[j, :L[j]]), bytes(70 + v for v in letters[j, :L[j]])) for j in range(n)])
    bcs = [(b"ACGTAC", b"TTGCAAT"), (b"GGATCC", b"CATGCAT"), (b"TTTTAC", b"AGAGAGT")]
    idx = [ragged_index_reads(rng, n, (1, 2)[k], (6, 7)[k], bcs, k) for k in range(2)]
    codes = rng.integers(0, 7, n)
    codes[codes == 6] = UND
    return Batch(plan, 3, ins + idx, codes, seed=32)


@pytest.mark.parametrize("n", N_PAIRS)
def test_pairs_per_launch(torch_cuda, pool, n):
    m = pool.model(("n", n), n=n)
    assert len(set(m["len1"])) > 1 or n == 1
    _same(pool.run(m, n=n, shift=3), m, n)


def _codes_for(kind, S, n, rng):
    nd = 2 * S + 1
    if kind == "first_empty":  # only the last destinations, Undetermined among them
        d = rng.integers(max(nd - 3, 1), nd, n)
    elif kind == "undetermined_empty":
        d = rng.choice(sorted({0, 1, 2 * S - 2, 2 * S - 1}), n)
    elif kind == "only_undetermined":
        d = np.full(n, nd - 1)
    elif kind == "ends_only":  # the first destination and Undetermined: a run of empty destinations between them
        d = rng.choice([0, nd - 1], n)
    elif kind == "above_2S":  # codes at and above 2 * S are Undetermined's
        d = rng.choice([0, 1, nd - 1, nd, nd + 1, 0xFFFE], n)
    else:  # "sparse": 40 destinations anywhere, Undetermined among them
        d = rng.choice(np.append(rng.choice(nd - 1, min(39, nd - 1), replace=False), nd - 1), n)
    codes = d.astype(np.uint16)
    codes[d == nd - 1] = UND
    if kind == "above_2S":
        codes[::5] = nd - 1  # 2 * S itself, not as 0xFFFF
    return codes


@pytest.mark.parametrize("kind", ["first_empty", "undetermined_empty", "only_undetermined", "ends_only", "above_2S", "sparse"])
@pytest.mark.parametrize("S", [1, 127, 128, 1536])
def test_destinations(torch_cuda, pool, S, kind):
    n = 1500
    codes = _codes_for(kind, S, n, np.random.default_rng(S + len(kind)))
    m = pool.model(("dest", S, kind), n=n, codes=codes, S=S)
    nd, first = 2 * S + 1, m["first"]
    empty = [f == RM.NONE for f in first]
    if kind == "first_empty":
        assert empty[0] and not empty[nd - 1]
    if kind in ("undetermined_empty",):
        assert empty[nd - 1] and not empty[0]
    if kind == "only_undetermined":
        assert all(empty[:-1]) and first[nd - 1] == 0
    if kind == "ends_only":
        assert not empty[0] and not empty[nd - 1] and all(empty[1:-1])
    if kind == "above_2S":
        assert {int(c) for c in codes} >= {nd - 1, nd, nd + 1, 0xFFFE, UND} and set(m["dest"]) == {0, 1, nd - 1}
    if kind == "sparse" and S > 127:
        assert len({d >> 8 for d in m["dest"]}) > 1 and len({d & 255 for d in m["dest"]}) > 8  # both radix digits order the pairs
    _same(pool.run(m, n=n, codes=codes, S=S, shift=9), m, (S, kind))


@pytest.mark.parametrize("flags", [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)])
def test_write_flags_and_drop(torch_cuda, pool, flags):
    n = 300
    dest = np.array([RM.destination(int(c), pool.S) for c in pool.codes[:n]])
    drops = {"absent": None, "sparse": (np.arange(n) % 7 == 0).astype(np.uint8) * 3, "a_destination": (dest == 2).astype(np.uint8),
             "everything": np.full(n, 5, dtype=np.uint8)}
    assert (dest == 2).any() and len(set(dest)) == 7
    for name, drop in drops.items():
        m = pool.model(("flags", flags, name), n=n, flags=flags, drop=drop)
        if name == "everything" or flags == (0, 0, 0):
            assert m["used"] == 0 and m["g1"][n] == 0
        elif name == "a_destination":
            assert m["first"][2] != RM.NONE and not m["text"][(2, 0)] and (not flags[0] or m["text"][(0, 0)])
        _same(pool.run(m, n=n, flags=flags, drop=drop, shift=6), m, (flags, name))
    m = pool.model(("flags", (1, 1, 1), "absent"), n=n)
    with pytest.raises(hb.QuadeHipError) as ei:  # a buffer that is too small: nothing is formatted, the need is reported
        hb.dev_route_format(pool.plan, pool.S, ALL, pool.texts, [t[:n] for t in pool.tables], pool.codes[:n], out_cap=m["used"] - 1)
    assert ei.value.code == hb.QD_ERR_INVALID and ei.value.used == m["used"]


# ---- index rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("plan_name", PLANS)
def test_rows(torch_cuda, plan_name, n):
    rng = np.random.default_rng(n + len(plan_name))
    plan = make_plan(plan_name)
    lay = hb.plan_layout(plan)
    ni, w = lay.n_streams, RM.windows(plan)
    lens = _index_window_lengths(plan) + [254]
    reads = [_index_reads_of_lengths(rng, [lens[(j + 5 * k + n) % len(lens)] for j in range(n)], b"ACGTACGTAC", w[k][0]) for k in range(ni)]
    built = [build_fastq(r, [int(v) for v in rng.integers(0, 8, n)]) for r in reads]
    texts, tables = [t for t, _ in built], [tb for _, tb in built]
    streams = [[(r[1], r[2]) for r in s] for s in reads]
    short = RM.short_set(lay, streams)
    seq, qual, lrow, short_idx, n_short = hb.dev_pack_rows(lay, texts, tables, short_cap=n + 4)
    for k in range(ni):
        ms, mq, ml = RM.rows(lay, k, streams[k])
        hs, hq, hl, _full = hb.pack_index_reads(lay, k, [s for s, _ in streams[k]], [q for _, q in streams[k]])
        assert [bytes(r) for r in seq[k]] == ms == [bytes(r) for r in hs], k  # padding bytes included
        assert [bytes(r) for r in qual[k]] == mq == [bytes(r) for r in hq], k
        assert [int(v) for v in lrow[k]] == ml == [int(v) for v in hl], k
        if n > 200:
            assert {254, 255} <= set(ml) and {254, 255, 256, 300} <= {len(s) for s, _ in streams[k]}
    assert n_short == len(short)
    got = [int(v) for v in short_idx[:n_short]]
    assert len(set(got)) == len(got) and set(got) == short and (short_idx[n_short:] == RM.NONE).all()
    if len(short) > 1:  # a list that is too small: the count is whole, nothing is written behind the list's end
        cap = len(short) // 2
        _, _, _, short_idx, n_short = hb.dev_pack_rows(lay, texts, tables, short_cap=cap, short_room=len(short) + 8)
        got = [int(v) for v in short_idx[:cap]]
        assert n_short == len(short) and len(set(got)) == cap and set(got) <= short and (short_idx[cap:] == RM.NONE).all()
    if n > 200:
        assert 0 < len(short) < n


# ---- members -------------------------------------------------------------------------------------------------------------------------
def _bound(x):
    return int(hb.load_library().qd_huffman_member_bound(x))


MEMBER_LENS = (0, 1, 15, 16, 17, 4095, 65535, 65536, 65537)


@pytest.mark.parametrize("n,piece,pick", [
    (0, 1, "any"), (1, 65537, "each"), (1, 65536, "each"), (2, 65537, "any"), (2, 12, "any"), (23, 65537, "any"), (23, 65536, "any"),
    (1023, 1, "any"), (1024, 12, "any"), (1025, 1, "any"), (1025, 12, "zero"), (2049, 12, "any"), (2049, 1, "any")])
def test_members(torch_cuda, n, piece, pick):
    """Slots of qd_huffman_member_bound(piece) bytes: 1028 and 75780 are no multiples of 16, 1040 and 75776 are.  Offsets beyond 4 GiB
    are out of scope here: they need more memory than a test of a few seconds should take."""
    stride = _bound(piece)
    assert stride == {1: 1028, 12: 1040, 65536: 75776, 65537: 75780}[piece] and (stride % 16 == 0) == (piece in (12, 65536))
    rng = np.random.default_rng(n + piece)
    choices = [v for v in MEMBER_LENS if v <= stride] + [stride - 1, stride]
    runs = [[v] for v in choices] if pick == "each" else [[0] * n] if pick == "zero" else [[int(v) for v in rng.choice(choices, n)]]
    if pick == "any" and n >= 2:
        runs[0][0], runs[0][-1] = stride, 17  # a full slot first, a vector step and a byte behind it last
    for lens in runs:
        slots = rng.integers(0, 256, max(n * stride, 1), dtype=np.uint8)
        cap = sum(lens) + 40
        offsets, packed = hb.dev_pack_members(slots, stride, lens, cap)
        want_off, want = RM.pack_members(slots.tobytes(), stride, lens, cap)
        assert [int(v) for v in offsets] == want_off, (n, stride)
        assert packed.tobytes() == want, (n, stride, lens[:8])

