"""What the mismatch and unknown-barcode GPU tests share: the plan shapes, sample sheets and index reads with planted mismatches;
and the tight and combinatorial sheets with the whole neighbourhoods of their barcodes (no GPU needed to build them)."""
import collections
import functools
import itertools
import zlib

import numpy as np

from quade_amd import hip_backend as hb
from quade_amd import synth


# shapes: (plan, barcode bases per index read (w1, w2), read length per index read)
SHAPES = {
    "single8": (hb.make_plan(False, 25, (0, 8)), (8, 0), 8),
    "dual8": (synth.config_plan("cfg3"), (8, 8), 8),
    "wide10": (synth.config_plan("wide10"), (10, 10), 10),
    "kit6": (synth.config_plan("kit6"), (6, 6), 6),
    "kit8u9": (synth.config_plan("kit8u9"), (8, 8), 17),
}


def make_reads(shape, bcs, n, m1, m2, seed, short_frac=0.0):
    """Index reads (lists of bytes per stream: sequences, qualities) of n pairs over the sample sheet bcs: exact barcodes, one
    or two substitutions (by another symbol of ACGTN) in either part, uniform reads, lower case, low-quality barcode
    positions, and (short_frac) reads cut inside their barcode slice."""
    plan, (w1, w2), L = SHAPES[shape]
    rng = np.random.default_rng(seed)
    K = w1 + w2
    bc = np.array([np.frombuffer(b.encode(), np.uint8) for b in bcs], dtype=np.uint8).reshape(len(bcs), K)
    key = bc[rng.integers(0, len(bcs), n)].copy()
    kind = rng.integers(0, 100, n)
    acgtn = np.frombuffer(b"ACGTN", np.uint8)

    def substitute(rows, lo, hi):
        pos = rng.integers(lo, hi, rows.size)
        new = acgtn[rng.integers(0, 5, rows.size)]
        same = new == key[rows, pos]
        new[same] = np.where(key[rows, pos][same] == ord("N"), ord("A"), ord("N"))
        key[rows, pos] = new

    parts = [(0, w1)] + ([(w1, K)] if w2 else [])
    one = np.flatnonzero((kind >= 40) & (kind < 70))
    side = rng.integers(0, len(parts), one.size)
    for i, p in enumerate(parts):
        substitute(one[side == i], *p)
    two = np.flatnonzero((kind >= 70) & (kind < 85))
    substitute(two, 0, K)
    substitute(two, 0, K)
    rnd = np.flatnonzero(kind >= 92)
    key[rnd] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (rnd.size, K))]
    lc = np.flatnonzero(rng.integers(0, 100, n) < 5)
    key[lc, rng.integers(0, K, lc.size)] |= 0x20
    q = (rng.integers(30, 41, (n, K)) + 33).astype(np.uint8)
    bad = np.flatnonzero(rng.integers(0, 100, n) < 20)
    q[bad, rng.integers(0, K, bad.size)] = (rng.integers(2, 25, bad.size) + 33).astype(np.uint8)
    streams = []
    ns = 2 if plan.dual else 1
    cut = rng.integers(0, 100, n) < int(100 * short_frac)
    for k in range(ns):
        iw = w1 if k == 0 else w2
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
        seq[:, :iw] = key[:, k * w1:k * w1 + iw]
        qual = np.full((n, L), ord("I"), np.uint8)
        qual[:, :iw] = q[:, k * w1:k * w1 + iw]
        lens = np.where(cut & (rng.integers(0, 2, n) == k), rng.integers(1, iw, n), L)
        streams.append(([bytes(seq[r, :lens[r]]) for r in range(n)], [bytes(qual[r, :lens[r]]) for r in range(n)]))
    return streams


def rows_on_device(torch, layout, streams):
    seq, qual, lens, full = [], [], [], True
    for k, (s, q) in enumerate(streams):
        sr, qr, lr, f = hb.pack_index_reads(layout, k, s, q)
        full = full and f
        seq.append(torch.from_numpy(sr).cuda())
        qual.append(torch.from_numpy(qr).cuda())
        lens.append(torch.from_numpy(lr).cuda())
    return seq, qual, lens, full


def sheet(shape, S, m1, m2, seed=1):
    _, (w1, w2), _ = SHAPES[shape]
    return synth.make_far_barcodes(S, w1, w2, m1, m2, seed=seed)


# ---- tight and combinatorial sheets with their whole neighbourhoods -------------------------------------------------------------
# The sheets above are uniform draws: no two samples share a part and the barcodes lie about six substitutions apart.  The ones
# below are as close as the collision rule allows (pairs at exactly 2m + 1), share whole parts between samples as combinatorial
# kits do, and come with EVERY key within budget of every barcode plus a seeded sample of the keys one substitution too far.
ACGT, ACGTN = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"ACGTN", np.uint8)
Shape = collections.namedtuple("Shape", "plan w1 w2 lens")  # lens: the index reads' lengths
TIGHT = {
    "dual8": Shape(hb.make_plan(True, 25, (0, 8), (0, 8)), 8, 8, (8, 8)),
    "kit6": Shape(hb.make_plan(True, 25, (0, 6), (0, 6)), 6, 6, (6, 6)),
    "wide10": Shape(hb.make_plan(True, 25, (0, 10), (0, 10)), 10, 10, (10, 10)),
    "single8": Shape(hb.make_plan(False, 25, (0, 8)), 8, 0, (8,)),
    # slices at offsets 1 and 2 of 12-base reads, a molecular index behind the first one
    "offset7": Shape(hb.make_plan(True, 25, (1, 8), (2, 9), mol1=(8, 11)), 7, 7, (12, 12)),
    # the molecular slices in front: the index slices sit at offsets 3 and 1 of the packed rows too, not only of the reads
    "offset7b": Shape(hb.make_plan(True, 25, (3, 10), (1, 8), mol1=(0, 2), mol2=(0, 1)), 7, 7, (12, 12)),
    "uneven": Shape(hb.make_plan(True, 25, (0, 6), (0, 10)), 6, 10, (6, 10)),
    # parts too narrow for budget + 1 segments: the rescue walks every barcode
    "single2": Shape(hb.make_plan(False, 25, (0, 2)), 2, 0, (4,)),
    "dual1": Shape(hb.make_plan(True, 25, (0, 1), (0, 1)), 1, 1, (1, 1)),
}
# name: shape, budgets, sizes of the two tight lists, cap on each just-outside shell per barcode, alphabet of the barcodes
CORPORA = {
    "comb_8x12": ("dual8", (1, 1), (8, 12), 600, b"ACGT"),
    "comb_12x8_m10": ("dual8", (1, 0), (12, 8), 600, b"ACGT"),
    "comb_12x8_m01": ("dual8", (0, 1), (8, 12), 600, b"ACGT"),  # the mirror image: the parts and their budgets swapped
    "asym_21": ("dual8", (2, 1), (3, 4), 3000, b"ACGT"),
    "asym_12": ("dual8", (1, 2), (4, 3), 3000, b"ACGT"),
    "kit6_22": ("kit6", (2, 2), (2, 2), 6000, b"ACGT"),
    "wide10": ("wide10", (1, 1), (4, 6), 1500, b"ACGT"),
    "single8_m1": ("single8", (1, 0), (12,), 3000, b"ACGT"),
    "single8_m2": ("single8", (2, 0), (4,), 3000, b"ACGT"),
    "offset_7x7": ("offset7", (1, 1), (4, 6), 1500, b"ACGT"),
    "offset_mol_first": ("offset7b", (1, 1), (4, 6), 1500, b"ACGT"),
    "uneven_6_10": ("uneven", (1, 2), (4, 3), 3000, b"ACGT"),
    "with_N": ("dual8", (1, 1), (4, 6), 1500, b"ACGTN"),
    "mixed_len": ("dual8", (1, 1), (8, 12), 600, b"ACGT"),  # comb_8x12's sheet plus barcodes of 15, 13 and 8 bases
    "comb_96x96": ("dual8", (1, 1), (96, 96), 600, b"ACGT"),  # neighbourhoods of 64 seeded barcodes and the tight pair's four
}
NO_SEGMENTS = {"single2": (2, 0), "dual1": (1, 1)}  # shape: budgets; one sample, all 5^K keys


def tight_codes(n, w, m, rng, alphabet=b"ACGT"):
    """n codes of w bases (list of str) at pairwise Hamming distance >= 2m + 1 (>= 1 when m = 0).  Every code but the first is made
    from an earlier one by exactly 2m + 1 substitutions -- code 1 from code 0 -- so the list is as tight as the collision rule
    allows, where uniform draws lie far apart."""
    A = np.frombuffer(alphabet, np.uint8)
    d = max(1, 2 * m + 1)
    assert w >= d
    codes = [A[rng.integers(0, A.size, w)]]
    for _ in range(200000):
        if len(codes) == n:
            break
        new = codes[0 if len(codes) == 1 else int(rng.integers(0, len(codes)))].copy()
        for p in rng.choice(w, d, replace=False):
            others = A[A != new[p]]
            new[p] = others[rng.integers(0, others.size)]
        if all(int((new != c).sum()) >= d for c in codes):
            codes.append(new)
    assert len(codes) == n, "no room for %d codes of %d bases at distance %d" % (n, w, d)
    return [bytes(c).decode() for c in codes]


def combinatorial_sheet(c1, c2):
    """every a + b: the samples share whole parts"""
    return [a + b for a in c1 for b in c2]


@functools.lru_cache(maxsize=None)
def _sphere(code, d):
    """all strings over ACGTN at Hamming distance exactly d from code (bytes) -> uint8 [C(w, d) * 4^d, w]"""
    base = np.frombuffer(code, np.uint8)
    w = base.size
    if d == 0:
        return base[None, :].copy()
    if d > w:
        return np.zeros((0, w), np.uint8)
    others = np.array([[s for s in ACGTN if s != b] for b in base], dtype=np.uint8).reshape(w, 4)
    digits = np.array(list(itertools.product(range(4), repeat=d)), dtype=np.int64)
    out = []
    for pos in itertools.combinations(range(w), d):
        rows = np.repeat(base[None, :], digits.shape[0], axis=0)
        for j, p in enumerate(pos):
            rows[:, p] = others[p, digits[:, j]]
        out.append(rows)
    return np.concatenate(out)


def _ball(code, m):
    """(strings within m of code, their distances)"""
    parts = [_sphere(code, d) for d in range(m + 1)]
    return np.concatenate(parts), np.concatenate([np.full(p.shape[0], d, np.int64) for d, p in enumerate(parts)])


def neighbourhood(sheet, w1, m1, m2, cap, rng, only=None):
    """For every barcode (of those listed in `only`): ALL keys over ACGTN within budget -- the full product of the two per-part
    balls -- and the two just-outside shells, at most `cap` keys of each drawn by rng: exactly m1 + 1 on part 1 and within budget
    on part 2; within budget on part 1 and exactly m2 + 1 on part 2.
    -> (keys uint8 [n, K], origin: the barcode a key was made from, d1, d2: its distances from that barcode)"""
    keys, origin, dist1, dist2 = [], [], [], []
    for s in (range(len(sheet)) if only is None else only):
        a, b = sheet[s][:w1].encode(), sheet[s][w1:].encode()
        (in1, din1), (in2, din2) = _ball(a, m1), _ball(b, m2)
        out1, out2 = _sphere(a, m1 + 1), _sphere(b, m2 + 1)
        for (x, dx), (y, dy), limit in (((in1, din1), (in2, din2), None),
                                        ((out1, np.full(out1.shape[0], m1 + 1)), (in2, din2), cap),
                                        ((in1, din1), (out2, np.full(out2.shape[0], m2 + 1)), cap)):
            total = x.shape[0] * y.shape[0]
            pick = np.arange(total) if limit is None or total <= limit else np.sort(rng.choice(total, limit, replace=False))
            i, j = pick // max(1, y.shape[0]), pick % max(1, y.shape[0])
            keys.append(np.concatenate([x[i], y[j]], axis=1))
            origin.append(np.full(pick.size, s, np.int64))
            dist1.append(dx[i])
            dist2.append(dy[j])
    return np.concatenate(keys), np.concatenate(origin), np.concatenate(dist1), np.concatenate(dist2)


def longest_candidate_lists(sheet, K, w1, m1, m2):
    """Per part, the longest list of K-long barcodes that share one of the part's m + 1 segments (segment j of a part of width w
    at offset o: bytes o + w*j // (m+1) up to o + w*(j+1) // (m+1)), None for a part narrower than m + 1.  The rescue looks its
    candidates up by the segments of ONE part: DESIGN.md 4.8 has it take the part whose longest list is shorter, the first on a tie."""
    out = []
    for off, w, m in ((0, w1, m1), (w1, K - w1, m2)):
        if w < m + 1:
            out.append(None)
            continue
        lists = collections.Counter()
        for b in sheet:
            if len(b) == K:
                lists.update((j, b[off + w * j // (m + 1):off + w * (j + 1) // (m + 1)]) for j in range(m + 1))
        out.append(max(lists.values()))
    return out


def _rows_as_bytes(a):
    buf, L = a.tobytes(), a.shape[1]
    return [buf[r * L:(r + 1) * L] for r in range(a.shape[0])]


def reads_from_keys(shape, keys, subst, rng):
    """Index reads per stream (lists of bytes: sequences, qualities) that carry the keys, and the slices' quality bytes [n, K].
    The slice sits at the plan's offset with random bases before and behind it; every tenth key carries one lower-case letter;
    the slice qualities follow one of four patterns by i % 4 -- all 40; one position exactly min_qual; min_qual - 1 at a
    substituted position (subst: bool [n, K], where the key differs from the barcode it was made from); min_qual - 1 at an
    unsubstituted position of the other part -- and the qualities outside the slice are low, so a gate that looks beyond the
    slice fails."""
    plan, w1, w2 = shape.plan, shape.w1, shape.w2
    n, K = keys.shape
    rows = np.arange(n)
    tie = rng.random((n, K))
    anywhere = rng.integers(0, K, n)

    def one_of(mask):
        return np.where(mask.any(axis=1), np.where(mask, tie, -1.0).argmax(axis=1), anywhere)

    in_part2 = np.arange(K)[None, :] >= w1
    first_is_hit = subst[:, :w1].any(axis=1) | ~subst.any(axis=1)
    other = in_part2 == first_is_hit[:, None] if w2 else np.ones((n, K), bool)
    q = np.full((n, K), 40 + 33, np.uint8)
    for pattern, pos, value in ((1, anywhere, plan.min_qual), (2, one_of(subst), plan.min_qual - 1),
                                (3, one_of(~subst & other), plan.min_qual - 1)):
        sel = rows[rows % 4 == pattern]
        q[sel, pos[sel]] = value + 33
    seq_key = keys.copy()
    lower = rows[rows % 10 == 0]
    seq_key[lower, rng.integers(0, K, lower.size)] |= 0x20
    starts = (plan.idx1_start, plan.idx2_start)
    streams = []
    for k, L in enumerate(shape.lens):
        iw, at = (w1, w2)[k], k * w1
        seq = ACGTN[rng.integers(0, 5, (n, L))]
        qual = np.full((n, L), 2 + 33, np.uint8)
        seq[:, starts[k]:starts[k] + iw] = seq_key[:, at:at + iw]
        qual[:, starts[k]:starts[k] + iw] = q[:, at:at + iw]
        streams.append((_rows_as_bytes(seq), _rows_as_bytes(qual)))
    return streams, q


class Corpus(object):
    """One case: sheet, budgets, keys with where they come from, the reads that carry them and what the model says of them.
    short: the reads cut below their slice (mixed_len, no_segments), whose codes are written down by hand in `codes`."""

    def __init__(self, name, shape, budgets, sheet, keys, origin, d1, d2, seed):
        from tests import mismatch_model as MM
        self.name, self.shape, self.sheet = name, shape, sheet
        (self.m1, self.m2), self.K, self.w1 = budgets, shape.w1 + shape.w2, shape.w1
        self.keys, self.origin, self.d1, self.d2 = keys, origin, d1, d2
        self.n = keys.shape[0]
        bc = np.array([np.frombuffer(sheet[s].encode(), np.uint8) for s in sorted(set(origin.tolist()))], dtype=np.uint8)
        where = np.zeros(len(sheet), np.int64)
        where[sorted(set(origin.tolist()))] = np.arange(bc.shape[0])
        self.subst = keys != bc[where[origin]]
        assert ((self.subst[:, :self.w1].sum(axis=1) == d1) & (self.subst[:, self.w1:].sum(axis=1) == d2)).all()
        self.streams, self.quals = reads_from_keys(shape, keys, self.subst, np.random.default_rng(seed))
        self.codes = MM.codes_for_keys(keys, self.quals, sheet, self.K, self.w1, self.m1, self.m2, shape.plan.min_qual)
        self.exact = MM.codes_for_keys(keys, self.quals, sheet, self.K, self.w1, 0, 0, shape.plan.min_qual)
        self.short = np.zeros(self.n, bool)

    @property
    def rescued(self):
        return (self.codes != 0xFFFF) & (self.exact == 0xFFFF)

    def cut(self, r, reads, code, exact_code):
        """pair r carries these (shorter) reads instead, per stream (sequence, qualities); its codes with and without budgets"""
        for k, (s, q) in enumerate(reads):
            self.streams[k][0][r], self.streams[k][1][r] = s, q
        self.short[r], self.codes[r], self.exact[r] = True, code, exact_code

    def molecular(self):
        """the pairs' molecular bytes: the reads' molecular slices, index read 1's in front"""
        p = self.shape.plan
        second = self.streams[1][0] if len(self.streams) > 1 else [b""] * self.n
        return [a[p.mol1_start:p.mol1_end] + b[p.mol2_start:p.mol2_end] for a, b in zip(self.streams[0][0], second)]

    def counts(self, codes=None):
        from tests import mismatch_model as MM
        return MM.counts_for_codes(self.codes if codes is None else codes, len(self.sheet))

    def sample(self, limit, seed=0):
        """a seeded sub-sample of at most `limit` pairs (sorted indices), every cut pair among them"""
        rng = np.random.default_rng(seed)
        pick = set(np.flatnonzero(self.short)[:limit // 2].tolist())
        rest = np.setdiff1d(np.arange(self.n), np.fromiter(pick, np.int64, len(pick)))
        pick |= set(rng.choice(rest, min(rest.size, limit - len(pick)), replace=False).tolist())
        return np.array(sorted(pick), dtype=np.int64)


SHORT_BARCODES = ("ACCGTTAGGCATTCA", "TGGACTCAATGCC", "GTCAAGTC")  # 15, 13 and 8 bases: 8 + 7, 8 + 5 and 5 + 3 over the two reads


@functools.lru_cache(maxsize=None)
def corpus(name):
    shape_name, (m1, m2), sizes, cap, alphabet = CORPORA[name]
    shape = TIGHT[shape_name]
    seed = zlib.crc32(("comb_8x12" if name == "mixed_len" else name).encode()) & 0xFFFF  # a case's draws do not depend on the other cases
    rng = np.random.default_rng(seed)
    lists = [tight_codes(n, w, m, rng, alphabet) for n, w, m in zip(sizes, (shape.w1, shape.w2), (m1, m2))]
    bcs = combinatorial_sheet(*lists) if len(lists) == 2 else list(lists[0])
    only = None
    if name == "comb_96x96":
        four = [0, 1, sizes[1], sizes[1] + 1]
        only = four + sorted(rng.choice(np.setdiff1d(np.arange(len(bcs)), four), 64, replace=False).tolist())
    keys, origin, d1, d2 = neighbourhood(bcs, shape.w1, m1, m2, cap, rng, only)
    if name == "mixed_len":  # a tenth more pairs (their keys are copies, so no key of the corpus is lost) for the cut reads
        bcs = bcs + list(SHORT_BARCODES)
        n = keys.shape[0]
        keys, origin, d1, d2 = (np.concatenate([a, a[:n:10]]) for a in (keys, origin, d1, d2))
    c = Corpus(name, shape, (m1, m2), bcs, keys, origin, d1, d2, seed + 1000)
    c.lists = lists
    if name == "mixed_len":  # those pairs' reads cut to the short barcodes' lengths: half equal one, half one substitution away
        S, fail_q = len(bcs) - len(SHORT_BARCODES), chr(shape.plan.min_qual - 1 + 33).encode()
        for i, r in enumerate(range(n, c.n)):
            j = i % len(SHORT_BARCODES)
            b = bytearray(SHORT_BARCODES[j].encode())
            cut1 = (8, 8, 5)[j]
            hit, gate_fails = i % 2 == 0, i % 4 >= 2
            if not hit:
                p = int(rng.integers(0, len(b)))
                b[p] = ord("A") if b[p] != ord("A") else ord("N")
            if i % 3 == 0:
                b[int(rng.integers(0, len(b)))] |= 0x20
            q = bytearray(b"I" * len(b))
            if gate_fails:
                q[int(rng.integers(0, len(b)))] = fail_q[0]
            code = (2 * (S + j) + int(gate_fails)) if hit else 0xFFFF
            c.cut(r, [(bytes(b[:cut1]), bytes(q[:cut1])), (bytes(b[cut1:]), bytes(q[cut1:]))], code, code)
    return c


@functools.lru_cache(maxsize=None)
def no_segments_corpus(shape_name):
    """one sample; all 5^K keys under each of the four quality patterns, then the same keys in reads cut inside the slice"""
    shape, (m1, m2) = TIGHT[shape_name], NO_SEGMENTS[shape_name]
    K = shape.w1 + shape.w2
    bcs = ["AC"]
    keys = np.array(list(itertools.product(ACGTN.tolist(), repeat=K)), dtype=np.uint8)
    keys = np.concatenate([np.repeat(keys, 4, axis=0)] * 2)
    full = keys.shape[0] // 2
    bc = np.frombuffer(bcs[0].encode(), np.uint8)
    d = keys != bc[None, :]
    c = Corpus("no_segments_" + shape_name, shape, (m1, m2), bcs, keys, np.zeros(keys.shape[0], np.int64),
               d[:, :shape.w1].sum(axis=1), d[:, shape.w1:].sum(axis=1), 77)
    for r in range(full, c.n):  # the second copy: one read loses the end of its slice
        k = r % len(shape.lens)
        reads = [(s[r], q[r]) for s, q in c.streams]
        keep = shape.w1 - 1 if k == 0 else shape.w2 - 1
        reads[k] = (reads[k][0][:keep], reads[k][1][:keep])
        c.cut(r, reads, 0xFFFF, 0xFFFF)
    return c
