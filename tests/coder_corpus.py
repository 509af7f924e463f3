"""Texts built for the seams of the device's gzip coders (quade_amd/csrc/quade_deflate.hip): what fastq text and a few random
pieces never reach.  Every text has a name and the condition it exists for; tests/test_host_coder_corpus.py proves from the bytes
that the texts are what they claim, tests/test_gpu_coder_corpus.py reads from the members (tests/deflate_reader.py) that the coder
got where the text was sent.

What the texts rely on about the coder: a match is at least 4 bytes and at most 256, reaches back at most 32 768 positions and
never leaves its 64 KiB sub-block; a position finds an earlier copy through a table of few entries per hash; a match is taken only
where it is cheaper than its literals.  So
  * FILLER is a run of one byte: whatever the hash, a run occupies one bucket, and a far candidate survives it;
  * planted copies lie at least 520 positions apart (the look-ups of one round of positions see only the rounds before);
  * short units are made of bytes that are rare in their piece (dear literals), and of no bases (a match inside a sequence line
    must be 12 long).
  * where counts of matches matter (the lengths' first copies, the distance code's limit), sources lie at the end of a round of
    ROUND look-ups: positions of one round with one hash keep the last of them only.  This leans on the round's size: with
    another one these texts are to be shaped again (their tests say which condition they miss), though the coder is right.
Seeded and deterministic: the same bytes in every process.  `group(name)` is built once per process.
"""
from collections import namedtuple

import numpy as np

from tests.deflate_forge import DBASE, DEXT, expand

SUB = 65536          # text per sub-block of the level-1 coder
STRETCH = 64         # positions the parse walks at a time
PART = 8192          # a wave's part of a sub-block
ROUND = 512          # positions that are looked up before any of them is entered
NONBASE = bytes(b for b in range(33, 127) if b not in b"ACGTN")  # printable, no bases
DOT = ord(".")       # the printable filler
UNIT_BYTES = bytes(b for b in NONBASE if b != DOT)
ANY_BYTES = bytes(b for b in range(1, 256) if b not in b"ACGTN" and b != DOT)  # for unique literals: 249 values

# meta: what the tests assert, by group (see the builders)
Text = namedtuple("Text", "name why data meta")


def _draw(rng, n, alphabet):
    a = np.frombuffer(alphabet, np.uint8)
    return bytes(a[rng.integers(0, len(a), n)])


def _differing(rng, n, alphabet):
    """n different bytes of the alphabet"""
    a = np.frombuffer(alphabet, np.uint8)
    return bytes(a[rng.permutation(len(a))[:n]])


def fastq_like(rng, n_bytes, binned=True):
    """records whose names repeat most of their predecessor's and (binned) whose qualities come in runs"""
    out, size, i = [], 0, 0
    while size < n_bytes:
        seq = _draw(rng, 150, b"ACGT")
        if binned:
            q = np.full(150, ord("F"), np.uint8)
            for _ in range(int(rng.integers(0, 6))):
                a = int(rng.integers(0, 150))
                q[a:a + int(rng.integers(1, 12))] = b":,#"[int(rng.integers(0, 3))]
            qual = bytes(q)
        else:
            qual = bytes(rng.integers(35, 74, 150).astype(np.uint8))
        rec = b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT+TTGCAATC\n%s\n+\n%s\n" % (1101 + i // 3000, 1000 + (i * 37) % 30000,
                                                                                       1000 + (i * 101) % 35000, seq, qual)
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


# ---- 1. far distances -------------------------------------------------------------------------------------------------------------
FAR_DISTANCES = (32767, 32768, 32769, 40000, 65000)


def _far_text(rng, d, zero):
    """lead | U | filler | U | tail: the second U at distance d; what follows (and precedes) the two copies differs"""
    fill = 0 if zero else DOT
    u = bytearray(_draw(rng, 64, UNIT_BYTES))
    if zero:
        for k in (7, 8, 30, 31, 32, 50):
            u[k] = 0
    lead, tail = _differing(rng, 16, UNIT_BYTES), _differing(rng, 8, UNIT_BYTES)
    data = lead + bytes(u) + bytes([fill]) * (d - 64) + bytes(u) + tail
    return data, {"p1": 16, "p2": 16 + d, "n": 64, "d": d, "fill": fill}


def group_far():
    rng = np.random.default_rng(101)
    out = []
    for zero in (False, True):
        for d in FAR_DISTANCES:
            data, meta = _far_text(rng, d, zero)
            out.append(Text("far d=%d%s" % (d, " zeros" if zero else ""),
                            "a repeat at distance %d behind a run of %s: the window's bound" % (d, "zero bytes" if zero else "one byte"), data, meta))
    return out


# ---- 2. every length --------------------------------------------------------------------------------------------------------------
UNIT_LENGTHS = tuple(range(4, 257)) + (257, 258, 300, 600)
MIN_APART = 520


class _Layout(object):
    """pieces of at most one sub-block, filled with planted pairs: pre1 U post1 filler pre2 U post2, the bytes around the two
    copies all different; plants: (p1, p2, n) in the piece"""

    def __init__(self, rng, limit=SUB - 1024):
        self.rng, self.limit = rng, limit
        self.pieces, self.cur, self.plants = [], bytearray(), []

    def close(self):
        if self.cur:
            self.pieces.append((bytes(self.cur), self.plants))
        self.cur, self.plants = bytearray(), []

    def pair(self, n, start_residue=None, end_residue=None, p2=None):
        if len(self.cur) + 2 * n + MIN_APART + 200 + ROUND > self.limit:
            self.close()
        cur = self.cur
        u = _draw(self.rng, n, UNIT_BYTES)
        edge = _differing(self.rng, 4, bytes(b for b in UNIT_BYTES if b != u[0] and b != u[-1]))
        # the first copy starts on the last position of a round of look-ups: positions of one round with one hash keep the
        # last of them only, and the unit's own later positions must not push its first one out
        cur += bytes([DOT]) * ((ROUND - 2 - len(cur)) % ROUND)
        cur.append(edge[0])
        p1 = len(cur)
        assert p1 % ROUND == ROUND - 1
        cur += u
        cur.append(edge[1])
        at = max(p1 + MIN_APART, len(cur) + 16 + 1)  # the earliest second copy
        if p2 is None:
            p2 = at
            if end_residue is not None:
                start_residue = (end_residue - n) % STRETCH
            if start_residue is not None:
                p2 += (start_residue - p2) % STRETCH
        assert p2 >= at, (p2, at)
        cur += bytes([DOT]) * (p2 - 1 - len(cur))
        cur.append(edge[2])
        cur += u
        cur.append(edge[3])
        self.plants.append((p1, p2, n))


def group_lengths():
    rng = np.random.default_rng(203)
    out = []
    lay = _Layout(rng)
    for i, n in enumerate(UNIT_LENGTHS):
        lay.pair(n, start_residue=i % STRETCH)
    for e in (63, 0, 1):  # second copies that end one before, on and one behind a stretch's end
        for n in (5, 37, 200):
            lay.pair(n, end_residue=e)
    lay.close()
    for k, (data, plants) in enumerate(lay.pieces):
        out.append(Text("lengths %d" % k, "a unit of every length twice, the second copies at every residue of the parse's stretches",
                        data, {"plants": plants, "kind": "sweep"}))
    lay = _Layout(np.random.default_rng(2020), limit=SUB)  # second copies across the ends of the waves' parts
    for k, n in zip(range(1, 8), (40, 100, 24, 300, 64, 9, 200)):
        lay.pair(n, p2=PART * k - max(4, n // 3))
    lay.close()
    assert len(lay.pieces) == 1
    out.append(Text("lengths straddle", "second copies across positions 8192 k: a match ends with its wave's part",
                    lay.pieces[0][0], {"plants": lay.pieces[0][1], "kind": "straddle"}))
    for n, keep in ((200, 100), (40, 20), (600, 300), (12, 5)):  # the piece ends inside the second copy
        lay = _Layout(rng)
        lay.pair(9, start_residue=3)
        lay.pair(n, start_residue=61)
        lay.close()
        data, plants = lay.pieces[0]
        data = data[:plants[-1][1] + keep]
        out.append(Text("lengths cut %d of %d" % (keep, n), "the piece ends inside a second copy: a match ends with the text",
                        data, {"plants": plants, "kind": "cut", "keep": keep}))
    return out


# ---- 3. every distance code -------------------------------------------------------------------------------------------------------
CODE_DISTANCES = tuple(sorted({DBASE[s] + e for s in range(30) for e in (0, (1 << DEXT[s]) - 1)}))


def group_distances():
    rng = np.random.default_rng(303)
    out = []
    for d in CODE_DISTANCES:
        if d <= 512:  # periodic text; a period without a repeated byte where it is short
            unit = _differing(rng, d, UNIT_BYTES) if d <= 8 else _draw(rng, d, UNIT_BYTES)
            data = (unit * (640 // d + 2))[:640]
            meta = {"d": d, "periodic": True}
        else:
            lead, tail, u = _differing(rng, 8, UNIT_BYTES), _differing(rng, 8, UNIT_BYTES), _draw(rng, 64, UNIT_BYTES)
            data = lead + u + bytes([DOT]) * (d - 64) + u + tail
            meta = {"d": d, "periodic": False, "p1": 8, "p2": 8 + d, "n": 64}
        out.append(Text("distance %d" % d, "first or last distance of its distance code", data, meta))
    return out


# ---- 4. long tokens ---------------------------------------------------------------------------------------------------------------
def group_long_tokens():
    """One sub-block of mostly unique literals (long literal codes, many tokens).  First some 3 000 matches of 4 bytes, built as a
    token list: 513 .. 4 096 back, the nearer the more (common length and distance symbols, the distance symbols graded so that
    the rare ones lie deep).  Then twice: 34 units of 136 .. 256 bytes, a run, and the units again, each 20 497 (then 16 401) positions and more
    behind its first copy -- lengths of 131 and more (5 extra bits, four length symbols of some 17 matches each) at distances with
    13 extra bits.  A unit is longer than 131 because its first positions may have lost their place in the table."""
    rng = np.random.default_rng(419)
    n_far, lo_unit, near_bytes = 34, 136, 14000
    text = bytearray(_draw(rng, 1100, ANY_BYTES))
    while len(text) < near_bytes:
        j = min(int(rng.geometric(0.5)) - 1, 5)
        lo = (513, 769, 1025, 1537, 2049, 3073)[j]
        d = int(rng.integers(lo, lo + (256, 256, 512, 512, 1024, 1024)[j]))
        if d > len(text):
            d = int(rng.integers(513, 1025))
        expand([(4, d)], text)
        text.extend(_draw(rng, 1, ANY_BYTES))
    plants = []
    for dist in (20497, 16401):  # (the first: distances whose 13 extra bits begin with a one -- what spills into the third word)
        a0 = len(text)
        units = [int(u) for u in rng.integers(lo_unit, 257, n_far)]
        starts = [a0 + sum(units[:k]) for k in range(n_far)]
        text += _draw(rng, sum(units), ANY_BYTES)
        text += bytes([DOT]) * (dist - sum(units))
        for k in range(n_far):
            text += _draw(rng, int(rng.integers(1, 4)), ANY_BYTES)
            plants.append((starts[k], len(text), units[k]))
            text += text[starts[k]:starts[k] + units[k]]
    assert len(text) <= SUB, len(text)
    return [Text("long tokens", "long codes + 5 length extra bits + 13 distance extra bits: a token that reaches a third word",
                 bytes(text), {"plants": plants})]


# ---- 6. the 15-bit limit at level 1 -----------------------------------------------------------------------------------------------
# Fibonacci counts are the borderline of a Huffman code that is as deep as it has symbols: the end-of-block code's one more count
# lets equal weights meet, and the code of 1 1 2 3 5 .. over 22 values and one more 1 is 12 deep, not 21.  Counts that grow by 1.7
# keep every sum below the count after the next: 20 values, 58 059 bytes, 18 deep with the end-of-block code.
LIMIT_COUNTS = tuple(max(1, round(1.7 ** k)) for k in range(20))


def group_limit_literals():
    """The counts above over 20 byte values, shuffled, but never a fourth equal byte in a row.  The commonest values cost 1 .. 3
    bits each, so a match of fewer than some 16 bytes is dearer than its literals: a dozen matches, the rest stays literals."""
    rng = np.random.default_rng(606)
    vals = [ord("a") + i for i in range(len(LIMIT_COUNTS))]
    pool = np.repeat(np.array(vals, np.uint8), LIMIT_COUNTS)
    out, held = [], []
    for b in pool[rng.permutation(len(pool))].tolist():  # a byte that would be the fourth equal one in a row waits for its place
        cand, held = [b] + held, []
        for c in cand:
            if len(out) >= 3 and out[-1] == out[-2] == out[-3] == c:
                held.append(c)
            else:
                out.append(c)
    for c in held:  # what the end could not take goes where it makes no run
        for p in range(3, len(out) - 3):
            if c not in out[p - 3:p + 3]:
                out.insert(p, c)
                break
    return [Text("limit literals", "literal counts that grow by 1.7 over 20 values: the literal/length code needs the 15-bit limit at level 1",
                 bytes(out), {"values": vals})]


# The distance code: 18 codes, 4 .. 21 (distances 5 .. 2 048), whose match counts grow by 1.63 -- every sum of the k rarest stays
# 2.7 % below the count after the next, and the code is 17 deep where 16 would do.  (20 codes with Fibonacci counts are 17 710
# matches and do not fit a sub-block; these are 11 641 matches of 4 bytes with a literal between.)
LIMIT_DIST_CODES = tuple(range(4, 22))
LIMIT_DIST_COUNTS = tuple(round(1.63 ** k) for k in range(16)) + (4700, 3000)  # by code; the last two only have to be large enough


def _dist_code(d):
    return max(s for s in range(30) if DBASE[s] <= d)


def group_limit_distances():
    """A token list: literals that are all different where it matters, and matches of 4 bytes, each followed by a literal that ends
    it.  Every match of round R (the ROUND positions that are looked up before any of them is entered) copies one of four sources:
    the last position of round R - 1, the 6th from the end of R - 2, the 11th of R - 3 and the 16th of R - 4 (apart, so that a copy
    with a chance byte before it holds no other source).  Such a source has next to nothing behind it in its own round with which
    it could share a bucket (the later position would stay), it is not seen from its own round, and each is used from one round
    only, so no nearer copy of it is in the table when it is looked up.
    The first has no round entered over it and the second one: two entries per bucket keep both.  Their distance follows from the
    position in the round: the codes 4 .. 17 from the first source, 18 and 19 from the second -- these 16 counts are kept as planted.
    The third and fourth source (codes 20 and 21) have two and three rounds entered over them and may lose their bucket, with all
    their round's matches; they carry the two largest counts, which have no upper bound to keep, and a fifth more than they need.
    The last and first positions of every round are literals: the sources and what they copy."""
    rng = np.random.default_rng(707)
    left = dict(zip(LIMIT_DIST_CODES, LIMIT_DIST_COUNTS))
    low = LIMIT_DIST_CODES[:14]
    share = {c: -(-left[c] // 60) for c in low}  # of a round, so that the near codes are spread over the text's first 60 rounds
    text = bytearray(_draw(rng, ROUND + 3, ANY_BYTES))
    plants, in_round, this_round = [], {}, -1

    def back(j):
        return 5 * j - 4  # the source of j rounds back, counted from its round's end: 1, 6, 11, 16

    while any(left.values()):
        p = len(text)
        r, start = p % ROUND, p - p % ROUND
        if r >= ROUND - 17 or r < 3:
            text += _draw(rng, 1, ANY_BYTES)
            continue
        if start != this_round:
            this_round, in_round = start, dict.fromkeys(low, 0)
        due = [c for c in low if left[c] and in_round[c] < share[c]]
        near = _dist_code(r + 1)
        if near in due:
            j = 1
        elif any(0 < DBASE[c] - 1 - r <= 4 for c in due):  # a near code that is due begins within a token's length: wait for it
            text += _draw(rng, 1, ANY_BYTES)
            continue
        else:
            far = [j for j in (2, 3, 4) if start - ROUND * (j - 1) - back(j) >= 0 and left.get(_dist_code(r + ROUND * (j - 1) + back(j)))]
            if not far:
                text += _draw(rng, 1, ANY_BYTES)
                continue
            weights = np.cumsum([left[_dist_code(r + ROUND * (j - 1) + back(j))] for j in far])
            j = far[int(np.searchsorted(weights, rng.integers(0, weights[-1]), "right"))]
        d = r + ROUND * (j - 1) + back(j)
        c = _dist_code(d)
        if j == 1:
            in_round[c] += 1
        expand([(4, d)], text)
        text += _differing(rng, 1, bytes(b for b in ANY_BYTES if b != text[p + 4 - d]))  # the copy ends here
        left[c] -= 1
        plants.append((p, d))
    assert len(text) <= SUB, len(text)
    return [Text("limit distances", "match counts that grow by 1.63 over 18 distance codes: the distance code needs the 15-bit limit",
                 bytes(text), {"plants": plants})]


# ---- 5. header sweeps -------------------------------------------------------------------------------------------------------------
def _two_values(rng, lo, hi):
    """64 bytes over two values, both present, without a run of 4 or a repeated 4-gram to speak of: lo hi lo lo hi hi ..."""
    pat = rng.integers(0, 2, 64).astype(np.uint8)
    pat[0], pat[1] = 0, 1
    return bytes(np.where(pat == 0, lo, hi).astype(np.uint8))


def group_headers():
    rng = np.random.default_rng(505)
    out = []
    for g in range(1, 255):
        out.append(Text("zero run %d" % g, "a zero run of %d between two used literals" % g, _two_values(rng, 0, g + 1), {"gap": g, "lo": 0, "hi": g + 1}))
    for g in range(1, 255):
        out.append(Text("zero run %d up to 255" % g, "the same, the last literal being 255", _two_values(rng, 254 - g, 255), {"gap": g, "lo": 254 - g, "hi": 255}))
    for g in range(1, 254):
        out.append(Text("zero run %d up to 254" % g, "the same, the last literal being 254", _two_values(rng, 253 - g, 254), {"gap": g, "lo": 253 - g, "hi": 254}))
    for k in range(1, 41):
        base = 60 + 3 * k
        vals = np.arange(base, base + k, dtype=np.uint8)
        out.append(Text("equal counts %d" % k, "%d adjacent byte values equally often: runs of equal non-zero lengths" % k,
                        bytes(vals[rng.permutation(k)]), {"k": k, "base": base}))
    out.append(Text("seam run", "the last literal/length length and the first distance lengths are equal: a run across the two lists",
                    seam_text(), {"seam": True}))
    return out


SEAM_EXTRA = 10


def seam_text(extra=SEAM_EXTRA):
    """Six matches of 253 .. 256 bytes (one length symbol, the last one in use) among a few literals, at distances 1 1 2 258 3 258:
    four distance codes, 0 1 2 and 16, of two bits each, and two bits for the length symbol.  A distance below 512 is only found
    right behind the start of a round of 512 look-ups, so the periodic stretches begin a few bytes before positions 512 and 1 024."""
    text = bytearray(b"Z" * 510)
    text += (b"ab" * 256)[:511]                   # 510 .. 1 020: a match of 256 at 512, distance 2; the rest from 258 back
    text += (b"cde" * 171)[:512]                  # 1 021 .. 1 532: a match of 256 at 1 024, distance 3; the rest from 258 back
    text += bytes(range(0x30, 0x30 + extra))      # literals that make the length symbol a quarter of the tokens
    return bytes(text)


# ---- 7. sizes ---------------------------------------------------------------------------------------------------------------------
SIZES = tuple(sorted(set(list(range(1, 71)) + [PART * k + e for k in range(1, 9) for e in (-1, 0, 1, 3)] + list(range(65533, 65540)))))
SIZE_KINDS = ("fastq", "run", "zeros behind", "0xFF behind")


def sized(kind, base, n):
    if kind == "run":
        return b"Q" * n
    if kind == "fastq":
        return base[:n]
    tail = bytes([0 if kind == "zeros behind" else 0xFF]) * min(n, 40)
    return base[:n - len(tail)] + tail


def group_sizes(kind, sizes=SIZES):
    base = fastq_like(np.random.default_rng(808), max(sizes))
    return [Text("%s %d" % (kind, n), "a piece of %d bytes: the ends of tiles, parts, slices and sub-blocks" % n, sized(kind, base, n), {"n": n})
            for n in sizes]


CRC_SIZES = tuple(sorted({132 * k + e for k in (1, 2, 3, 7, 31, 32, 33, 64, 100, 255, 256, 400, 496) for e in (-1, 0, 1)}))


# ---- 8. many pieces ---------------------------------------------------------------------------------------------------------------
EMPTY_PIECES = (0, 1, 700, 1500, 1501, 2222, 2999)


def group_many():
    rng = np.random.default_rng(909)
    base = fastq_like(rng, 300_000, binned=False)
    out = []
    for i in range(3000):
        n = 0 if i in EMPTY_PIECES else int(rng.integers(1, 201))
        a = int(rng.integers(0, len(base) - 200))
        out.append(Text("small %d" % i, "one of 3 000 small pieces of a launch", base[a:a + n], {"n": n}))
    return out


def group_alternating():
    """20 sub-blocks: runs, fastq text, random bytes in turn -- blocks of a few hundred and of 70 000 bytes, so that the sub-blocks
    land at many byte offsets in the member"""
    rng = np.random.default_rng(910)
    parts = []
    for k in range(20):
        if k % 3 == 0:
            parts.append(bytes([65 + k]) * SUB)
        elif k % 3 == 1:
            parts.append(fastq_like(rng, SUB, binned=k % 2 == 0))
        else:
            parts.append(bytes(rng.integers(0, 256, SUB).astype(np.uint8)))
    return [Text("alternating", "20 sub-blocks of alternating compressibility in one member", b"".join(parts), {"subs": 20})]


_GROUPS = {}
_BUILDERS = {
    "far": group_far, "lengths": group_lengths, "distances": group_distances, "long tokens": group_long_tokens, "headers": group_headers,
    "limit literals": group_limit_literals, "limit distances": group_limit_distances,
    "many": group_many, "alternating": group_alternating,
}
for _kind in SIZE_KINDS:
    _BUILDERS["sizes " + _kind] = (lambda kind: lambda: group_sizes(kind))(_kind)
GROUP_NAMES = tuple(_BUILDERS)


def group(name):
    """the texts of one group, built once per process"""
    if name not in _GROUPS:
        _GROUPS[name] = _BUILDERS[name]()
    return _GROUPS[name]


def total_bytes():
    return sum(len(t.data) for g in GROUP_NAMES for t in group(g))
