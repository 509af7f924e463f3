"""The device's gzip coders (quade_amd/csrc/quade_deflate.hip) on texts built for their seams (tests/coder_corpus.py).

zlib is the judge of every member.  tests/deflate_reader.py then reads from the member itself that the text reached the seam it
was built for: the conditions below are conditions on the corpus, not tolerances -- a text that misses its condition is changed
(seed, spacing), the assertion stays.  No member's bytes are expected: the coder is free to change them."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

from tests import coder_corpus as CC
from tests import deflate_reader as R

pytestmark = pytest.mark.gpu
SUB = CC.SUB


class _Coder(object):
    def __init__(self):
        from quade_amd import hip_backend as hb
        self.hb, self.lib = hb, hb.load_library()
        self.d = C.c_void_p()
        assert self.lib.qd_deflater_create(0, C.byref(self.d)) == 0

    def close(self):
        self.lib.qd_deflater_destroy(self.d)

    def run(self, pieces, level, crc=True):
        """the members of the pieces; crc=False: crc32 == NULL, the CRC-32s come from the coder"""
        lib, hb = self.lib, self.hb
        assert lib.qd_deflater_set_level(self.d, level) == 0
        n = len(pieces)
        keep, ptrs = [], (C.c_void_p * n)()
        for i, t in enumerate(pieces):
            b = np.frombuffer(t, np.uint8) if len(t) else np.zeros(1, np.uint8)
            keep.append(b)
            ptrs[i] = b.ctypes.data
        lens = np.array([len(t) for t in pieces], np.int64)
        crcs = np.array([zlib.crc32(t) for t in pieces], np.uint32)
        stride = lib.qd_huffman_member_bound(int(lens.max()))
        out = np.zeros(n * stride, np.uint8)
        ml = np.zeros(n, np.int64)
        rc = lib.qd_deflater_run(self.d, n, ptrs, hb._ptr(lens), hb._ptr(crcs) if crc else None, 0, hb._ptr(out), stride, hb._ptr(ml))
        assert rc == 0, lib.qd_deflater_last_error(self.d)
        return [bytes(out[i * stride:i * stride + int(ml[i])]) for i in range(n)]


@pytest.fixture(scope="module")
def coder():
    c = _Coder()
    yield c
    c.close()


def _check(coder, texts, level, read=True):
    """what holds for every member; returns what the reader made of them"""
    pieces = [t.data for t in texts]
    members = coder.run(pieces, level)
    assert coder.run(pieces, level) == members, "a second run gives other bytes"
    out = []
    for t, m in zip(texts, members):
        data = t.data
        assert len(m) >= 20 and gzip.decompress(m) == data, (t.name, level, len(m))
        if not read:
            continue
        r = R.read_member(m)
        assert r.text == data and r.crc32 == zlib.crc32(data) and r.isize == len(data) and r.length == len(m) and r.header_bytes == 10, (t.name, level)
        if level == 1:
            # per 64 KiB of text one dynamic block of exactly that text and an empty stored block, then the empty final block
            n_sub = (len(data) + SUB - 1) // SUB
            assert len(r.blocks) == 2 * n_sub + 1, (t.name, len(r.blocks))
            for k in range(n_sub):
                b, s = r.blocks[2 * k], r.blocks[2 * k + 1]
                assert b.kind == "dynamic" and not b.final and b.text_start == k * SUB and b.text_len == min(SUB, len(data) - k * SUB), (t.name, k)
                assert b.bit_start % 8 == 0
                assert s.kind == "stored" and not s.final and s.text_len == 0, (t.name, k)
                assert all(tok[4] <= tok[2] - b.text_start for tok in b.tokens), (t.name, k, "a distance reaches back before its sub-block")
            last = r.blocks[-1]
            assert last.final and last.text_len == 0 and not last.tokens and (last.bit_end + 7) // 8 == len(m) - 8, t.name
        else:
            assert len(r.blocks) == 1, t.name
            b = r.blocks[0]
            assert b.kind == "dynamic" and b.final and all(tok[3] == 1 for tok in b.tokens), t.name
        out.append(r)
    return out


def _tokens(r):
    return [tok for b in r.blocks for tok in b.tokens]


def _matches(r):
    return [tok for tok in _tokens(r) if tok[4]]


def test_far_distances(coder):
    texts = CC.group("far")
    _check(coder, texts, -1)
    for t, r in zip(texts, _check(coder, texts, 1)):
        p2, d = t.meta["p2"], t.meta["d"]
        over = [tok for tok in _tokens(r) if tok[2] < p2 + 64 and tok[2] + tok[3] > p2]
        if d <= 32768:
            assert (p2, 64, d) in [tok[2:] for tok in over], (t.name, [tok[2:] for tok in over][:8])
        else:  # beyond the window: the second copy is not a copy
            assert all(tok[4] == 0 for tok in over), (t.name, [tok[2:] for tok in over if tok[4]])


def test_every_length(coder):
    texts = CC.group("lengths")
    _check(coder, texts, -1)
    seen = set()
    for t, r in zip(texts, _check(coder, texts, 1)):
        toks = {tok[2]: tok for tok in _tokens(r)}
        seen |= {tok[3] for tok in toks.values() if tok[4]}
        kind, plants = t.meta["kind"], t.meta["plants"]
        if kind == "cut":
            plants, (p1, p2, n) = plants[:-1], plants[-1]
            last = _tokens(r)[-1]
            assert last[4] == p2 - p1 and last[2] + last[3] == len(t.data) and last[2] >= p2, (t.name, last)
        for p1, p2, n in plants:
            if kind == "straddle":
                edge = (p2 + n) // CC.PART * CC.PART
                assert p2 < edge < p2 + n
                for pos in (edge - 1, edge):  # both sides of the parts' border lie in matches from the first copy
                    cover = [tok for tok in toks.values() if tok[2] <= pos < tok[2] + tok[3]]
                    assert cover and cover[0][4] == p2 - p1, (t.name, p2, n, cover)
                continue
            at, left = p2, n
            while left >= 4:  # a unit longer than the longest match decodes as several
                assert at in toks and toks[at][3:] == (min(left, 256), p2 - p1), (t.name, (p1, p2, n), at, toks.get(at))
                at, left = at + min(left, 256), left - min(left, 256)
    assert seen == set(range(4, 257)), sorted(set(range(4, 257)) ^ seen)


def test_every_distance_code(coder):
    texts = CC.group("distances")
    _check(coder, texts, -1)
    seen = set()
    for t, r in zip(texts, _check(coder, texts, 1)):
        ds = {tok[4] for tok in _matches(r)}
        assert t.meta["d"] in ds, (t.name, sorted(ds))
        seen.add(t.meta["d"])
    from tests.deflate_forge import DBASE, DEXT
    assert seen == {DBASE[s] + e for s in range(30) for e in (0, (1 << DEXT[s]) - 1)}


def test_long_tokens(coder):
    texts = CC.group("long tokens")
    _check(coder, texts, -1)
    b = _check(coder, texts, 1)[0].blocks[0]
    widest = max(tok[1] for tok in b.tokens)
    far = [tok for tok in b.tokens if tok[3] >= 131 and tok[4] >= 16385]
    assert len(far) >= 64, len(far)
    third = [tok for tok in b.tokens if (tok[0] - b.bit_start) % 32 + tok[1] > 64]
    # ... and what reaches it is not nothing: the token's bits from the 64th on, as they stand in the member
    stream = int.from_bytes(coder.run([texts[0].data], 1)[0], "little")
    spill = [tok for tok in third if (stream >> (tok[0] + 64 - (tok[0] - b.bit_start) % 32)) & ((1 << ((tok[0] - b.bit_start) % 32 + tok[1] - 64)) - 1)]
    print("largest token: %d bits; %d tokens reach a third word, %d with a one there" % (widest, len(third), len(spill)))
    assert third, "no token reaches a third word; the largest token has %d bits, %d long far matches" % (widest, len(far))
    assert spill, "the tokens that reach a third word have only zeros there; the largest token has %d bits" % widest


def test_literal_code_needs_the_limit_at_level_1(coder):
    texts = CC.group("limit literals")
    _check(coder, texts, -1)
    b = _check(coder, texts, 1)[0].blocks[0]
    counts = [0] * 286
    counts[256] = 1
    for tok in b.tokens:
        if tok[4]:
            counts[257 + max(s for s in range(29) if R.LBASE[s] <= tok[3])] += 1
        else:
            counts[texts[0].data[tok[2]]] += 1
    assert [bool(c) for c in counts[:b.hlit]] == [bool(n) for n in b.litlens], "the block's code is not for its own counts"
    assert max(b.litlens) == 15 and R.huffman_depth(counts) > 15, (max(b.litlens), R.huffman_depth(counts))


def test_distance_code_needs_the_limit_at_level_1(coder):
    texts = CC.group("limit distances")
    _check(coder, texts, -1)
    b = _check(coder, texts, 1)[0].blocks[0]
    counts = [0] * 30
    for tok in b.tokens:
        if tok[4]:
            counts[max(s for s in range(30) if R.DBASE[s] <= tok[4])] += 1
    print("matches by distance code:", counts, "code lengths:", b.distlens)
    assert [bool(c) for c in counts[:b.hdist]] == [bool(n) for n in b.distlens] and not any(counts[b.hdist:]), "the block's code is not for its own counts"
    assert max(b.distlens) == 15 and R.huffman_depth(counts) > 15, (max(b.distlens), R.huffman_depth(counts), counts)


def test_header_sweeps(coder):
    texts = CC.group("headers")
    _check(coder, texts, -1)
    ops16, ops17, ops18, split, across = set(), set(), set(), 0, []
    for t, r in zip(texts, _check(coder, texts, 1)):
        b = r.blocks[0]
        at = 0
        zero_ops = []  # (start, count) of the operations that send zeros
        for s, n in b.cl_ops:
            {16: ops16, 17: ops17, 18: ops18}.get(s, set()).add(n)
            if s in (0, 17, 18):
                zero_ops.append((at, n))
            # a run that lies in both lists: a repeat counts from the length it repeats
            first = at - 1 if s == 16 else at
            if s >= 16 and first < b.hlit < at + n:
                across.append((t.name, s, n, at, b.hlit))
            at += n
        assert at == b.hlit + b.hdist
        if "gap" in t.meta:
            lo, hi, g = t.meta["lo"], t.meta["hi"], t.meta["gap"]
            assert b.litlens[lo] and b.litlens[hi] and not any(b.litlens[lo + 1:hi]), t.name
            if g >= 139 and len([1 for a, n in zero_ops if lo < a < hi]) > 1:
                split += 1
        if "seam" in t.meta:
            assert b.litlens[-1] == b.distlens[0] == b.distlens[1] == b.distlens[2] and across and across[-1][0] == t.name, (
                b.litlens[257:], b.distlens, b.cl_ops[-8:])
    assert ops16 >= {3, 4, 5, 6}, sorted(ops16)
    assert ops17 >= set(range(3, 11)), sorted(ops17)
    assert {11, 138} <= ops18 and len(ops18 - {11, 138}) >= 100, sorted(ops18)
    assert split >= 100, split
    assert across, "no operation's run spans the literal/length and the distance lengths"


def test_slot_too_small_at_level_1(coder):
    """A piece of two sub-blocks, random bytes and fastq text, and slots that are too small.  A slot 64 bytes under
    qd_huffman_member_bound still holds the member of any piece: random bytes cost 8 bits and a little, the bound allows 9 1/8 and
    1 024 bytes (on the MI355X this piece of 130 000 bytes makes a member of 101 396, the bound is 149 308).  There the member must
    be whole.  In a slot 64 bytes under what the member needs, and in the smallest slot the call takes, member_len is 0, the bytes
    behind the slot are untouched, and the next call with a proper slot succeeds."""
    lib, hb = coder.lib, coder.hb
    t = bytes(np.random.default_rng(77).integers(0, 256, 60000).astype(np.uint8)) + CC.group("alternating")[0].data[SUB:SUB + 70000]
    whole = coder.run([t], 1)[0]
    assert gzip.decompress(whole) == t
    buf, lens, crc = np.frombuffer(t, np.uint8), np.array([len(t)], np.int64), np.array([zlib.crc32(t)], np.uint32)
    ptrs = (C.c_void_p * 1)(buf.ctypes.data)
    bound = lib.qd_huffman_member_bound(len(t))
    for stride, fits in ((bound - 64, True), ((len(whole) - 64) & ~3, False), (64, False)):
        out = np.full(stride + 256, 0xAB, np.uint8)
        ml = np.full(1, -1, np.int64)
        assert lib.qd_deflater_run(coder.d, 1, ptrs, hb._ptr(lens), hb._ptr(crc), 0, hb._ptr(out), stride, hb._ptr(ml)) == 0
        print("slot %d bytes, member %d bytes, bound %d: member_len %d" % (stride, len(whole), bound, ml[0]))
        assert (out[stride:] == 0xAB).all(), stride
        if fits:
            assert bytes(out[:int(ml[0])]) == whole
        else:
            assert ml[0] == 0, (stride, ml[0])
        assert coder.run([t], 1)[0] == whole


@pytest.mark.parametrize("kind", CC.SIZE_KINDS)
def test_sizes(coder, kind):
    texts = CC.group("sizes " + kind)
    _check(coder, texts, -1)
    _check(coder, texts, 1)


def test_many_pieces(coder):
    texts = CC.group("many")
    for level in (-1, 1):
        rs = _check(coder, texts, level)
        for i in CC.EMPTY_PIECES:
            assert rs[i].text == b"" and rs[i].isize == 0 and rs[i].crc32 == 0


def test_alternating_sub_blocks(coder):
    texts = CC.group("alternating")
    _check(coder, texts, -1, read=False)
    r = _check(coder, texts, 1)[0]
    offsets = [b.bit_start // 8 for b in r.blocks if b.kind == "dynamic"]
    assert len(offsets) == 20 and {o % 4 for o in offsets} == {0, 1, 2, 3}, offsets


def test_crc_from_the_coder(coder):
    """crc32 == NULL at level 1: the members' CRC-32s come from the sub-block kernel's own stage and the combine over a piece's
    sub-blocks, as in the device pipeline; at level -1 NULL is refused"""
    base = CC.group("sizes fastq")[-1].data
    long = CC.group("alternating")[0].data
    pieces = [t.data for k in CC.SIZE_KINDS for t in CC.group("sizes " + k)]
    pieces += [CC.sized(k, base, n) for k in CC.SIZE_KINDS for n in CC.CRC_SIZES]
    pieces += [long[SUB:3 * SUB - 5], long[:17 * SUB - 100], b"", long[5:SUB + 6]]
    members = coder.run(pieces, 1, crc=False)
    for t, m in zip(pieces, members):
        assert len(m) >= 20 and int.from_bytes(m[-8:-4], "little") == zlib.crc32(t) and int.from_bytes(m[-4:], "little") == len(t), len(t)
        assert gzip.decompress(m) == t
    assert members == coder.run(pieces, 1, crc=True)
    lib, hb = coder.lib, coder.hb
    assert lib.qd_deflater_set_level(coder.d, -1) == 0
    buf, lens, ml = np.frombuffer(b"abc", np.uint8), np.array([3], np.int64), np.zeros(1, np.int64)
    out = np.zeros(4096, np.uint8)
    assert lib.qd_deflater_run(coder.d, 1, (C.c_void_p * 1)(buf.ctypes.data), hb._ptr(lens), None, 0, hb._ptr(out), 4096, hb._ptr(ml)) == hb.QD_ERR_INVALID
