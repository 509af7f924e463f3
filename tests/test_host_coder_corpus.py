"""No GPU: the DEFLATE reader (tests/deflate_reader.py) against zlib's own streams and the forged corpus, and the texts of
tests/coder_corpus.py against what they claim -- computed from their bytes."""
import time
import zlib

import numpy as np
import pytest

from tests import coder_corpus as CC
from tests import deflate_forge as F
from tests import deflate_reader as R


def _expanded(blocks):
    """the text the blocks' tokens stand for (stored blocks carry none: their text is taken as read)"""
    return sum(sum(tok[3] for tok in b.tokens) if b.kind != "stored" else b.text_len for b in blocks)


@pytest.fixture(scope="module")
def fastq():
    return CC.fastq_like(np.random.default_rng(1), 150_000)


@pytest.mark.parametrize("level,strategy,kinds", [(0, zlib.Z_DEFAULT_STRATEGY, {"stored"}), (1, zlib.Z_DEFAULT_STRATEGY, {"dynamic"}),
                                                  (6, zlib.Z_DEFAULT_STRATEGY, {"dynamic"}), (9, zlib.Z_DEFAULT_STRATEGY, {"dynamic"}),
                                                  (6, zlib.Z_FIXED, {"fixed"}), (6, zlib.Z_RLE, {"dynamic"}), (6, zlib.Z_HUFFMAN_ONLY, {"dynamic"})])
def test_reader_reads_zlibs_streams(fastq, level, strategy, kinds):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    gz = c.compress(fastq) + c.flush()
    t0 = time.perf_counter()
    m = R.read_member(gz)
    spent = time.perf_counter() - t0
    assert m.text == fastq and m.crc32 == zlib.crc32(fastq) and m.isize == len(fastq) and m.length == len(gz)
    assert {b.kind for b in m.blocks} == kinds and [b.final for b in m.blocks] == [0] * (len(m.blocks) - 1) + [1]
    assert _expanded(m.blocks) == len(fastq)
    at = 0
    for b in m.blocks:  # blocks and tokens follow each other in the text and in the member
        assert b.text_start == at and b.bit_end > b.bit_start
        for tok in b.tokens:
            assert tok[2] == at and b.bit_start < tok[0] and tok[0] + tok[1] <= b.bit_end
            assert (tok[4] == 0 and tok[3] == 1) or (3 <= tok[3] <= 258 and 1 <= tok[4] <= min(32768, at))
            at += tok[3]
        if b.kind == "stored":
            at += b.text_len
        if b.kind == "dynamic":
            assert len(b.litlens) == b.hlit and len(b.distlens) == b.hdist and sum(n for _, n in b.cl_ops) == b.hlit + b.hdist
            assert all((s < 16 and n == 1) or (s == 16 and 3 <= n <= 6) or (s == 17 and 3 <= n <= 10) or (s == 18 and 11 <= n <= 138) for s, n in b.cl_ops)
        if strategy == zlib.Z_HUFFMAN_ONLY:
            assert all(tok[4] == 0 for tok in b.tokens)
        if strategy == zlib.Z_RLE:
            assert all(tok[4] <= 1 for tok in b.tokens)
    assert spent < 10.0, spent  # (a 64 KiB block reads in a tenth of a second; the ceiling only catches a reader gone bit by bit, on a busy machine too)


def test_reader_reads_members_in_a_row():
    a, b = b"first member " * 100, b""
    gz = F.gzip_member(zlib.compress(a, 6)[2:-4], a, name=b"a.txt", extra=b"xy", hcrc=True) + F.gzip_member(b"\x03\x00", b)
    c = zlib.compressobj(1, zlib.DEFLATED, 31)
    gz += c.compress(a[::-1]) + c.flush()
    ms = R.read_members(gz)
    assert [m.text for m in ms] == [a, b, a[::-1]] and sum(m.length for m in ms) == len(gz)
    assert ms[0].header_bytes > 10 and ms[1].blocks[0].kind == "fixed" and ms[1].crc32 == 0


def test_reader_reads_the_forged_streams():
    """every legal stream of the forge: text, block kinds and token expansions as zlib's"""
    for name, raw, text, tags in F.corpus():
        if text is None:
            continue
        got, blocks, bit = R.read_deflate(raw)
        assert bytes(got) == text == zlib.decompress(raw, -15), name
        assert (bit + 7) // 8 == len(raw) and blocks[-1].final and _expanded(blocks) == len(text), name
        rebuilt = bytearray()
        for b in blocks:
            if b.kind == "stored":
                rebuilt += text[b.text_start:b.text_start + b.text_len]
            else:
                F.expand([text[tok[2]] if not tok[4] else (tok[3], tok[4]) for tok in b.tokens], rebuilt)
        assert bytes(rebuilt) == text, name
    name, raw, text, tags = F.case("L4 runs")
    ops = R.read_deflate(raw)[1][0].cl_ops
    assert (18, 138) in ops and (16, 6) in ops and (17, 3) in ops, ops
    with pytest.raises(ValueError):
        R.read_deflate(b"\x07")  # block type 3


def test_unrestricted_huffman_depth():
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    assert R.huffman_depth(fib) == 23 and R.huffman_depth([7] * 16) == 4 and R.huffman_depth([0, 5, 0]) == 1 and R.huffman_depth([]) == 0
    assert R.huffman_depth([1, 1, 2, 4, 8, 0, 16]) == 5


def test_corpus_is_small_and_the_same_every_time():
    assert CC.total_bytes() < 8.5e6
    assert CC.group_far()[3].data == CC.group("far")[3].data and CC.group_lengths()[1].data == CC.group("lengths")[1].data
    for g in CC.GROUP_NAMES:
        for t in CC.group(g):
            assert t.name and t.why and (len(t.data) <= 2 * CC.SUB or g == "alternating"), t.name


def test_planted_copies_are_where_they_claim():
    for t in CC.group("far") + [t for t in CC.group("distances") if not t.meta["periodic"]]:
        d, p1, p2, n = t.meta["d"], t.meta["p1"], t.meta["p2"], t.meta["n"]
        x = t.data
        assert p2 - p1 == d and x[p1:p1 + n] == x[p2:p2 + n] and x[p1 + n] != x[p2 + n] and x[p1 - 1] != x[p2 - 1], t.name
        assert len(set(x[p1 + n:p2])) == 1 and p2 + n < len(x) <= CC.SUB, t.name  # quiet text between, inside one sub-block
    assert [t.meta["d"] for t in CC.group("far")] == list(CC.FAR_DISTANCES) * 2
    assert all(0 in t.data[t.meta["p1"]:t.meta["p1"] + 64] and t.meta["fill"] == 0 for t in CC.group("far")[5:])
    for t in CC.group("distances"):
        if t.meta["periodic"]:
            d, x = t.meta["d"], t.data
            assert x[d:] == x[:-d] and all(x[e:] != x[:-e] for e in range(1, d)) and len(x) >= 512 + 64, t.name
    assert {t.meta["d"] for t in CC.group("distances")} == {F.DBASE[s] + e for s in range(30) for e in (0, (1 << F.DEXT[s]) - 1)}


def test_units_of_every_length_at_every_residue():
    starts, ends, lengths, two_stretches = set(), set(), [], 0
    for t in CC.group("lengths"):
        x = t.data
        plants = t.meta["plants"]
        for k, (p1, p2, n) in enumerate(plants):
            cut = t.meta["kind"] == "cut" and k == len(plants) - 1
            m = t.meta["keep"] if cut else n
            assert p2 - p1 >= CC.MIN_APART and x[p1:p1 + m] == x[p2:p2 + m] and x[p1 - 1] != x[p2 - 1], (t.name, p1, p2, n)
            assert not set(x[p1:p1 + n]) & set(b"ACGTN")
            if cut:
                assert p2 + m == len(x) and m < n
                continue
            assert x[p1 + n] != x[p2 + n]
            if t.meta["kind"] == "sweep":
                starts.add(p2 % 64)
                ends.add((p2 + n) % 64)
                lengths.append(n)
                two_stretches += (p2 + 63) // 64 * 64 + 128 <= p2 + n
            if t.meta["kind"] == "straddle":
                assert p2 // CC.PART != (p2 + n - 1) // CC.PART and p2 % CC.PART >= CC.PART - n + 4 and (p2 + n) % CC.PART >= 4
    assert starts == set(range(64)) and {63, 0, 1} <= ends and two_stretches >= 10
    assert sorted(set(lengths)) == sorted(CC.UNIT_LENGTHS)
    assert {t.meta["kind"] for t in CC.group("lengths")} == {"sweep", "straddle", "cut"}


def test_long_token_text():
    t = CC.group("long tokens")[0]
    x = t.data
    assert len(x) <= CC.SUB and len(t.meta["plants"]) >= 64 and len(set(x)) > 240
    for p1, p2, n in t.meta["plants"]:
        assert x[p1:p1 + n] == x[p2:p2 + n] and p2 - p1 >= 16385 and n >= 131 + 5
        assert x[p1 + n:p2].count(CC.DOT) >= 9000  # a run between the two copies


def test_limit_text():
    t = CC.group("limit literals")[0]
    x = t.data
    counts = sorted(x.count(v) for v in t.meta["values"])
    assert counts == sorted(CC.LIMIT_COUNTS) and len(counts) >= 20 and len(x) == sum(counts) <= CC.SUB
    assert not any(x[i] == x[i + 1] == x[i + 2] == x[i + 3] for i in range(len(x) - 3))
    assert R.huffman_depth(counts + [1]) > 15  # with the end-of-block code
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    assert R.huffman_depth(fib + [1]) <= 15  # why the counts are not Fibonacci numbers


def test_limit_distance_text():
    t = CC.group("limit distances")[0]
    x = t.data
    assert len(x) <= CC.SUB
    counts, at = [0] * 30, 0
    for p, d in t.meta["plants"]:  # copies of 4 bytes, each ended by its literal, none inside another; all else is literals
        assert p >= at and d <= p and x[p:p + 4] == x[p - d:p - d + 4] and x[p + 4] != x[p - d + 4], (p, d)
        assert d > p % CC.ROUND and (p - d) % CC.ROUND >= CC.ROUND - 16  # the source: late in a round before the copy's
        counts[max(s for s in range(30) if F.DBASE[s] <= d)] += 1
        at = p + 5
    assert tuple(counts[4:22]) == CC.LIMIT_DIST_COUNTS and sum(counts) == sum(CC.LIMIT_DIST_COUNTS)
    assert sum(1 for c in counts if c) >= 17 and R.huffman_depth(counts) > 15 + 1  # a level to spare
    exact = sorted(CC.LIMIT_DIST_COUNTS[:16])  # the counts that are kept as planted: each sum below the count after the next
    assert all(sum(exact[:k + 1]) * 1.02 < exact[k + 2] for k in range(14))
    assert min(CC.LIMIT_DIST_COUNTS[16:]) > 1.2 * sum(exact[:15]) and CC.LIMIT_DIST_COUNTS[16] > 1.15 * sum(exact)  # a sixth may go
    assert not any(x[i] == x[i + 1] == x[i + 2] == x[i + 3] for i in range(len(x) - 3))


def test_header_sweep_alphabets():
    texts = CC.group("headers")
    gaps = {}
    for t in texts:
        if "seam" in t.meta:
            x = t.data  # periodic stretches of periods 1, 2, 3 that begin a few bytes before a round's start
            assert x[:510] == b"Z" * 510 and x[512:1021] == x[510:1019] and x[1024:1533] == x[1021:1530] and len(set(x[1533:])) == len(x) - 1533
        elif "gap" in t.meta:
            assert len(t.data) == 64 and set(t.data) == {t.meta["lo"], t.meta["hi"]} and t.meta["hi"] - t.meta["lo"] - 1 == t.meta["gap"], t.name
            gaps.setdefault(255 if "up to 255" in t.name else 254 if "up to 254" in t.name else 0, set()).add(t.meta["gap"])
        else:
            k, base = t.meta["k"], t.meta["base"]
            assert sorted(t.data) == list(range(base, base + k)), t.name
    assert gaps[0] == set(range(1, 255)) and gaps[255] == set(range(1, 255)) and gaps[254] == set(range(1, 254))
    assert {t.meta["k"] for t in texts if "k" in t.meta} == set(range(1, 41))
    assert max(len(t.data) for t in texts if "seam" not in t.meta) <= 64 and sum("seam" in t.meta for t in texts) == 1


def test_sizes_and_pieces():
    want = set(range(1, 71)) | {8192 * k + e for k in range(1, 9) for e in (-1, 0, 1, 3)} | set(range(65533, 65540))
    for kind in CC.SIZE_KINDS:
        texts = CC.group("sizes " + kind)
        assert {len(t.data) for t in texts} == want == {t.meta["n"] for t in texts}
        for t in texts:
            n = len(t.data)
            if kind == "run":
                assert len(set(t.data)) == 1
            if kind in ("zeros behind", "0xFF behind"):
                assert t.data[-40:] == bytes([0 if kind == "zeros behind" else 255]) * min(n, 40)
    many = CC.group("many")
    assert len(many) == 3000 and all(len(t.data) <= 200 for t in many) and all(len(many[i].data) == 0 for i in CC.EMPTY_PIECES)
    assert 0 in CC.EMPTY_PIECES and 2999 in CC.EMPTY_PIECES and len(CC.EMPTY_PIECES) >= 5 and max(len(t.data) for t in many) == 200
    assert len(CC.group("alternating")[0].data) == 20 * CC.SUB
    assert len(CC.CRC_SIZES) >= 36 and all((n + 1) % 132 < 3 for n in CC.CRC_SIZES)
