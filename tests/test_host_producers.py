"""No GPU: the producer corpus (tests/producer_corpus.py) -- DEFLATE as libdeflate, pigz and GNU gzip write it, and two decoys -- proven
against zlib first, then read block by block (tests/deflate_reader.py): every stream has the shape it was built for, so that a quiet
change of a library cannot empty tests/test_gpu_producers.py."""
import shutil
import zlib

import pytest

from tests import deflate_reader as R
from tests import producer_corpus as P

TEXT_BYTES = frozenset([9, 10, 13] + list(range(32, 127)))  # what the gzip probe's text filter lets a literal code cover
FASTQ_TEXTS = ("fastq", "fastq, 4 qualities, one read length")

needs_gzip = pytest.mark.skipif(shutil.which("gzip") is None, reason="no gzip program on this machine")


def _shape(c):
    return P.shape(c[0], c[1])[1]


def _of(producer, **tags):
    return [c for c in P.corpus() if c[3]["producer"] == producer and all(c[3].get(k) == v for k, v in tags.items())]


def test_libdeflate_is_here():
    """the library the product writes its own files with: its cases do not skip"""
    assert P.libdeflate() is not None
    assert len(_of("libdeflate")) == len(P.LIBDEFLATE_LEVELS) * len(P.texts()) and P.case("decoy (a)")


def test_every_stream_inflates_with_zlib_to_its_text():
    names = [c[0] for c in P.corpus()]
    assert len(set(names)) == len(names) and P.corpus() is P.corpus()
    assert len(_of("pigz")) == len(P.texts()) and P.case("decoy (b)")
    for name, raw, text, tags in P.corpus():
        assert zlib.decompress(raw, -15) == text, name
    for name, pieces, tags in P.bgzf_cases():
        assert all(zlib.decompress(raw, -15) == text and len(text) <= P.BGZF_TEXT for raw, text in pieces), name
        assert all(len(raw) <= 65536 - 26 for raw, _ in pieces), name


def test_libdeflate_blocks_are_longer_than_any_zlib_writes():
    for lv in (6, 9, 12):
        for tname in FASTQ_TEXTS:
            (c,) = _of("libdeflate", level=lv, text=tname)
            blocks = _shape(c)
            assert any(b["tokens"] > 32767 and b["text_len"] > 200_000 and b["kind"] == "dynamic" for b in blocks), (c[0], [(b["tokens"], b["text_len"]) for b in blocks])
            # ... and than the units of the tests' small geometry and the stretches of the probe: a lane crosses several without a start
            assert max(b["bit_end"] - b["bit_start"] for b in blocks) > 8 * 5 * P.STRETCH, c[0]
    assert len(_shape(_of("libdeflate", level=6, text="fastq")[0])) == 8
    far = [max(b["max_dist"] for b in _shape(c)) for lv in (9, 12) for c in _of("libdeflate", level=lv, text="fastq")]
    assert max(far) > 32506, far
    (c,) = _of("libdeflate", level=6, text="runs")
    assert any(b["max_dist"] == 1 and b["tokens"] > 1000 for b in _shape(c))
    for lv in P.LIBDEFLATE_LEVELS:
        (c,) = _of("libdeflate", level=lv, text="random bytes")
        assert all(b["kind"] == "stored" for b in _shape(c)), c[0]
        (c,) = _of("libdeflate", level=lv, text="short")
        assert len(_shape(c)) == 1


def test_a_libdeflate_piece_of_one_bgzf_block_is_one_deflate_block():
    """65 280 bytes of fastq with 41 qualities: ONE dynamic block of more than 32 767 tokens at every level (zlib cuts there).  With 11
    qualities (30 500 tokens at level 6) one block at levels 6 / 9 / 12; level 1 cuts that text in two, at 46 000 bytes."""
    n = {}
    for name, pieces, tags in P.bgzf_cases():
        if tags["producer"] != "libdeflate" or tags["piece"] != P.BGZF_TEXT:
            continue
        for raw, text in pieces:
            if len(text) == P.BGZF_TEXT:
                _, blocks, _ = R.read_deflate(raw)
                if tags["text"] == "fastq, 41 qualities":
                    assert len(blocks) == 1 and blocks[0].kind == "dynamic" and len(blocks[0].tokens) > 32767, (name, len(blocks), len(blocks[0].tokens))
                elif tags["level"] > 1:
                    assert len(blocks) == 1 and blocks[0].kind == "dynamic" and len(blocks[0].tokens) > 20_000, (name, len(blocks))
                else:
                    assert len(blocks) <= 2, (name, len(blocks))
                n[tags["text"]] = n.get(tags["text"], 0) + 1
    assert n == {"fastq": 4 * len(P.LIBDEFLATE_LEVELS), "fastq, 41 qualities": 2 * len(P.LIBDEFLATE_LEVELS)}


def test_libdeflate_writes_every_block_type_here():
    kinds = set()
    for c in _of("libdeflate"):
        kinds |= {b["kind"] for b in _shape(c)}
    assert kinds == {"stored", "fixed", "dynamic"}, kinds


def test_pigz_shape_has_a_sync_flush_per_chunk_and_matches_into_the_chunk_before():
    for c in _of("pigz"):
        blocks, chunks = _shape(c), c[3]["chunks"]
        assert sum(1 for b in blocks if b["final"]) == 1 and blocks[-1]["final"], c[0]
        empty_stored = [b["text_start"] for b in blocks if b["kind"] == "stored" and b["text_len"] == 0]
        assert empty_stored == [k * P.PIGZ_CHUNK for k in range(1, chunks)], (c[0], empty_stored)
    (c,) = _of("pigz", text="fastq")
    assert c[3]["chunks"] == 19 and sum(b["cross"] for b in _shape(c)) > 1000


@needs_gzip
def test_gnu_gzip_streams_are_its_own():
    assert len(_of("gzip")) == len(P.GZIP_LEVELS) * len(P.texts())
    for lv in P.GZIP_LEVELS:
        (c,) = _of("gzip", level=lv, text="fastq")
        assert c[1] != P.zlib_raw(c[2], lv) and len(_shape(c)) > 10


def test_the_decoys_hold_a_dynamic_header_where_no_block_starts():
    decoys = [(c[0], c[1], c[3]["decoy_byte"], True) for c in _of("decoy") if "decoy_byte" in c[3]]
    decoys += [(name, pieces[0][0], tags["decoy_byte"], False) for name, pieces, tags in P.bgzf_cases() if tags["producer"] == "decoy"]
    assert len(decoys) == 3
    for name, raw, at, in_stretch in decoys:
        _, (b,), _ = R.read_deflate(raw, bit=8 * at, max_blocks=1)
        assert b.kind == "dynamic" and not b.final and len(b.tokens) > 500, name
        assert not [s for s in range(256) if b.litlens[s] and s not in TEXT_BYTES], name
        _, blocks, _ = R.read_deflate(raw)
        inside = [k for k, x in enumerate(blocks) if x.bit_start < 8 * at < x.bit_end]
        assert len(inside) == 1 and blocks[inside[0]].kind == "stored", name
        assert raw[at:at + 40] == P.decoy_bytes()[:40]
        # directly behind the stored block a dynamic block of ~300 KB (one BGZF block's rest) begins, at (a) ... in the decoy's stretch of
        # the probe, at the default stretch size and at half of it: the first header that holds there is the decoy's
        hidden = blocks[inside[0] + 1] if name.startswith("decoy (a)") else blocks[inside[0] + 2]
        assert hidden.kind == "dynamic" and hidden.text_len > (250_000 if in_stretch else 50_000), name
        if in_stretch:
            assert len(hidden.tokens) > 60_000 and hidden.bit_end - hidden.bit_start > 8 * 6 * P.STRETCH, name
            for stretch in (P.STRETCH, P.STRETCH // 2):
                assert at // stretch == hidden.bit_start // (8 * stretch) and at % stretch < 64, (name, at, hidden.bit_start)
                assert not any(x.kind == "dynamic" and x.bit_start // (8 * stretch) == at // stretch and x.bit_start < 8 * at for x in blocks), name
    # (b): the true start is the small dynamic block in front of the boundary, the first block start of ITS stretch
    name, raw, at, _ = [d for d in decoys if d[0].startswith("decoy (b)")][0]
    _, blocks, _ = R.read_deflate(raw)
    k = [k for k, x in enumerate(blocks) if x.bit_start < 8 * at < x.bit_end][0]
    true_start = blocks[k - 1]
    assert true_start.kind == "dynamic" and blocks[k + 1].kind == "fixed" and 0 < 8 * at - true_start.bit_start < 8 * 1000
    for stretch in (P.STRETCH, P.STRETCH // 2):
        assert true_start.bit_start // (8 * stretch) == at // stretch - 1
        assert not any(x.kind == "dynamic" and x.bit_start // (8 * stretch) == at // stretch - 1 and x.bit_start < true_start.bit_start for x in blocks)


def test_decoy_c_spells_a_header_inside_the_block_the_member_begins_with():
    name, raw, text, tags = P.case("decoy (c)")
    bit, hdr = tags["decoy_bit"], tags["header_bits"]
    v, nbits, hdr2 = P.decoy_block(tags["decoy_source"])
    assert hdr2 == hdr > 200 and (int.from_bytes(raw[bit // 8:bit // 8 + 100], "little") >> (bit % 8)) & ((1 << hdr) - 1) == v & ((1 << hdr) - 1)
    _, (b,), _ = R.read_deflate(v.to_bytes((nbits + 7) // 8, "little"), max_blocks=1)
    assert b.kind == "dynamic" and not b.final and not [s for s in range(256) if b.litlens[s] and s not in TEXT_BYTES]
    blocks = _shape((name, raw))
    first = blocks[0]
    # one block from the member's start, longer in tokens than eight slots a byte up to the decoy hold; the decoy just behind the
    # first stretch boundary (at the default stretch size and at half of it), no block boundary in front of it
    assert first["bit_start"] == 0 < bit < first["bit_end"] and first["kind"] == "dynamic" and not first["final"]
    assert first["tokens"] > 8 * (bit // 8) + 4096 + 10_000 and first["long_codes"] == 2
    assert 0 < bit - 8 * P.STRETCH < 128 and blocks[-1]["final"]


def test_no_block_has_more_long_codes_than_the_device_holds():
    """Beyond 112 codes longer than 7 bits a block may be refused by design (deflate_forge's long_codes tag): none of these comes near,
    so tests/test_gpu_producers.py may ask that no stream is refused."""
    worst = 0
    for c in P.corpus():
        worst = max([worst] + [b["long_codes"] for b in _shape(c)])
    for name, pieces, tags in P.bgzf_cases():
        for raw, _ in pieces:
            worst = max([worst] + [P.long_codes(b) for b in R.read_deflate(raw)[1] if b.kind == "dynamic"])
    assert 0 < worst <= 112, worst
