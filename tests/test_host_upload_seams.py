"""The inputs of tests/upload_seams.py proven on the host: every framing inflates to its text with Python's gzip (the reference's
reader), and every fact the GPU tests rest on is counted here from the bytes on disk -- file sizes and uploads per stream, the seams of
gz_members and bgzf_seams at their claimed offsets, the forged block and the damaged bytes behind the first upload, dense's text per
buffer, the precondition of "one upload per top-up" -- and the library's host reader reads the healthy framings of `long` to the
oracle reader's records."""
import gzip
import zlib

import numpy as np
import pytest

from oracle import quade_oracle as qo
from tests import record_geometry as G
from tests import upload_seams as U

S = U.S
HEALTHY_LONG = ("gz", "bgzf", "gz_members", "bgzf_seams", "bgzf_then_gz")
ALL_FIELDS = 2 | 4 | 8 | 16  # FHCRC, FEXTRA, FNAME, FCOMMENT


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    """files(framing): the framing's files, written once per module"""
    made = {}

    def files(framing):
        if framing not in made:
            made[framing] = U.frame(framing, tmp_path_factory.mktemp(framing))
        return made[framing]
    yield files
    U.forget()


def _raw(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("framing", sorted(U.FRAMINGS))
def test_pythons_gzip_reads_every_file_to_its_text(framing, on_disk):
    """the reference opens its inputs with gzip.open: zero padding, an empty member and BGZF followed by a gzip member included"""
    p, files = U.texts(U.FRAMINGS[framing]), on_disk(framing)
    for k in G.STREAMS:
        assert len(files[k]) == p.n_chunks
        for c, path in enumerate(files[k]):
            raw = _raw(path)
            if framing.endswith("damaged_late") and k == "seq_R1":
                try:
                    assert gzip.decompress(raw) != p.chunks[c][k]
                except (OSError, EOFError, zlib.error):
                    pass
            else:
                assert gzip.decompress(raw) == p.chunks[c][k], (k, c)


def test_text_sets_hold_what_they_claim():
    p = U.texts("long")
    assert p.batch_pairs == 97 and p.n_chunks == 1 and p.facts["pairs"] == U.N_LONG and p.facts["kept"][0] == {k: U.N_LONG for k in G.STREAMS}
    for k, mean in (("seq_R1", U.LEN_R1), ("seq_R2", U.LEN_R2)):
        lines = p.chunks[0][k].split(b"\n")
        reads = [len(ln) for ln in lines[1::4]]
        assert len(reads) == U.N_LONG and min(reads) >= 0.9 * mean and max(reads) <= 1.1 * mean and max(reads) - min(reads) > 0.15 * mean
        seen = np.bincount(np.frombuffer(b"".join(lines[1::4] + lines[3::4]), dtype=np.uint8), minlength=256)
        assert seen[:33].sum() == 0 and seen[127:].sum() == 0 and seen[33:127].min() > 0.9 * seen.sum() / 94  # uniform over 33 .. 126
    # "one upload per top-up": a window asks for batch_pairs records of the learned size, 3 % more and 4 KiB; while that is less than
    # an upload's bytes, and a byte of the file stands for at least one of text, top_up stops after one upload
    for name in U.SETS:
        q = U.texts(name)
        mean = max(len(c[k]) / float(len(G.records_of(c[k]))) for c in q.chunks for k in G.STREAMS)
        assert 97 * mean * 1.03 + 4096 < S, (name, mean)
    p = U.texts("ends_early")
    assert p.n_chunks == 2 and p.facts["pairs_per_chunk"] == [U.N_EARLY_INDEX_R2, U.N_EARLY_NEXT] == [150, 300]
    assert p.facts["kept"][0] == {"seq_R1": U.N_EARLY, "seq_R2": U.N_EARLY, "index_R1": U.N_EARLY, "index_R2": 150}
    p = U.texts("dense")
    assert p.n_chunks == 1 and p.facts["pairs"] == U.N_DENSE
    recs = G.records_of(p.chunks[0]["seq_R1"])
    assert all(100_000 < n < (1 << 20) for _, n, _ in recs)  # below one output member: larger records are out of scope
    assert p.chunks[0]["seq_R1"].count(b"A" * U.LEN_DENSE + b"\n+\n" + b"I" * U.LEN_DENSE + b"\n") == U.N_DENSE
    assert U.texts("long").chunks == U.texts.__wrapped__("long").chunks  # the same texts for the same seed


@pytest.mark.parametrize("framing", [f for f in sorted(U.FRAMINGS) if U.FRAMINGS[f] == "long"])
def test_long_is_four_uploads_of_seq_r1_and_two_of_seq_r2(framing, on_disk):
    files = on_disk(framing)
    sizes = {k: len(_raw(files[k][0])) for k in G.STREAMS}
    assert sizes["seq_R1"] > 3 * S and sizes["seq_R2"] > S and sizes["index_R1"] < S and sizes["index_R2"] < S, sizes
    want = {"seq_R1": 4, "seq_R2": 2, "index_R1": 1, "index_R2": 1}
    for k in G.STREAMS:
        path = files[k][0]
        if U.bgzf_layout(path) and not (framing == "bgzf_then_gz" and k == "seq_R1"):
            assert sum(b[1] for b in U.bgzf_layout(path)) == sizes[k]  # BGZF to the end
            assert len(U.bgzf_cuts(path)) == want[k], (k, len(U.bgzf_cuts(path)))
        else:
            assert U.uploads(path) == want[k], (k, sizes[k])


def test_gz_members_seams_lie_where_they_are_claimed(on_disk):
    files = on_disk("gz_members")
    p = U.texts("long")
    ms, rest = U.members(files["seq_R1"][0])
    assert len(ms) == 6 and sum(m[4] for m in ms) == len(p.chunks[0]["seq_R1"])
    assert rest == bytes(4096)                                               # zero padding behind the last member
    assert any(tr + 8 == S for _, _, _, tr, _ in ms)                         # a trailer that ends exactly at S
    assert any(at == S and n == 0 for at, _, _, _, n in ms)                  # an empty member directly behind that seam
    assert any(tr == 2 * S - 4 for _, _, _, tr, _ in ms)                     # CRC in [2S - 4, 2S), ISIZE in [2S, 2S + 4)
    assert any(at == 3 * S - 5 and flg == ALL_FIELDS and data > 3 * S for at, flg, data, _, _ in ms)  # a full header across 3S
    assert any(n == 10 for _, _, _, _, n in ms)
    assert all(data - at < 4096 for at, _, data, _, _ in ms)                 # (gz_steps reads a header from 64 KiB of the file)
    ms, rest = U.members(files["seq_R2"][0])
    assert len(ms) == 2 and rest == b"" and S + (1 << 20) < ms[1][0] < len(_raw(files["seq_R2"][0])) - (1 << 20)  # they meet inside the second upload
    for k in ("index_R1", "index_R2"):
        assert len(U.members(files[k][0])[0]) == 1


def test_bgzf_seams_lie_where_the_cut_model_puts_them(on_disk):
    path = on_disk("bgzf_seams")["seq_R1"][0]
    text = U.texts("long").chunks[0]["seq_R1"]
    blocks, cuts = U.bgzf_layout(path), U.bgzf_cuts(path)
    assert sum(b[1] for b in blocks) == len(_raw(path)) and sum(b[4] for b in blocks) == len(text)
    assert all(b[4] <= U.BLOCK_TEXT and b[1] <= 65536 for b in blocks)
    ends = [pos + S for pos, _ in cuts[:-1]]  # where a buffer ends with more of the file behind it
    assert len(cuts) == 4 and len(ends) == 3
    assert any(b[0] + b[1] == e for b in blocks for e in ends)                                   # a block ends exactly at a buffer's end
    assert any(1 <= e - b[0] <= 17 for b in blocks for e in ends)                                # fewer than 18 bytes of a header
    assert any(b[2] == 200 and 18 <= e - b[0] <= 150 and e - b[0] < 12 + b[2] for b in blocks for e in ends)  # 18 or more, but not its extra field
    assert blocks[-1][4] == 0 and blocks[-1][1] == 28                                            # bgzip's EOF marker
    assert any(b[4] == 0 and 0 < i < len(blocks) - 1 for i, b in enumerate(blocks))              # an empty block in the middle
    # every buffer but the first starts inside a record: the one before it ends with a part of one
    starts = {at for at, _, _ in G.records_of(text)}
    assert all(inside[0][3] not in starts for _, inside in cuts[1:])
    # the other framings' BGZF files are cut inside a block, as bgzip's blocks of one size always are
    plain = U.bgzf_cuts(on_disk("bgzf")["seq_R1"][0])
    assert all(inside[-1][0] + inside[-1][1] < pos + S for pos, inside in plain[:-1])


def test_bgzf_then_gz_switches_behind_the_first_upload(on_disk):
    path = on_disk("bgzf_then_gz")["seq_R1"][0]
    raw, blocks = _raw(path), U.bgzf_layout(path)
    at = blocks[-1][0] + blocks[-1][1]
    assert S + (1 << 20) <= at < 2 * S and at < len(raw)
    assert raw[at:at + 4] == b"\x1f\x8b\x08\x00"  # an ordinary member: no extra field
    d = zlib.decompressobj(-15)
    rest = d.decompress(raw[at + 10:])
    assert d.eof and len(d.unused_data) == 8 and sum(b[4] for b in blocks) + len(rest) == len(U.texts("long").chunks[0]["seq_R1"])


def test_gz_refused_late_has_its_forged_block_behind_the_first_upload(on_disk):
    path = on_disk("gz_refused_late")["seq_R2"][0]
    raw, text = _raw(path), U.texts("long").chunks[0]["seq_R2"]
    n = len(text) - U.FORGED_TEXT
    d = zlib.decompressobj(-15)
    assert d.decompress(raw[10:], n - 1) == text[:n - 1]  # (one byte short: the inflater stops in front of the flush)
    near = len(raw) - len(d.unconsumed_tail)
    at = raw.index(b"\x00\x00\xff\xff", near - 16) + 4  # the full flush's empty stored block: the forged stream starts behind it
    d = zlib.decompressobj(-15)
    assert d.decompress(raw[10:at]) == text[:n] and not d.eof and d.unused_data == b""
    assert at > S and U.uploads(path) == 2
    assert raw[at] & 7 == 4  # not final, dynamic: the block of 256 codes of 15 bits
    assert (raw[at] >> 3) + 257 == 286  # HLIT: all 286 literal/length symbols are listed


def test_damaged_bytes_lie_in_payload_behind_the_first_upload(on_disk):
    for fmt in ("gz", "bgzf"):
        good, bad = _raw(on_disk(fmt)["seq_R1"][0]), _raw(on_disk(fmt + "_damaged_late")["seq_R1"][0])
        assert len(good) == len(bad)
        diff = np.flatnonzero(np.frombuffer(good, dtype=np.uint8) != np.frombuffer(bad, dtype=np.uint8))
        assert len(diff) == 1 and S + (1 << 20) <= diff[0] <= 2 * S
        at = int(diff[0])
        if fmt == "gz":
            ms, _ = U.members(on_disk("gz")["seq_R1"][0])
            assert len(ms) == 1 and ms[0][2] <= at < ms[0][3]
        else:
            b = next(b for b in U.bgzf_layout(on_disk("bgzf")["seq_R1"][0]) if b[0] <= at < b[0] + b[1])
            assert b[0] + 12 + b[2] <= at < b[0] + b[1] - 8
        assert _raw(on_disk(fmt)["seq_R2"][0]) == _raw(on_disk(fmt + "_damaged_late")["seq_R2"][0])  # (the other files are whole)


def test_ends_early_chunk_0_is_three_uploads_per_insert_stream(on_disk):
    for framing in ("ends_early_gz", "ends_early_bgzf"):
        files = on_disk(framing)
        for k in U.INSERTS:
            path = files[k][0]
            assert len(_raw(path)) > 2 * S
            assert (len(U.bgzf_cuts(path)) if framing.endswith("bgzf") else U.uploads(path)) == 3
            assert len(_raw(files[k][1])) < S
        # the index streams end long before: 150 records against 1 050
        assert len(_raw(files["index_R2"][0])) < 4096


def test_dense_buffer_holds_more_text_than_a_segment_takes(on_disk):
    path = on_disk("dense")["seq_R1"][0]
    cuts = U.bgzf_cuts(path)
    assert len(cuts) == 1 and len(_raw(path)) < S
    assert sum(b[4] for b in cuts[0][1]) > U.SEG_TEXT_MAX
    assert len(G.bgzf_blocks(path)) == len(cuts[0][1]) > 2000


# ---- the readers ----------------------------------------------------------------------------------------------------------------
def _host_reader_text(path, B):
    from quade_amd.fastq_reader import FastqStream
    stream, parts, sizes = FastqStream(path, B, queue_depth=2), [], []
    while True:
        b = stream.take()
        parts.append(bytes(b.text[:b.off[b.n]]) if b.n else b"")
        sizes.append(b.n)
        b.release()
        if b.n < B:
            break
    stream.close()
    return b"".join(parts), sizes


@pytest.mark.parametrize("framing", HEALTHY_LONG)
def test_host_reader_equals_the_oracle_reader(framing, on_disk):
    """fastq_reader (qd_reader) reads the multi-upload files to the same records as the oracle's reader: every record's bytes, in
    batches of 97"""
    p, files = U.texts("long"), on_disk(framing)
    for k in U.INSERTS:
        text = p.chunks[0][k]
        got, sizes = _host_reader_text(files[k][0], 97)
        assert got == text, k
        assert all(n == 97 for n in sizes[:-1]) and len(sizes) == U.N_LONG // 97 + 1
        if k == "seq_R1" or framing == "gz_members":  # (seq_R2 differs from framing to framing only there)
            lines = text.split(b"\n")
            want = [(h[1:].split()[0].decode("latin-1"), s.decode("latin-1")) for h, s in zip(lines[0:-1:4], lines[1::4])]
            n = 0
            for r, w in zip(qo.FastqReader(files[k][0]), want):
                assert (r.name, r.seq) == w and len(r.qual) == len(r.seq)
                n += 1
            assert n == len(want) == U.N_LONG
