"""The record-geometry profiles (tests/record_geometry.py) on the host: their facts, counted here once more from the texts in another
way; the three file formats read back; the oracle's pairs per chunk; and the library's host reader against the oracle's reader on
reads of 0 to 200 000 bases."""
import re

import numpy as np
import pytest

from oracle import quade_oracle as qo
from tests import record_geometry as G
from tests.run_support import _conf

SEED = 20


def _lines(text):
    """(line without its end, bytes with its end) of a text: counted with a regular expression, not with the generator's walk"""
    return [(m.group(1), len(m.group(0))) for m in re.finditer(rb"([^\n]*?)\r?(?:\n|\Z)", text) if m.group(0)]


def _records(text):
    """[(bytes, kept, name)] of the whole records of a text"""
    ln = _lines(text)
    out = []
    for r in range(len(ln) // 4):
        four = ln[4 * r:4 * r + 4]
        f = four[0][0][1:].split()
        out.append((sum(n for _, n in four), len(four[1][0]) == len(four[3][0]), f[0].decode("latin-1") if f else ""))
    return out


@pytest.fixture(scope="module")
def texts():
    """{profile: [{stream: records}]}: every text walked once for all tests of the module"""
    return {name: [{k: _records(c[k]) for k in G.STREAMS} for c in G.profile(name, SEED).chunks] for name in G.NAMES}


def _kept(recs):
    return sum(1 for r in recs if r[1])


@pytest.mark.parametrize("name", G.NAMES)
def test_pairs_per_chunk_are_the_shortest_streams_kept_records(name, texts):
    p = G.profile(name, SEED)
    want = [min(_kept(c[k]) for k in G.STREAMS) for c in texts[name]]
    assert p.facts["pairs_per_chunk"] == want and p.facts["pairs"] == sum(want)
    assert [{k: _kept(c[k]) for k in G.STREAMS} for c in texts[name]] == p.facts["kept"]
    assert [{k: len(c[k]) for k in G.STREAMS} for c in texts[name]] == p.facts["records"]
    assert sum(want) <= 3000  # what the oracle is asked to process
    assert len(p.samples) == G.N_SAMPLES
    assert G.profile(name, SEED).chunks == G.profile.__wrapped__(name, SEED).chunks  # the same texts for the same seed


def test_ragged_lengths_line_ends_and_tile_edges(texts):
    p = G.profile("ragged", SEED)
    assert p.batch_pairs == 97 and p.n_chunks == 1 and p.facts["pairs"] == 2500
    c = p.chunks[0]
    reads = {k: [ln[0] for ln in _lines(c[k])[1::4]] for k in G.STREAMS}
    heads = {k: [ln[0] for ln in _lines(c[k])[0::4]] for k in G.STREAMS}
    for k in ("seq_R1", "seq_R2"):
        L = [len(r) for r in reads[k]]
        usual = [v for v in L if v <= 300]
        assert min(usual) == 0 and max(usual) == 300 and len(set(usual)) > 250
        # every 400th: records 0, 400 .. 2 400 of seq_R1, records 200, 600 .. 2 200 of seq_R2
        assert sorted(v for v in L if v > 300) == sorted([16383, 16384, 16385] * 2 + ([16383] if k == "seq_R1" else []))
    for k in ("index_R1", "index_R2"):
        L = [len(r) for r in reads[k]]
        assert min(L) == 0 and max(L) == 30 and len(set(L)) == 31
    names = [len(h[1:].split()[0]) for h in heads["seq_R1"]]
    assert min(names) == 1 and max(names) == 200
    assert c["seq_R2"].count(b"\r\n") == c["seq_R2"].count(b"\n") == 4 * 2500
    assert all(b"\r" not in c[k] for k in ("seq_R1", "index_R1", "index_R2"))
    plus = [ln[0] for ln in _lines(c["index_R2"])[2::4]]
    assert all(len(x) > 1 and x[1:] == h[1:].split()[0] for x, h in zip(plus, heads["index_R2"]))
    assert not c["seq_R1"].endswith(b"\n") and c["seq_R2"].endswith(b"\n")
    assert all(r[1] for k in G.STREAMS for r in texts["ragged"][0][k])  # nothing dropped: ragged, not malformed


def test_regimes_change_the_bytes_per_record_twentyfold_both_ways(texts):
    p = G.profile("regimes", SEED)
    B = p.batch_pairs
    assert B == 97 and p.facts["pairs"] == 3000
    ratio = {}
    for k in ("seq_R1", "seq_R2"):
        size = [r[0] for r in texts["regimes"][0][k]]
        front = sum(size[:1500]) / 1500.0
        ratio[k] = sum(size[1500:1500 + B]) / (B * front)
        assert ratio[k] == pytest.approx(p.facts["regime_ratio"][k], rel=1e-12)
    assert ratio["seq_R1"] >= 20 and ratio["seq_R2"] <= 1 / 20.0


def test_chunk_regimes_outgrows_the_line_table_the_chunk_before_left(texts):
    p = G.profile("chunk_regimes", SEED)
    B = p.batch_pairs
    assert B == 500 and p.facts["pairs_per_chunk"] == [600, 700, 600]
    text = p.chunks[1]["seq_R1"]
    assert text == G.MINIMAL_RECORD * 24000
    lines = len(_lines(text))
    assert lines == 96000 == p.facts["lines"]
    # scan_window sizes the table as guess x 1.25 + 65 536 lines with guess = window bytes / bytes per record x 4.4, and regrows it only
    # when guess + 4 096 exceeds it: chunk 0's windows hold about B records, and chunk 1 brings no reason to regrow
    assert p.facts["line_cap_left"] == 5.5 * B + 65536 + 4096 and lines > p.facts["line_cap_left"]
    # ... and chunk 0 taught records of 4 KB where these have 6 bytes
    assert sum(r[0] for r in texts["chunk_regimes"][0]["seq_R1"]) / 600.0 > 4000
    used = sum(r[0] for r in texts["chunk_regimes"][1]["seq_R1"][:700])
    assert (used, len(text) - used) == (p.facts["bytes_used"], p.facts["bytes_left"])
    assert len(text) - used >= 10 * used


def test_ends_put_every_streams_end_around_a_batch_boundary(texts):
    p = G.profile("ends", SEED)
    B = p.batch_pairs
    assert B == 97 and p.n_chunks == 11
    short = {}
    for c in range(8):
        kept = {k: _kept(texts["ends"][c][k]) for k in G.STREAMS}
        k = G.STREAMS[c % 4]
        assert kept[k] in (3 * B - 1, 3 * B, 3 * B + 1) and all(v == 400 for s, v in kept.items() if s != k)
        short.setdefault(k, []).append(kept[k])
    assert sorted(short) == sorted(G.STREAMS) and {v for vs in short.values() for v in vs} == {3 * B - 1, 3 * B, 3 * B + 1}
    assert len(_lines(p.chunks[8]["index_R1"])) % 4 == 3
    assert len(_lines(p.chunks[9]["seq_R2"])) == 1
    assert p.facts["pairs_per_chunk"] == [290, 291, 292, 290, 291, 292, 290, 291, 200, 0, 300]


def test_dropped_runs_shift_the_streams_by_six_batches(texts):
    p = G.profile("dropped_runs", SEED)
    B = p.batch_pairs
    recs = texts["dropped_runs"][0]
    bad = {k: [i for i, r in enumerate(recs[k]) if not r[1]] for k in G.STREAMS}
    assert bad["index_R1"] == list(range(1000, 1600)) and bad["seq_R2"] == list(range(1800, 2800, 2))
    assert bad["seq_R1"] == bad["index_R2"] == [] and all(len(recs[k]) == 3000 for k in G.STREAMS)
    assert len(bad["index_R1"]) > 6 * B
    # a dropped record shifts its stream, it takes no pair away: the chunk ends with index_R1's 2 400 kept records, and by then
    # seq_R2 has dropped 300 of its 500
    assert p.facts["pairs"] == 3000 - 600
    kept = {k: np.cumsum([r[1] for r in recs[k]]) for k in G.STREAMS}
    shift = max(int(np.abs(kept[a] - kept[b]).max()) for a in G.STREAMS for b in G.STREAMS)
    assert shift == 600 == p.facts["max_shift"]


def test_sparse_uploads_hold_fewer_kept_records_than_a_batch(texts):
    """What the issue's six profiles cannot hold at a few thousand pairs: a stream of more than one upload whose uploads bring fewer
    kept records than batch_pairs.  A window then takes batches short of B while its stream has more, and the run needs more batches
    than ceil(pairs / B)."""
    p = G.profile("sparse", SEED)
    B = p.batch_pairs
    assert B == 97 and p.n_chunks == 1 and p.facts["pairs"] == 840
    text, recs = p.chunks[0]["seq_R2"], texts["sparse"][0]["seq_R2"]
    starts = np.concatenate([[0], np.cumsum([r[0] for r in recs])])[:-1]
    kept_at = starts[np.array([r[1] for r in recs])]
    per = [int(((kept_at >= k * G.UPLOAD_TEXT) & (kept_at < (k + 1) * G.UPLOAD_TEXT)).sum()) for k in range(len(text) // G.UPLOAD_TEXT)]
    assert per == p.facts["kept_per_upload"] and len(per) >= 5
    # the first three reads of 8 MiB bring most of a batch each, not all of it: the loop takes what is there (0.8 x B is enough) ...
    assert all(0.8 * B <= v < B for v in per[:3])
    # ... the fourth too little for that: the window is topped up again before its batch
    assert 0 < per[3] < 0.8 * B
    # three batches of at most 83 pairs: the pairs do not fit into ceil(pairs / B) batches any more
    n = -(-p.facts["pairs"] // B)
    assert sum(per[:3]) + (n - 3) * B < p.facts["pairs"]
    # the other streams are ordinary and hold every pair in one upload
    assert all(len(p.chunks[0][k]) < G.UPLOAD_TEXT for k in G.STREAMS if k != "seq_R2")
    assert _kept(recs) == 840 and len(recs) - 840 == 250 * 25 + 90 * 50


# ---- the files ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    """files(name, fmt): the profile's files in that format, written once per module"""
    made = {}

    def files(name, fmt):
        if (name, fmt) not in made:
            made[name, fmt] = G.write(G.profile(name, SEED), tmp_path_factory.mktemp("%s_%s" % (name, fmt)), fmt)
        return made[name, fmt]
    return files


@pytest.mark.parametrize("fmt", G.FORMATS)
@pytest.mark.parametrize("name", G.NAMES)
def test_every_format_reads_back(name, fmt, on_disk):
    p = G.profile(name, SEED)
    files = on_disk(name, fmt)
    for k in G.STREAMS:
        assert len(files[k]) == p.n_chunks
        for c, path in enumerate(files[k]):
            assert G.read_text(path) == p.chunks[c][k], (k, c)
            with open(path, "rb") as fh:
                head = fh.read(16)
            if fmt == "plain":
                assert not path.endswith(".gz") and head == p.chunks[c][k][:16]
            else:  # BGZF says so in an extra field of every member; gzip.open writes none
                assert path.endswith(".gz") and head[:3] == b"\x1f\x8b\x08" and (head[3] & 4 != 0) == (fmt == "bgzf")


def test_giant_record_spans_four_bgzf_blocks(on_disk, texts):
    p = G.profile("giant", SEED)
    assert p.batch_pairs == 500 and p.facts["pairs"] == 1200
    for k, (at, bases) in G.GIANTS.items():
        recs = texts["giant"][0][k]
        first = sum(r[0] for r in recs[:at])
        assert recs[at][0] > 2 * bases and all(r[0] < 400 for i, r in enumerate(recs) if i != at)
        assert recs[at][0] < (1 << 20)  # one output member holds it: larger records are out of scope
        blocks = G.bgzf_blocks(on_disk("giant", "bgzf")[k][0])
        assert sum(n for _, n in blocks) == len(p.chunks[0][k])
        spanned = sum(1 for b0, n in blocks if n and b0 < first + recs[at][0] and b0 + n > first)
        assert spanned >= (4 if k == "seq_R2" else 2), (k, spanned)
    assert G.GIANTS["seq_R1"][1] > (64 << 10) and G.GIANTS["seq_R2"][1] > 3 * (64 << 10)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_oracle_counts_the_facts_pairs_chunk_by_chunk(name, on_disk, tmp_path):
    """The whole run gives the profile's pairs with pass, fail and Undetermined among them; a run of each chunk alone gives the
    chunk's (the oracle's report does not tell chunks apart)."""
    p = G.profile(name, SEED)
    files = on_disk(name, "plain")
    conf = str(tmp_path / "conf.txt")
    _conf(conf, files, True, G.POSITIONS, G.MIN_QUAL, p.samples, (False, False, False))
    sset, codes = qo.run_quade(conf, outdir=str(tmp_path))
    total, n_pass, n_fail, n_und = sset.counts()[:4]
    assert total == len(codes) == p.facts["pairs"]
    assert n_pass > 0 and n_fail > 0 and n_und > 0
    with open(str(tmp_path / "Quade_report.csv")) as fh:
        rows = {}
        for ln in fh.read().split("\n")[2:]:  # (the run's own rows come first, the samples' rows of the same names behind them)
            if "\t" in ln:
                rows.setdefault(*ln.split("\t"))
    assert [int(rows[k]) for k in ("Pair pass quality", "Pair fail quality", "Pair Undetermined")] == [n_pass, n_fail, n_und]
    if p.n_chunks > 1:
        at = 0
        for c in range(p.n_chunks):
            _conf(conf, {k: [files[k][c]] for k in G.STREAMS}, True, G.POSITIONS, G.MIN_QUAL, p.samples, (False, False, False))
            sub, sub_codes = qo.run_quade(conf, outdir=str(tmp_path))
            assert sub.counts()[0] == p.facts["pairs_per_chunk"][c], c
            assert sub_codes == codes[at:at + len(sub_codes)], c
            at += len(sub_codes)
        assert at == len(codes)


# ---- the library's host reader ----------------------------------------------------------------------------------------------------
def _names_of(stream):
    names, sizes = [], []
    while True:
        b = stream.take()
        text = bytes(b.text[:b.off[b.n]]) if b.n else b""
        for r in range(b.n):
            f = text[b.off[r] + 1:text.index(b"\n", b.off[r])].split()
            names.append(f[0].decode("latin-1") if f else "")
        sizes.append(b.n)
        b.release()
        if b.n < stream.batch_records:
            break
    stream.close()
    return names, sizes


def _batch_sizes(name, c, k):
    """1, 97 and 5 000 records per batch; one record per batch costs a call each, so not for the 24 000 records of chunk_regimes'
    chunk 1, and `giant` keeps it for the two streams that hold the long reads"""
    if (name, c, k) == ("chunk_regimes", 1, "seq_R1") or (name == "giant" and k.startswith("index")):
        return (97, 5000)
    return (1, 97, 5000)


@pytest.mark.parametrize("fmt", G.FORMATS)
@pytest.mark.parametrize("name", G.NAMES)
def test_host_reader_batches_equal_the_oracle_reader(name, fmt, on_disk, texts):
    from quade_amd.fastq_reader import FastqStream
    p = G.profile(name, SEED)
    files = on_disk(name, fmt)
    for c in range(p.n_chunks):
        for k in G.STREAMS:
            expect = [r.name for r in qo.FastqReader(files[k][c])]
            assert expect == [r[2] for r in texts[name][c][k] if r[1]]
            assert len(expect) == p.facts["kept"][c][k]
            for B in _batch_sizes(name, c, k):
                names, sizes = _names_of(FastqStream(files[k][c], B, queue_depth=2))
                assert names == expect, (k, c, B)
                assert all(n == B for n in sizes[:-1]) and 0 <= sizes[-1] <= B, (k, c, B)
                assert len(sizes) == len(expect) // B + 1, (k, c, B)
