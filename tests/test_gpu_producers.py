"""The device inflaters on DEFLATE as the writers of real .fastq.gz files make it (tests/producer_corpus.py; its shapes are proven by
tests/test_host_producers.py): libdeflate at levels 1 / 6 / 9 / 12 -- blocks of 300 KB of text and 130 000 tokens, distances up to
32 768 --, pigz's shape, GNU gzip's own deflate, and three decoys (a dynamic block's header where no block starts).  Gzip members through
hb.dev_gunzip (gz_probe, inflate3_tokens, gz_resolve, gz_windows, gz_fixup) at three geometries, BGZF blocks through all three forms of
hb.Inflater, and one pipeline run per file set.  Every comparison is byte equality with the text zlib gives; no stream here may be
refused (no block has more than 112 long codes: test_host_producers.py)."""
import gzip
import shutil
import zlib

import numpy as np
import pytest

from tests import deflate_forge as F
from tests import producer_corpus as P

pytestmark = pytest.mark.gpu

# (step, stretch, unit): small stretches and units, references and blocks cross all of their boundaries; the defaults; steps shorter
# than one libdeflate block (150 KB of compressed bytes) -- qd_dev_gunzip doubles the step until the block fits
GEOMETRIES = {"small": (1 << 20, 8 << 10, 64 << 10), "defaults": (64 << 20, 0, 0), "short steps": (64 << 10, 0, 0)}


def _skip_unless(needs):
    """libdeflate's cases may be left out only where the product itself found no libdeflate, GNU gzip's only without the program"""
    from quade_amd import hip_backend as hb
    if needs == "libdeflate" and hb.load_library().qd_io_backend() == 0:
        pytest.skip("the library found no libdeflate on this machine")
    if needs == "gzip" and shutil.which("gzip") is None:
        pytest.skip("no gzip program on this machine")
    if needs == "libdeflate":
        assert P.libdeflate() is not None


def _zlib_member(text, level=6):
    return F.gzip_member(P.zlib_raw(text, level), text)


def _gunzip_all(files, geometry):
    """files: [(name, gzip file image, text, members)].  Every file through hb.dev_gunzip; the statistics are printed (DESIGN 4.7's
    table is made from them), the bytes and the member count asserted."""
    from quade_amd import hip_backend as hb
    step, stretch, unit = GEOMETRIES[geometry]
    wrong, stats = [], {}
    for name, gz, want, members in files:
        try:
            got, st = hb.dev_gunzip(gz, len(want) + 16, step_bytes=step, stretch_bytes=stretch, unit_text=unit)
        except hb.QuadeHipError as e:
            assert e.code != hb.QD_ERR_HIP, name
            print("PRODUCER_STATS\t%s\t%s\trefused %d\t%r" % (geometry, name, e.code, e.stats))
            wrong.append((name, "refused", e.code, e.stats))
            continue
        print("PRODUCER_STATS\t%s\t%s\t%d -> %d bytes\t%r" % (geometry, name, len(gz), len(want), st))
        stats[name] = st
        if got != want or st["members"] != members:
            wrong.append((name, "other bytes" if got != want else "members", st))
    assert not wrong, wrong
    return stats


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("producer,needs", [("libdeflate", "libdeflate"), ("pigz", None), ("gzip", "gzip")])
def test_gzip_members_of_every_producer(producer, needs, geometry):
    _skip_unless(needs)
    cases = [c for c in P.corpus() if c[3]["producer"] == producer]
    assert len(cases) == len(P.texts()) * {"libdeflate": 4, "pigz": 1, "gzip": 3}[producer]
    _gunzip_all([(name, F.gzip_member(raw, text), text, 1) for name, raw, text, _ in cases], geometry)


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_gzip_files_of_several_members(geometry):
    """two libdeflate members back to back (the second begins anywhere in a stretch, a unit, a step); a libdeflate member, a zlib one
    and a pigz-shaped one in one file; members of 300, 30 and 0 bytes between long ones"""
    _skip_unless("libdeflate")
    m = {name: F.gzip_member(raw, text, name=b"reads.fastq") for name, raw, text, _ in P.corpus()}
    t = {name: text for name, _, text, _ in P.corpus()}
    z = P.texts()["fastq, 4 qualities, one read length"][:900_000]
    files = []
    for label, names in (("two libdeflate members", ["libdeflate 6, fastq, 4 qualities, one read length", "libdeflate 12, fastq"]),
                         ("libdeflate, short ones, libdeflate", ["libdeflate 9, fastq, 4 qualities, one read length", "libdeflate 12, tiny", "libdeflate 1, empty", "libdeflate 6, short",
                                                                 "libdeflate 6, runs", "libdeflate 6, random bytes", "libdeflate 1, fastq"])):
        files.append((label, b"".join(m[k] for k in names), b"".join(t[k] for k in names), len(names)))
    files.append(("libdeflate, zlib, pigz shape", m["libdeflate 9, fastq"] + _zlib_member(z) + m["pigz shape, fastq"], t["libdeflate 9, fastq"] + z + t["pigz shape, fastq"], 3))
    _gunzip_all(files, geometry)


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("which,needs", [("decoy (a)", "libdeflate"), ("decoy (b)", None), ("decoy (c)", None)])
def test_a_header_where_no_block_starts(which, needs, geometry):
    """The probe finds the planted header (the first that holds in its stretch) and not the start of the 300 KB block behind it; the unit
    in front runs through both with token room for the short span to the decoy.  (c): the header stands INSIDE the 300 000-token
    block the member begins with -- the step's first unit has room for one stretch, and no block boundary to fall back to.  At the
    default geometry the chain must have dropped the decoy's unit (chain_retries): otherwise the probe did not take the bait and the
    decoy is built wrongly."""
    _skip_unless(needs)
    name, raw, text, tags = P.case(which)
    files = [(name, F.gzip_member(raw, text), text, 1)]
    # ... and as the second member: the decoy and the long block anywhere in the step's stretches
    lead = P.texts()["fastq"][2_000_000:2_150_000]
    files.append((name + ", second member", _zlib_member(lead) + F.gzip_member(raw, text), lead + text, 2))
    stats = _gunzip_all(files, geometry)
    if geometry == "defaults":
        assert stats[name]["chain_retries"] >= 1, stats[name]


# ---- BGZF ----------------------------------------------------------------------------------------------------------------------------
def _healthy(k):
    text = b"".join(b"@SIM:1:FC:%d:%d 1:N:0:\nACGTTGCAACGTNACGT\n+\nIIIIFFFF####IIIIF\n" % (k, i) for i in range(40))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return F.bgzf_block(c.compress(text) + c.flush(), text), text


def _bgzf(pieces):
    return b"".join(F.bgzf_block(raw, text) for raw, text in pieces), b"".join(text for _, text in pieces)


class TestBgzf(object):
    @pytest.fixture(autouse=True, params=["1", "2", "3"])
    def inflater_form(self, request, monkeypatch):
        """every test with each kernel of the BGZF inflater (tests/test_gpu_inflate.py)"""
        monkeypatch.setenv("QUADE_INFLATE_FORM", request.param)
        return request.param

    @pytest.mark.parametrize("producer", ["libdeflate", "gzip"])
    def test_bgzf_blocks_of_every_producer(self, producer, inflater_form):
        """every case alone; third among healthy zlib blocks; all pieces of all levels in one run, twice over"""
        from quade_amd import hip_backend as hb
        _skip_unless(producer)
        cases = [c for c in P.bgzf_cases() if c[2]["needs"] == producer]
        assert len(cases) == {"libdeflate": 4 * 4 + 1, "gzip": 3 * 3}[producer] and any(c[2]["producer"] == "decoy" for c in cases) == (producer == "libdeflate")
        (h0, t0), (h1, t1) = _healthy(0), _healthy(1)
        wrong = []
        with hb.Inflater(0) as inf:
            every = []
            for name, pieces, tags in cases:
                comp, want = _bgzf(pieces)
                every.append((comp, want))
                for label, c, w in (("alone", comp, want), ("among healthy blocks", h0 + h1 + comp + h0, t0 + t1 + want + t0)):
                    try:
                        if inf.run(c, len(w)) != w:
                            wrong.append((name, label, "other bytes"))
                    except hb.QuadeHipError as e:
                        assert e.code != hb.QD_ERR_HIP, (name, str(e))
                        wrong.append((name, label, str(e)))
            comp, want = b"".join(c for c, _ in every), b"".join(w for _, w in every)
            try:
                if inf.run(comp + comp, 2 * len(want)) != want + want:
                    wrong.append(("all in one run", "other bytes"))
            except hb.QuadeHipError as e:
                assert e.code != hb.QD_ERR_HIP, str(e)
                wrong.append(("all in one run", str(e)))
        assert not wrong, wrong


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
_DATASET = {}


def _gz_dataset(tmp_path_factory):
    """~2 000 pairs as four gzip inputs, made once: (files, samples, the four texts)"""
    if not _DATASET:
        from tests.run_support import _dataset
        d = tmp_path_factory.mktemp("producer_data")
        files, samples = _dataset(str(d), np.random.default_rng(29), 1, 2000, 5, fmt="gz")
        _DATASET["x"] = (files, samples, {k: gzip.open(v[0]).read() for k, v in files.items()})
    return _DATASET["x"]


@pytest.mark.parametrize("writer,needs", [("libdeflate 6", "libdeflate"), ("pigz shape", None)])
def test_pipeline_on_inputs_of_another_writer(writer, needs, tmp_path, tmp_path_factory):
    """All four inputs written again as single members by libdeflate 6 (the index reads: one block each; the inserts: blocks of 300 KB
    of text), or in pigz's shape: outputs and counters are oracle.run_quade's, and the device took every member -- a fallback on a
    clean, legal file is silent in production and costs 17 x the CPU."""
    from tests.run_support import _run_and_compare
    _skip_unless(needs)
    files, samples, texts = _gz_dataset(tmp_path_factory)
    for k, v in files.items():
        text = texts[k]
        assert len(text) > 80_000
        raw = P.libdeflate_raw(text, 6) if needs else P.pigz_raw(text)
        with open(v[0], "wb") as fh:
            fh.write(F.gzip_member(raw, text, name=b"reads.fastq"))
        assert gzip.open(v[0]).read() == text
    base = tmp_path / "run"
    base.mkdir()
    st = _run_and_compare(base, files, samples, "[gpu]\nbatch_pairs : 700\n")  # outputs byte-equal to oracle.run_quade, or it raises
    print("PRODUCER_STATS\tpipeline\t%s\t%r" % (writer, {k: st[k] for k in sorted(st) if k.startswith("gzip") or k in ("pairs", "text_segments")}))
    assert st["pairs"] == 2000 and st["gzip_members"] == 4 and st["gzip_fallbacks"] == 0 and st["text_segments"] == 0, st
