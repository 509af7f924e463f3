"""The device inflaters on the forged DEFLATE corpus (tests/deflate_forge.py; proven against zlib by tests/test_host_forge.py): streams
that are DEFLATE but that zlib and libdeflate never write -- distances up to 32 768, 258 as 284 + 31, 15-bit codes with 13 extra bits,
degenerate and run-length coded tables, dozens of tiny blocks of every type, every framing field -- and one stream per refusal.
BGZF blocks through all three forms of hb.Inflater (quade_inflate.hip, quade_inflate3.hip), gzip members through hb.dev_gunzip, and
one small pipeline run.  Every comparison is byte equality with the text zlib gives, or an error code."""
import re
import zlib

import numpy as np
import pytest

from tests import deflate_forge as F

pytestmark = pytest.mark.gpu

ST_LENGTH, ST_CRC, ST_TABLE_SPACE = 8, 9, 10  # quade_amd/csrc/quade_inflate.h


@pytest.fixture(autouse=True, params=["1", "2", "3"])
def inflater_form(request, monkeypatch):
    """every test with each kernel of the BGZF inflater (tests/test_gpu_inflate.py); the gzip path has one form and ignores it"""
    monkeypatch.setenv("QUADE_INFLATE_FORM", request.param)
    return request.param


def _healthy(k):
    text = b"".join(b"@SIM:1:FC:%d:%d 1:N:0:\nACGTTGCAACGTNACGT\n+\nIIIIFFFF####IIIIF\n" % (k, i) for i in range(40))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return F.bgzf_block(c.compress(text) + c.flush(), text), text


def _fits_bgzf(c):
    return not c[3].get("gzip_only") and len(c[1]) <= 65536 - 26 - 16


def _hip_fault(e):
    from quade_amd import hip_backend as hb
    return e.code == hb.QD_ERR_HIP


def test_bgzf_legal_streams_give_zlibs_text_in_every_form(inflater_form):
    from quade_amd import hip_backend as hb
    cases = [c for c in F.corpus() if c[2] is not None and _fits_bgzf(c)]
    assert len(cases) >= 15 and any(c[3].get("long_codes", 0) > 112 for c in cases) and any(c[3].get("isize_64k") for c in cases)
    (h0, t0), (h1, t1) = _healthy(0), _healthy(1)
    wrong = []
    with hb.Inflater(0) as inf:
        for name, raw, text, tags in cases:
            # the case alone, with other extra subfields around 'BC', and third among healthy blocks
            for comp, want in ((F.bgzf_block(raw, text), text), (F.bgzf_block(raw, text, before=F.subfield(b"AA", b"\x01\x02\x03"), after=F.subfield(b"ZZ", b"")), text),
                               (h0 + h1 + F.bgzf_block(raw, text) + h0, t0 + t1 + text + t0)):
                try:
                    if inf.run(comp, len(want)) != want:
                        wrong.append((name, "other bytes"))
                except hb.QuadeHipError as e:
                    assert not _hip_fault(e), (name, str(e))
                    wrong.append((name, str(e)))
        # all of them in one run: under form 3 the blocks no lane configuration holds (L2x: "table space") take the second launch
        # through the older forms, and their states come back to the right places
        comp = b"".join(F.bgzf_block(c[1], c[2]) for c in cases)
        want = b"".join(c[2] for c in cases)
        try:
            if inf.run(comp + comp, 2 * len(want)) != want + want:
                wrong.append(("all in one run", "other bytes"))
        except hb.QuadeHipError as e:
            wrong.append(("all in one run", str(e)))
    assert not wrong, wrong


def test_bgzf_illegal_streams_are_refused_by_the_decoder_not_by_the_trailer(inflater_form):
    """every refusal DEFLATE asks for: QD_ERR_FORMAT naming the block, by a decoder status that is not the CRC's or the length's (no
    text exists whose CRC the trailer could carry: it holds the CRC of nothing, and the ISIZE a decoder that overlooked the defect
    would arrive at) -- and the inflater goes on to decode a healthy run"""
    from quade_amd import hip_backend as hb
    cases = [c for c in F.corpus() if c[2] is None]
    assert len(cases) >= 17
    (h0, t0), (h1, t1) = _healthy(0), _healthy(1)
    wrong = []
    with hb.Inflater(0) as inf:
        for name, raw, _, tags in cases:
            bad = F.bgzf_block(raw, b"", isize=tags["isize"])
            try:
                inf.run(h0 + h1 + bad + h0, 2 * len(t0) + len(t1) + tags["isize"])
                wrong.append((name, "decoded"))
            except hb.QuadeHipError as e:
                assert not _hip_fault(e), (name, str(e))
                m = re.search(r"decoder status (\d+)", str(e))
                if e.code != hb.QD_ERR_FORMAT or e.bad_block != 2 or not m or int(m.group(1)) in (0, ST_LENGTH, ST_CRC, ST_TABLE_SPACE):
                    wrong.append((name, e.code, e.bad_block, str(e)))
            assert inf.run(h1 + h0, len(t1) + len(t0)) == t1 + t0, name
    assert not wrong, wrong


GEOMETRIES = {"small": (1 << 20, 8 << 10, 64 << 10), "defaults": (64 << 20, 0, 0)}


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_gzip_members_through_the_device(geometry, inflater_form):
    """hb.dev_gunzip at (step 1 MiB, stretch 8 KiB, unit 64 KiB) and at the defaults (the gzip path has one form: the fixture's
    setting does not reach it).  Only a block with more long codes than any lane
    configuration holds (tag long_codes > 112) may be refused -- by an error, never by other bytes; the pipeline's host takes it then."""
    from quade_amd import hip_backend as hb
    step, stretch, unit = GEOMETRIES[geometry]
    wrong = []
    for name, raw, text, tags in F.corpus():
        if text is None:
            try:
                hb.dev_gunzip(F.gzip_member(raw, b"", isize=tags["isize"]), 1 << 20, step_bytes=step, stretch_bytes=stretch, unit_text=unit)
                wrong.append((name, "decoded"))
            except hb.QuadeHipError as e:
                if e.code != hb.QD_ERR_FORMAT:
                    wrong.append((name, e.code))
            continue
        framings = [(F.gzip_member(raw, text), text, 1)]
        if len(text) < 100_000:  # every header field at once, and two such members back to back
            m = F.gzip_member(raw, text, extra=F.subfield(b"XY", b"abc"), name=b"reads.fastq", comment=b"forged", hcrc=True)
            framings += [(m, text, 1), (m + m, text + text, 2)]
        for gz, want, members in framings:
            try:
                got, st = hb.dev_gunzip(gz, len(want) + 16, step_bytes=step, stretch_bytes=stretch, unit_text=unit)
                if got != want or st["members"] != members:
                    wrong.append((name, members, "other bytes" if got != want else st))
            except hb.QuadeHipError as e:
                assert e.code != hb.QD_ERR_HIP, name
                if not (tags.get("long_codes", 0) > 112 and e.code == hb.QD_ERR_FORMAT):
                    wrong.append((name, members, e.code))
    assert not wrong, wrong


def _pipeline_run(base, files, samples):
    from tests.run_support import _run_and_compare
    base.mkdir()
    return _run_and_compare(base, files, samples, "[gpu]\nbatch_pairs : 700\n")  # outputs byte-equal to oracle.run_quade, or it raises


def test_pipeline_with_a_forged_gzip_member_falls_back_and_with_forged_bgzf_does_not(tmp_path):
    """~2 000 pairs.  One of four gzip inputs re-framed as a member that begins with a block no lane configuration decodes (L2x code,
    long_codes = 256) and goes on with flush blocks and matches 32 768 back: the device refuses it, the host inflates it, the outputs
    are the oracle's -- and the control run with zlib's framing never falls back.  One of four BGZF inputs rebuilt from forged blocks
    (empty stored and fixed blocks, far matches): the device takes every block."""
    import gzip
    from tests.run_support import _dataset
    rng = np.random.default_rng(23)
    for fmt in ("gz", "bgzf"):
        data = tmp_path / ("data_" + fmt)
        data.mkdir()
        files, samples = _dataset(str(data), rng, 1, 2000, 5, fmt=fmt)
        if fmt == "gz":
            st = _pipeline_run(tmp_path / "control", files, samples)
            assert st["gzip_fallbacks"] == 0 and st["gzip_members"] == 4, st
        path = files["seq_R1"][0]
        text = gzip.open(path).read()
        assert len(text) > 200_000
        with open(path, "wb") as fh:
            fh.write(F.gzip_member(F.forge_stream(text), text, name=b"forged.fastq") if fmt == "gz" else F.forge_bgzf_file(text))
        assert gzip.open(path).read() == text
        st = _pipeline_run(tmp_path / ("forged_" + fmt), files, samples)
        assert st["pairs"] == 2000, st
        if fmt == "gz":
            assert st["gzip_fallbacks"] >= 1, st
        else:
            assert st["host_inflated_runs"] == 0 and st["bgzf_blocks"] > 0 and st["text_segments"] == 0, st
