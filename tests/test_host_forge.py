"""No GPU: the forged DEFLATE corpus (tests/deflate_forge.py) -- streams that are DEFLATE but that zlib and libdeflate never write, and
one stream per refusal a decoder owes -- proven against zlib first (a case that fails there is a bug of the forge, not of the project),
then through the host's inflaters: the parallel gunzip (quade_amd/csrc/quade_pgz.cpp) and the third inflater's lane decoder
(quade_amd/csrc/inflate3_lane.h) in all five configurations.  Every comparison is byte equality with zlib's output, or an error."""
import ctypes as C
import gzip
import os
import subprocess
import time
import zlib

import numpy as np
import pytest

from tests import deflate_forge as F
from tests.run_support import write_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_corpus_is_what_zlib_says_it_is():
    t0 = time.time()
    cases = F.corpus()
    assert F.corpus() is cases  # built once per process
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    for prefix in ["L1", "L2 ", "L2x", "L3", "L4", "L5", "L6"] + ["I%d " % k for k in range(1, 17)]:
        assert any(n.startswith(prefix) for n in names), prefix
    for name, raw, text, tags in cases:
        if text is None:
            with pytest.raises(zlib.error):
                zlib.decompress(raw, -15)
        else:
            assert zlib.decompress(raw, -15) == text, name
    assert sum(1 for c in cases if c[3].get("long_codes", 0) > 112) == 1
    assert sum(len(c[1]) + len(c[2] or b"") for c in cases) < 3 << 20 and time.time() - t0 < 10


def test_the_corpus_states_the_corners_it_claims():
    """what makes a case worth having is in its bytes: checked here by a small independent reader of the header fields"""
    def fields(raw, bit=0):
        v = int.from_bytes(raw[:40], "little") >> bit
        return v & 1, (v >> 1) & 3, ((v >> 3) & 31) + 257, ((v >> 8) & 31) + 1, ((v >> 13) & 15) + 4
    assert fields(F.case("L2 widest")[1])[1:] == (2, 286, 30, 19)
    assert fields(F.case("L2 smallest")[1])[1:] == (2, 257, 1, 5)
    assert fields(F.case("L2x")[1])[1:3] == (2, 286)
    assert fields(F.case("I8")[1])[2] == 287 and fields(F.case("I9")[1])[3] == 31
    assert len(F.case("L6 chains")[2]) == 65536
    # 258 as 284 + 31 costs 5 extra bits a match over symbol 285 in the same nearly flat code: the two L1 streams differ
    assert F.case("L1 far")[1] != F.case("L1 258 as")[1]
    # the framing helpers against Python's gzip module
    raw, text = F.case("L5 block mix, final aligned")[1:3]
    member = F.gzip_member(raw, text, extra=F.subfield(b"XY", b"abc"), name=b"reads.fastq", comment=b"forged", hcrc=True)
    assert member[3] == 2 | 4 | 8 | 16 and gzip.decompress(member + member) == text + text
    blk = F.bgzf_block(raw, text, before=F.subfield(b"AA", b"1"), after=F.subfield(b"ZZ", b""))
    assert gzip.decompress(blk) == text and len(blk) == 1 + int.from_bytes(blk[12 + 5 + 4:12 + 5 + 6], "little")


def test_a_given_text_in_forged_blocks():
    """what the pipeline tests re-frame an input file with: zlib reads the text back, and the far matches are there"""
    text = b"".join(b"@SIM:1:FC:0:%d:%d 1:N:0:\n%s\n+\n%s\n" % (i, 7 * i, b"ACGTTGCA"[i % 5:] * 7, b"IIFF##II"[i % 3:] * 7) for i in range(900))
    for t in (text, text[:700], b""):
        assert zlib.decompress(F.forge_stream(t), -15) == t and gzip.decompress(F.forge_bgzf_file(t)) == t
    far = [t for t in F.far_tokens(text, 0, len(text)) if not isinstance(t, int)]
    assert len(far) > 100 and all(32504 <= d <= 32768 for _, d in far) and any(d > 32506 for _, d in far)


def _gunzip(comp, chunk, cap):
    from quade_amd import hip_backend as hb
    lib = hb.load_library()
    out = np.empty(max(cap, 1), np.uint8)
    n = C.c_int64(0)
    st = np.zeros(5, np.int64)
    src = np.frombuffer(comp, np.uint8)
    rc = lib.qd_gunzip_buffer(hb._ptr(src), len(comp), chunk, hb._ptr(out), cap, C.byref(n), hb._ptr(st))
    return rc, bytes(out[:n.value]), int(st[3])


@pytest.mark.parametrize("chunk", [65536, 0])
def test_host_gunzip_on_the_forged_corpus(chunk):
    """qd_gunzip_buffer with small chunks (speculative starts inside the far-match cases) and the default: legal streams give zlib's
    bytes, alone and as two members with every header field; illegal ones an error"""
    from quade_amd import hip_backend as hb
    for name, raw, text, tags in F.corpus():
        if text is None:
            rc, got, _ = _gunzip(F.gzip_member(raw, b"", isize=tags["isize"]), chunk, 1 << 20)
            assert rc == hb.QD_ERR_FORMAT, (name, rc)
            continue
        rc, got, members = _gunzip(F.gzip_member(raw, text), chunk, len(text) + 16)
        assert rc == 0 and got == text and members == 1, (name, rc)
        if len(text) < 100_000:
            m = F.gzip_member(raw, text, extra=F.subfield(b"XY", b"abc"), name=b"reads.fastq", comment=b"forged", hcrc=True)
            rc, got, members = _gunzip(m + m, chunk, 2 * len(text) + 16)
            assert rc == 0 and got == text + text and members == 2, (name, rc)


def build_lane_test(tmp_path, header_dir=None):
    """header_dir: a directory with another inflate3_lane.h (a mutated copy, to see which cases notice it)"""
    exe = str(tmp_path / "inflate3_lane_test")
    src = os.path.join(ROOT, "tests", "native", "inflate3_lane_test.cpp")
    if header_dir:
        text = open(src).read().replace('#include "../../quade_amd/csrc/inflate3_lane.h"', '#include "%s/inflate3_lane.h"' % header_dir)
        src = str(tmp_path / "lane_test_mutant.cpp")
        open(src, "w").write(text)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, src, "-lz"])
    return exe


def test_lane_decoder_on_the_forged_corpus(tmp_path):
    d = tmp_path / "corpus"
    d.mkdir()
    write_corpus(d)
    exe = build_lane_test(tmp_path)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
    assert r.stdout.count("forged corpus done") == 5
