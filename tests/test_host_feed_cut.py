"""No GPU: the cut of the feeder's upload buffers into segments of whole BGZF blocks and the look at a file's first buffer
(quade_amd/csrc/feed_cut.h), which the pipeline's feeder and peek_record_bytes share -- tests/native/feed_cut_test.cpp, built with g++ as
a stand-alone program and run plain and under AddressSanitizer + UBSan (the cutter sees every buffer in a heap block of exactly its
length)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_the_cut_of_upload_buffers_into_bgzf_segments(tmp_path, flags):
    exe = str(tmp_path / "feed_cut_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "native", "feed_cut_test.cpp"), "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
