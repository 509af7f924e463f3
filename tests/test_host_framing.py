"""No GPU: the one reader of gzip and BGZF framing and the one gzip member walk (quade_amd/csrc/gz_framing.h) that qd_dev_gunzip, the
pipeline's feeder and gz_steps, and the host readers share -- tests/native/gz_framing_test.cpp, built with g++ as a stand-alone program
and run plain and under AddressSanitizer + UBSan (every parser sees exactly the bytes it is given, in a heap block of their own)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_gzip_and_bgzf_framing_and_the_member_walk(tmp_path, flags):
    exe = str(tmp_path / "gz_framing_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "native", "gz_framing_test.cpp"), "-lz"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
