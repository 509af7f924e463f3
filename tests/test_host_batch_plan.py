"""No GPU: the host's plan of a batch's output (quade_amd/csrc/out_plan.h: regions -> gzip members -> 64 KiB sub-blocks -> CRC ranges,
which the pipeline and the stand-alone deflater share) and the sizes of a batch's buffers (quade_amd/csrc/batch_sizes.h, which the
pipeline's reservation and its per-batch path share) -- tests/native/batch_plan_test.cpp, built with g++ as a stand-alone program and
run plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_the_output_plan_and_the_buffer_sizes(tmp_path, flags):
    exe = str(tmp_path / "batch_plan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "native", "batch_plan_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
