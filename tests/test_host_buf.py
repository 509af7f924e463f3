"""No GPU: the one owner of device and page-locked memory in the host code (quade_amd/csrc/quade_buf.h) -- its growth rules, what a
failed allocation leaves behind, moves, and that every block goes back exactly once -- over a counting source that backs each
allocation with malloc: tests/native/quade_buf_test.cpp, built with g++ as a stand-alone program that links no HIP, and run plain and
under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")  # for <hip/hip_runtime_api.h>: hipError_t and hipStream_t, nothing is linked


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_the_owner_of_device_and_pinned_memory(tmp_path, flags):
    exe = str(tmp_path / "quade_buf_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include")] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "native", "quade_buf_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-3000:], r.stderr[-3000:])
