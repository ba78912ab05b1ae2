"""The host half of the ID mattes (csrc/matte_host.cpp on csrc/matte_spec.h) in a stand-alone program under AddressSanitizer + UBSan
(tests/sanitize/matte_fuzz.cpp): folds against a fold written with arrays, every one cut in two, ranks and extracts of the states
they leave; 4000 hostile states (INT32_MIN / INT32_MAX counts and ids, holes, duplicates) through the state check and all three
twins; null pointers, sizes of 0 and below, a 131 072-entry set.  The build step also holds matte_host.cpp to its promise: plain C++,
warnings as errors, no ROCm include path.  Nothing is loaded into Python."""
import json
import os
import subprocess

from chunkyclplugin_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matte_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "matte_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "matte_fuzz.cpp"), os.path.join(native.CSRC, "matte_host.cpp"),
           os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    assert not any("rocm" in a.lower() for a in cmd)
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0
    runs = 5 * 5 * 4  # sizes x alphabets x pass counts
    assert out["folds"] >= runs and out["accepted"] >= runs and out["refused"] > 0
    assert out["extracts"] == 2 * (runs - 5 * 5) + 2
