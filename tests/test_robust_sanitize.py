"""The host half of firefly-robust accumulation (csrc/robust_host.cpp over csrc/robust_spec.h) in a stand-alone program under
AddressSanitizer + UBSan (tests/sanitize/robust_fuzz.cpp): images of 1 x 1, 3 x 2, 17 x 5 and 16 x 16, every bucket count, sample
counts around the bucket count, first indices up to INT32_MAX, ordinary and non-finite / huge / denormal values, every mode and gains
up to 3e38, each array in a heap block of exactly its size."""
import json
import os
import subprocess

from chunkyclplugin_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_robust_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "robust_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "robust_fuzz.cpp"), os.path.join(native.CSRC, "robust_host.cpp"),
           os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    runs = 4 * 7 * 6 * 3 * 2  # images x bucket counts x sample counts x first indices x (ordinary, odd)
    assert out["failures"] == 0 and out["folds"] == runs and out["resolves"] == runs * 3 * 7 and out["refused"] == 4 * (2 * 7 + 7)
