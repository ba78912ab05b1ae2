"""The step function of adaptive continuation (csrc/adaptive_spec.h ad_step and the grid helpers) called directly from a stand-alone
program under AddressSanitizer + UBSan (tests/sanitize/adaptive_step_fuzz.cpp): the hand-written cases — on the grid unchecked and
checked, off the grid, below min_spp, one pass left, INT_MAX parameters — and, for 8 x 7 x 40 (min_spp, check_interval, max_spp),
the walk from the empty state against the single run's loop round for round, and every cut of it continued to the end."""
import json
import os
import subprocess

from chunkyclplugin_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ad_step_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "adaptive_step_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "adaptive_step_fuzz.cpp"), "-o", exe]
    assert os.path.exists(os.path.join(native.CSRC, "adaptive_spec.h"))
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0 and out["walks"] == 8 * 7 * 40 and out["splits"] == 8 * 7 * sum(range(40))
