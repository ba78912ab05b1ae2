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


HOST_ONLY = ["capi_error.cpp", "adaptive_host.cpp", "denoise_host.cpp", "capi_host.cpp"]
STATE_RULES = {"size_below_first", "negative_passes", "last_check", "active_is_2", "active_wrong_count", "inactive_off_grid",
               "inactive_past_last_check", "state_active", "summary_passes", "summary_samples", "params", "dims", "summary_counts"}


def test_adaptive_state_under_asan_ubsan(tmp_path):
    """The parser of a caller-supplied adaptive state (csrc/adaptive_host.cpp adaptive_state_valid) through chunky_adaptive_state_check,
    chunky_adaptive_host_begin and _resume, in a stand-alone program (tests/sanitize/adaptive_state_fuzz.cpp): images of 1 x 1, 3 x 2,
    17 x 5 and 16 x 16, 3 x 3 x 3 (min_spp, check_interval, max_spp), headers of the first version's size, of sizeof and of sizeof + 24
    in heap blocks of exactly that size.  Every state a run leaves is accepted, every rule of the check broken in turn is refused with
    that rule's message and nothing written, and the caller's size and the bytes beyond sizeof survive.  The build step also holds the
    device-free files to their promise: each compiles as plain C++ with warnings as errors and no ROCm include path."""
    for src in HOST_ONLY:
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
               os.path.join(native.CSRC, src)]
        assert not any("rocm" in a.lower() for a in cmd)
        proc = subprocess.run(cmd, capture_output=True, text=True)
        assert proc.returncode == 0, (src, proc.stderr[-3000:])
    exe = str(tmp_path / "adaptive_state_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "adaptive_state_fuzz.cpp"), os.path.join(native.CSRC, "adaptive_host.cpp"),
           os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0 and out["images"] == 4
    assert set(out["sizes"]) == {out["first_version"], out["sizeof"], out["sizeof"] + 24}
    starts = 4 * (3 * 3 * 3) * 3  # images x (min_spp, check_interval, max_spp) x sizes: each runs once uncut (d = 0) ...
    runs = 4 * (3 * 3) * (4 + 9 + 13) * 3  # ... and once per cut d = 1 .. max_spp - 1, max_spp = 4, 9, 13
    assert out["runs"] == runs and out["cuts"] == runs - starts and out["states_accepted"] == 2 * runs  # (two states per run: at the start or the cut, and at the end)
    assert 0 < out["active_at_end"]  # (and some pixels left: inactive_* below were reached)
    assert set(out["refused"]) == STATE_RULES and all(n > 0 for n in out["refused"].values()), out["refused"]
    # the rules that need nothing of the state were broken on every accepted state
    for rule, per_state in (("size_below_first", 3), ("negative_passes", 1), ("active_is_2", 2), ("state_active", 2), ("summary_passes", 2),
                            ("summary_samples", 2), ("params", 14), ("dims", 3), ("summary_counts", 4)):
        assert out["refused"][rule] == per_state * out["states_accepted"], rule
