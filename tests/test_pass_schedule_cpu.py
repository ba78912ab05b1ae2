"""How the passes of a call become launches is decided by csrc/pass_schedule.hpp, plain C++ with no device call: the most passes a launch
carries (launch_pass_cap), the cut of seeds[0 .. n) into launches (for_each_launch) and the staging rule with its halving when memory is
short (stage_passes).  These tests build tests/sanitize/pass_schedule_fuzz.cpp under AddressSanitizer + UBSan — a program of its own;
nothing is loaded into Python — and

  * compare launch_pass_cap over images x shards x budgets x most with tests/golden/pass_caps.npz, which was recorded from the function
    as it stood in capi_render.hip before it moved (the program also holds every cap to cap x slots x 12 <= budget and cap x slots < 2^31);
  * check that the cut tiles [0, n) in order with launches of at most cap passes (the program checks first_spp, the seeds in P.seed and
    the seeds handed through, launch by launch);
  * run the staging rule with an allocator that refuses above a limit and compare with the same rule written out here: the halving,
    which no device test can reach (an MI355X does not run out of memory under a test), growth only, and the reserve.
No GPU, nothing but g++."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pass_caps.npz")
PASS = 16 * 16 * 3 * 4  # staged bytes of one pass of a 16 x 16 image: one tile of 256 slots
ANY = 2 ** 64 - 1


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pass_schedule") / "pass_schedule_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "sanitize", "pass_schedule_fuzz.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]

    def run(mode):
        proc = subprocess.run([exe, mode], capture_output=True)
        assert proc.returncode == 0, proc.stderr.decode()[-3000:]  # (also: a check of the program's own, or a sanitizer report)
        return proc.stdout
    return run


def test_launch_pass_cap_is_the_recording(fuzz):
    g = np.load(GOLDEN)
    want = g["rows"]
    assert list(g["fields"]) == ["width", "height", "rank", "world", "tile", "n_local", "budget", "most", "cap"]
    got = np.frombuffer(fuzz("caps"), dtype="<i8").reshape(-1, 9)
    # 7 images x (the whole image + 4 shards at 2 ranks) x 5 budgets x 2 limits
    assert got.shape == want.shape == (7 * 9 * 5 * 2, 9)
    assert {tuple(r) for r in got[:, :2]} == {(1, 1), (15, 17), (16, 16), (17, 16), (1920, 1080), (8192, 8192), (32768, 32768)}
    assert set(got[:, 6]) == {0, 11, 12, 2 ** 20, 8 * 2 ** 30} and set(got[:, 7]) == {256, 1024}
    assert (got[(got[:, 0] == 1) & (got[:, 2] > 0)][:, 5] == 0).all()  # the last rank of a 1 x 1 image owns no tile
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, got[bad[0]].tolist(), want[bad[0]].tolist())


def test_the_cut_tiles_the_passes_in_order(fuzz):
    rows = {}
    for line in fuzz("cut").decode().splitlines():
        head, launches = line.split(":")
        n, cap = map(int, head.split())
        rows[(n, cap)] = list(map(int, launches.split()))
    assert set(rows) == {(n, cap) for n in (0, 1, 255, 256, 257, 300, 1024, 1025) for cap in (1, 2, 255, 256, 1024)}
    for (n, cap), launches in rows.items():
        assert sum(launches) == n and all(1 <= k <= cap for k in launches), (n, cap)
        assert launches == [cap] * (n // cap) + ([n % cap] if n % cap else []), (n, cap)  # every launch but the last is full
    assert rows[(257, 256)] == [256, 1]  # tests/test_list_route_cpu.py SPLIT_PASSES
    assert rows[(300, 256)] == [256, 44] and rows[(1025, 1024)] == [1024, 1] and rows[(0, 256)] == []


def rule(held, launch, cap, reserve, free, limit):
    """the staging rule as DESIGN.md section 5 states it: (bytes held, passes per launch, the sizes asked for)"""
    asked = []

    def try_alloc(b):
        asked.append(b)
        return b <= limit
    if held >= launch * PASS:
        return held, launch, asked
    ahead = min(reserve, cap, 256)
    if ahead > launch and ahead * PASS <= free // 2 and try_alloc(ahead * PASS):
        return ahead * PASS, launch, asked
    while not try_alloc(launch * PASS):
        if launch <= 1:
            return 0, 0, asked
        launch = (launch + 1) // 2
    return launch * PASS, launch, asked


# name: (held, launch, cap, reserve, free bytes, limit) as tests/sanitize/pass_schedule_fuzz.cpp stage() lists them
STAGE = {
    "halve_1": (0, 256, 256, 0, ANY, PASS), "halve_2": (0, 256, 256, 0, ANY, 2 * PASS), "halve_3": (0, 256, 256, 0, ANY, 3 * PASS),
    "halve_255": (0, 256, 256, 0, ANY, 255 * PASS), "halve_none": (0, 256, 256, 0, ANY, PASS - 1), "fits": (0, 256, 256, 0, ANY, 256 * PASS),
    "odd_300_of_1024": (0, 300, 1024, 0, ANY, 74 * PASS),
    "held_enough": (256 * PASS, 256, 256, 0, ANY, 0), "held_more": (300 * PASS, 8, 256, 64, ANY, 0), "held_short": (7 * PASS, 8, 256, 0, ANY, ANY),
    "nothing_to_stage": (0, 0, 256, 64, ANY, 0),
    "reserve": (0, 8, 256, 64, ANY, ANY), "reserve_half_free": (0, 8, 256, 64, 128 * PASS, ANY),
    "reserve_over_half_free": (0, 8, 256, 64, 128 * PASS - 1, ANY), "reserve_below_launch": (0, 64, 256, 8, ANY, ANY),
    "reserve_equals_launch": (0, 64, 256, 64, ANY, ANY), "reserve_clamped_to_cap": (0, 8, 100, 300, ANY, ANY),
    "reserve_clamped_to_256": (0, 8, 1024, 1024, ANY, ANY), "reserve_refused": (0, 8, 256, 64, ANY, 10 * PASS),
    "reserve_refused_then_halved": (0, 8, 256, 64, ANY, 5 * PASS), "reserve_held_short": (4 * PASS, 8, 256, 64, ANY, ANY),
}


def test_the_staging_rule_with_an_allocator_that_refuses(fuzz):
    got = {}
    for line in fuzz("stage").decode().splitlines():
        head, result, asked = line.split(":")
        name, held, limit = head.split()
        got[name] = (int(held), int(limit), *map(int, result.split()), list(map(int, asked.split())))
    assert set(got) == set(STAGE)
    for name, (held, launch, cap, reserve, free, limit) in STAGE.items():
        assert got[name][:2] == (held, limit), name  # the program ran the case this table means
        assert got[name][2:] == rule(held, launch, cap, reserve, free, limit), name
    # the halving, in numbers: 256 passes with room for L passes' worth give the first of 256, 128, 64 ... that fits
    assert [got[f"halve_{l}"][3] for l in (1, 2, 3, 255)] == [1, 2, 2, 128]
    assert got["halve_none"][2:4] == (0, 0) and got["halve_none"][4][-1] == PASS  # one pass was asked for, and refused
    assert got["odd_300_of_1024"][3] == 38  # 300, 150, 75, 38: (n + 1) / 2
    # an array that is large enough is never asked for again, let alone shrunk
    assert got["held_enough"][2:] == (256 * PASS, 256, []) and got["held_more"][2:] == (300 * PASS, 8, []) and got["nothing_to_stage"][4] == []
    # the reserve: only above the launch, at most half the free bytes, clamped to the cap and to 256 passes
    assert got["reserve"][2:] == (64 * PASS, 8, [64 * PASS]) and got["reserve_half_free"][2] == 64 * PASS
    assert got["reserve_over_half_free"][2:] == (8 * PASS, 8, [8 * PASS])
    assert got["reserve_below_launch"][4] == got["reserve_equals_launch"][4] == [64 * PASS]
    assert got["reserve_clamped_to_cap"][2] == 100 * PASS and got["reserve_clamped_to_256"][2] == 256 * PASS
    assert got["reserve_refused"][2:] == (8 * PASS, 8, [64 * PASS, 8 * PASS])
    assert got["reserve_refused_then_halved"][2:] == (4 * PASS, 4, [64 * PASS, 8 * PASS, 4 * PASS])
