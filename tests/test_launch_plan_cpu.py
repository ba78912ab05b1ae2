"""Which render kernel a launch runs is decided by plan_render (csrc/launch_plan.cpp), plain C++ with no device call.  These tests build
tests/sanitize/launch_plan_sweep.cpp with it under AddressSanitizer + UBSan — a program of its own; nothing is loaded into Python — and

  * compare its plans over a prime stride through every combination of the planner's inputs (a quarter of a million of the
    23 357 030 400 rows) with tests/golden/launch_plans.npz, which was recorded from the selection code as it stood before the planner
    existed (launch_pool, pool_kernel_applies, pool_kernel_bvh, launch_render_stats, launch_fallback, check_extended_opts, compiled with
    the HIP calls stubbed and the kernels returning their template arguments), after that code and the planner had agreed on every row;
  * spell out, case by case, the plan of every instantiation of render_pool and of every reason for leaving it: CASES is the table
    DESIGN.md section 5 describes, in a form that runs;
  * hold every plan to the list of instantiations the kernel files build their lookup from (launch_plan.hpp CHUNKY_POOL_INSTANCES).
No GPU, nothing but g++."""
import os
import subprocess

import numpy as np
import pytest

from chunkyclplugin_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.npz")

# the enumeration of tests/sanitize/launch_plan_sweep.cpp: a row number in mixed radix, the first dimension the fastest
DIMS = [
    ("variant", list(range(1024))),
    ("tree", ["none", "1 level", "2 levels", "3 levels", "4 levels", "5 levels", "3 levels, one not 3 bits", "6 levels"]),
    ("entities", ["none", "records", "no records"]),
    ("stack", [0, 10, 11, 64, 65]),
    ("addr32", [0, 3, 7]),
    ("blocks", ["sorted", "unsorted", "sorted, no block_info"]),
    ("opts", ["default", "nee", "draw depth 65536", "max depth 255", "nee, max depth 255"]),
    ("proj", [0, 1]),
    ("queue", [0, 1]),
    ("passes", [1, 15, 16, 31, 32, 63, 64, 256, 257, 1024, 1025]),
    ("seeds", [0, 1]),
    ("fold", [0, 1]),
    ("n_local", [0, 1, (3 << 17) - 1, 3 << 17, (3 << 18) - 1, 3 << 18]),
    ("shard", ["whole", "runs", "blocks with list", "blocks, no list"]),
]
N_ROWS = int(np.prod([len(v) for _n, v in DIMS], dtype=object))
DEFAULTS = dict(variant=0, tree="3 levels", entities="none", stack=0, addr32=7, blocks="unsorted", opts="default", proj=0, queue=1, passes=16,
                seeds=0, fold=0, n_local=3 << 18, shard="whole")
FIELDS = ["family", "tree", "park", "words", "group", "depth", "bvh", "ext", "stats", "sorted", "proj", "lds", "most", "needs_list", "status",
          "ext_refusal", "why"]
POOL, WAVES, LANES = 0, 1, 2
OK, INVALID, NOT_SUPPORTED = 0, 1, 2
EXT_DEFAULT_KERNEL, EXT_WIDE_TREE, EXT_MAX_DEPTH = 1, 2, 3
(WHY_LANES_FORCED, WHY_WAVES_FORCED, WHY_NO_QUEUE, WHY_DRAW_DEPTH, WHY_MAX_DEPTH, WHY_NO_WIDE_TREE, WHY_ADDR32, WHY_BVH_RECORDS,
 WHY_BVH_REFERENCE) = range(1, 10)


def encode(**inputs):
    """the row number of a combination; what is not named takes DEFAULTS"""
    assert set(inputs) <= set(DEFAULTS), inputs
    values = dict(DEFAULTS, **inputs)
    row, scale = 0, 1
    for name, domain in DIMS:
        row += domain.index(values[name]) * scale
        scale *= len(domain)
    return row


def decode(row):
    out = {}
    for name, domain in DIMS:
        out[name] = domain[row % len(domain)]
        row //= len(domain)
    return out


def pool(tree, park, lds, words=6, depth=0, bvh=0, ext=0, stats=0, sorted=0, proj=0):
    return dict(family=POOL, tree=tree, park=park, words=words, group=1, depth=depth, bvh=bvh, ext=ext, stats=stats, sorted=sorted, proj=proj,
                lds=lds, most=1024, needs_list=0, status=OK, ext_refusal=0, why=0)


def fallback(family, tree, group, why, lds=0, depth=0, bvh=0, needs_list=0, ext_refusal=0):
    return dict(family=family, tree=tree, park=-1, words=0, group=group, depth=depth, bvh=bvh, ext=0, stats=0, sorted=0, proj=0, lds=lds,
                most=256, needs_list=needs_list, status=OK, ext_refusal=ext_refusal, why=why)


def refused(family, status, why=0, most=256, needs_list=0, ext_refusal=0):
    return dict(family=family, tree=0, park=-1, words=0, group=0, depth=0, bvh=0, ext=0, stats=0, sorted=0, proj=0, lds=0, most=most,
                needs_list=needs_list, status=status, ext_refusal=ext_refusal, why=why)


ENT = dict(entities="records", stack=10)     # both entity BVHs, re-laid out, stacks of 10 entries: 32 parked paths still fit five groups per CU
ENT11 = dict(entities="records", stack=11)   # ... of 11 entries: 16 parked paths
# LDS of a workgroup of render_pool: 4 waves x (park x (16 x words + 8) + (64 + park) x depth x 4) bytes
CASES = [
    # -- every row of the instantiation list (launch_plan.hpp): (TREE, K, STATS, BVH, EXT, SORT)
    ("plain, no wide tree", dict(tree="none"), pool(0, 64, 26624)),
    ("plain, 1 level", dict(tree="1 level"), pool(16, 64, 26624)),
    ("plain, 2 levels", dict(tree="2 levels"), pool(17, 64, 26624)),
    ("plain, 3 levels", dict(), pool(18, 64, 26624)),
    ("plain, 4 levels", dict(tree="4 levels"), pool(19, 64, 26624)),
    ("plain, 5 levels", dict(tree="5 levels"), pool(-1, 64, 26624)),
    ("sorted, 1 level", dict(tree="1 level", blocks="sorted"), pool(16, 64, 26624, sorted=1)),
    ("sorted, 2 levels", dict(tree="2 levels", blocks="sorted"), pool(17, 64, 26624, sorted=1)),
    ("sorted, 3 levels", dict(blocks="sorted"), pool(18, 64, 26624, sorted=1)),
    ("sorted, 4 levels", dict(tree="4 levels", blocks="sorted"), pool(19, 64, 26624, sorted=1)),
    ("sorted, a level that is not 3 bits", dict(tree="3 levels, one not 3 bits", blocks="sorted"), pool(-1, 64, 26624, sorted=1)),
    ("statistics, 2 levels", dict(variant=4, tree="2 levels"), pool(17, 64, 26624, stats=1)),
    ("statistics, 3 levels: the generic walk", dict(variant=4), pool(-1, 64, 26624, stats=1)),
    ("statistics, sorted, 2 levels", dict(variant=4, tree="2 levels", blocks="sorted"), pool(17, 64, 26624, stats=1, sorted=1)),
    ("statistics, sorted, 3 levels", dict(variant=4, blocks="sorted"), pool(-1, 64, 26624, stats=1, sorted=1)),
    ("no parked paths, no wide tree", dict(variant=64, tree="none"), pool(0, 0, 0)),
    ("no parked paths: the generic walk", dict(variant=64), pool(-1, 0, 0)),
    ("32 parked paths, no wide tree", dict(variant=128, tree="none"), pool(0, 32, 13312)),
    ("32 parked paths: the generic walk, unsorted", dict(variant=128, blocks="sorted"), pool(-1, 32, 13312)),
    ("extended, 2 levels", dict(opts="nee", tree="2 levels"), pool(17, 32, 19456, words=9, ext=1)),
    ("extended, 3 levels", dict(opts="nee"), pool(18, 32, 19456, words=9, ext=1)),
    ("extended, 4 levels; the pool-size bits overridden", dict(opts="nee", tree="4 levels", variant=64), pool(-1, 32, 19456, words=9, ext=1)),
    ("entities, extended, 2 levels", dict(ENT, opts="nee", tree="2 levels"), pool(17, 16, 22528, words=9, depth=10, bvh=1, ext=1)),
    ("entities, extended, 3 levels", dict(ENT, opts="nee"), pool(18, 16, 22528, words=9, depth=10, bvh=1, ext=1)),
    ("entities, extended, 1 level", dict(ENT, opts="nee", tree="1 level"), pool(-1, 16, 22528, words=9, depth=10, bvh=1, ext=1)),
    ("entities, statistics, 2 levels", dict(ENT, variant=4, tree="2 levels"), pool(17, 16, 21504, words=8, depth=10, bvh=1, stats=1)),
    ("entities, statistics, 3 levels", dict(ENT, variant=4), pool(-1, 16, 21504, words=8, depth=10, bvh=1, stats=1)),
    ("entities, 2 levels", dict(ENT, tree="2 levels"), pool(17, 32, 32768, words=8, depth=10, bvh=1)),
    ("entities, 3 levels, never sorted", dict(ENT, blocks="sorted"), pool(18, 32, 32768, words=8, depth=10, bvh=1)),
    ("entities, 4 levels", dict(ENT, tree="4 levels"), pool(-1, 32, 32768, words=8, depth=10, bvh=1)),
    ("entities, deeper stacks, 2 levels", dict(ENT11, tree="2 levels"), pool(17, 16, 22784, words=8, depth=11, bvh=1)),
    ("entities, deeper stacks, 3 levels", dict(ENT11), pool(18, 16, 22784, words=8, depth=11, bvh=1)),
    ("entities, the reference's 64 entries, 6 levels", dict(entities="records", stack=65, tree="6 levels"), pool(-1, 16, 90624, words=8, depth=64, bvh=1)),
    # -- the other dimensions of a pool plan
    ("a projected camera: the same arguments", dict(proj=1, blocks="sorted"), pool(18, 64, 26624, sorted=1, proj=1)),
    ("sorting forced on", dict(variant=256), pool(18, 64, 26624, sorted=1)),
    ("sorting forced off", dict(variant=512, blocks="sorted"), pool(18, 64, 26624)),
    ("sorting needs the block records", dict(blocks="sorted, no block_info"), pool(18, 64, 26624)),
    ("sorting needs the re-laid-out tree", dict(variant=256, tree="none"), pool(0, 64, 26624)),
    ("the reference walk forced", dict(variant=1), pool(0, 64, 26624)),
    ("1024 passes with their seeds on the device", dict(passes=1024, seeds=1), pool(18, 64, 26624)),
    ("an empty share is planned like any other", dict(n_local=0, shard="runs"), pool(18, 64, 26624)),
    ("a share of blocks: render_pool maps them itself", dict(shard="blocks, no list"), pool(18, 64, 26624)),
    ("257 passes without device seeds", dict(passes=257), refused(POOL, INVALID, most=1024)),
    ("1025 passes", dict(passes=1025, seeds=1), refused(POOL, INVALID, most=1024)),
    # -- every reason for leaving render_pool
    ("variant bit 1: render_lanes", dict(variant=2), fallback(LANES, -1, 0, WHY_LANES_FORCED)),
    ("variant bit 3: render_waves", dict(variant=8), fallback(WAVES, -1, 8, WHY_WAVES_FORCED, lds=18432)),
    ("no queue: render_lanes", dict(queue=0, tree="none"), fallback(LANES, 0, 0, WHY_NO_QUEUE)),
    ("draw depth above 65535", dict(opts="draw depth 65536"), fallback(WAVES, -1, 8, WHY_DRAW_DEPTH, lds=18432)),
    ("draw depth above 65535 with entities: the 8-word record counts the steps", dict(ENT, opts="draw depth 65536"),
     pool(18, 32, 32768, words=8, depth=10, bvh=1)),
    ("max depth 255", dict(opts="max depth 255"), fallback(WAVES, -1, 8, WHY_MAX_DEPTH, lds=18432)),
    ("extended options with max depth 255", dict(opts="nee, max depth 255"),
     fallback(WAVES, -1, 8, WHY_MAX_DEPTH, lds=18432, ext_refusal=EXT_MAX_DEPTH)),
    ("no wide tree with entities", dict(ENT, tree="none"), fallback(WAVES, 0, 8, WHY_NO_WIDE_TREE, lds=10240 + 18432, depth=10, bvh=1)),
    ("no wide tree with the extended options", dict(opts="nee", tree="none"),
     fallback(WAVES, 0, 8, WHY_NO_WIDE_TREE, lds=18432, ext_refusal=EXT_WIDE_TREE)),
    ("no wide tree with statistics", dict(variant=4, tree="none"), fallback(WAVES, 0, 8, WHY_NO_WIDE_TREE, lds=18432)),
    ("arrays beyond the 32-bit offsets", dict(addr32=3), fallback(WAVES, -1, 8, WHY_ADDR32, lds=18432)),
    ("arrays beyond the 32-bit offsets with entities: their kernels read any scene", dict(ENT, addr32=0),
     pool(18, 32, 32768, words=8, depth=10, bvh=1)),
    ("entities without records", dict(entities="no records", stack=64), fallback(WAVES, -1, 8, WHY_BVH_RECORDS, lds=65536 + 18432, depth=64, bvh=1)),
    ("entities without records and the extended options", dict(entities="no records", stack=10, opts="nee"),
     fallback(WAVES, -1, 8, WHY_BVH_RECORDS, lds=10240 + 18432, depth=10, bvh=1, ext_refusal=EXT_DEFAULT_KERNEL)),
    ("entities with the reference walk forced", dict(ENT, variant=1), fallback(WAVES, 0, 8, WHY_BVH_REFERENCE, lds=10240 + 18432, depth=10, bvh=1)),
    ("extended options with statistics: planned, and refused by the C API", dict(opts="nee", variant=4),
     dict(pool(18, 32, 19456, words=9, ext=1), ext_refusal=EXT_DEFAULT_KERNEL)),
    # -- render_waves' lanes per pixel: by the share and the passes, forced by variant bits 4-5, 32 never with entities
    ("few pixels: 32 lanes per pixel", dict(variant=8, n_local=1, passes=64), fallback(WAVES, -1, 32, WHY_WAVES_FORCED, lds=8 * 2112)),
    ("few pixels with entities: 16", dict(ENT, variant=8, n_local=1, passes=64), fallback(WAVES, -1, 16, WHY_WAVES_FORCED, lds=10240 + 16 * 1088, depth=10, bvh=1)),
    ("few pixels, 63 passes: 16", dict(variant=8, n_local=1, passes=63), fallback(WAVES, -1, 16, WHY_WAVES_FORCED, lds=16 * 1088)),
    ("few pixels, 15 passes: one lane", dict(variant=8, n_local=1, passes=15), fallback(WAVES, -1, 1, WHY_WAVES_FORCED)),
    ("3 << 17 pixels: 16", dict(variant=8, n_local=3 << 17, passes=32), fallback(WAVES, -1, 16, WHY_WAVES_FORCED, lds=16 * 1088)),
    ("group 1 forced", dict(variant=8 + 16), fallback(WAVES, -1, 1, WHY_WAVES_FORCED)),
    ("group 16 forced", dict(variant=8 + 48, passes=1), fallback(WAVES, -1, 16, WHY_WAVES_FORCED, lds=16 * 1088)),
    # -- what the fallback kernels refuse
    ("the adaptive fold needs staged samples", dict(variant=8, fold=1), refused(WAVES, NOT_SUPPORTED, WHY_WAVES_FORCED)),
    ("257 passes on the fallback kernels", dict(variant=8, passes=257, seeds=1), refused(WAVES, INVALID, WHY_WAVES_FORCED)),
    ("a share of blocks without the pixel list", dict(variant=2, shard="blocks, no list"), refused(LANES, NOT_SUPPORTED, WHY_LANES_FORCED, needs_list=1)),
    ("a share of blocks from the pixel list: its length sizes the groups", dict(variant=8, shard="blocks with list", n_local=3 << 18, passes=64),
     fallback(WAVES, -1, 16, WHY_WAVES_FORCED, lds=16 * 1088, needs_list=1)),
]


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_sweep")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "sanitize", "launch_plan_sweep.cpp"), os.path.join(native.CSRC, "launch_plan.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]

    def run(*args):
        proc = subprocess.run([exe, *map(str, args)], capture_output=True)
        assert proc.returncode == 0, proc.stderr.decode()[-3000:]  # (also: a plan the program's own checks refuse, or a sanitizer report)
        return proc.stdout
    return run


def plans_of(raw):
    return np.frombuffer(raw, dtype="<i4").reshape(-1, len(FIELDS))


def test_the_enumeration_here_is_the_programs(sweep):
    dims = [line.split() for line in sweep("dims").decode().splitlines()]
    assert [(n, int(r)) for n, r in dims] == [(n, len(v)) for n, v in DIMS]
    assert N_ROWS == 23357030400 and decode(encode(variant=517, tree="6 levels", shard="runs", passes=257))["passes"] == 257


def test_the_stride_gives_the_plans_recorded_before_the_planner_existed(sweep):
    g = np.load(GOLDEN)
    first, stride, names, want = int(g["first"]), int(g["stride"]), list(g["fields"]), g["plans"].T
    assert names == FIELDS[:16] and stride == 93427 and want.shape[0] == (N_ROWS - first + stride - 1) // stride > 250000
    got = plans_of(sweep("stride", first, stride))
    assert got.shape[0] == want.shape[0]
    same = got[:, :16] == want
    bad = np.flatnonzero(~same.all(axis=1))
    if bad.size:
        k = int(bad[0])
        diff = {f: (int(got[k, i]), int(want[k, i])) for i, f in enumerate(FIELDS[:16]) if not same[k, i]}
        pytest.fail(f"{bad.size} rows differ; the first is row {first + k * stride}: {decode(first + k * stride)}: (planned, recorded) {diff}")


def test_named_cases(sweep):
    assert len({name for name, _i, _w in CASES}) == len(CASES)
    got = plans_of(sweep("rows", *[encode(**inputs) for _n, inputs, _w in CASES]))
    wrong = []
    for (name, inputs, want), row in zip(CASES, got):
        have = dict(zip(FIELDS, map(int, row)))
        if have != want:
            wrong.append((name, {f: (have[f], want[f]) for f in FIELDS if have[f] != want[f]}))
    assert not wrong, wrong


def test_every_listed_instantiation_has_a_case_and_every_case_a_listed_instantiation(sweep):
    listed = [tuple(map(int, line.split())) for line in sweep("list").decode().splitlines()]
    assert len(listed) == 22 + 11 and len(set(listed)) == 33
    named = {(w["tree"], w["park"], w["stats"], w["bvh"], w["ext"], w["sorted"]) for _n, _i, w in CASES if w["family"] == POOL and w["status"] == OK}
    assert named == set(listed)
    # ... and every pool plan of the stride names one (the program checks the same, and words and LDS bytes, for every row it prints)
    got = plans_of(sweep("stride", 0, 93427))
    pool_rows = got[(got[:, 0] == POOL) & (got[:, 14] == OK)]
    assert len(pool_rows) > 3000
    assert {tuple(map(int, r)) for r in pool_rows[:, [1, 2, 8, 6, 7, 9]]} <= set(listed)
    reasons = {w["why"] for _n, _i, w in CASES}
    assert reasons == set(range(10))
