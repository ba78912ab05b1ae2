"""Host-side code that runs on caller-supplied ints, under AddressSanitizer + UBSan on the CPU (GPU sanitizers do not exist on this
pool): the records every scene upload derives from its palettes, BVHs and octree (csrc/scene_records.cpp), and the octree re-layout (csrc/widetree.cpp) on random well-formed trees — every cell's leaf value and level
equal to the reference descent (K/octree.h:81-89) — and on damaged ones (wild branches, cycles, branches below level 0, pointers that do
not fit), which have to be refused or expressed without a single out-of-bounds access; and the arithmetic of the shard-to-pixel map
(csrc/shard_map.hpp), which takes any tile and any world an int holds, against a brute-force owner table."""
import json
import os
import subprocess

from chunkyclplugin_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_widetree_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "widetree_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "sanitize", "widetree_fuzz.cpp"), os.path.join(native.CSRC, "widetree.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    proc = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["rounds"] == 1500 and out["expressed"] > 1000 and out["refused"] > 100 and out["cells_compared"] > 10 ** 7


def test_capi_host_parsers_under_asan_ubsan(tmp_path):
    """derive_records / build_quad_aux / bvh_links_height / build_bvh_records / bvh_leaves_sound / list_emitters of csrc/scene_records.cpp"""
    exe = str(tmp_path / "scene_records_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "scene_records_fuzz.cpp"), os.path.join(native.CSRC, "scene_records.cpp"),
           os.path.join(native.CSRC, "widetree.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe, "3000"], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [json.loads(x) for x in proc.stdout.strip().splitlines()]
    assert lines[0]["blocks_switched_off"] > 500 and lines[0]["on_records"] > 1000 and lines[0]["on_packed_path"] > 1000
    assert lines[1]["records_built"] > 1000 and lines[1]["refused"] > 100
    assert lines[2]["emitter_rounds"] == 3000


def test_shard_map_under_asan_ubsan(tmp_path):
    """n_local_slots / make_shard_view / member_shard / block_pixel_list / fast_div of csrc/shard_map.hpp against a brute-force owner table:
    every rank of every (width, height, world, tile) of a 40 x 36 grid, the extremes of what chunky_render_set_shard takes (tile and
    world up to INT_MAX, images of 2^30 pixels), group members inside an outer share, and the division by a launch constant."""
    exe = str(tmp_path / "shard_map_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "sanitize", "shard_map_fuzz.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["geometries"] == 40 * 36 * 9 * 19 and out["ranks"] == 40 * 36 * 45 * 19 and out["pixels_enumerated"] == out["geometries"] // 1440 * sum(
        w * h for w in range(1, 41) for h in range(1, 37))  # every pixel of every geometry exactly once
    assert out["extreme_views"] > 1000 and out["refused_views"] > 0 and out["member_shares"] > 1000 and out["member_refusals"] > 100
    assert out["member_sets"] > 1000 and out["quotients"] > 4100 * 70
