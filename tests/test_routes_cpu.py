"""The exhibits of tests/route_scenes.py on the CPU: the C restatement (and, where it is built, the reference build) against
tests/golden/routes.npz bit for bit; the census that keeps the fixture honest — the REFERENCE's own rays must reach every route often
enough, camera rays and later ones — and the route scene_records.cpp picks for every exhibit, pinned through a stand-alone host
program under AddressSanitizer + UBSan.

profiles/route_census.json holds the census; the test compares what it counts with that file (ROUTE_CENSUS_WRITE=1 rewrites it, and
then also counts the 1920 x 1080 `water` camera rows, which take too long for every run)."""
import json
import os
import subprocess

import numpy as np
import pytest

import golden_scenes as gs
import route_scenes as rs
from chunkyclplugin_amd import native, scenes
from oracle import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = os.path.join(ROOT, "profiles", "route_census.json")
MIN_RECORDS, MIN_LATER = 64, 16   # per route, over every pixel x the 4 seeds: records in all, records that are not record 0
SEEDS = scenes.java_random_ints(rs.N_PASSES)


def check_fixture(tracer, name):
    g = rs.fixture()
    sc = rs.make(name)
    assert gs.input_digest(sc) == str(g[name + "_digest"]), "the regenerated scene is not the one the fixture was made from"
    assert np.array_equal(g["seeds"], SEEDS)
    h = binding.SceneHandle(sc)
    assert rs.first_difference(tracer.render_passes(h, SEEDS), g[name + "_res"], f"{name} radiance") is None
    assert np.array_equal(tracer.preview(h), g[name + "_preview"])
    if name in rs.RECORD_SCENES:
        want, cnt, rad = rs.fixture_records(name)
        got, got_cnt = rs.all_records(tracer, sc, SEEDS[:1], rs.RECORD_GIDS)
        assert rs.records_difference(got[:, 0], got_cnt[:, 0], want, cnt, name) is None
        got_rad = np.array([tracer.trace_records(h, int(SEEDS[0]), int(gid))[1] for gid in rs.RECORD_GIDS])
        assert rs.first_difference(got_rad, rad, f"{name} radiance of the recorded samples") is None


@pytest.mark.parametrize("name", rs.NAMES)
def test_restatement_equals_the_fixture(port, name):
    check_fixture(port, name)


@pytest.mark.parametrize("name", rs.NAMES)
def test_reference_still_gives_the_fixture(ref, name):
    check_fixture(ref, name)


def test_embedded_forms_render_the_same_image():
    """The same world under 1, 5 and 10 more levels of air: the reference's image does not change, so a difference on the GPU
    there is the tree form's."""
    g = rs.fixture()
    for d in rs.EMBED_DEPTHS:
        assert rs.first_difference(g[f"routes_d{d}_res"], g["routes_res"], f"depth {d}") is None


def check_helpers(tracer, which):
    g = rs.fixture()
    rows = rs.helper_rows(which)
    assert gs.rows_digest(rows) == str(g[f"in{which}_sha256"])
    want = g[f"out{which}"]
    got = tracer.helpers(rs.make("routes"), which, rows)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"helper {which}: {int((~same).any(axis=1).sum())} rows differ, first {np.argwhere(~same)[0].tolist()}"
    return rows, want


@pytest.mark.parametrize("which", rs.HELPER_KINDS)
def test_restatement_helpers_equal_the_fixture(port, which):
    rows, want = check_helpers(port, which)
    if which == 12:   # Material_sample: the rows reach the water tint and the emittance texture
        mats = rows[:, 0].view(np.int32)
        _sc, _B, m = rs.base()
        for k in ("water", "water_flat", "emit6a", "emit6b", "emit2"):
            assert (mats == m[k]).sum() >= 16, k
    assert np.isfinite(want[:, 0]).mean() > 0.4


@pytest.mark.parametrize("which", rs.HELPER_KINDS)
def test_reference_helpers_still_give_the_fixture(ref, which):
    check_helpers(ref, which)


# ---- the census ----
def tint3_blocks(sc):
    """Block pointers of `sc` with a tint-3 material behind them (full cubes, AABB and quad models)."""
    B, M = np.asarray(sc.block_palette), np.asarray(sc.material_palette)
    A, Q = np.asarray(sc.aabb_models), np.asarray(sc.quad_models)
    is3 = lambda ptr: ((int(M[ptr + 1]) >> 24) & 0xFF) == 3
    out = []
    for k in range(len(B) // 2):
        kind, ptr = int(B[2 * k]), int(B[2 * k + 1])
        if kind == 1:
            mats = [ptr]
        elif kind == 2:
            mats = [int(A[ptr + 1 + 13 * i + 7 + w]) for i in range(int(A[ptr])) for w in range(1, 6)]
        elif kind == 3:
            mats = [int(Q[ptr + 1 + 15 * i + 13]) for i in range(int(Q[ptr]))]
        else:
            mats = []
        if any(is3(p) for p in mats):
            out.append(2 * k)
    return out


def water_golden_census(port):
    """Records that land on a tint-3 block in the existing `water` goldens: every pixel, the golden seeds."""
    seeds = scenes.java_random_ints(gs.N_PASSES)
    out = {}
    for key, chunks in (("water_golden_depth6", 2), ("water_golden_depth7", gs.DEEP_CHUNKS)):
        sc = gs.make("water", chunks)
        blocks = tint3_blocks(sc)
        assert len(blocks) == 1
        rec, cnt = rs.all_records(port, sc, seeds)
        out[key] = {"traces": int(cnt.sum()), "tint3_records": int(((rec["hit"] == 1) & np.isin(rec["material"], blocks)).sum())}
    return out


def water_rows_census(port):
    """The same on the eight rows of the 1920 x 1080 `water` camera view, all eight timed passes."""
    sc = gs.camera_view("water")
    blocks = tint3_blocks(sc)
    gids = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in gs.camera_rows(sc)])
    rec, cnt = rs.all_records(port, sc, scenes.java_random_ints(gs.TIMED_PASSES), gids)
    return {"water_camera_rows": {"traces": int(cnt.sum()), "tint3_records": int(((rec["hit"] == 1) & np.isin(rec["material"], blocks)).sum())}}


def never_hit_census(port):
    _sc, B, _m = rs.base()
    rec, _cnt = rs.all_records(port, rs.make("routes"), SEEDS)
    return {k: int(((rec["hit"] == 1) & (rec["material"] == B[k])).sum()) for k in rs.NEVER_HIT}


def test_census_every_route_is_reached_by_the_reference_rays(port):
    found = {"thresholds": {"records": MIN_RECORDS, "later": MIN_LATER}, "pixels": rs.W * rs.H, "seeds": rs.N_PASSES,
             "routes": rs.census(port, SEEDS), "never_hit": never_hit_census(port), "tint3_elsewhere": water_golden_census(port)}
    for name, c in found["routes"].items():
        print(name, c)
        assert c["records"] >= MIN_RECORDS and c["later"] >= MIN_LATER, (name, c)
    assert set(found["routes"]) == set(rs.routes())
    assert all(v == 0 for v in found["never_hit"].values()), found["never_hit"]
    if os.environ.get("ROUTE_CENSUS_WRITE"):
        full = json.loads(json.dumps(found))
        full["tint3_elsewhere"].update(water_rows_census(port))
        with open(CENSUS, "w") as f:
            json.dump(full, f, indent=1, sort_keys=True)
            f.write("\n")
    kept = json.load(open(CENSUS))
    rows = kept["tint3_elsewhere"].pop("water_camera_rows")
    assert kept == json.loads(json.dumps(found)), "profiles/route_census.json is not what the census counts (ROUTE_CENSUS_WRITE=1 rewrites it)"
    # what DESIGN.md section 3 says about the older fixtures: no ray of the `water` goldens reaches the water tint, and of the
    # 400 726 traces of the timed `water` rows (counted when the file is written) a handful do
    assert 0 <= rows["tint3_records"] < MIN_RECORDS and rows["traces"] > 100000
    assert all(v["tint3_records"] == 0 and v["traces"] > 10000 for v in kept["tint3_elsewhere"].values())


# ---- which route the derivation picks ----
def write_scene_file(sc, path):
    with open(path, "wb") as f:
        for a in (sc.block_palette, sc.material_palette, sc.aabb_models, sc.quad_models, sc.world_bvh, sc.actor_bvh, sc.bvh_trigs):
            a = np.ascontiguousarray(a, np.int32)
            f.write(np.int64(a.size).tobytes())
            f.write(a.tobytes())
        empty = [int(np.array_equal(b, scenes.empty_bvh())) for b in (sc.world_bvh, sc.actor_bvh)]
        f.write(np.array(empty, np.int32).tobytes())


@pytest.fixture(scope="module")
def route_pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route_pin") / "route_pin")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "route_pin.cpp"), os.path.join(native.CSRC, "scene_records.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]

    def run(sc, tmp_path):
        path = str(tmp_path / (sc.name + ".bin"))
        write_scene_file(sc, path)
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-3000:]
        return json.loads(p.stdout.strip().splitlines()[-1])
    return run


def test_every_exhibit_takes_the_route_it_stands_for(route_pin, tmp_path):
    sc, B, _m = rs.base()
    out = route_pin(sc, tmp_path)
    assert len(out["word7"]) == len(sc.block_palette) // 2 and out["quad_aux"]
    for name, on_records in rs.ON_RECORDS.items():
        k = B[name] // 2
        assert out["type"][k] == int(sc.block_palette[2 * k]) in (2, 3), (name, out["type"][k])   # well-formed: not switched off
        assert (out["word7"][k] != 0) == on_records, (name, out["word7"][k])
        if on_records:
            count = int((sc.aabb_models if out["type"][k] == 2 else sc.quad_models)[int(sc.block_palette[2 * k + 1])])
            assert out["word7"][k] & 0xFF == count, (name, out["word7"][k])
    # two palette blocks on one model share its records
    for a, b in (("shared_box_a", "shared_box_b"), ("shared_quad_a", "shared_quad_b")):
        assert B[a] != B[b] and out["word7"][B[a] // 2] == out["word7"][B[b] // 2] != 0
    assert not out["bvh_records"] or out["tri_records"] == 0   # no entities in the base scene


@pytest.mark.parametrize("name", rs.ENTITY_SCENES)
def test_entity_variants_take_the_route_they_stand_for(route_pin, tmp_path, name):
    out = route_pin(rs.make(name), tmp_path)
    assert out["bvh_records"] == rs.BVH_ON_RECORDS[name], out
    if name == "routes_leaf63":
        assert out["tri_records"] == 65 and out["bvh_inner_records"] == 1
    if name == "routes_tris":
        assert out["tri_records"] == 32
