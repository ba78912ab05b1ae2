"""The emitter light groups (chunky_render_light_set_emitter_groups, include/chunky_hip.h) without a device: the header declares the
calls and the library exports them, NULL handles are errors, scenes.emitter_ids lists what the fixtures hold, and the specification
in emitter_groups_spec.py has the properties the GPU tests and the documentation lean on — darkening nothing is the identity, bit for
bit; darkening everything leaves no light; the groups light what the issue measured; they sum to EMITTERS within the header's one-pass
bound.  The host validator (csrc/lights_host.cpp) runs every refusal in a stand-alone program under AddressSanitizer + UBSan
(tests/sanitize/light_groups_fuzz.cpp); nothing is loaded into Python under a sanitizer."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import emitter_groups_spec as es
import golden_scenes as gs
import route_scenes as rs
from lights_spec import expected_lights
from chunkyclplugin_amd import native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["chunky_render_light_set_emitter_groups", "chunky_render_light_read_group", "chunky_render_light_mix_groups"]
SEEDS = native.java_random_ints(rs.N_PASSES)
MAX_DEPTH = 5
ROUTES_EMITTERS = [8, 10, 12, 18, 20, 32, 34]   # the block pointers of `routes` with an emissive material


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def emitters(port, sc, seeds=SEEDS):
    return expected_lights(port, sc, seeds, groups=("emitters",))["emitters"]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(native.HEADER).read()
    assert re.search(r"#define\s+CHUNKY_LIGHT_MAX_EMITTER_GROUPS\s+8\b", text)
    assert native.LIGHT_MAX_EMITTER_GROUPS == 8
    declared = native.declared_symbols()
    L = native.lib()
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    for src in ("lights_groups.hip", "lights_host.cpp"):
        assert src in native.SOURCES


def test_null_handles_are_errors():
    L = native.lib()
    ids = np.array([8], np.int32)
    groups = np.zeros(1, np.uint8)
    out = np.zeros(12, np.float32)
    w = np.ones(2, np.float32)
    assert L.chunky_render_light_set_emitter_groups(None, 1, ids.ctypes.data, groups.ctypes.data, 1) == native.E_INVALID
    assert b"NULL" in L.chunky_last_error()
    assert L.chunky_render_light_set_emitter_groups(None, 0, None, None, 0) == native.E_INVALID
    assert L.chunky_render_light_read_group(None, 0, out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_light_mix_groups(None, 1.0, 1.0, w.ctypes.data, 2, out.ctypes.data, out.size) == native.E_INVALID


def test_emitter_ids_of_the_fixtures():
    ptrs, world, actor = scenes.emitter_ids(rs.make("routes"))
    assert ptrs.dtype == np.int32 and ptrs.tolist() == ROUTES_EMITTERS and (world, actor) == (False, False)
    ptrs, world, actor = scenes.emitter_ids(rs.make("routes_tris"))
    assert ptrs.tolist() == ROUTES_EMITTERS and (world, actor) == (True, False)
    ptrs, world, actor = scenes.emitter_ids(es.routes_tris_actor_emits())
    assert ptrs.tolist() == ROUTES_EMITTERS and (world, actor) == (False, True)
    sc, B, m = rs.base()
    for name in ("emit6a", "emit2", "glow", "emit_box", "emit_quad", "mat_mod6_box", "mat_mod6_quad"):   # flag 2, a byte, models of both kinds
        assert B[name] in ROUTES_EMITTERS, name
    assert B["stone"] not in ROUTES_EMITTERS and B["plain_quad"] not in ROUTES_EMITTERS
    assert scenes.emitter_ids(gs.make("outdoor_nosun"))[1:] == (False, False)


@pytest.mark.parametrize("name", ["routes", "routes_tris", "indoor", "outdoor", "indoor_sun"])
def test_darkening_nothing_is_the_identity(port, name):
    sc = rs.make(name) if name.startswith("routes") else gs.make(name)
    seeds = SEEDS if name.startswith("routes") else SEEDS[:gs.N_PASSES]
    want = emitters(port, sc, seeds)
    assert want.any()
    got = emitters(port, es.darkened(sc, []), seeds)
    np.testing.assert_array_equal(bits(got), bits(want))
    # one group holding everything is EMITTERS too
    np.testing.assert_array_equal(bits(es.expected_groups(port, sc, {}, 1, seeds)[0]), bits(want))


@pytest.mark.parametrize("name", ["routes", "routes_tris"])
def test_darkening_everything_leaves_no_light(port, name):
    sc = rs.make(name)
    assert not bits(emitters(port, es.darkened(sc, es.all_emitters(sc)))).any()


def test_darkened_scene_keeps_tree_and_pointers():
    sc = rs.make("routes_tris")
    dark = es.darkened(sc, [8, 18, 32, es.WORLD])
    assert np.array_equal(dark.octree, sc.octree) and np.array_equal(dark.world_bvh, sc.world_bvh) and np.array_equal(dark.actor_bvh, sc.actor_bvh)
    b0, b1 = np.asarray(sc.block_palette), np.asarray(dark.block_palette)
    assert len(b0) == len(b1) and np.array_equal(b0[0::2], b1[0::2])                 # every block keeps its place and kind
    changed = np.flatnonzero(b0[1::2] != b1[1::2]) * 2
    assert changed.tolist() == [8, 18, 32]
    m0, m1 = np.asarray(sc.material_palette), np.asarray(dark.material_palette)
    assert np.array_equal(m0, m1[:len(m0)]) and len(m1) > len(m0)                    # copies are appended, no record is changed
    copies = m1[len(m0):].reshape(-1, 6)
    assert not (copies[:, 0] & 2).any() and not copies[:, 4].any()
    assert scenes.emitter_ids(dark)[0].tolist() == [p for p in ROUTES_EMITTERS if p not in (8, 18, 32)]
    assert scenes.emitter_ids(dark)[1:] == (False, False)


def test_routes_splits_into_three_lit_groups(port):
    """The reference's figures: 9.7 %, 5.8 % and 4.0 % of the pixels; the rest (group 0) has no emitter left."""
    sc = rs.make("routes")
    mapping, n = es.routes_split()
    assert n == 4 and sorted(mapping) == ROUTES_EMITTERS
    groups = es.expected_groups(port, sc, mapping, n, SEEDS)
    shares = [es.lit_share(g) for g in groups]
    print("lit shares", shares)
    assert shares[0] == 0 and min(shares[1:]) >= 0.01
    assert [round(100 * s, 1) for s in shares[1:]] == [9.7, 5.8, 4.0]


def test_entity_groups(port):
    """routes_tris: the world sheet emits (18.3 % of the pixels), the actor sheet does not; the variant the other way round."""
    seeds = SEEDS
    rest, world, actor = es.expected_groups(port, rs.make("routes_tris"), {es.WORLD: 1, es.ACTOR: 2}, 3, seeds)
    assert round(100 * es.lit_share(world), 1) == 18.3 and not bits(actor).any() and rest.any()
    rest2, world2, actor2 = es.expected_groups(port, es.routes_tris_actor_emits(), {es.WORLD: 1, es.ACTOR: 2}, 3, seeds)
    assert es.lit_share(actor2) >= 0.01 and not bits(world2).any()
    assert rest2.any()


@pytest.mark.parametrize("name", ["routes", "routes_tris"])
def test_groups_sum_to_emitters_within_the_one_pass_bound(port, name):
    """One pass, first_spp 0, the header's bound for recombined light groups: every term is non-negative, a group's sum and EMITTERS'
    take at most max_depth additions of hit terms each (far fewer than the 2 * max_depth + 1 the bound allows), and the groups are
    recombined in float64: |sum of groups - EMITTERS| <= 4 * (2 * max_depth + 3) * 2^-24 * EMITTERS per float."""
    sc = rs.make(name)
    ids = es.all_emitters(sc)
    mapping = {i: k for k, i in enumerate(ids)}   # every emitter a group of its own: 7 or 8 groups
    n = len(ids)
    assert n in (7, 8)
    seeds = SEEDS[:1]
    groups = es.expected_groups(port, sc, mapping, n, seeds)
    want = emitters(port, sc, seeds).astype(np.float64)
    total = np.zeros_like(want)
    for g in groups:
        total += g
    bound = 4 * (2 * MAX_DEPTH + 3) * 2.0 ** -24
    err = np.abs(total - want)
    worst = float((err / np.maximum(want, 1e-30)).max())
    print(f"{name}: worst relative error {worst:.3g} (bound {bound:.3g})")
    assert want.any() and (err <= bound * want).all(), worst


def test_numpy_mix_rounds_once_per_operation():
    rng = np.random.default_rng(3)
    sky, sun, g0, g1 = (rng.random(64, np.float32) for _ in range(4))
    got = es.mix(sky, sun, [g0, g1], 0.3, 1.7, [2.5, 0.1])
    f = np.float32
    want = [f(f(f(f(f(0.3) * a) + f(f(1.7) * b)) + f(f(2.5) * c)) + f(f(0.1) * d)) for a, b, c, d in zip(sky, sun, g0, g1)]
    assert bits(got).tolist() == bits(np.array(want, f)).tolist()


def test_host_validator_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "light_groups_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "light_groups_fuzz.cpp"), os.path.join(native.CSRC, "lights_host.cpp"),
           os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    assert not any("rocm" in a.lower() for a in cmd)
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0
    assert out["refusal_kinds"] >= 22 and out["accepted"] >= 500 and out["refused"] >= 500 and out["lookups"] >= 10000
