"""Biome tints by block position without a device: the ABI's symbol, the specification module on the oracle (tests/biome_spec.py) and
the device-free launch plan (csrc/launch_plan.cpp plan_biome).

  * expand with a map of the three constants is the original world's image and preview, bit for bit, on the C restatement and on the
    reference build: replacing tint types 1 - 3 by constant tints, and a tinted leaf by copies of its block, changes no bit;
  * expand keeps the tree's shape and touches nothing outside the map;
  * the census: pass 0 of both fixtures lands on every tint type they hold, inside and outside the map, on first hits and on bounces —
    the bounds are the counts measured on the oracle;
  * plan_biome over the plans of tests/golden/launch_plans.npz names only instantiations that exist, or refuses."""
import dataclasses
import os

import numpy as np
import pytest

import biome_spec as bs
from chunkyclplugin_amd import native, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = scenes.java_random_ints(4)  # (the same stream as native.java_random_ints, without loading the library while tests are collected)
FIXTURES = {"exhibit": bs.exhibit, "water": bs.water_world}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_symbol_option_and_null_scene():
    L = native.lib()
    assert hasattr(L, "chunky_scene_set_biome_tints") and "chunky_scene_set_biome_tints" in native.declared_symbols()
    rgb = np.zeros(3, np.int32)
    assert L.chunky_scene_set_biome_tints(None, native.ptr(rgb), 0, 0, 1, 1) == native.E_INVALID
    assert b"NULL scene" in L.chunky_last_error()
    assert native.OPT_BIOME_TINT == 9
    text = open(native.HEADER).read()
    assert "CHUNKY_OPT_BIOME_TINT = 9" in text and f"CHUNKY_BIOME_MAX_CELLS (1 << {native.BIOME_MAX_CELLS.bit_length() - 1})" in text


def test_patch_generator_and_scene_files(tmp_path):
    m = scenes.biome_patches(20, 23, 4, seed=78)
    assert m.shape == (23, 20, 3) and m.dtype == np.int32 and (m >= 0).all() and (m < 1 << 24).all()
    assert (m[:4, :4] == m[0, 0]).all() and (m[20:, 16:] == m[22, 19]).all()
    assert len({tuple(t) for t in m.reshape(-1, 3).tolist()}) == 5 * 6  # one triple per patch, all distinct
    assert np.array_equal(m, scenes.biome_patches(20, 23, 4, seed=78))
    sc = bs.exhibit()
    path = str(tmp_path / "scene.npz")
    scenes.save_scene(sc, path)
    back = scenes.load_scene(path)
    assert back.biome[:2] == sc.biome[:2] and np.array_equal(back.biome[2], sc.biome[2])
    scenes.save_scene(dataclasses.replace(sc, biome=None), path)
    assert scenes.load_scene(path).biome is None and "biome_rgb" not in np.load(path).files
    assert scenes.tiny_scene().biome is None


def test_scene_json_flag():
    from chunkyclplugin_amd import octree2
    assert octree2.biome_tint_option({}) == 1 and octree2.biome_tint_option({"biomeColors": True}) == 1
    assert octree2.biome_tint_option({"biomeColors": False}) == 0


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_constants_map_is_the_original_world(port, name):
    sc = FIXTURES[name]()
    x0, z0, rgb = sc.biome
    plain = dataclasses.replace(sc, biome=None)
    same = bs.expand(sc, (x0, z0, bs.constants_map(rgb.shape[1], rgb.shape[0])))
    assert len(same.block_palette) > len(sc.block_palette)  # copies were made: the comparison is of another world
    assert bits(port.render_passes(plain, SEEDS)).tobytes() == bits(port.render_passes(same, SEEDS)).tobytes()
    assert np.array_equal(port.preview(plain), port.preview(same))
    tinted = bs.expand(sc)
    assert bits(port.render_passes(plain, SEEDS)).tobytes() != bits(port.render_passes(tinted, SEEDS)).tobytes()  # the fixtures do see the tint


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_constants_map_is_the_original_world_on_the_reference_build(ref, name):
    sc = FIXTURES[name]()
    x0, z0, rgb = sc.biome
    plain = dataclasses.replace(sc, biome=None)
    same = bs.expand(sc, (x0, z0, bs.constants_map(rgb.shape[1], rgb.shape[0])))
    assert bits(ref.render_passes(plain, SEEDS)).tobytes() == bits(ref.render_passes(same, SEEDS)).tobytes()
    assert np.array_equal(ref.preview(plain), ref.preview(same))


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_expand_keeps_the_tree_and_everything_outside_the_map(name):
    sc = FIXTURES[name]()
    ex, origin = bs.expand(sc, with_origin=True)
    assert ex.biome is None
    a, b = np.asarray(sc.octree), np.asarray(ex.octree)
    assert a.shape == b.shape and np.array_equal(a > 0, b > 0) and np.array_equal(a[a > 0], b[b > 0])  # the same branches at the same places
    changed = np.flatnonzero(a != b)
    assert len(changed) and set((-b[changed]).tolist()) == set(origin)
    assert all(origin[int(-b[i])] == int(-a[i]) for i in changed)
    n = len(sc.block_palette)
    assert np.array_equal(ex.block_palette[:n], sc.block_palette) and np.array_equal(ex.material_palette[:len(sc.material_palette)], sc.material_palette)
    for f in ("world_bvh", "actor_bvh", "bvh_trigs", "atlas", "sky", "sun", "camera"):
        assert np.array_equal(getattr(ex, f), getattr(sc, f)), f
    # every copy's tinted materials carry a constant tint, and nothing else of them changed
    mats = np.asarray(ex.material_palette).reshape(-1, 6)
    new = mats[len(sc.material_palette) // 6:]
    assert len(new) and (((new[:, 1] >> 24) & 0xFF) == 0xFF).all()
    # leaves outside the map's rectangle are untouched
    idx, pos, size, _data = bs.tinted_leaves(sc)
    x0, z0, rgb = sc.biome
    outside = (pos[:, 0] + size <= x0) | (pos[:, 0] >= x0 + rgb.shape[1]) | (pos[:, 2] + size <= z0) | (pos[:, 2] >= z0 + rgb.shape[0])
    assert outside.any() and not outside.all()
    assert np.array_equal(a[idx[outside]], b[idx[outside]]) and (a[idx[~outside]] != b[idx[~outside]]).all()


def test_the_water_world_has_merged_tinted_leaves():
    """... so "for a leaf larger than one cell, the march point's cell" is part of what the water fixture compares (expand asserts that
    each lies within one colour triple); the deep world of the 1080p parity row has them too."""
    assert bs.merged_tinted_leaves(bs.water_world()) == 11
    assert bs.merged_tinted_leaves(bs.exhibit()) == 0


# measured on the C restatement, pass 0 (SEEDS[0]) of each fixture: {(tint type, in / out of the map): hits}
CENSUS = {
    "exhibit": {"first": {(1, "in"): 29, (1, "out"): 47, (2, "in"): 87, (2, "out"): 177, (3, "in"): 21, (3, "out"): 20},
                "later": {(1, "in"): 116, (1, "out"): 227, (2, "in"): 233, (2, "out"): 468, (3, "in"): 18, (3, "out"): 16}},
    "water": {"first": {(1, "in"): 161, (2, "in"): 543, (2, "out"): 1009}, "later": {(1, "in"): 541, (2, "in"): 1143, (2, "out"): 1650}},
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_census(port, name):
    got = bs.census(port, FIXTURES[name](), int(SEEDS[0]))
    for kind in ("first", "later"):
        for key, least in CENSUS[name][kind].items():
            assert got[kind].get(key, 0) >= least, (kind, key, got[kind].get(key, 0), least)
    if name == "exhibit":  # every tint type, inside and outside the map, on first hits and on bounces
        assert all(got[kind].get((t, where), 0) > 0 for kind in ("first", "later") for t in (1, 2, 3) for where in ("in", "out"))


def test_plan_biome_names_only_what_exists():
    g = np.load(os.path.join(ROOT, "tests", "golden", "launch_plans.npz"))
    names, plans = list(g["fields"]), np.ascontiguousarray(g["plans"].T)
    col = {f: i for i, f in enumerate(names)}
    out, why = native.plan_biome(plans)
    ok = plans[:, col["status"]] == 0
    # a plan plan_render refused comes back as it is
    assert np.array_equal(out[~ok], plans[~ok]) and not why[~ok].any()
    want_why = np.where(plans[:, col["ext"]] != 0, 2, np.where(plans[:, col["stats"]] != 0, 1, np.where(plans[:, col["proj"]] != 0, 3, 0)))
    assert np.array_equal(why[ok], want_why[ok])
    assert {1, 2, 3} <= set(why[ok].tolist())
    served = out[ok & (why == 0)]
    asked = plans[ok & (why == 0)]
    assert len(served) > 50000
    fam, tree, park, bvh = (served[:, col[f]] for f in ("family", "tree", "park", "bvh"))
    assert set(fam.tolist()) == {0, 2}  # the pool kernel and render_lanes: no biome render_waves exists
    assert not served[:, [col["ext"], col["stats"], col["sorted"], col["proj"]]].any()
    pool, lanes = fam == 0, fam == 2
    assert np.array_equal(pool, asked[:, col["family"]] == 0)  # what ran the pool kernel still does
    plain, ents = pool & (bvh == 0), pool & (bvh != 0)
    assert set(tree[plain].tolist()) == set(native.BIOME_POOL_FORMS) and set(park[plain].tolist()) == {native.BIOME_POOL_PARK}
    assert set(tree[ents].tolist()) == set(native.BIOME_POOL_BVH_FORMS) and set(park[ents].tolist()) <= set(native.BIOME_POOL_BVH_PARKS)
    assert set(tree[lanes].tolist()) == set(native.BIOME_LANES_FORMS) and (served[lanes][:, col["group"]] == 0).all()
    # tree forms: kept where an instantiation has them, else the generic walk
    at = asked[:, col["tree"]]
    assert np.array_equal(tree[plain], np.where(np.isin(at[plain], native.BIOME_POOL_FORMS), at[plain], -1))
    assert np.array_equal(tree[ents], np.where(at[ents] == 17, 17, -1))
    assert np.array_equal(tree[lanes], at[lanes])
    # LDS: the pool's record and stacks for the pool size that runs; the to-visit stacks alone under render_lanes
    words, depth, lds = served[:, col["words"]], served[:, col["depth"]], served[:, col["lds"]]
    assert np.array_equal(lds[pool], 4 * (park[pool] * 16 * words[pool] + park[pool] * 8 + (64 + park[pool]) * depth[pool] * 4))
    assert np.array_equal(lds[lanes], depth[lanes] * 256 * 4)
    assert (lds <= 160 << 10).all()
    # what a launch may carry and whether it needs the pixel list do not change
    assert np.array_equal(served[:, [col["most"], col["needs_list"], col["words"], col["depth"], col["bvh"]]],
                          asked[:, [col["most"], col["needs_list"], col["words"], col["depth"], col["bvh"]]])


def test_the_lists_in_the_source_are_the_lists_here():
    text = open(os.path.join(native.CSRC, "launch_plan.hpp")).read()
    a = text.index("#define CHUNKY_POOL_BIOME_INSTANCES(X)")
    b = text.index("#define CHUNKY_POOL_BIOME_BVH_INSTANCES(X)")
    import re
    plain = re.findall(r"X\((-?\d+), kPoolBiomePark, false, false, false, false\)", text[a:b])
    ents = re.findall(r"X\((-?\d+), (\d+), false, true, false, false\)", text[b:b + 600])
    assert tuple(int(t) for t in plain) == native.BIOME_POOL_FORMS
    assert {int(t) for t, _k in ents} == set(native.BIOME_POOL_BVH_FORMS) and {int(k) for _t, k in ents} == set(native.BIOME_POOL_BVH_PARKS)
    assert "constexpr int kPoolBiomePark = kPoolPark;" in text and native.BIOME_POOL_PARK == 64
    assert all(s in native.SOURCES for s in ("render_pool_biome.hip", "render_pool_biome_bvh.hip", "render_biome.hip", "aov_biome.hip"))
