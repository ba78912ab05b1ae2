"""Translucent blocks without a GPU: the CPU specification (tests/glass_port.c over csrc/glass_spec.h) against the
oracle with the feature off and with nothing translucent in view, known answers and totality of the header's functions, analytic images
(pane transmission, the white furnace, the shadow filter, the cap), the census of the exhibit world with its re-hit bound, and the
device-free part of the C API (chunky_translucency_check, plan_glass)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import glass_spec
import golden_scenes as gs
from chunkyclplugin_amd import native, scenes
from oracle.binding import PortExt

INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def glass():
    return glass_spec.lib()


# ---- 1. feature off, and feature on with nothing translucent in view: the oracle's integrator, bit for bit ----
@pytest.mark.parametrize("name", ["outdoor", "indoor", "entities"])
@pytest.mark.parametrize("ext", [{}, dict(bsdf=1, nee=1, sun_sampling=1)], ids=["defaults", "bsdf-nee-sun"])
def test_off_and_nothing_translucent_are_the_oracle(port, glass, name, ext):
    sc = gs.make(name).with_view(96, 64)
    seeds = scenes.java_random_ints(4)
    with PortExt(port, sc, **ext):
        want = port.render_passes(sc, seeds)
    gids = np.arange(0, 96 * 64, 7, dtype=np.int32)
    off = glass_spec.render(sc, seeds, None, ext=ext)
    off_listed = glass_spec.render(sc, seeds, None, ext=ext, gids=gids)
    on, census = glass_spec.render(sc, seeds, glass_spec.DEFAULT, ext=ext, census=True)
    on_listed = glass_spec.render(sc, seeds, glass_spec.DEFAULT, ext=ext, gids=gids)
    np.testing.assert_array_equal(bits(off), bits(want))
    np.testing.assert_array_equal(bits(on), bits(want))
    for listed in (off_listed, on_listed):
        np.testing.assert_array_equal(bits(listed.reshape(-1, 3)[gids]), bits(want.reshape(-1, 3)[gids]))
    assert not any(census.values()), census   # nothing translucent: no crossing, no run, no cap
    assert want.max() > 0


# ---- 2. the header's functions ----
def test_known_answers(glass):
    f = np.float32
    rows = [(0.5, 0.99, 0, 8, 1), (0.99, 0.99, 0, 8, 0), (0.98999995, 0.99, 0, 8, 1), (255 / 256, 0.99, 0, 8, 0), ((255 / 256) ** 2, 0.99, 0, 8, 0),
            (0.5, 0.99, 8, 8, 0), (0.5, 0.99, 7, 8, 1), (0.5, 0.99, 31, 31, 0), (np.nan, 0.99, 0, 8, 0), (0.0, 0.99, 0, 8, 1), (1.0, 1.0, 0, 8, 0),
            (0.999, 1.0, 0, 8, 1), (-INF, 0.99, 0, 8, 1), (INF, 0.99, 0, 8, 0)]
    got = glass.helpers_glass(0, np.array([r[:4] for r in rows], np.float32))[:, 0]
    assert [int(g) for g in got] == [r[4] for r in rows]
    # tc = (1 - a) + a c and fs = (1 - a) tc, each operation rounded once
    a = np.array([0.5, 0.25, 0.75, 0.6875, 0.0, 1.0, 0.5, 0.5], np.float32)
    c = np.array([0.0, 1.0, 0.5, 0.3, 0.7, 0.7, 1.0, 2.0], np.float32)
    tc = glass.helpers_glass(1, np.stack([a, c], axis=1))[:, 0]
    fs = glass.helpers_glass(2, np.stack([a, c], axis=1))[:, 0]
    want_tc = (f(1) - a) + a * c
    np.testing.assert_array_equal(bits(tc), bits(want_tc.astype(np.float32)))
    np.testing.assert_array_equal(bits(fs), bits(((f(1) - a) * want_tc).astype(np.float32)))
    assert tc[0] == 0.5 and fs[0] == 0.25 and tc[1] == 1.0 and tc[4] == 1.0 and fs[5] == 0.0 and tc[6] == 1.0
    # the restart: through the surface, against the ray; a zero normal (+0 or -0) leaves p alone
    k2 = f(0.0002)
    rows = np.array([[1, 2, 3, 0, -1, 0, 4, 0, 1, 0], [1, 2, 3, 0, -1, 0, 4, 0, -1, 0], [1, 2, 3, 0, 1, 0, 4, 0, 1, 0], [1, 2, 3, 1, 0, 0, 2, 0, 1, 0],
                     [1, 2, 3, 0, -1, 0, 4, 0, 0, 0], [1, 2, 3, 0, -1, 0, 4, -0.0, -0.0, -0.0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.float32)
    o = glass.helpers_glass(3, rows)[:, :3]
    assert tuple(o[0]) == (1, f(-2) - k2, 3)            # from above onto a floor: on below it
    assert tuple(o[1]) == (1, f(-2) - k2, 3)            # the same with the normal the other way round: n_f is turned against d
    assert tuple(o[2]) == (1, f(6) + k2, 3)             # from below
    assert tuple(o[3]) == (3, f(2) - k2, 3)             # grazing (dot = 0): n_f = n
    assert tuple(o[4]) == (1, -2, 3) and tuple(o[5]) == (1, -2, 3) and tuple(o[6]) == (0, 0, 0)


def test_functions_are_total(glass):
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1e-45, 3e38, -3e38, INF, -INF, np.nan], np.float32)
    ac = np.array(np.meshgrid(vals, vals), np.float32).reshape(2, -1).T
    both = np.isfinite(ac).all(axis=1)
    for which in (1, 2):
        out = glass.helpers_glass(which, ac)[:, 0]
        assert not np.isnan(out).any()                  # no argument gives a NaN
        assert np.isfinite(out[both]).all()             # finite arguments: finite results (3e38 x 3e38 is held at FLT_MAX)
    t = glass.helpers_glass(0, np.array([[a, 0.99, 0, 8] for a in vals], np.float32))[:, 0]
    assert set(t) <= {0.0, 1.0} and t[-1] == 0          # a NaN alpha is opaque
    rng = np.random.default_rng(5)
    rows = vals[rng.integers(0, len(vals), (20000, 10))]
    rows[:200, 7:10] = 0.0                               # zero normals, +0 and -0
    rows[100:200, 7:10] = -0.0
    o = glass.helpers_glass(3, rows)[:, :3]
    assert not np.isnan(o).any()
    assert np.isfinite(o[np.isfinite(rows).all(axis=1)]).all()
    zero_n = np.isfinite(rows[:200]).all(axis=1)
    with np.errstate(all="ignore"):
        p = rows[:200, 0:3] + rows[:200, 3:6] * rows[:200, 6:7]
    ok = zero_n & np.isfinite(p).all(axis=1)
    np.testing.assert_array_equal(o[:200][ok], p[ok])   # a zero normal: o' = p


# ---- 3. analytic images: an empty 16^3 world under a constant white sky, layers of cubes across it, vertical rays from below ----
W, H, PASSES = 64, 48, 8
SKY_SLACK = 2.0 ** -21      # a white sky's four bilinear weights sum to 1 within four binary32 steps: a sample that sees it is 1 +- this


def layered_world(layers, materials, size=16, rays=None, sky=255, sky_intensity=1.0, sun=None, atlas=None, floor=None):
    """Air in a size^3 octree; layers = {y: block name}, materials = {block name: Palettes.material keywords}; blocks that share a
    material dict object share the material.  Every pixel looks straight up from below (or along `rays`)."""
    pal = scenes.Palettes()
    pal.block_invisible()
    mats, blocks = {}, {}
    for name, kw in materials.items():
        if id(kw) not in mats:
            mats[id(kw)] = pal.material(**kw)
        blocks[name] = pal.block_cube(mats[id(kw)])
    depth = int(np.log2(size))
    t = np.zeros((size, size, size), np.int32)
    for y, name in layers.items():
        t[:, y, :] = blocks[name]
    if floor is not None:
        t[:, 0, :] = blocks[floor]
    b, m, a, q = pal.arrays()
    if rays is None:
        rays = np.zeros((W * H, 6), np.float32)
        rays[:, 0] = 2.137 + 11.7 * (np.arange(W * H) % W) / W   # (off the cell boundaries)
        rays[:, 1] = 1.5
        rays[:, 2] = 2.291 + 11.3 * (np.arange(W * H) // W) / H
        rays[:, 4] = 1.0
        rays[1::2, 4] = 2.0   # (directions of length 2 among them)
    return scenes.PackedScene(octree=scenes.build_octree(t, depth), octree_depth=depth, block_palette=b, material_palette=m, aabb_models=a,
                              quad_models=q, world_bvh=scenes.empty_bvh(), actor_bvh=scenes.empty_bvh(), bvh_trigs=np.zeros(1, np.int32),
                              atlas=np.zeros((1, 16, 16, 4), np.uint8) if atlas is None else atlas, sky=np.full((8, 8, 4), sky, np.uint8),
                              sky_intensity=sky_intensity, sun=scenes.pack_sun(0.6, 1.2, 1.0, False) if sun is None else sun,
                              camera=np.asarray(rays, np.float32).reshape(-1), projector_type=-1, width=W, height=H, name="layers")


def per_pass(sc, setting=glass_spec.DEFAULT, max_depth=1, ext=None):
    """one sample per pixel and pass: (PASSES, W * H, 3)"""
    return np.stack([glass_spec.render(sc, [s], setting, ext=ext, max_depth=max_depth).reshape(-1, 3).copy() for s in scenes.java_random_ints(PASSES)])


BLACK_80 = dict(argb=0x80000000)   # alpha byte 0x80: a = 0.5 exactly; black
PANES = [
    ("one layer", {8: "a"}, {"a": BLACK_80}, 0.25, 1),
    ("two layers, air between", {8: "a", 11: "a"}, {"a": BLACK_80}, 0.0625, 2),
    # (cells 9 and 10: not the two halves of one larger leaf)
    ("two adjacent layers of one block: one run", {9: "a", 10: "a"}, {"a": BLACK_80}, 0.25, 1),
    ("two adjacent layers of two blocks with one material", {9: "a", 10: "b"}, {"a": BLACK_80, "b": BLACK_80}, 0.0625, 2),
]


@pytest.mark.parametrize("what, layers, materials, mean, crossed", PANES, ids=[p[0] for p in PANES])
def test_pane_transmission(what, layers, materials, mean, crossed):
    """(1 - a) tc per interface met: the ray crosses with probability 1 - a and keeps tc = (1 - a) + a 0 of its throughput; the reflect
    branch ends on a black surface at max depth 1."""
    x = per_pass(layered_world(layers, materials)).astype(np.float64)
    assert (x[..., 0] == x[..., 1]).all() and (x[..., 0] == x[..., 2]).all()
    x = x[..., 0]
    v = 0.5 ** crossed                      # what a sample that got through carries; it does so with probability p = v
    assert ((x == 0) | (np.abs(x - v) <= SKY_SLACK)).all()
    se = v * np.sqrt(v * (1 - v) / x.size)  # v x Bernoulli(p = v)
    print(f"{what}: mean {x.mean():.6f}, expected {mean}, standard error {se:.6f}, N {x.size}")
    assert abs(x.mean() - mean) <= 5 * se
    _, c = glass_spec.render(layered_world(layers, materials), scenes.java_random_ints(2), max_depth=1, census=True)
    assert c["main_crossings"] > 0 and c["reflect_vertices"] > 0 and c["rm_resets"] > 0 and c["rehits"] == 0, c
    # a crossing restarts inside the leaf it crossed into, which the march steps through — and, in a run of two leaves, the next one
    assert c["rm_skipped"] == (2 if what.startswith("two adjacent layers of one block") else 1) * c["main_crossings"], c


def test_the_cap_makes_the_second_pane_opaque():
    sc = layered_world({8: "a", 11: "a"}, {"a": BLACK_80})
    img, c = glass_spec.render(sc, scenes.java_random_ints(PASSES), (0.99, 1), max_depth=1, census=True)
    assert (img == 0).all()                 # behind the second pane: nothing
    assert c["capped"] > 0 and c["main_crossings"] > 0, c
    free, c = glass_spec.render(sc, scenes.java_random_ints(PASSES), (0.99, 2), max_depth=1, census=True)
    assert free.max() > 0 and c["capped"] == 0, c


def white_tile(alpha):
    t = np.full((16, 16, 4), 255, np.uint8)
    t[..., 3] = alpha
    return t


def test_white_furnace_conserves_energy():
    """All-white surfaces, opaque and translucent, under a white sky: every path that ends in the sky carries 1."""
    ab = scenes.AtlasBuilder(2, 2)
    ids = [ab.add(white_tile(a)) for a in (255, 128, 64)]
    atlas, recs = ab.build()
    mats = {"wall": dict(texture=recs[ids[0]]), "g128": dict(texture=recs[ids[1]]), "g64": dict(texture=recs[ids[2]])}
    pal_layers = {5: "g128", 6: "g128", 9: "g64", 12: "g128"}
    rng = np.random.default_rng(9)
    rays = np.zeros((W * H, 6), np.float32)
    rays[:, :3] = (8.0, 2.5, 8.0)
    d = rng.normal(size=(W * H, 3))
    d[:, 1] = np.abs(d[:, 1])
    rays[:, 3:] = d / np.linalg.norm(d, axis=1, keepdims=True)
    sc = layered_world(pal_layers, mats, rays=rays, atlas=atlas, floor="wall")
    x = per_pass(sc, max_depth=64).astype(np.float64)[..., 0]
    assert ((x == 0) | (np.abs(x - 1) <= SKY_SLACK)).all()
    se = x.std(ddof=1) / np.sqrt(x.size)
    print(f"furnace: mean {x.mean():.8f}, standard error of the samples {se:.3g}, samples at 0: {(x == 0).sum()} of {x.size}")
    assert abs(x.mean() - 1) <= 5 * se + SKY_SLACK
    _, c = glass_spec.render(sc, scenes.java_random_ints(1), max_depth=64, census=True)
    assert c["main_crossings"] > 0 and c["reflect_vertices"] > 0 and c["rm_skipped"] > 0, c


def ulps(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


@pytest.mark.parametrize("argb", [0x8040C080, 0x40E03030, 0xC03050E0])
def test_shadow_filter(glass, argb):
    """A white floor under a pane, the sun sampled, a black sky, max depth 1, the camera under the pane: every pixel is the pixel of the
    scene without the pane times fs — no draw differs between the two, so pixel by pixel."""
    ab = scenes.AtlasBuilder(4, 4)
    t_floor, t_sun = ab.add(white_tile(255)), ab.add(np.full((32, 32, 4), 255, np.uint8))
    atlas, recs = ab.build()
    sun = scenes.pack_sun(0.9, 0.3, 1.25, True, recs[t_sun])
    rays = np.zeros((W * H, 6), np.float32)
    rays[:, 0] = 1.137 + 6.7 * (np.arange(W * H) % W) / W
    rays[:, 1] = 2.9
    rays[:, 2] = 1.291 + 6.3 * (np.arange(W * H) // W) / H
    rays[:, 3:] = (1.0, -0.15, 0.6)       # a long way to the floor: the sun ray is clipped at the record's distance (the kept quirk)
    mats = {"floor": dict(texture=recs[t_floor]), "pane": dict(argb=argb)}
    with_pane = layered_world({3: "pane"}, mats, size=32, rays=rays, sky_intensity=0.0, sun=sun, atlas=atlas, floor="floor")
    without = layered_world({}, mats, size=32, rays=rays, sky_intensity=0.0, sun=sun, atlas=atlas, floor="floor")
    a = np.float32(((argb >> 24) & 0xFF) / 256.0)
    c = np.array([(argb >> 16) & 0xFF, (argb >> 8) & 0xFF, argb & 0xFF], np.float32) / np.float32(256.0)
    fs = glass.helpers_glass(2, np.stack([np.full(3, a, np.float32), c], axis=1))[:, 0]
    assert np.allclose(fs, (1 - a) * ((1 - a) + a * c))
    for seed in scenes.java_random_ints(3):
        ext = dict(sun_sampling=1)
        got, census = glass_spec.render(with_pane, [seed], ext=ext, max_depth=1, census=True)
        base = glass_spec.render(without, [seed], ext=ext, max_depth=1)
        got, base = got.reshape(-1, 3), base.reshape(-1, 3)
        assert (base > 0).all(axis=1).mean() > 0.9          # the floor is lit nearly everywhere
        assert census["sun_crossings"] > 0 and census["main_crossings"] == 0 and census["reflect_vertices"] == 0, census
        worst = int(ulps(got, base * fs[None, :]).max())
        print(f"pane {argb:#x}: worst {worst} ulp")
        assert worst <= 2
    opaque = glass_spec.render(with_pane, scenes.java_random_ints(1), None, ext=dict(sun_sampling=1), max_depth=1)
    assert (opaque == 0).all()                               # with the feature off the pane is a lid


# ---- 4. the exhibit world ----
def test_greenhouse_census_and_rehits():
    sc = scenes.greenhouse()
    assert sc.width == 96 and sc.height == 64 and sc.octree_depth == 5
    seeds = scenes.java_random_ints(6)
    img, c = glass_spec.render(sc, seeds, ext=dict(bsdf=1, nee=1), census=True)
    off = glass_spec.render(sc, seeds, None, ext=dict(bsdf=1, nee=1))
    print("greenhouse:", c, "re-hit share", c["rehits"] / max(c["crossings"], 1))
    assert np.isfinite(img).all() and not np.array_equal(bits(img), bits(off))
    for k in ("main_crossings", "reflect_vertices", "sun_crossings", "emitter_crossings", "rm_skipped", "rm_resets"):
        assert c[k] > 0, (k, c)
    assert c["crossings"] == c["main_crossings"] + c["sun_crossings"] + c["emitter_crossings"]
    assert c["rehits"] <= 0.01 * c["crossings"], c          # the condition on the restart rule
    _, one = glass_spec.render(sc, seeds, (0.99, 1), census=True)
    assert one["capped"] > 0, one
    tris = scenes.add_entities(sc, 60, seed=4, region=((2, 4, 2), (19, 18, 19)), material=_glass_material(sc))
    _, t = glass_spec.render(tris, seeds, census=True)
    assert t["tri_crossings"] > 0 and t["rehits"] <= 0.01 * t["crossings"], t


def _glass_material(sc):
    """the material pointer of the greenhouse's 0x80 glass"""
    m = np.asarray(sc.material_palette).reshape(-1, 6)
    (k,) = np.nonzero(m[:, 3].astype(np.uint32) == 0x8030D040)
    return 6 * int(k[0])


# ---- 5. the device-free C API ----
def test_translucency_check_accepts_and_refuses():
    assert C.sizeof(native.Translucency) == 16
    assert native.translucency_check(native.translucency_struct()) == 0
    assert native.translucency_check(None) == 0                              # NULL: off
    assert native.translucency_check(native.translucency_struct(1.0, 31)) == 0
    assert native.translucency_check(native.translucency_struct(1e-6, 1)) == 0
    for a, n in ((0.0, 8), (-0.5, 8), (1.0000001, 8), (np.nan, 8), (np.inf, 8), (0.99, 0), (0.99, 32), (0.99, -1)):
        assert native.translucency_check(native.translucency_struct(a, n)) == native.E_INVALID, (a, n)
        assert native.lib().chunky_last_error()
    small = native.translucency_struct()
    small.size = C.sizeof(native.Translucency) - 4
    assert native.translucency_check(small) == native.E_INVALID
    zero = native.translucency_struct()
    zero.size = 0
    assert native.translucency_check(zero) == native.E_INVALID

    class Bigger(C.Structure):
        _fields_ = [("t", native.Translucency), ("later", C.c_float * 4)]

    big = Bigger()
    big.t = native.translucency_struct()
    big.t.size = C.sizeof(Bigger)
    check = native.lib().chunky_translucency_check
    assert check(C.cast(C.pointer(big), C.POINTER(native.Translucency))) == 0
    big.later[2] = 1.0
    assert check(C.cast(C.pointer(big), C.POINTER(native.Translucency))) == native.E_INVALID
    huge = native.translucency_struct()
    huge.size = 1 << 20
    assert native.translucency_check(huge) == native.E_INVALID


def test_plan_glass_names_the_six_kernels_and_refuses_the_rest():
    #        kernel word, projector, max depth, wide, bvh, records, biome, wide levels, fog
    ok = [[0, 0, 5, 1, 0, 1, 0, 2, 0], [0, -1, 5, 1, 0, 1, 0, 3, 0], [0, 0, 254, 1, 0, 1, 0, 1, 0], [0, 0, 5, 1, 0, 1, 0, 4, 0], [0, 0, 5, 1, 0, 1, 0, 5, 0],
          [0, 0, 5, 1, 1, 1, 0, 2, 0], [0, -1, 5, 1, 1, 1, 0, 3, 0], [0, 0, 5, 1, 1, 1, 0, 1, 0], [64, 0, 5, 1, 0, 1, 0, 2, 0], [256, 0, 5, 1, 0, 1, 0, 2, 0]]
    out, text = native.plan_glass(ok)
    want_tree = [17, 18, -1, -1, -1, 17, 18, -1, 17, 17]
    for row, o, t, tree in zip(ok, out, text, want_tree):
        assert (o[0], o[1], t) == (0, 0, ""), (row, o, t)
        assert o[2] == tree and o[3] == (native.GLASS_POOL_BVH_PARK if row[4] else native.GLASS_POOL_PARK) and o[4] == row[4] and o[5] == 1 and o[6] == 0, (row, o)
        assert o[7] == native.GLASS_POOL_WORDS and tree in native.GLASS_POOL_FORMS
    refused = {"fog": ([0, 0, 5, 1, 0, 1, 0, 2, 1], "fog layer"), "biome": ([0, 0, 5, 1, 0, 1, 1, 2, 0], "biome map"),
               "stats": ([4, 0, 5, 1, 0, 1, 0, 2, 0], "phase-statistics"), "rig_bits": ([2, 0, 5, 1, 0, 1, 0, 2, 0], "default kernel"),
               "projected": ([0, 3, 5, 1, 0, 1, 0, 2, 0], "projected cameras"), "max_depth": ([0, 0, 255, 1, 0, 1, 0, 2, 0], "max depth <= 254"),
               "wide_tree": ([0, 0, 5, 0, 0, 1, 0, 0, 0], "wide re-layout"), "bvh_records": ([0, 0, 5, 1, 1, 0, 0, 2, 0], "entity BVHs")}
    out, text = native.plan_glass([r for r, _ in refused.values()])
    for (name, (row, words)), o, t in zip(refused.items(), out, text):
        assert native.GLASS_REFUSALS[o[1]] == name, (row, o, t)
        assert t.startswith("translucency: ") and words in t, (name, t)
    # the refusals are plan_fog's, with plan_fog's reasons: the same rows, the same names
    rows = [r for r, _ in list(refused.values())[1:]]
    fog_out, fog_text = native.plan_fog([r[:8] for r in rows])
    for o, fo, t, ft in zip(out[1:], fog_out, text[1:], fog_text):
        assert native.GLASS_REFUSALS[o[1]] == native.FOG_REFUSALS[fo[1]]
        assert t.split(": ", 1)[1].split(";")[0].replace("translucency", "fog") == ft.split(": ", 1)[1].split(";")[0]   # the reason, word for word
    for word in (1, 8, 1 | 4):   # the other rig bits that pick another walk or kernel
        out, _ = native.plan_glass([[word, 0, 5, 1, 0, 1, 0, 2, 0]])
        assert native.GLASS_REFUSALS[out[0][1]] in ("rig_bits", "stats")


def test_host_file_is_plain_cpp_and_in_the_build():
    for src in ("glass_host.cpp", "capi_glass.hip", "render_pool_glass.hip", "render_pool_glass_bvh.hip"):
        assert src in native.SOURCES
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
           os.path.join(native.CSRC, "glass_host.cpp")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    # the header is C99: the specification compiles it as C, the kernels as HIP
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-x", "c", os.path.join(native.CSRC, "glass_spec.h")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]


def test_glass_host_under_asan_ubsan(tmp_path):
    """chunky_translucency_check over structs in heap blocks of exactly their declared size and plan_glass over every combination of its
    inputs, in a stand-alone program (tests/sanitize/glass_host_fuzz.cpp) under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "glass_host_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "glass_host_fuzz.cpp"), os.path.join(native.CSRC, "glass_host.cpp"),
           os.path.join(native.CSRC, "launch_plan.cpp"), os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0 and out["accepted"] > 0 and out["refused"] > out["accepted"] and 0 < out["planned"] < out["plans"], out
