"""Parity of the HIP kernels on octrees deeper than 10 levels, and on scenes that have no wide tree at all.

The default split of the wide tree (csrc/widetree.cpp) is a dense top node over ONE 8^3 level up to depth 10 (tree forms 16, 17:
everything else the suite renders), over TWO at depth 11 - 13 (form 18), over THREE at 14 - 15 (form 19); an octree deeper than 15
levels keeps the reference layout only (form 0).  The worlds here are the golden scenes inside such octrees
(scenes.embed_deeper: the same world, a few 8-int groups in front), so they cost what the depth-6 ones cost.  Every case asserts
kernel_info() / aov_info(): the test proves which instantiation ran.  Images are compared with the reference build's
(tests/golden/deep.npz, tests/test_deep_goldens.py) where one is committed, with the C restatement otherwise."""
import dataclasses
import os

import numpy as np
import pytest

import golden_scenes as gs
from aov_spec import expected_aov
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader
from oracle import binding
from oracle.binding import PortExt
from test_gpu_camera_projections import equivalent, projected
from test_gpu_extensions import with_spec_words
from test_gpu_parity import assert_radiance, bits
from test_list_route_cpu import scene as list_route_scene

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "deep.npz"))
SEEDS = scenes.java_random_ints(gs.N_PASSES)
FORM = gs.EMBED_FORM
_want = {}


def make_renderer(gpu_instance, sc, variant=0):
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    return loader, r


def expected(port, name, depth, sc):
    """(image, preview) of golden scene `name` at the origin of a depth-`depth` octree: the reference build's where committed."""
    key = f"{name}_d{depth}"
    if key + "_res" in GOLD.files:
        assert gs.input_digest(sc) == str(GOLD[key + "_digest"])
        return GOLD[key + "_res"], GOLD[key + "_preview"]
    if key not in _want:
        h = binding.SceneHandle(sc)
        _want[key] = (port.render_passes(h, SEEDS), port.preview(h))
    return _want[key]


def check_image(r, want, what):
    assert_radiance(r.read(), want[0], f"{what} res")
    np.testing.assert_array_equal(r.preview(), want[1], err_msg=what)


# ---- render_pool<18 | 19 | 0, 64>, plain and with sorted block tests ----
# (the sorted instantiations exist for the wide forms only: variant bit 8 on a scene without a wide tree changes nothing)
PLAIN_CASES = [(name, depth, variant) for name in ("outdoor", "inside", "pregen") for depth in (11, 12, 13, 14, 15, 16, 20)
               for variant in (0, 256)]


@pytest.mark.parametrize("name,depth,variant", PLAIN_CASES)
def test_plain_and_sorted_kernels_on_deep_octrees(gpu_instance, port, name, depth, variant):
    """Depth 11 - 13: pool_kernel<18, 64>; 14 - 15: <19, 64>; 16, 20: <0, 64> (no wide tree); variant bit 8: the sorted twins of 18
    and 19."""
    sc = gs.embedded(name, depth)
    loader, r = make_renderer(gpu_instance, sc, variant)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"], info["ext"]) == (FORM[depth], 64, False, False), info
    assert info["sorted"] == (variant == 256 and FORM[depth] != 0), info
    check_image(r, expected(port, name, depth, sc), f"{name} depth {depth} variant {variant}")
    r.close()
    loader.close()


def test_ragged_view_on_three_levels(gpu_instance, port):
    """33 x 17: padded 16 x 16 tiles in both directions, on the three-level form."""
    sc = gs.embedded("outdoor", 15).with_view(33, 17)
    loader, r = make_renderer(gpu_instance, sc)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["pool"]) == (19, 64), info
    h = binding.SceneHandle(sc)
    check_image(r, (port.render_passes(h, SEEDS), port.preview(h)), "33 x 17")
    r.close()
    loader.close()


# ---- entity BVHs ----
@pytest.mark.parametrize("depth", [11, 13, 14, 15, 16])
def test_entity_kernels_on_deep_octrees(gpu_instance, port, depth):
    """With entity BVHs render_pool has the two-level form (18, 32 or 16 parked paths) and the generic walk (-1: here over the FOUR
    levels of depth 14 - 15).  A scene WITHOUT a wide tree (depth 16) has no render_pool instantiation with BVH phases: it runs the
    fallback kernel's reference-layout walk over the packed BVH (pool_kernel_applies; before, launch_pool picked the generic
    wide-tree walk for it, which with no levels reads nothing and sees an empty world)."""
    sc = gs.embedded("entities", depth)
    loader, r = make_renderer(gpu_instance, sc)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["bvh"] and not info["ext"] and not info["sorted"], info
    if depth <= 13:
        assert info["tree"] == 18 and info["pool"] in (16, 32), info
    elif depth <= 15:
        assert info["tree"] == -1 and info["pool"] in (16, 32), info
    else:
        assert info["tree"] == 0 and info["pool"] < 0, info
    check_image(r, expected(port, "entities", depth, sc), f"entities depth {depth}")
    r.close()
    loader.close()


# ---- proj::render_pool ----
@pytest.mark.parametrize("depth", [12, 15])
def test_projected_camera_on_deep_octrees(gpu_instance, port, depth):
    """A fisheye camera (projector type 2) runs proj::render_pool with the same template arguments; its image is the restatement's on
    the equivalent ray tables (tests/test_gpu_camera_projections.py)."""
    sc = projected(gs.embedded("outdoor", depth), native.PROJ_FISHEYE)
    assert sc.projector_type == native.PROJ_FISHEYE > 0
    loader, r = make_renderer(gpu_instance, sc)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"]) == (FORM[depth], 64, False), info
    assert_radiance(r.read(), equivalent(port, sc, SEEDS), f"fisheye depth {depth}")
    r.close()
    loader.close()


# ---- the extended light-transport options ----
EXT = dict(bsdf=1, nee=1)


def with_ext(r):
    r.set_option(native.OPT_BSDF, EXT["bsdf"])
    r.set_option(native.OPT_EMITTER_NEE, EXT["nee"])


@pytest.mark.parametrize("depth", [12, 15])
def test_extended_kernels_on_deep_octrees(gpu_instance, port, depth):
    sc = with_spec_words(gs.embedded("outdoor", depth))
    loader, r = make_renderer(gpu_instance, sc)
    with_ext(r)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["ext"] and info["pool"] == 32 and info["tree"] == (18 if depth == 12 else -1), info
    with PortExt(port, sc, **EXT):
        want = port.render_passes(sc, SEEDS)
    np.testing.assert_array_equal(bits(r.read()), bits(want))
    assert not np.array_equal(bits(want), bits(port.render_passes(sc, SEEDS))), "the options changed nothing"
    r.close()
    loader.close()


def test_extended_options_refuse_a_scene_without_a_wide_tree(gpu_instance, port):
    """The extended instantiations walk the wide tree only: on a depth-16 octree chunky_render_passes refuses with CHUNKY_E_STATE
    (before: the generic walk over no levels, an empty world); with the options back at their defaults the scene renders."""
    sc = with_spec_words(gs.embedded("outdoor", 16))
    loader, r = make_renderer(gpu_instance, sc)
    with_ext(r)
    with pytest.raises(native.ChunkyHipError) as e:
        r.render_passes(SEEDS)
    assert e.value.code == native.E_STATE
    r.set_option(native.OPT_BSDF, 0)
    r.set_option(native.OPT_EMITTER_NEE, 0)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["ext"]) == (0, 64, False), info
    assert_radiance(r.read(), port.render_passes(sc, SEEDS), "depth 16 after the refusal")
    r.close()
    loader.close()


# ---- the other kernels ----
@pytest.mark.parametrize("variant", [8, 8 | 16, 2])
@pytest.mark.parametrize("depth", [12, 16])
@pytest.mark.parametrize("name", ["outdoor", "entities"])
def test_fallback_kernels_on_deep_octrees(gpu_instance, port, name, depth, variant):
    """render_waves (bit 3; bit 4: one lane per pixel) and render_lanes (bit 1): the generic walk over three levels, the reference
    layout at depth 16."""
    sc = gs.embedded(name, depth)
    loader, r = make_renderer(gpu_instance, sc, variant)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["pool"] < 0 and info["tree"] == (-1 if depth == 12 else 0) and info["bvh"] == (name == "entities"), info
    check_image(r, expected(port, name, depth, sc), f"{name} depth {depth} variant {variant}")
    r.close()
    loader.close()


@pytest.mark.parametrize("variant,park", [(64, 0), (128, 32)])
@pytest.mark.parametrize("depth", [12, 16])
def test_small_pools_on_deep_octrees(gpu_instance, port, depth, variant, park):
    """render_pool with no / 32 parked paths (variant bits 6 - 7): the generic walk, or the reference layout."""
    sc = gs.embedded("outdoor", depth)
    loader, r = make_renderer(gpu_instance, sc, variant)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["pool"]) == (-1 if depth == 12 else 0, park), info
    check_image(r, expected(port, "outdoor", depth, sc), f"depth {depth} variant {variant}")
    r.close()
    loader.close()


def test_phase_statistics_without_a_wide_tree(gpu_instance, port):
    """Variant bit 2 (phase statistics) has wide-tree instantiations only: a depth-16 scene renders on the fallback kernel."""
    sc = gs.embedded("outdoor", 16)
    loader, r = make_renderer(gpu_instance, sc, 4)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["tree"] == 0 and info["pool"] < 0, info
    check_image(r, expected(port, "outdoor", 16, sc), "depth 16 variant 4")
    r.close()
    loader.close()


@pytest.mark.parametrize("name,form,variant,want", [("outdoor", 17, 4 | 512, (17, 64, False)), ("outdoor", 18, 4 | 512, (-1, 64, False)),
                                                    ("entities", 17, 4, (17, 16, True)), ("entities", 18, 4, (-1, 16, True))])
def test_phase_statistics_kernels(gpu_instance, port, name, form, variant, want):
    """Variant bit 2 on a wide tree: render_pool<17 | -1, 64, STATS> (bit 9: unsorted; the sorted twins run in
    tests/test_gpu_camera_lens_ods.py) and, with entity BVHs, <17 | -1, 16, STATS, BVH> — the dense top of one level and, for every
    other form, the generic walk.  40 x 24: tiles padded on both edges; three passes, one launch."""
    sc = list_route_scene(name, form).with_view(40, 24)  # (the golden scene in the octree that selects the form)
    loader, r = make_renderer(gpu_instance, sc, variant)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"]) == want and not info["ext"] and not info["sorted"], info
    assert_radiance(r.read(), port.render_passes(binding.SceneHandle(sc), SEEDS), f"{name} form {form} variant {variant}")
    r.close()
    loader.close()


# ---- AOV passes ----
@pytest.mark.parametrize("depth", [12, 15, 16])
@pytest.mark.parametrize("name", ["outdoor", "entities"])
def test_aov_passes_on_deep_octrees(gpu_instance, port, name, depth):
    sc = gs.embedded(name, depth)
    loader, r = make_renderer(gpu_instance, sc)
    r.render_aov(SEEDS)
    info = r.aov_info()
    bvh = name == "entities"
    assert (info["tree"], info["bvh"]) == ({12: 18, 15: -1 if bvh else 19, 16: 0}[depth], bvh), info
    gids = np.arange(0, sc.width * sc.height, 3)
    want = expected_aov(port, binding.SceneHandle(sc), SEEDS, gids)
    got = (r.read_aov(native.AOV_ALBEDO).reshape(-1, 3)[gids], r.read_aov(native.AOV_NORMAL).reshape(-1, 3)[gids])
    for kind, g, w in zip(("albedo", "normal"), got, want):
        same = (bits(np.ascontiguousarray(g)) == bits(w)).all(axis=1)
        assert same.all(), f"{name} depth {depth}: {kind} differs at {int((~same).sum())} of {len(gids)} pixels (first gid {int(gids[np.argmin(same)])})"
    assert (want[1] != 0).any(axis=1).mean() > 0.25, "the view hardly sees the world"
    r.close()
    loader.close()


# ---- trace records ----
@pytest.mark.parametrize("depth", [12, 16])
def test_trace_records_on_deep_octrees(gpu_instance, port, depth):
    sc = gs.embedded("entities", depth)
    loader, r = make_renderer(gpu_instance, sc)
    rec, cnt, rad = r.trace_records(int(SEEDS[0]), gs.RECORD_GIDS)
    h = binding.SceneHandle(sc)
    hits = 0
    for i, g in enumerate(gs.RECORD_GIDS):
        want, wrad = port.trace_records(h, int(SEEDS[0]), int(g))
        n = len(want)
        assert int(cnt[i]) == n, (depth, int(g))
        got = rec[i, :n]
        assert got["hit"].tolist() == want["hit"].tolist(), (depth, int(g))
        assert got["material"].tolist() == want["material"].tolist(), (depth, int(g))
        for f in ("distance", "normal", "color", "emittance"):
            assert_radiance(got[f], want[f], f"depth {depth} gid {int(g)} {f}")
        hit = want["hit"] == 1
        hits += int(hit.sum())
        assert_radiance(got["point"][hit], want["point"][hit], f"depth {depth} gid {int(g)} point")
        assert_radiance(rad[i], wrad, f"depth {depth} gid {int(g)} radiance")
    assert hits > len(gs.RECORD_GIDS) // 2
    r.close()
    loader.close()


def test_device_octree_march_on_two_levels(gpu_instance, port):
    """Helper row kind 14 (the octree march alone) on the depth-12 world: helpers_selftest_kernel<18> and <0> against the
    restatement's march, on the rays of the depth-6 scene (the world has not moved)."""
    from test_helper_kats import assert_same
    sc = gs.embedded("entities", 12)
    rows = gs.helper_rows(gs.make("entities"), 14)
    want = port.helpers(sc, 14, rows)
    assert np.isfinite(want[:, 0]).mean() > 0.4
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    a, ta = loader.selftest_helpers(14, rows, tree=0)
    b, tb = loader.selftest_helpers(14, rows, tree=1)
    assert (ta, tb) == (0, 18)
    assert_same(a, want, 14)
    assert_same(b, want, 14)
    loader.close()


# ---- leaves of the new levels: one that is hit, one that is walked through ----
def test_offset_world_beside_a_full_cube_leaf(gpu_instance):
    """"outdoor" at x = z = 1024 of a depth-12 octree, a 64^3 stone leaf (level 6) diagonally behind it: the reference build's image."""
    sc = gs.embedded_offset()
    assert gs.input_digest(sc) == str(GOLD[gs.EMBED_OFFSET + "_digest"])
    for variant, sorted_ in ((0, False), (256, True)):
        loader, r = make_renderer(gpu_instance, sc, variant)
        r.render_passes(SEEDS)
        info = r.kernel_info()
        assert (info["tree"], info["pool"], info["sorted"]) == (18, 64, sorted_), info
        check_image(r, (GOLD[gs.EMBED_OFFSET + "_res"], GOLD[gs.EMBED_OFFSET + "_preview"]), f"offset world, variant {variant}")
        r.close()
        loader.close()


def test_rays_cross_a_level_14_leaf_that_cannot_be_hit(gpu_instance, port):
    """"outdoor" at the origin of a depth-15 octree whose half above y = 16384 is ONE ANY_TYPE leaf (level 14, the last but one value
    of the wide entry's 4-bit level field): every ray that leaves upwards exits that leaf's box.  With the camera of "inside" (between the
    blocks) as well."""
    for cam in ("outdoor", "inside"):
        sc = dataclasses.replace(gs.embedded_any(), camera=gs.make(cam).camera)
        data, level, _n = native.widetree_lookup(sc.octree, 15, [[5, 16384, 5], [5, 16383, 5]])
        assert (data.tolist(), level.tolist()) == ([scenes.ANY_TYPE, 0], [14, 13])
        loader, r = make_renderer(gpu_instance, sc)
        r.render_passes(SEEDS)
        info = r.kernel_info()
        assert (info["tree"], info["pool"]) == (19, 64), info
        h = binding.SceneHandle(sc)
        check_image(r, (port.render_passes(h, SEEDS), port.preview(h)), f"ANY_TYPE above, camera of {cam}")
        r.close()
        loader.close()
