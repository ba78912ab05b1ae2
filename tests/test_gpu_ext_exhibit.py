"""The extended integrator on the exhibit world of tests/ext_scenes.py: render_pool's extended instantiations (csrc/render_pool.hip
shade_phase_ext, through the C ABI) against their specification, oracle/port.c trace_sample_ext under PortExt — bit for bit, at
64 x 48 and 5 passes.  The exhibit holds what the older extended fixtures lack: emitter leaves of level 1 and 2,
an emitter texture with alpha-0 texels and four different quadrants, emitters the list cannot hold behind emitter samples, every
branch of the specular vertex; tests/test_ext_census_cpu.py counts that the rays of these very cases reach them.  Every case asserts
kernel_info(): which instantiation ran."""
import ctypes as C

import numpy as np
import pytest

import ext_scenes as es
from chunkyclplugin_amd import native, parallel
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance
from oracle.binding import PortCull, PortExt
from test_gpu_camera_projections import equivalent, projected

pytestmark = pytest.mark.gpu
SEEDS = es.seeds()
NP = es.W * es.H
EXT_OPTS = {"sun_sampling": native.OPT_SUN_SAMPLING, "emitters": native.OPT_EMITTERS, "bsdf": native.OPT_BSDF, "nee": native.OPT_EMITTER_NEE}
# variant suffix -> (tree argument, entity phases): depth 6 has the generic walk, 7 the one-level form, 11 the two-level form
INSTANTIATIONS = {"": (-1, False), "_d7": (17, False), "_d11": (18, False),
                  "_entities": (-1, True), "_entities_d7": (17, True), "_entities_d11": (18, True)}
_want = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(instance, sc, opts, more=None):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    for k, v in opts.items():
        r.set_option(EXT_OPTS[k], v)
    for k, v in (more or {}).items():
        r.set_option(k, v)
    return loader, r


def want(port, name, key):
    """The specification's image of variant `name` under option set `key`, computed once."""
    if (name, key) not in _want:
        _want[name, key] = es.expected(port, name, es.OPTION_SETS[key][1])
        _want[name, key].setflags(write=False)
    return _want[name, key]


def assert_same(got, expected, what):
    same = (bits(got).reshape(-1, 3) == bits(expected).reshape(-1, 3)).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} pixels differ (first: pixel {int(np.argmin(same))})"


def check_info(r, tree, bvh):
    info = r.kernel_info()
    assert info["ext"] and info["tree"] == tree and info["bvh"] == bvh and not info["sorted"], info
    assert info["pool"] in ((16, 32) if bvh else (32,)), info


# ---- the emitter list ----
def list_from(loader, cap):
    n = C.c_int32(-1)
    out = np.full((max(cap, 1), 4), -7, np.int32)
    native.check(native.lib().chunky_scene_emitters(loader._h, out.ctypes.data if cap else None, cap, C.byref(n)))
    return out, n.value


def test_emitter_list_levels_caps_and_a_broken_block(gpu_instance, port):
    sc = es.make("exhibit")
    with PortExt(port, sc) as e:
        listed = e.emitters[:e.n_emitters].copy()
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    np.testing.assert_array_equal(loader.emitters(), listed)
    levels = (listed[:, 3] >> 25) & 15
    assert {k: int((levels == k).sum()) for k in range(3)} == es.expected_levels()
    _out, n = list_from(loader, 0)                    # cap 0: the count only
    assert n == len(listed)
    out, n = list_from(loader, 5)                     # a cap below the count: the first entries, nothing behind them
    assert n == len(listed)
    np.testing.assert_array_equal(out, listed[:5])
    out, n = list_from(loader, len(listed) + 3)
    np.testing.assert_array_equal(out[:n], listed)
    assert (out[n:] == -7).all()
    # the 4^3 block less one cell: the level-2 leaf becomes 7 level-1 and 7 level-0 leaves
    broken = es.make("exhibit_broken")
    tree = np.ascontiguousarray(broken.octree, np.int32)
    native.check(native.lib().chunky_scene_set_octree(loader._h, tree.ctypes.data, tree.size, int(broken.octree_depth)))
    with PortExt(port, broken) as e:
        after = e.emitters[:e.n_emitters].copy()
    np.testing.assert_array_equal(loader.emitters(), after)
    levels = (after[:, 3] >> 25) & 15
    assert {k: int((levels == k).sum()) for k in range(3)} == es.expected_levels(broken=True) and len(after) == len(listed) + 13
    # ... and the kernels sample the new list
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_EMITTER_NEE, 1)
    r.render_passes(SEEDS)
    check_info(r, -1, False)
    expected = es.expected(port, "exhibit_broken", dict(nee=1))
    assert_same(r.read(), expected, "after the octree update")
    assert not np.array_equal(bits(expected), bits(want(port, "exhibit", "nee")))
    r.close()
    loader.close()


# ---- option sets x instantiations ----
@pytest.mark.parametrize("suffix", list(INSTANTIATIONS), ids=[s.strip("_") or "plain" for s in INSTANTIATIONS])
@pytest.mark.parametrize("key", list(es.OPTION_SETS))
def test_option_sets_across_the_instantiations(gpu_instance, port, key, suffix):
    base, opts = es.OPTION_SETS[key]
    name = base + suffix
    sc = es.make(name)
    loader, r = make(gpu_instance, sc, opts)
    r.render_passes(SEEDS)
    check_info(r, *INSTANTIATIONS[suffix])
    expected = want(port, name, key)
    assert_same(r.read(), expected, f"{name} {key}")
    default = port.render_passes(sc, SEEDS)
    assert not np.array_equal(bits(default), bits(expected)), "the options changed nothing on this scene"
    if suffix.endswith(("_d7", "_d11")):              # the same world under more levels of air: the same image
        assert_same(expected, want(port, name.rsplit("_", 1)[0], key), f"{name} against its depth-6 twin")
    r.close()
    loader.close()


@pytest.mark.parametrize("key", list(es.OPTION_SETS))
def test_option_sets_on_a_projected_camera(gpu_instance, port, key):
    """proj::render_pool's extended twin (a fisheye camera), on the entity variant: the restatement on the equivalent ray tables."""
    base, opts = es.OPTION_SETS[key]
    sc = projected(es.make(base + "_entities"), native.PROJ_FISHEYE)
    loader, r = make(gpu_instance, sc, opts)
    r.render_passes(SEEDS)
    check_info(r, -1, True)
    with PortExt(port, sc, **opts):
        expected = equivalent(port, sc, SEEDS)
    assert_same(r.read(), expected, f"fisheye {key}")
    assert not np.array_equal(bits(equivalent(port, sc, SEEDS)), bits(expected)), "the options changed nothing on this view"
    r.close()
    loader.close()


# ---- edges of the vertex rule ----
@pytest.mark.parametrize("max_depth", [1, 2, 3])
def test_the_last_vertex_samples_no_emitter(gpu_instance, port, max_depth):
    """CHUNKY_OPT_MAX_DEPTH 1, 2, 3: at depth 1 no vertex samples the list at all (the image is the implicit one), from 2 on all but
    the last do."""
    name, opts = "exhibit_entities", dict(nee=1, bsdf=1)
    loader, r = make(gpu_instance, es.make(name), opts, {native.OPT_MAX_DEPTH: max_depth})
    r.render_passes(SEEDS)
    check_info(r, -1, True)
    expected = es.expected(port, name, opts, max_depth=max_depth)
    assert_same(r.read(), expected, f"max depth {max_depth}")
    implicit = es.expected(port, name, dict(bsdf=1), max_depth=max_depth)
    assert np.array_equal(bits(implicit), bits(expected)) == (max_depth == 1)
    r.close()
    loader.close()


def test_emitter_scale_and_bvh_cull(gpu_instance, port):
    name, opts = "exhibit_entities", dict(nee=1, bsdf=1)
    sc = es.make(name)
    loader, r = make(gpu_instance, sc, opts, {native.OPT_EMITTER_SCALE: 2.75})
    r.render_passes(SEEDS)
    check_info(r, -1, True)
    expected = es.expected(port, name, opts, emitter_scale=2.75)
    assert_same(r.read(), expected, "emitter scale 2.75")
    assert not np.array_equal(bits(expected), bits(want(port, name, "nee_bsdf")))
    r.set_option(native.OPT_EMITTER_SCALE, 13.0)
    r.set_option(native.OPT_BVH_CULL_BEHIND, 1)
    r.reset()
    r.render_passes(SEEDS)
    check_info(r, -1, True)
    with PortCull(port):
        culled = es.expected(port, name, opts)
    assert_same(r.read(), culled, "entity boxes behind the origin culled")
    assert_same(culled, want(port, name, "nee_bsdf"), "the cull changes no image")
    r.close()
    loader.close()


# ---- the same image by other routes ----
@pytest.mark.parametrize("world,tile", [(2, 0), (3, 7)], ids=["block_pair", "runs_of_7"])
def test_shards_give_the_same_image(gpu_instance, port, world, tile):
    name, key = "exhibit_entities", "nee_bsdf"
    sc = es.make(name)
    expected = want(port, name, key).reshape(NP, 3)
    ranks = range(world) if tile == 0 else (1,)
    seen = np.zeros(NP, bool)
    for rank in ranks:
        loader, r = make(gpu_instance, sc, es.OPTION_SETS[key][1])
        r.set_shard(rank, world, tile)
        r.render_passes(SEEDS)
        check_info(r, -1, True)
        got = r.read().reshape(NP, 3)
        own = parallel.owned_gids(NP, rank, world, tile, es.W)
        assert 0 < len(own) < NP
        assert_same(got[own], expected[own], f"rank {rank} of {world}, tile {tile}")
        rest = np.ones(NP, bool)
        rest[own] = False
        assert not got[rest].any(), "a pixel of another rank was written"
        seen[own] = True
        r.close()
        loader.close()
    assert seen.all() == (tile == 0)


def test_a_group_of_two_gives_the_same_image(port):
    name, key = "exhibit_entities", "nee_bsdf"
    group = RendererInstance.group([0, 0])
    try:
        assert group.group_size() == 2
        loader, r = make(group, es.make(name), es.OPTION_SETS[key][1])
        r.render_passes(SEEDS)
        info = r.kernel_info()
        assert info["ext"] and info["bvh"] and info["tree"] == -1, info
        assert_same(r.read(), want(port, name, key), "a group of two members on one device")
        r.close()
        loader.close()
    finally:
        group.close()


def test_the_pixel_list_route(gpu_instance, port):
    """chunky_selftest_render_list with a hand-made list: a permuted, ragged subset (331 pixels, no multiple of a tile), and a pixel
    twice is not in it."""
    name, key = "exhibit_entities_d11", "nee_bsdf"
    sc = es.make(name)
    listed = ((np.arange(331, dtype=np.int64) * 1013 + 77) % NP).astype(np.int32)
    assert len(set(listed.tolist())) == len(listed)
    loader, r = make(gpu_instance, sc, es.OPTION_SETS[key][1])
    r.render_list(listed, SEEDS)
    check_info(r, 18, True)
    got = r.read().reshape(NP, 3)
    with PortExt(port, sc, **es.OPTION_SETS[key][1]):
        expected = port.render_gids(sc, SEEDS, listed).reshape(NP, 3)
    assert_same(got[listed], expected[listed], "listed pixels")
    assert_same(expected[listed], want(port, name, key).reshape(NP, 3)[listed], "the list route's expectation against the whole image's")
    r.close()
    loader.close()


# ---- what would have caught the findings ----
def test_the_image_depends_on_level_bits_and_texture_orientation(gpu_instance, port):
    """The kernels' image is the specification's, and NOT the one of an emitter list without its level bits, nor the one of an
    emitter sample with tu / tv swapped (tests/test_ext_census_cpu.py test_mutated_expectations_differ: mutated copies of the
    inputs on the CPU, never the library)."""
    name, key = "exhibit", "nee"
    sc = es.make(name)
    loader, r = make(gpu_instance, sc, es.OPTION_SETS[key][1])
    r.render_passes(SEEDS)
    check_info(r, -1, False)
    got = r.read()
    assert_same(got, want(port, name, key), "the real expectation")
    listed = loader.emitters()
    flat = listed.copy()
    flat[:, 3] &= es.LEVEL_MASK
    twin, n = es.transposed_twin(listed)
    assert n == 5 and (flat[:, 3] != listed[:, 3]).sum() == 4
    for what, mutated in (("level bits masked off", flat), ("tu and tv swapped", twin)):
        other = es.expected(port, name, es.OPTION_SETS[key][1], emitters=mutated)
        assert not np.array_equal(bits(other), bits(got)), what
    r.close()
    loader.close()
