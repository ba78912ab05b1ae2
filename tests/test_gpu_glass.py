"""Translucent blocks on the GPU: chunky_render_passes on the six glass instantiations of render_pool against the
CPU specification tests/glass_port.c — bit for bit — with a census of every case's specification run, so that a case that no longer
reaches what it is meant to reach fails; shards, a canvas window, an external buffer, the feature off again, and the refusals."""
import dataclasses
import functools

import numpy as np
import pytest
import torch  # before the library loads: torch brings a HIP runtime of its own, and the second runtime of a process finds no device

import glass_spec
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader

pytestmark = pytest.mark.gpu

W, H = 96, 64
SEEDS = scenes.java_random_ints(6)
OPTS = {"sun_sampling": native.OPT_SUN_SAMPLING, "emitters": native.OPT_EMITTERS, "bsdf": native.OPT_BSDF, "nee": native.OPT_EMITTER_NEE}
ON = glass_spec.DEFAULT
ALWAYS = ("main_crossings", "reflect_vertices", "rm_skipped", "rm_resets")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu_instance, sc, glass=None, max_depth=5, **ext):
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    for k, v in ext.items():
        r.set_option(OPTS[k], v)
    if max_depth != 5:
        r.set_option(native.OPT_MAX_DEPTH, max_depth)
    if glass is not None:
        r.set_translucency(*glass)
    return loader, r


def close(r, loader):
    r.close()
    loader.close()


def glass_material(sc):
    """the material pointer of the greenhouse's 0x80 glass"""
    m = np.asarray(sc.material_palette).reshape(-1, 6)
    (k,) = np.nonzero(m[:, 3].astype(np.uint32) == 0x8030D040)
    return 6 * int(k[0])


def with_triangles(sc):
    """translucent entity triangles inside the room (world and actor BVHs)"""
    return scenes.add_entities(sc, 60, seed=4, actor_tris=24, region=((2, 4, 2), (19, 18, 19)), material=glass_material(sc))


def rays_from_inside(sc):
    """Pre-generated rays: most from the camera's position, every seventh origin inside a cell of the east window's glass, every eleventh
    inside the pool's water; directions of lengths 0.5 to 2."""
    rng = np.random.default_rng(23)
    n = W * H
    rays = np.zeros((n, 6), np.float32)
    rays[:, :3] = np.asarray(sc.camera[:3], np.float32)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3:] = d * rng.uniform(0.5, 2.0, size=(n, 1))
    glass = np.arange(0, n, 7)
    rays[glass, :3] = np.stack([21.0 + rng.uniform(0.1, 0.9, len(glass)), rng.integers(5, 11, len(glass)) + rng.uniform(0.1, 0.9, len(glass)),
                                rng.integers(4, 10, len(glass)) + rng.uniform(0.1, 0.9, len(glass))], axis=1)
    water = np.arange(3, n, 11)
    rays[water, :3] = np.stack([rng.integers(3, 9, len(water)) + rng.uniform(0.1, 0.9, len(water)), rng.integers(1, 3, len(water)) + rng.uniform(0.1, 0.9, len(water)),
                                rng.integers(11, 17, len(water)) + rng.uniform(0.1, 0.9, len(water))], axis=1)
    return rays


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, setting, extended options, max depth, (tree form, entity BVHs), the census entries the case must reach, those it must not)"""
    sc = scenes.greenhouse()
    if name == "default":
        return sc, ON, {}, 5, (-1, False), ALWAYS + ("sun_crossings",), ("emitter_crossings", "capped", "tri_crossings")
    if name == "bsdf_nee":             # lamps behind glass: emitter samples through the panes; the specular glass
        return sc, ON, dict(bsdf=1, nee=1), 5, (-1, False), ALWAYS + ("sun_crossings", "emitter_crossings"), ()
    if name == "sun_off":
        return sc, ON, dict(sun_sampling=0), 5, (-1, False), ALWAYS, ("sun_crossings", "emitter_crossings")
    if name == "cap_1":                # one crossing per ray: the second translucent hit is opaque
        return sc, (0.99, 1), {}, 5, (-1, False), ALWAYS + ("sun_crossings", "capped"), ()
    if name == "depth_1":
        return sc, ON, {}, 1, (-1, False), ALWAYS + ("sun_crossings",), ()
    if name == "depth_12":
        return sc, ON, dict(nee=1), 12, (-1, False), ALWAYS + ("sun_crossings", "emitter_crossings"), ()
    if name == "deeper_17":            # the room inside octrees two and six levels deeper: the dense tops
        return scenes.embed_deeper(sc, 7), ON, {}, 5, (17, False), ALWAYS + ("sun_crossings",), ()
    if name == "deeper_18":
        return scenes.embed_deeper(sc, 11), ON, dict(bsdf=1), 5, (18, False), ALWAYS + ("sun_crossings",), ()
    if name == "triangles":            # translucent entity triangles: the walk's hits are crossed, the run is left alone
        return with_triangles(sc), ON, dict(nee=1), 5, (-1, True), ALWAYS + ("sun_crossings", "emitter_crossings", "tri_crossings"), ()
    if name == "triangles_17":
        return with_triangles(scenes.embed_deeper(sc, 7)), ON, {}, 5, (17, True), ALWAYS + ("sun_crossings", "tri_crossings"), ()
    if name == "triangles_18":
        return with_triangles(scenes.embed_deeper(sc, 11)), (0.99, 2), dict(bsdf=1), 5, (18, True), ALWAYS + ("sun_crossings", "tri_crossings", "capped"), ()
    if name == "rays_inside":          # pre-generated rays, some origins inside glass and water cells
        return (sc.with_view(W, H, camera=rays_from_inside(sc).reshape(-1), projector_type=-1), ON, {}, 5, (-1, False), ALWAYS + ("sun_crossings",), ())
    raise KeyError(name)


CASES = ["default", "bsdf_nee", "sun_off", "cap_1", "depth_1", "depth_12", "deeper_17", "deeper_18", "triangles", "triangles_17", "triangles_18", "rays_inside"]


@functools.lru_cache(maxsize=None)
def spec(name):
    """the specification's image and census of a case, and the image with the feature off: computed once, never written to"""
    sc, glass, ext, max_depth, _, _, _ = case(name)
    want, census = glass_spec.render(sc, SEEDS, glass, ext=ext, max_depth=max_depth, census=True)
    opaque = glass_spec.render(sc, SEEDS, None, ext=ext, max_depth=max_depth)
    want.setflags(write=False)
    opaque.setflags(write=False)
    return want, census, opaque


def test_the_cases_cover_the_six_instantiations():
    assert {case(n)[4] for n in CASES} == {(t, b) for t in native.GLASS_POOL_FORMS for b in (False, True)}


@pytest.mark.parametrize("name", CASES)
def test_glass_kernels_match_the_specification(gpu_instance, name):
    sc, glass, ext, max_depth, (tree, bvh), reached, not_reached = case(name)
    want, census, opaque = spec(name)
    print(name, census)
    for k in reached:
        assert census[k] > 0, (k, census)
    for k in not_reached:
        assert census[k] == 0, (k, census)
    assert census["rehits"] <= 0.01 * census["crossings"], census
    loader, r = make(gpu_instance, sc, glass, max_depth, **ext)
    before = r.kernel_info()
    assert before["glass"] and before["blocks"] == 0 and (before["tree"], before["bvh"]) == (tree, bvh), before   # named before the first launch
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["glass"] and not info["ext"] and not info["biome"] and not info["fog"] and info["blocks"] > 0, info
    assert (info["tree"], info["bvh"], info["pool"]) == (tree, bvh, native.GLASS_POOL_BVH_PARK if bvh else native.GLASS_POOL_PARK), info
    got = r.read()
    np.testing.assert_array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(want), bits(opaque)), "the feature changed nothing on this scene"
    assert r.translucency() == {"enabled": True, "opaque_alpha": float(np.float32(glass[0])), "max_crossings": glass[1]}
    close(r, loader)


def test_block_shards_sum_to_the_whole_image(gpu_instance):
    sc, glass, ext, max_depth, _, _, _ = case("default")
    want = spec("default")[0]
    total = np.zeros_like(want)
    for rank in range(2):
        loader, r = make(gpu_instance, sc, glass, max_depth, **ext)
        r.set_shard(rank, 2, 0)
        r.render_passes(SEEDS)
        assert r.kernel_info()["glass"]
        part = r.read()
        assert part.any() and (bits(part) == 0).reshape(-1, 3).all(axis=1).any()
        total += part   # (every pixel is 0 on one of the two ranks: the sum is exact)
        close(r, loader)
    np.testing.assert_array_equal(bits(total), bits(want))


def test_a_canvas_window_is_the_crop(gpu_instance):
    sc, glass, ext, max_depth, _, _, _ = case("bsdf_nee")
    want = spec("bsdf_nee")[0].reshape(H, W, 3)
    x0, y0, w, h = 21, 9, 50, 37   # neither corner nor size on the 16 x 16 tile grid
    loader, r = make(gpu_instance, sc.with_view(w, h), glass, max_depth, **ext)
    r.set_canvas(W, H, x0, y0)
    r.render_passes(SEEDS)
    assert r.kernel_info()["glass"]
    np.testing.assert_array_equal(bits(r.read().reshape(h, w, 3)), bits(want[y0:y0 + h, x0:x0 + w]))
    close(r, loader)


def test_external_buffer_and_continued_passes(gpu_instance):
    """two calls continue one running mean, in a caller-owned device buffer"""
    sc, glass, ext, max_depth, _, _, _ = case("default")
    loader, r = make(gpu_instance, sc, glass, max_depth, **ext)
    buf = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.set_device_buffer(buf.data_ptr())
    r.render_passes(SEEDS[:2])
    r.render_passes(SEEDS[2:], first_buffer_spp=2)
    np.testing.assert_array_equal(bits(buf.cpu().numpy()), bits(spec("default")[0]))
    r.set_device_buffer(None)
    close(r, loader)


def test_off_again_is_the_parent(gpu_instance, port):
    sc, glass, ext, max_depth, _, _, _ = case("default")
    loader, r = make(gpu_instance, sc, glass, max_depth, **ext)
    r.render_passes(SEEDS)
    assert r.kernel_info()["glass"]
    r.set_translucency(None)
    assert not r.translucency()["enabled"]
    r.reset()
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert not info["glass"] and not info["ext"] and info["pool"] == 64 and info["tree"] == 16, info   # the plain kernel of this world again
    np.testing.assert_array_equal(bits(r.read()), bits(port.render_passes(sc, SEEDS)))
    np.testing.assert_array_equal(bits(r.read()), bits(spec("default")[2]))
    close(r, loader)


def refused(call):
    with pytest.raises(native.ChunkyHipError) as e:
        call()
    assert e.value.code == native.E_STATE, e.value
    return str(e.value)


def test_refusals_leave_the_target_alone(gpu_instance):
    sc, glass, ext, max_depth, _, _, _ = case("default")
    loader, r = make(gpu_instance, sc, glass, max_depth, **ext)
    r.render_passes(SEEDS[:2])
    image = r.read().copy()
    r.robust_begin(3)   # (state only: nothing is rendered)

    def unchanged():
        np.testing.assert_array_equal(bits(r.read()), bits(image))
        assert r.robust_bucket(0)[1] == 0

    assert "translucent" in refused(lambda: r.render_lights(SEEDS[:1]))
    unchanged()
    many = scenes.java_random_ints(32)   # (enough for the default min_spp: parameter errors come first)
    assert "translucent" in refused(lambda: r.render_adaptive(many))
    unchanged()
    assert "translucent" in refused(lambda: r.render_adaptive_ex(many))
    unchanged()
    assert "translucent" in refused(lambda: r.resume_adaptive(many))
    unchanged()
    assert "translucent" in refused(lambda: r.robust_passes(SEEDS[:1]))
    unchanged()
    assert "translucent" in refused(lambda: r.set_fog(0.05, 0.0, 16.0))
    assert r.fog()["density"] == 0.0
    r.set_fog(0.0)   # "off" is no layer: accepted
    unchanged()
    r.robust_begin(0)
    for word, text in ((1, "default kernel"), (2, "default kernel"), (8, "default kernel"), (4, "phase-statistics")):
        r.set_option(native.OPT_KERNEL, word)
        assert text in refused(lambda: r.render_passes(SEEDS[2:], first_buffer_spp=2))
        np.testing.assert_array_equal(bits(r.read()), bits(image))
    r.set_option(native.OPT_KERNEL, 0)
    r.set_option(native.OPT_MAX_DEPTH, 255)
    assert "max depth" in refused(lambda: r.render_passes(SEEDS[2:], first_buffer_spp=2))
    r.set_option(native.OPT_MAX_DEPTH, 5)
    fisheye = np.asarray(sc.camera, np.float32)[:15].copy()
    fisheye[12], fisheye[13], fisheye[14] = 0.0, 0.0, 180.0
    r.set_camera(native.PROJ_FISHEYE, fisheye)
    assert "projected cameras" in refused(lambda: r.render_passes(SEEDS[2:], first_buffer_spp=2))
    r.set_camera(sc.projector_type, sc.camera)
    # a fog layer set while translucency was off: the passes refuse the pair
    r.set_translucency(None)
    r.set_fog(0.05, 0.0, 16.0)
    r.set_translucency(*glass)
    assert "fog layer" in refused(lambda: r.render_passes(SEEDS[2:], first_buffer_spp=2))
    np.testing.assert_array_equal(bits(r.read()), bits(image))
    r.set_translucency(None)
    r.set_fog(0.0)
    r.set_translucency(*glass)
    loader.set_biome_tints(0, 0, np.full((8, 8, 3), 0x808080, np.int32))
    assert "biome map" in refused(lambda: r.render_passes(SEEDS[2:], first_buffer_spp=2))
    np.testing.assert_array_equal(bits(r.read()), bits(image))
    r.set_option(native.OPT_BIOME_TINT, 0)   # the target ignores the map: the glass kernels again, and the image goes on where it stopped
    r.render_passes(SEEDS[2:], first_buffer_spp=2)
    np.testing.assert_array_equal(bits(r.read()), bits(spec("default")[0]))
    # a setting the check refuses changes nothing
    for bad in ((0.0, 8), (0.99, 0), (0.99, 32), (float("nan"), 8)):
        with pytest.raises(native.ChunkyHipError) as e:
            r.set_translucency(*bad)
        assert e.value.code == native.E_INVALID
        assert r.translucency() == {"enabled": True, "opaque_alpha": float(np.float32(glass[0])), "max_crossings": glass[1]}
    close(r, loader)


def test_first_hit_passes_ignore_translucency(gpu_instance):
    """AOV, matte and occlusion passes treat every hit as opaque: the same images with the feature on and off."""
    sc, glass, ext, max_depth, _, _, _ = case("default")
    images = []
    for setting in (glass, None):
        loader, r = make(gpu_instance, sc, setting, max_depth, **ext)
        r.render_aov(SEEDS[:2])
        r.render_occlusion(SEEDS[:2], 6.0)
        r.render_matte(SEEDS[:2])
        images.append([r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL), r.read_occlusion(native.AOV_AO), *r.read_matte()[:2]])
        close(r, loader)
    for a, b in zip(*images):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
