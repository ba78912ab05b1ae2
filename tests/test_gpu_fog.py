"""The ground-fog layer on the GPU: chunky_render_passes on the six fog instantiations of render_pool against the
CPU specification tests/fog_port.c — bit for bit — with a census of every case's specification run, so that a case that no longer
reaches what it is meant to reach fails; shards, a canvas window, fog off again, and the refusals."""
import dataclasses
import functools

import numpy as np
import pytest
import torch  # before the library loads: torch brings a HIP runtime of its own, and the second runtime of a process finds no device

import fog_spec
import golden_scenes as gs
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader

pytestmark = pytest.mark.gpu

W, H = 96, 64
SEEDS = scenes.java_random_ints(6)
OPTS = {"sun_sampling": native.OPT_SUN_SAMPLING, "emitters": native.OPT_EMITTERS, "bsdf": native.OPT_BSDF, "nee": native.OPT_EMITTER_NEE}
BLUE = (0.7, 0.8, 1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu_instance, sc, fog=None, max_depth=5, **ext):
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    for k, v in ext.items():
        r.set_option(OPTS[k], v)
    if max_depth != 5:
        r.set_option(native.OPT_MAX_DEPTH, max_depth)
    if fog is not None:
        r.set_fog(*fog)
    return loader, r


def close(r, loader):
    r.close()
    loader.close()


def horizontal_rays(sc):
    """Pre-generated rays round sc's camera (golden_scenes.pregen_rays: lengths from 0.05 to 20, components that are exactly +-0, one
    origin in 16 above the octree) with every fifth direction exactly horizontal, alternately +0 and -0."""
    rays = gs.pregen_rays(sc, W, H, seed=41).reshape(-1, 6).copy()
    rays[::5, 4] = 0.0
    rays[2::10, 4] = -0.0
    return rays


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, fog layer, extended options, max depth, (tree form, entity BVHs), the census entries the case must reach, those it must not)"""
    if name == "outdoor":              # the slab lies over the terrain surface: medium and surface sun rays (every option at its default)
        return gs.make("outdoor").with_view(W, H), (0.06, 8.0, 40.0, BLUE), {}, 5, (-1, False), ("segments", "medium", "medium_sun", "surface_sun"), ("emitter",)
    if name == "outdoor_nosun":        # deep world: the one-level dense top
        return (gs.make("outdoor_nosun", gs.DEEP_CHUNKS).with_view(W, H), (0.05, 0.0, 48.0, (1.0, 1.0, 1.0)), dict(sun_sampling=1, bsdf=1), 5, (17, False),
                ("segments", "medium", "medium_sun", "surface_sun"), ())
    if name == "indoor_nee":           # emitter samples through the fog
        return gs.make("indoor").with_view(W, H), (0.08, 0.0, 32.0, (0.9, 0.9, 0.9)), dict(nee=1), 5, (-1, False), ("segments", "medium", "emitter"), ()
    if name == "indoor_sun_off":
        return gs.make("indoor").with_view(W, H), (0.08, 2.0, 9.0, (0.9, 0.9, 0.9)), dict(sun_sampling=0), 5, (-1, False), ("segments", "medium"), ("medium_sun", "surface_sun")
    if name == "entities":
        return (gs.make("entities").with_view(W, H), (0.05, 10.0, 44.0, BLUE), dict(bsdf=1, nee=1), 5, (-1, True),
                ("segments", "medium", "medium_sun", "surface_sun", "emitter"), ())
    if name == "entities_17":          # the entity world inside octrees one and five levels deeper: the dense tops with the BVH walk
        return scenes.embed_deeper(gs.make("entities"), 7).with_view(W, H), (0.05, 10.0, 44.0, BLUE), {}, 5, (17, True), ("segments", "medium", "medium_sun", "surface_sun"), ()
    if name == "entities_18":
        return gs.embedded("entities", 11).with_view(W, H), (0.05, 10.0, 44.0, BLUE), dict(nee=1), 5, (18, True), ("segments", "medium", "medium_sun", "emitter"), ()
    if name == "camera_inside":        # the camera stands in the slab
        return gs.make("inside").with_view(W, H), (0.1, 4.0, 14.0, BLUE), {}, 5, (-1, False), ("segments", "medium", "medium_sun", "surface_sun"), ()
    if name == "camera_above":         # ... and above it, looking down
        sc = gs.make("outdoor").with_view(W, H)
        return (dataclasses.replace(sc, camera=scenes.look_at_camera((16.0, 70.0, 16.0), (18.0, 0.0, 20.0), 70.0)), (0.1, 20.0, 45.0, BLUE), {}, 5, (-1, False),
                ("segments", "medium", "medium_sun", "surface_sun"), ())
    if name == "horizontal_rays":      # pre-generated rays: exactly horizontal directions inside and outside the slab, non-unit lengths
        sc = gs.make("outdoor").with_view(W, H)
        return (sc.with_view(W, H, camera=horizontal_rays(sc).reshape(-1), projector_type=-1), (0.05, 12.0, 60.0, BLUE), {}, 5, (-1, False),
                ("segments", "medium", "medium_sun", "parallel"), ())
    if name == "depth_12":             # a world five levels deeper: the two-level dense top; long paths
        return gs.embedded("outdoor", 11).with_view(W, H), (0.08, 0.0, 64.0, (1.0, 1.0, 1.0)), {}, 12, (18, False), ("segments", "medium", "medium_sun", "surface_sun"), ()
    if name == "depth_1":              # one vertex: a medium vertex ends the path behind its sun ray
        return gs.embedded("outdoor", 11).with_view(W, H), (0.08, 0.0, 64.0, (1.0, 1.0, 1.0)), {}, 1, (18, False), ("segments", "medium", "medium_sun", "surface_sun"), ()
    raise KeyError(name)


CASES = ["outdoor", "outdoor_nosun", "indoor_nee", "indoor_sun_off", "entities", "entities_17", "entities_18", "camera_inside", "camera_above",
         "horizontal_rays", "depth_12", "depth_1"]


@functools.lru_cache(maxsize=None)
def spec(name):
    """the specification's image and census of a case, and the image without the layer: computed once, never written to"""
    sc, fog, ext, max_depth, _, _, _ = case(name)
    want, census = fog_spec.render(sc, SEEDS, fog, ext=ext, max_depth=max_depth, census=True)
    clear = fog_spec.render(sc, SEEDS, (0.0, 0.0, 1.0, (0, 0, 0)), ext=ext, max_depth=max_depth)
    want.setflags(write=False)
    clear.setflags(write=False)
    return want, census, clear


def test_the_cases_cover_the_six_instantiations():
    assert {case(n)[4] for n in CASES} == {(t, b) for t in native.FOG_POOL_FORMS for b in (False, True)}


@pytest.mark.parametrize("name", CASES)
def test_fog_kernels_match_the_specification(gpu_instance, name):
    sc, fog, ext, max_depth, (tree, bvh), reached, not_reached = case(name)
    want, census, clear = spec(name)
    print(name, census)
    for k in reached:
        assert census[k] > 0, (k, census)
    for k in not_reached:
        assert census[k] == 0, (k, census)
    if name == "horizontal_rays":   # horizontal directions inside the slab and outside it, +0 and -0
        rays = np.asarray(sc.camera, np.float32).reshape(-1, 6)
        flat = rays[:, 4] == 0
        inside = (rays[:, 1] >= fog[1]) & (rays[:, 1] < fog[2])
        assert (flat & inside).sum() > 50 and (flat & ~inside).sum() > 50 and np.signbit(rays[flat, 4]).any() and not np.signbit(rays[flat, 4]).all()
        assert census["parallel"] >= len(SEEDS) * flat.sum()
    loader, r = make(gpu_instance, sc, fog, max_depth, **ext)
    before = r.kernel_info()
    assert before["fog"] and before["blocks"] == 0 and (before["tree"], before["bvh"]) == (tree, bvh), before   # named before the first launch
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["fog"] and not info["ext"] and not info["biome"] and info["blocks"] > 0, info
    assert (info["tree"], info["bvh"], info["pool"]) == (tree, bvh, native.FOG_POOL_BVH_PARK if bvh else native.FOG_POOL_PARK), info
    got = r.read()
    np.testing.assert_array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(want), bits(clear)), "the layer changed nothing on this scene"
    assert r.fog() == {"density": np.float32(fog[0]), "y_min": fog[1], "y_max": fog[2], "color": tuple(float(np.float32(c)) for c in fog[3])}
    close(r, loader)


def test_block_shards_sum_to_the_whole_image(gpu_instance):
    sc, fog, ext, max_depth, _, _, _ = case("outdoor")
    want = spec("outdoor")[0]
    total = np.zeros_like(want)
    for rank in range(2):
        loader, r = make(gpu_instance, sc, fog, max_depth, **ext)
        r.set_shard(rank, 2, 0)
        r.render_passes(SEEDS)
        assert r.kernel_info()["fog"]
        part = r.read()
        assert part.any() and (bits(part) == 0).reshape(-1, 3).all(axis=1).any()
        total += part   # (every pixel is 0 on one of the two ranks: the sum is exact)
        close(r, loader)
    np.testing.assert_array_equal(bits(total), bits(want))


def test_a_canvas_window_is_the_crop(gpu_instance):
    sc, fog, ext, max_depth, _, _, _ = case("camera_inside")
    want = spec("camera_inside")[0].reshape(H, W, 3)
    x0, y0, w, h = 21, 9, 50, 37   # neither corner nor size on the 16 x 16 tile grid
    loader, r = make(gpu_instance, sc.with_view(w, h), fog, max_depth, **ext)
    r.set_canvas(W, H, x0, y0)
    r.render_passes(SEEDS)
    assert r.kernel_info()["fog"]
    np.testing.assert_array_equal(bits(r.read().reshape(h, w, 3)), bits(want[y0:y0 + h, x0:x0 + w]))
    close(r, loader)


def test_external_buffer_and_continued_passes(gpu_instance):
    """two calls continue one running mean, in a caller-owned device buffer"""
    sc, fog, ext, max_depth, _, _, _ = case("outdoor")
    loader, r = make(gpu_instance, sc, fog, max_depth, **ext)
    buf = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.set_device_buffer(buf.data_ptr())
    r.render_passes(SEEDS[:2])
    r.render_passes(SEEDS[2:], first_buffer_spp=2)
    np.testing.assert_array_equal(bits(buf.cpu().numpy()), bits(spec("outdoor")[0]))
    r.set_device_buffer(None)
    close(r, loader)


def test_fog_off_again_is_the_parent(gpu_instance, port):
    sc, fog, ext, max_depth, _, _, _ = case("outdoor")
    loader, r = make(gpu_instance, sc, fog, max_depth, **ext)
    r.render_passes(SEEDS)
    assert r.kernel_info()["fog"]
    r.set_fog(0.0)
    assert r.fog()["density"] == 0.0
    r.reset()
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert not info["fog"] and not info["ext"] and info["pool"] == 64 and info["tree"] == 16, info   # the plain kernel of this world again
    np.testing.assert_array_equal(bits(r.read()), bits(port.render_passes(sc, SEEDS)))
    close(r, loader)


def refused(call):
    with pytest.raises(native.ChunkyHipError) as e:
        call()
    assert e.value.code == native.E_STATE, e.value
    return str(e.value)


def test_refusals_leave_the_target_alone(gpu_instance):
    sc, fog, ext, max_depth, _, _, _ = case("outdoor")
    loader, r = make(gpu_instance, sc, fog, max_depth, **ext)
    r.render_passes(SEEDS[:2])
    image = r.read().copy()
    r.robust_begin(3)   # (state only: nothing is rendered)

    def unchanged():
        np.testing.assert_array_equal(bits(r.read()), bits(image))
        assert r.robust_bucket(0)[1] == 0

    assert "fog" in refused(lambda: r.render_lights(SEEDS[:1]))
    unchanged()
    many = scenes.java_random_ints(32)   # (enough for the default min_spp: parameter errors come first)
    assert "fog" in refused(lambda: r.render_adaptive(many))
    unchanged()
    assert "fog" in refused(lambda: r.render_adaptive_ex(many))
    unchanged()
    assert "fog" in refused(lambda: r.resume_adaptive(many))
    unchanged()
    assert "fog" in refused(lambda: r.robust_passes(SEEDS[:1]))
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
    loader.set_biome_tints(0, 0, np.full((8, 8, 3), 0x808080, np.int32))
    assert "biome map" in refused(lambda: r.render_passes(SEEDS[2:], first_buffer_spp=2))
    np.testing.assert_array_equal(bits(r.read()), bits(image))
    r.set_option(native.OPT_BIOME_TINT, 0)   # the target ignores the map: the fog kernels again, and the image goes on where it stopped
    r.render_passes(SEEDS[2:], first_buffer_spp=2)
    np.testing.assert_array_equal(bits(r.read()), bits(spec("outdoor")[0]))
    # a layer the check refuses changes nothing
    with pytest.raises(native.ChunkyHipError) as e:
        r.set_fog(0.1, 5.0, 5.0)
    assert e.value.code == native.E_INVALID
    assert r.fog()["density"] == np.float32(fog[0])
    close(r, loader)


def test_first_hit_passes_ignore_fog(gpu_instance):
    """AOV, matte and occlusion passes see the world in clear air: the same images with the layer and without it."""
    sc, fog, ext, max_depth, _, _, _ = case("outdoor")
    images = []
    for layer in (fog, None):
        loader, r = make(gpu_instance, sc, layer, max_depth, **ext)
        r.render_aov(SEEDS[:2])
        r.render_occlusion(SEEDS[:2], 6.0)
        r.render_matte(SEEDS[:2])
        images.append([r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL), r.read_occlusion(native.AOV_AO), *r.read_matte()[:2]])
        close(r, loader)
    for a, b in zip(*images):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
