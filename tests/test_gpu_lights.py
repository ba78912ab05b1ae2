"""chunky_render_light_passes / _read / _mix (csrc/lights.hip) on the device, bit for bit against the specification on the C
restatement of the reference (lights_spec.expected_lights: a group image is the oracle's image with the other two scalars at zero;
tests/test_lights_cpu.py shows what that means): the golden scenes whole, ALL against the target's own beauty image, path depths,
emitter scales, the BVH cull option, every tree form, a projected camera with a lens, split calls and the launch cut, shards, a group,
scene updates, the refusal of the extended options, the isolation from every other image of the target, the device mix, and the ABI's
errors.  Every comparison is over every pixel and every channel, without tolerance."""
import dataclasses

import numpy as np
import pytest

import golden_scenes as gs
from lights_spec import IMAGES, WHICH, expected_lights
from chunkyclplugin_amd import native
from chunkyclplugin_amd.native import ChunkyHipError, check, ptr
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays
from chunkyclplugin_amd.scenes import f2i
from test_camera_lens_ods_cpu import GPU_LENS, projected

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(gs.N_PASSES)
WHOLE = ["outdoor", "outdoor_nosun", "entities", "dof", "pregen", "inside", "indoor_sun", "water"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(instance, sc, lens=None):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    if lens is not None:
        r.set_lens(*lens)
    return loader, r


def close(*xs):
    for x in xs:
        x.close()


def images(r):
    """{"sky", "sun", "emitters", "all"}: (3 * pixels,) float32 as chunky_render_light_read delivers them"""
    out = {k: r.read_light(WHICH[k]).reshape(-1) for k in IMAGES}
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def assert_same(got, want, what, keep=None):
    """every float of every image; `keep`: a mask over pixels"""
    for k in IMAGES:
        g, w = bits(got[k]).reshape(-1, 3), bits(want[k]).reshape(-1, 3)
        if keep is not None:
            g, w = g[keep], w[keep]
        same = (g == w).all(axis=1)
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what}: {k} differs at {int((~same).sum())} of {len(same)} pixels (first at row {i}: "
                        f"{g[i].view(np.float32).tolist()!r} against {w[i].view(np.float32).tolist()!r})")


@pytest.fixture(scope="module")
def golden(port):
    """The four images of the golden scenes for SEEDS on the oracle, computed once per (scene, options) and never changed."""
    cache = {}

    def get(name, **options):
        key = (name, tuple(sorted(options.items())))
        if key not in cache:
            img = expected_lights(port, gs.make(name), SEEDS, **options)
            for v in img.values():
                v.setflags(write=False)
            cache[key] = img
        return cache[key]
    return get


@pytest.mark.parametrize("name", WHOLE)
def test_golden_scene_whole_images(gpu_instance, golden, name):
    """Sun on and off (both RNG orders), the BVH walk, lens draws before the sun draws, pre-generated rays, a closed room."""
    sc = gs.make(name)
    loader, r = make(gpu_instance, sc)
    r.render_lights(SEEDS)
    got = images(r)
    assert_same(got, golden(name), name)
    info = r.lights_info()
    assert info["launches"] == 1 and info["bvh"] == (name == "entities"), info
    assert r.lights_time()[1] == 1
    assert got["all"].any()
    if name == "outdoor_nosun":
        assert not bits(got["sun"]).any()
    close(r, loader)


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun", "dof"])
def test_all_is_the_beauty_image(gpu_instance, name):
    """ALL against the target's own chunky_render_passes for the same seeds: the new kernel tied to the one every other test pins."""
    loader, r = make(gpu_instance, gs.make(name))
    r.render_passes(SEEDS)
    r.render_lights(SEEDS)
    beauty, light = r.read(), r.read_light(native.LIGHT_ALL).reshape(-1)
    assert beauty.any()
    assert bits(beauty).tobytes() == bits(light).tobytes()
    close(r, loader)


@pytest.mark.parametrize("depth", [1, 2, 8])
def test_max_depth(gpu_instance, golden, depth):
    loader, r = make(gpu_instance, gs.make("outdoor"))
    r.set_option(native.OPT_MAX_DEPTH, depth)
    r.render_lights(SEEDS)
    assert_same(images(r), golden("outdoor", max_depth=depth), f"outdoor, max depth {depth}")
    close(r, loader)


@pytest.mark.parametrize("scale", [2.75, 0.0])
def test_emitter_scale(gpu_instance, golden, scale):
    loader, r = make(gpu_instance, gs.make("indoor_sun"))
    r.set_option(native.OPT_EMITTER_SCALE, scale)
    r.render_lights(SEEDS)
    got = images(r)
    assert_same(got, golden("indoor_sun", emitter_scale=scale), f"indoor_sun, emitter scale {scale}")
    assert got["emitters"].any() == (scale != 0)
    close(r, loader)


def test_bvh_cull_option(gpu_instance, golden):
    loader, r = make(gpu_instance, gs.make("entities"))
    r.set_option(native.OPT_BVH_CULL_BEHIND, 1)
    r.render_lights(SEEDS)
    assert r.lights_info()["bvh"]
    assert_same(images(r), golden("entities", cull=True), "entities, BVH cull")
    close(r, loader)


FORM_CASES = list(gs.form_cases(ragged=True))


@pytest.mark.parametrize("key,build,kernel", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_tree_forms(gpu_instance, port, key, build, kernel):
    """The lookup forms 17 / 18 / 19 / 0 and the entity form 18 with the walk, whole images; the form-19 case at 33 x 17."""
    sc = build()
    loader, r = make(gpu_instance, sc)
    r.render_lights(SEEDS)
    info = r.lights_info()
    assert (info["tree"], info["bvh"]) == kernel, info
    if (sc.width, sc.height) == gs.RAGGED_VIEW:
        assert info["blocks"] == 6   # 24 claims, one per wave of four-wave workgroups: the grid cap, not the device's size
    assert_same(images(r), expected_lights(port, sc, SEEDS), key)
    close(r, loader)


def test_projected_camera_with_a_lens(gpu_instance, port):
    """A pass of a projected camera is the pass on the table of its rays, with the lens as without."""
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind]
    loader, r = make(gpu_instance, sc, lens)
    r.render_lights(SEEDS)
    want = None
    for i, seed in enumerate(SEEDS):
        table = dataclasses.replace(sc, camera=camera_rays(kind, sc.camera, sc.width, sc.height, int(seed), lens), projector_type=-1)
        want = expected_lights(port, table, [seed], first_spp=i, init=want)
    assert_same(images(r), want, "fisheye with a lens")
    assert want["sky"].any() and want["sun"].any() and want["emitters"].any()
    close(r, loader)


def test_two_calls_equal_one(gpu_instance, golden):
    loader, r = make(gpu_instance, gs.make("entities"))
    r.render_lights(SEEDS[:2])
    r.render_lights(SEEDS[2:], first_buffer_spp=2)
    assert_same(images(r), golden("entities"), "2 + 1 passes")
    close(r, loader)


def test_launch_cut_is_invisible(gpu_instance, port):
    sc = gs.make("outdoor").with_view(8, 8)
    seeds = native.java_random_ints(300)
    loader, r = make(gpu_instance, sc)
    r.render_lights(seeds)
    assert r.lights_info()["launches"] == 2  # 256 + 44
    assert r.lights_time()[1] == 2
    got = images(r)
    assert_same(got, expected_lights(port, sc, seeds), "300 passes")
    r.reset_lights()
    r.render_lights(seeds[:100])
    r.render_lights(seeds[100:], first_buffer_spp=100)
    assert r.lights_info()["launches"] == 1
    assert_same(images(r), got, "100 + 200 passes")
    close(r, loader)


def test_first_buffer_spp(gpu_instance, port):
    """The running means continue from whatever the images hold: spp = 7 weighs the (zero) images seven times."""
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    r.render_lights(SEEDS, first_buffer_spp=7)
    assert_same(images(r), expected_lights(port, sc, SEEDS, first_spp=7), "first_buffer_spp 7")
    close(r, loader)


def owner(sc, world, tile):
    gid = np.arange(sc.width * sc.height)
    if tile > 0:
        return (gid // tile) % world
    bw = (sc.width + 15) // 16
    return ((gid // sc.width // 16) * bw + (gid % sc.width) // 16) % world


@pytest.mark.parametrize("tile", [0, 7])
def test_shards(gpu_instance, golden, tile):
    """Block shards (tile 0) and run shards of 7 pixels: each rank's pixels are the whole image's, every other word stays 0."""
    sc = gs.make("entities")
    want = golden("entities")
    for rank in range(3):
        loader, r = make(gpu_instance, sc)
        r.set_shard(rank, 3, tile)
        r.render_lights(SEEDS)
        got = images(r)
        mine = owner(sc, 3, tile) == rank
        assert mine.any() and not mine.all()
        assert_same(got, want, f"rank {rank} of 3, tile {tile}", keep=mine)
        for k in IMAGES:
            assert not bits(got[k]).reshape(-1, 3)[~mine].any(), k
        close(r, loader)


def test_group_equals_one_context(gpu_instance, golden):
    g = RendererInstance.group([0, 0])
    sc = gs.make("entities")
    lg, rg = make(g, sc)
    rg.render_lights(SEEDS[:2])
    rg.render_lights(SEEDS[2:], first_buffer_spp=2)
    assert_same(images(rg), golden("entities"), "a two-member group")
    info = rg.lights_info()
    assert info["bvh"] and info["launches"] == 1, info
    assert rg.lights_time()[1] == 2
    mixed = rg.mix_lights([1, 1, 1]).reshape(-1)
    assert mixed.any()
    rg.reset_lights()
    assert not any(bits(v).any() for v in images(rg).values())
    close(rg, lg, g)


def with_sun_intensity(sc, factor):
    sun = np.array(sc.sun, np.int32)
    sun[3] = f2i(float(np.float32(factor) * sun[3:4].view(np.float32)[0]))
    return dataclasses.replace(sc, sun=sun)


UPDATES = {
    "sky intensity": lambda sc: dataclasses.replace(sc, sky_intensity=float(np.float32(0.37) * np.float32(sc.sky_intensity))),
    "sun intensity": lambda sc: with_sun_intensity(sc, 1.7),
    "sun flag cleared": lambda sc: dataclasses.replace(sc, sun=gs.make("outdoor_nosun").sun),
}


@pytest.mark.parametrize("what", sorted(UPDATES))
def test_scene_update_takes_effect_in_the_next_call(gpu_instance, port, golden, what):
    """chunky_scene_set_sky / _set_sun between two calls: the next call renders the new scene, as a fresh upload of it does."""
    before = gs.make("outdoor")
    after = UPDATES[what](before)
    loader, r = make(gpu_instance, before)
    r.render_lights(SEEDS)
    assert_same(images(r), golden("outdoor"), "before the update")
    if what == "sky intensity":
        sky = np.ascontiguousarray(after.sky, np.uint8)
        check(native.lib().chunky_scene_set_sky(loader._h, ptr(sky), sky.shape[1], sky.shape[0], float(after.sky_intensity)))
    else:
        s = np.ascontiguousarray(after.sun, np.int32)
        check(native.lib().chunky_scene_set_sun(loader._h, ptr(s)))
    r.reset_lights()
    r.render_lights(SEEDS)
    got = images(r)
    lf, fresh = make(gpu_instance, after)
    fresh.render_lights(SEEDS)
    assert_same(got, images(fresh), f"after {what}, against a fresh upload")
    want = expected_lights(port, after, SEEDS)
    assert_same(got, want, f"after {what}, against the specification")
    changed = {"sky intensity": "sky", "sun intensity": "sun", "sun flag cleared": "sun"}[what]
    assert bits(want[changed]).tobytes() != bits(golden("outdoor")[changed]).tobytes()
    close(r, loader, fresh, lf)


@pytest.mark.parametrize("option,value", [(native.OPT_SUN_SAMPLING, 0), (native.OPT_SUN_SAMPLING, 1), (native.OPT_EMITTERS, 0), (native.OPT_BSDF, 1),
                                          (native.OPT_EMITTER_NEE, 1)], ids=["sun-never", "sun-always", "emitters-off", "bsdf", "nee"])
def test_extended_options_are_refused(gpu_instance, option, value):
    """They change what the beauty image is and the pass does not implement them: CHUNKY_E_STATE, nothing rendered, nothing allocated."""
    loader, r = make(gpu_instance, gs.make("outdoor"))
    r.set_option(option, value)
    with pytest.raises(ChunkyHipError) as e:
        r.render_lights(SEEDS)
    assert e.value.code == native.E_STATE
    with pytest.raises(ChunkyHipError) as e:
        r.read_light(native.LIGHT_ALL)
    assert e.value.code == native.E_STATE            # a refused call allocates nothing
    r.set_option(option, -1 if option == native.OPT_SUN_SAMPLING else 1 - value)
    r.render_lights(SEEDS[:1])                       # back at the default: accepted
    assert r.read_light(native.LIGHT_ALL).any()
    close(r, loader)


def other_state(r):
    """every image of the target the light calls must not touch, as bytes"""
    out = {"beauty": r.read().tobytes()}
    for which in range(native.AOV_BLOCK + 1):
        out[f"aov {which}"] = r.read_aov_ex(which).tobytes()
    ids, counts, other, passes = r.read_matte()
    out.update({"matte ids": ids.tobytes(), "matte counts": counts.tobytes(), "matte other": other.tobytes(), "matte passes": passes})
    for which in (native.AOV_AO, native.AOV_SUN):
        out[f"occlusion {which}"] = r.read_occlusion(which).tobytes()
    return out


def other_launches(r):
    return (r.kernel_time()[1], r.aov_kernel_time()[1], r.matte_kernel_time()[1], r.occlusion_time()[1])


def test_isolation(gpu_instance):
    sc = gs.make("entities")
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    r.render_aov_ex(SEEDS)
    r.render_matte(SEEDS)
    r.render_occlusion(SEEDS, 4.0)
    before = other_state(r)
    assert min(other_launches(r)) >= 1
    r.render_lights(SEEDS)
    r.mix_lights([1, 2, 3])
    assert other_state(r) == before
    assert other_launches(r) == (0, 0, 0, 0)   # (drained above: no other timer saw the launches)
    assert r.lights_time()[1] == 1
    held = {k: bits(v).tobytes() for k, v in images(r).items()}
    assert all(np.frombuffer(v, np.uint32).any() for v in held.values())
    # the other passes and every other reset leave the four images alone, and the light timer sees none of their launches
    r.reset_aov()
    r.reset_matte()
    r.reset_occlusion()
    r.reset()
    r.render_passes(SEEDS)
    r.render_aov_ex(SEEDS)
    r.render_matte(SEEDS)
    r.render_occlusion(SEEDS, 4.0)
    assert {k: bits(v).tobytes() for k, v in images(r).items()} == held
    assert r.lights_time()[1] == 0
    assert other_state(r) == before            # ... and they render what they rendered without a light pass in between
    r.reset_lights()
    assert not any(bits(v).any() for v in images(r).values())
    assert other_state(r) == before
    close(r, loader)


@pytest.mark.parametrize("weights", [(1, 1, 1), (0.5, 2, 0), (0, 0, 3)], ids=["sum", "regrade", "emitters-only"])
def test_light_mix(gpu_instance, weights):
    """(w0 * SKY + w1 * SUN) + w2 * EMITTERS per float in float32, each operation rounded once."""
    loader, r = make(gpu_instance, gs.make("indoor_sun"))
    r.render_lights(SEEDS)
    img = images(r)
    w = np.asarray(weights, np.float32)
    want = (w[0] * img["sky"] + w[1] * img["sun"]) + w[2] * img["emitters"]
    assert want.dtype == np.float32 and want.any()
    got = r.mix_lights(weights)
    assert got.shape == (gs.H, gs.W, 3) and got.dtype == np.float32
    assert bits(got.reshape(-1)).tobytes() == bits(want).tobytes()
    assert_same(images(r), img, "the mix changes no image")
    close(r, loader)


def test_abi_errors_on_a_device(gpu_instance):
    L = native.lib()
    sc = gs.make("outdoor")
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    seeds = native.java_random_ints(2)
    n = 3 * sc.width * sc.height
    out = np.zeros(n, np.float32)
    w = np.ones(3, np.float32)
    info = np.zeros(4, np.int32)
    assert L.chunky_render_light_passes(r._h, seeds.ctypes.data, 2, 0) == native.E_STATE   # before set_camera
    r.set_camera(sc.projector_type, sc.camera)
    for which in range(4):
        assert L.chunky_render_light_read(r._h, which, out.ctypes.data, n) == native.E_STATE      # before the first pass
    assert L.chunky_render_light_mix(r._h, w.ctypes.data, out.ctypes.data, n) == native.E_STATE   # nothing to mix
    assert L.chunky_render_light_reset(r._h) == 0                                                 # (nothing to zero)
    assert L.chunky_render_light_passes(r._h, seeds.ctypes.data, -1, 0) == native.E_INVALID
    assert L.chunky_render_light_passes(r._h, None, 2, 0) == native.E_INVALID
    assert L.chunky_render_light_passes(r._h, seeds.ctypes.data, 2, -3) == native.E_INVALID
    assert L.chunky_render_light_read(r._h, native.LIGHT_ALL, out.ctypes.data, n) == native.E_STATE   # a refused call allocates nothing
    assert L.chunky_render_light_passes(r._h, None, 0, 0) == 0                                    # n == 0: allocates the images
    assert r.lights_info()["launches"] == 0 and r.lights_time()[1] == 0
    for which in range(4):
        out[:] = 1
        assert L.chunky_render_light_read(r._h, which, out.ctypes.data, n) == 0 and not out.any()
    out[:] = 1
    assert L.chunky_render_light_mix(r._h, w.ctypes.data, out.ctypes.data, n) == 0 and not out.any()
    for which in (-1, 4, native.AOV_AO):
        assert L.chunky_render_light_read(r._h, which, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_light_read(r._h, native.LIGHT_SKY, out.ctypes.data, n - 1) == native.E_INVALID
    assert L.chunky_render_light_read(r._h, native.LIGHT_SKY, out.ctypes.data, n // 3) == native.E_INVALID
    assert L.chunky_render_light_read(r._h, native.LIGHT_SKY, None, n) == native.E_INVALID
    assert L.chunky_render_light_mix(r._h, None, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_light_mix(r._h, w.ctypes.data, None, n) == native.E_INVALID
    assert L.chunky_render_light_mix(r._h, w.ctypes.data, out.ctypes.data, n - 3) == native.E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for i in range(3):
            wb = np.ones(3, np.float32)
            wb[i] = bad
            assert L.chunky_render_light_mix(r._h, wb.ctypes.data, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_light_kernel_info(r._h, None) == native.E_INVALID
    r.render_lights(seeds)
    held = images(r)
    assert L.chunky_render_light_passes(r._h, None, 0, 2) == 0                                    # n == 0 changes nothing
    assert all(bits(images(r)[k]).tobytes() == bits(held[k]).tobytes() for k in IMAGES)
    assert L.chunky_render_light_kernel_info(r._h, info.ctypes.data) == 0 and info[3] == 0
    close(r, loader)
