"""Device code takes `1.0f / x` in a short form (csrc/rt_short_forms.h): rcp3 in trace_setup and octree_hit, the reciprocal lengths of
the sampling block, of cosine_direction and of normalize (rt_rlen3), the emitter sampling's 1 / distance.
tests/test_gpu_exact_divsqrt.py holds the form equal to the division for every float; here the kernels that were compiled with it give
port.c's image (`port.render_gids`), every pixel bit for bit, at the shapes of tests/test_gpu_shade_round_trips.py: 33 x 17, a small
outdoor world in a depth-7 octree so that the tree form is the timed one (17).

  kernel forms   render_pool<17, 64> with the sun on and off, its sorted instantiation, no parked paths, entity BVHs, the extended
                 integrator, a projected camera (proj::render_pool: chosen by the projector type alone, launch_pool; kernel_info
                 has no field that says which copy of the kernel's text ran)
  fallback       render_waves and render_lanes: they share rcp3, octree_hit and rt_rlen3
  passes         1, 5 and 64 per launch, and a second launch on top of the first
  cameras        pinhole, an aperture, pre-generated rays
  the ray table  golden_scenes.pregen_rays has direction components that are exactly +0 and -0; `edge_rays` adds denormal ones and
                 2^-127, of both signs, each in one lane among ordinary lanes: a wave that holds one takes the compiler's division
                 for all of its lanes, the others the short form, and the march's -0 guard (inv = -inf) sees the reciprocals it
                 always saw."""
import dataclasses
import functools

import numpy as np
import pytest

import golden_scenes as gs
from oracle import binding
from oracle.binding import PortExt

from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, camera_rays

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
W, H = 33, 17
N_PIXELS = W * H
SEEDS = native.java_random_ints(5 + 64, seed=7303)
ALL = np.arange(N_PIXELS, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def scene(sun=True):
    sc = scenes.outdoor_world(chunks=4, height=64, emitters=0.02, width=W, img_height=H, sun_flag=sun)
    assert sc.octree_depth == 6
    return scenes.embed_deeper(sc, 7)


def edge_rays(sc):
    """pregen_rays' table with, in addition to its exact zeros, a direction component per listed pixel that is denormal (2^-127 among
    them) or the smallest normal number — the inputs rcp3's range test sends to the compiler's division, and the first it does not.
    The pixels are spread so that they stand alone among ordinary pixels (no two within a 2 x 2 sub-block, several tiles)."""
    rays = gs.pregen_rays(sc, W, H, seed=43).reshape(-1, 6).copy()
    d = rays[:, 3:].view(np.uint32)
    edge = {3: (0, 0x00000001), 40: (1, 0x80000001), 77: (2, 0x007FFFFF), 118: (0, 0x807FFFFF), 155: (2, 0x00400000),   # denormals; 2^-127
            196: (0, 0x80400000), 233: (1, 0x00400000), 270: (0, 0x00000123), 311: (2, 0x80012345), 352: (0, 0x00800000),  # ... and 2^-126
            389: (2, 0x80000000), 430: (0, 0x00000000), 467: (1, 0x00000123), 508: (2, 0x00400000), 545: (0, 0x80800000)}
    for pixel, (axis, pattern) in edge.items():
        d[pixel, axis] = pattern
    table = rays.reshape(-1)
    zeros = (table.reshape(-1, 6)[:, 3:] == 0).sum()
    assert zeros >= 20 and np.signbit(table[table == 0]).any() and not np.signbit(table[table == 0]).all()
    return table


@functools.lru_cache(maxsize=None)
def camera_scene(kind):
    sc = scene(True)
    if kind == "pinhole":
        return sc
    if kind == "aperture":
        return gs.with_dof(sc, 0.08, 18.0)
    if kind == "pregenerated":
        return sc.with_view(W, H, camera=edge_rays(sc), projector_type=native.PROJ_PREGENERATED)
    cam = np.asarray(sc.camera, np.float32)[:15].copy()   # the pinhole camera's position and rotation as a 180-degree fisheye
    cam[12], cam[13], cam[14] = 0.0, 0.0, 180.0
    return dataclasses.replace(sc, camera=cam, projector_type=native.PROJ_FISHEYE)


def oracle(sc, seeds, first_spp=0, res=None):
    port = binding.port()
    if sc.projector_type <= 0:
        return port.render_gids(sc, seeds, ALL, first_spp=first_spp, res=res, threads=THREADS)
    res = np.zeros(3 * N_PIXELS, np.float32) if res is None else res
    for i, seed in enumerate(seeds):
        table = dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, W, H, int(seed)), projector_type=native.PROJ_PREGENERATED)
        port.render_gids(table, np.array([seed], np.int32), ALL, first_spp=first_spp + i, res=res, threads=THREADS)
    return res


@functools.lru_cache(maxsize=None)
def oracle_image(sun, passes, kind="pinhole"):
    """computed once, shared, read-only"""
    img = oracle(scene(sun) if kind == "pinhole" else camera_scene(kind), SEEDS[:passes])
    img.setflags(write=False)
    return img


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 3)


def assert_same(got, want, what):
    same = (bits(got) == bits(want)).all(axis=1)
    if not same.all():
        i = int(np.argmin(same))
        pytest.fail(f"{what}: {int((~same).sum())} of {len(same)} pixels differ from the oracle; first: pixel {i} got {bits(got)[i]!r} want {bits(want)[i]!r}")


def make(gpu_instance, sc, variant=0, options=()):
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    for k, v in options:
        r.set_option(k, v)
    return loader, r


def timed_kernel(info):
    return (info["tree"], info["pool"], info["bvh"], info["ext"]) == (17, 64, False, False)


@pytest.mark.parametrize("passes", [1, 5, 64])
@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_timed_kernel(gpu_instance, sun, passes):
    loader, r = make(gpu_instance, scene(sun))
    r.render_passes(SEEDS[:passes])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), oracle_image(sun, passes), f"sun {sun}, {passes} passes")
    r.close()
    loader.close()


def test_second_launch_on_top(gpu_instance):
    sc = scene(True)
    want = oracle(sc, SEEDS[5:5 + 64], first_spp=5, res=oracle_image(True, 5).copy())
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    r.render_passes(SEEDS[5:5 + 64], first_buffer_spp=5)
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), want, "5 passes, then 64 on top")
    r.close()
    loader.close()


@pytest.mark.parametrize("kind", ["aperture", "pregenerated", "fisheye"])
def test_cameras(gpu_instance, kind):
    sc = camera_scene(kind)
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), oracle_image(True, 5, kind), f"camera {kind}")
    r.close()
    loader.close()


@pytest.mark.parametrize("variant,tree,pool,sorted_", [(256, 17, 64, True), (1 << 6, -1, 0, False)], ids=["sorted", "no_parked"])
def test_other_plain_instantiations(gpu_instance, variant, tree, pool, sorted_):
    loader, r = make(gpu_instance, scene(True), variant)
    r.render_passes(SEEDS[:5])
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]) == (tree, pool, False, False, sorted_), info
    assert_same(r.read(), oracle_image(True, 5), f"OPT_KERNEL {variant}")
    r.close()
    loader.close()


@pytest.mark.parametrize("kind", ["pinhole", "pregenerated"])
@pytest.mark.parametrize("variant,name", [(8, "render_waves"), (2, "render_lanes")], ids=["render_waves", "render_lanes"])
def test_fallback_kernels(gpu_instance, variant, name, kind):
    """(with the edge rays too: octree_hit's rcp3 is theirs)"""
    loader, r = make(gpu_instance, camera_scene(kind), variant)
    r.render_passes(SEEDS[:5])
    info = r.kernel_info()
    assert info["pool"] < 0 and (info["group"] == 0) == (variant == 2), info
    assert_same(r.read(), oracle_image(True, 5, kind), f"{name}, {kind}")
    r.close()
    loader.close()


def test_entity_bvh_instantiation(gpu_instance):
    sc = scenes.add_entities(scene(True), 200, seed=5, actor_tris=40, region=((4, 24, 4), (60, 60, 60)))
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    info = r.kernel_info()
    assert (info["tree"], info["bvh"], info["ext"]) == (17, True, False) and info["pool"] > 0, info
    want = oracle(sc, SEEDS[:5])
    assert not np.array_equal(bits(want), bits(oracle_image(True, 5))), "no entity is in view"
    assert_same(r.read(), want, "entity BVHs")
    r.close()
    loader.close()


def test_extended_integrator_instantiation(gpu_instance):
    """(its emitter sampling divides by a distance: rcp_exact)"""
    sc = scene(True)
    loader, r = make(gpu_instance, sc, options=((native.OPT_BSDF, 1), (native.OPT_EMITTER_NEE, 1)))
    r.render_passes(SEEDS[:5])
    info = r.kernel_info()
    assert info["ext"] and info["tree"] == 17 and info["pool"] > 0, info
    port = binding.port()
    with PortExt(port, sc, bsdf=1, nee=1):
        want = port.render_gids(sc, SEEDS[:5], ALL, threads=THREADS)
    assert_same(r.read(), want, "extended integrator")
    r.close()
    loader.close()
