"""render_pool's block test starts the shadow ray or the bounce where it hits (render_pool.hip block_continues): a lane whose test
reports a hit, and whose path is known to go on, runs SHADE's continuation (path_continue.inc) and trace_setup there and leaves as a
marcher, instead of waiting for a SHADE execution that would do nothing else for it.  A path executes the same helpers on the same
values in the same order, its own RNG draws included — only which lanes run together moves — so every pixel here is compared with
oracle/port.c, bit for bit, at the smallest shapes at which the hand-over can go wrong:

  who is taken over     in scenes with the sun on, a main ray's hit (the shadow ray) and a shadow ray's hit (the bounce); with the sun
                        off every trace that ends goes to SHADE as before (the cases without sun pin that flow); a bounce
                        that reaches the depth limit stays SHADE's: maximum depths 1, 2 and 3 put the limit on the bounce behind the first
                        shadow ray (at 1 the main hit still starts that shadow ray in BLOCK), behind a shadow hit and behind a shadow
                        miss; 254 on a closed room with the sun on is the deepest path the kernel runs
  what is consumed      the hit's colour and emittance sit in the registers trace_setup overwrites (the six-word record): emitter scales 0
                        and 2.5 on a world with emitters run the emittance term of the continuation
  what follows          a draw depth of 24 ends traces in the march right after a continuation; in the closed room every trace hits and
                        every path ends at the depth limit
  model blocks          a model-dense world, plain, sorted (the model phase continues too) and forced unsorted: model hits, texels the
                        alpha test rejects (the lane keeps marching) and cubes and models in one execution
  launches              1, 5 and 64 passes per launch, and two launches in a row, the second on top of the first
  the edited text       the timed instantiation render_pool<17, 64> (a small outdoor world put into a depth-7 octree) throughout, and the
                        other forms that compile it: no parked paths, 32 parked, a fisheye camera (launch_pool sends every projector
                        type above 0 to proj::render_pool, the other copy of the text; kernel_info does not say which copy ran, so
                        that rests on the dispatch code), an aperture, pre-generated rays, shards by blocks and by runs of pixels
  untouched kernels     one entity-BVH scene and one extended-integrator run: their SHADE is the split shade_phase, their END is not SHADE"""
import dataclasses
import functools

import numpy as np
import pytest

import golden_scenes as gs
from oracle import binding
from oracle.binding import PortExt, PortOptions

from chunkyclplugin_amd import native, parallel, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, camera_rays

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
W, H = 33, 17
N_PIXELS = W * H
SEEDS = native.java_random_ints(64 + 64, seed=9091)
ALL = np.arange(N_PIXELS, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def scene(sun=True):
    """the small outdoor world of tests/test_gpu_shade_round_trips.py at 33 x 17, with emitters: depth 6 put into a depth-7 octree, so
    that the tree form is the timed one (17)"""
    sc = scenes.outdoor_world(chunks=4, height=64, emitters=0.02, width=W, img_height=H, sun_flag=sun)
    assert sc.octree_depth == 6
    return scenes.embed_deeper(sc, 7)


@functools.lru_cache(maxsize=None)
def camera_scene(kind):
    sc = scene(True)
    if kind == "aperture":
        return gs.with_dof(sc, 0.08, 18.0)
    if kind == "pregenerated":
        return sc.with_view(W, H, camera=gs.pregen_rays(sc, W, H, seed=43), projector_type=native.PROJ_PREGENERATED)
    cam = np.asarray(sc.camera, np.float32)[:15].copy()   # the pinhole camera's position and rotation as a 180-degree fisheye
    cam[12], cam[13], cam[14] = 0.0, 0.0, 180.0
    return dataclasses.replace(sc, camera=cam, projector_type=native.PROJ_FISHEYE)


def oracle(sc, seeds, gids=None, first_spp=0, res=None):
    """port.c's image of `sc` after the passes of `seeds` on the pixels `gids` (a projected camera: pass by pass on its table of rays,
    DESIGN.md section 11)"""
    port = binding.port()
    n = sc.width * sc.height
    gids = np.arange(n, dtype=np.int32) if gids is None else gids
    if sc.projector_type <= 0:
        return port.render_gids(sc, seeds, gids, first_spp=first_spp, res=res, threads=THREADS)
    res = np.zeros(3 * n, np.float32) if res is None else res
    for i, seed in enumerate(seeds):
        table = dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, sc.width, sc.height, int(seed)),
                                    projector_type=native.PROJ_PREGENERATED)
        port.render_gids(table, np.array([seed], np.int32), gids, first_spp=first_spp + i, res=res, threads=THREADS)
    return res


@functools.lru_cache(maxsize=None)
def oracle_image(sun, passes):
    """the pinhole image after the first `passes` seeds at the reference's constants: computed once, shared, read-only"""
    img = oracle(scene(sun), SEEDS[:passes])
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
    return (info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]) == (17, 64, False, False, False)


def plain_kernel(info, pool=64):
    """a plain instantiation on the one-level wide tree at the given pool (sorted or not)"""
    return info["tree"] in (16, 17) and (info["pool"], info["bvh"], info["ext"]) == (pool, False, False)


@pytest.mark.parametrize("passes", [1, 5, 64])
@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_passes_per_launch(gpu_instance, sun, passes):
    loader, r = make(gpu_instance, scene(sun))
    r.render_passes(SEEDS[:passes])
    info = r.kernel_info()
    assert timed_kernel(info), info
    assert info["passes_per_launch"] >= passes, info   # one launch
    assert_same(r.read(), oracle_image(sun, passes), f"sun {sun}, {passes} passes")
    r.close()
    loader.close()


@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_two_launches_in_a_row(gpu_instance, sun):
    sc = scene(sun)
    want = oracle(sc, SEEDS[64:128], first_spp=5, res=oracle_image(sun, 5).copy())
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    r.render_passes(SEEDS[64:128], first_buffer_spp=5)
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), want, f"sun {sun}: 5 passes, then 64 on top")
    r.close()
    loader.close()


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_depth_limit_on_a_bounce(gpu_instance, sun, depth):
    """the bounce that reaches the limit is SHADE's (it ends the path there); the shadow ray in front of it is started in BLOCK whatever
    the depth"""
    sc = scene(sun)
    loader, r = make(gpu_instance, sc, options=((native.OPT_MAX_DEPTH, depth),))
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    with PortOptions(binding.port(), max_depth=depth):
        want = oracle(sc, SEEDS[:5])
    assert not np.array_equal(bits(want), bits(oracle_image(sun, 5))), "the depth limit changed nothing"
    assert_same(r.read(), want, f"sun {sun}, max depth {depth}")
    r.close()
    loader.close()


def test_deepest_paths(gpu_instance):
    """max depth 254 (the most render_pool takes) in a closed room with the sun on: every hit is taken over, hundreds of times per path"""
    sc = gs.make("indoor_sun").with_view(40, 24)
    loader, r = make(gpu_instance, sc, options=((native.OPT_MAX_DEPTH, 254),))
    r.render_passes(SEEDS[:2])
    assert plain_kernel(r.kernel_info()), r.kernel_info()
    with PortOptions(binding.port(), max_depth=254):
        want = oracle(sc, SEEDS[:2])
    assert_same(r.read(), want, "indoor room with sun, max depth 254")
    r.close()
    loader.close()


@pytest.mark.parametrize("scale", [0.0, 2.5])
def test_emitter_scale(gpu_instance, scale):
    sc = scene(True)
    loader, r = make(gpu_instance, sc, options=((native.OPT_EMITTER_SCALE, scale),))
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    with PortOptions(binding.port(), emitter_scale=scale):
        want = oracle(sc, SEEDS[:5])
    assert not np.array_equal(bits(want), bits(oracle_image(True, 5))), "no emitter is in view"
    assert_same(r.read(), want, f"emitter scale {scale}")
    r.close()
    loader.close()


def test_traces_that_end_in_the_march(gpu_instance):
    sc = scene(True)
    loader, r = make(gpu_instance, sc, options=((native.OPT_DRAW_DEPTH, 24),))
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    with PortOptions(binding.port(), draw_depth=24):
        want = oracle(sc, SEEDS[:5])
    assert not np.array_equal(bits(want), bits(oracle_image(True, 5))), "no trace ran out of steps"
    assert_same(r.read(), want, "draw depth 24")
    r.close()
    loader.close()


def test_closed_room(gpu_instance):
    """no sun, no sky: every trace hits and every path ends at the depth limit (with the sun off the hits stay SHADE's)"""
    sc = gs.make("indoor").with_view(40, 24)
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    assert plain_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), oracle(sc, SEEDS[:5]), "closed room")
    r.close()
    loader.close()


@functools.lru_cache(maxsize=None)
def model_world():
    sc = scenes.tiny_scene(seed=14, size=48, width=72, height=48, entities=0, sun_flag=True)
    want = oracle(sc, SEEDS[:5])
    want.setflags(write=False)
    return sc, want


@pytest.mark.parametrize("variant", [0, 256, 512], ids=["default", "sorted", "unsorted"])
def test_model_dense_world(gpu_instance, variant):
    sc, want = model_world()
    loader, r = make(gpu_instance, sc, variant)
    r.render_passes(SEEDS[:5])
    info = r.kernel_info()
    assert plain_kernel(info), info
    if variant:
        assert info["sorted"] == (variant == 256), info
    assert_same(r.read(), want, f"model-dense world, OPT_KERNEL {variant}")
    r.close()
    loader.close()


@pytest.mark.parametrize("variant,pool", [(1 << 6, 0), (2 << 6, 32)], ids=["no_parked", "32_parked"])
@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_other_pools(gpu_instance, sun, variant, pool):
    loader, r = make(gpu_instance, scene(sun), variant)
    r.render_passes(SEEDS[:64])
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]) == (-1, pool, False, False, False), info
    assert_same(r.read(), oracle_image(sun, 64), f"sun {sun}, OPT_KERNEL {variant}")
    r.close()
    loader.close()


@pytest.mark.parametrize("kind", ["aperture", "pregenerated", "fisheye"])
def test_cameras(gpu_instance, kind):
    """(the plain pinhole camera is every other test of this file; the fisheye is dispatched to proj::render_pool by its projector type —
    kernel_info reports the template arguments, which both copies share, not the copy)"""
    sc = camera_scene(kind)
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), oracle(sc, SEEDS[:5]), f"camera {kind}")
    r.close()
    loader.close()


@pytest.mark.parametrize("rank,world,tile", [(1, 3, 0), (2, 5, 7)], ids=["blocks_1_of_3", "runs_of_7_2_of_5"])
def test_shards(gpu_instance, rank, world, tile):
    """the rank's pixels are the oracle's, everybody else's stay zero"""
    own = parallel.owned_gids(N_PIXELS, rank, world, tile, W)
    assert len(own)
    want = np.zeros((N_PIXELS, 3), np.float32)
    want[own] = oracle_image(True, 5).reshape(-1, 3)[own]
    loader, r = make(gpu_instance, scene(True))
    r.set_shard(rank, world, tile)
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), want, f"shard {rank} of {world}, tile {tile}")
    r.close()
    loader.close()


def test_entity_bvh_kernel_is_untouched(gpu_instance):
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


def test_extended_integrator_is_untouched(gpu_instance):
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
