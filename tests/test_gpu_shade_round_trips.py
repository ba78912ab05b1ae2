"""render_pool's SHADE reads its launch arguments and its seed in bursts: the deposit and the new-sample section take their words of
the argument segment as one block behind one wait (path_state.hpp sample_args), the pass's seed is requested before the pixel decode
and waited for where rng is formed, and the sky's four texels are requested before the sampling block and blended behind it
(shade_phase: sky_fetch ... sky_finish).  None of that changes a value — so every pixel here is compared with oracle/port.c
(`port.render_gids`), bit for bit, at the smallest shapes at which a moved load can go wrong:

  image     33 x 17: three by two tiles of 16 x 16 slots, padding slots in every tile, the last column of tiles one pixel wide and the
            last row one pixel high (a padding slot fetches a seed it discards)
  passes    1, 5, 64 and 257 per launch: 257 takes its seeds from device memory instead of the argument segment; 5 x 33 x 17 leaves a
            last claim batch that is not full; and two launches in a row, the second on top of the first (first_buffer_spp)
  shards    blocks dealt to rank 1 of 3, runs of seven pixel indices dealt to rank 2 of 5 (the general quotient path of the pixel
            decode), and a rank beyond the image's six blocks, which owns nothing
  cameras   pinhole, pinhole with an aperture, pre-generated rays, and one projected camera (proj::render_pool, the other copy of
            the kernel's text)
  sun       on — every unoccluded shadow ray then goes through the disc branch, and through the bounce that overwrites the
            direction the sky was looked up with — and off
  kernels   the timed instantiation render_pool<17, 64> throughout (a small outdoor world put into a depth-7 octree), plus the other
            forms that compile the edited text: block tests sorted, no parked paths, entity BVHs, the extended integrator."""
import dataclasses
import functools

import numpy as np
import pytest

import golden_scenes as gs
from oracle import binding
from oracle.binding import PortExt

from chunkyclplugin_amd import native, parallel, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, camera_rays

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
W, H = 33, 17
N_PIXELS = W * H
SEEDS = native.java_random_ints(257 + 64, seed=8086)
ALL = np.arange(N_PIXELS, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def scene(sun=True):
    """the small outdoor world of tests/test_gpu_pool_state_in_place.py at 33 x 17: depth 6 put into a depth-7 octree, so that the tree
    form is the timed one (17)"""
    sc = scenes.outdoor_world(chunks=4, height=64, emitters=0.02, width=W, img_height=H, sun_flag=sun)
    assert sc.octree_depth == 6
    return scenes.embed_deeper(sc, 7)


@functools.lru_cache(maxsize=None)
def camera_scene(kind):
    sc = scene(True)
    if kind == "pinhole":
        return sc
    if kind == "aperture":
        return gs.with_dof(sc, 0.08, 18.0)
    if kind == "pregenerated":
        return sc.with_view(W, H, camera=gs.pregen_rays(sc, W, H, seed=41), projector_type=native.PROJ_PREGENERATED)
    cam = np.asarray(sc.camera, np.float32)[:15].copy()   # the pinhole camera's position and rotation as a 180-degree fisheye
    cam[12], cam[13], cam[14] = 0.0, 0.0, 180.0
    return dataclasses.replace(sc, camera=cam, projector_type=native.PROJ_FISHEYE)


def oracle(sc, seeds, gids=ALL, first_spp=0, res=None):
    """port.c's image of `sc` after the passes of `seeds` on the pixels `gids` (a projected camera: pass by pass on its table of rays,
    DESIGN.md section 11)"""
    port = binding.port()
    if sc.projector_type <= 0:
        return port.render_gids(sc, seeds, gids, first_spp=first_spp, res=res, threads=THREADS)
    res = np.zeros(3 * N_PIXELS, np.float32) if res is None else res
    for i, seed in enumerate(seeds):
        table = dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, W, H, int(seed)), projector_type=native.PROJ_PREGENERATED)
        port.render_gids(table, np.array([seed], np.int32), gids, first_spp=first_spp + i, res=res, threads=THREADS)
    return res


@functools.lru_cache(maxsize=None)
def oracle_image(sun, passes):
    """the pinhole image after the first `passes` seeds: computed once, shared, read-only"""
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
    return (info["tree"], info["pool"], info["bvh"], info["ext"]) == (17, 64, False, False)


@pytest.mark.parametrize("passes", [1, 5, 64, 257])
@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_passes_per_launch(gpu_instance, sun, passes):
    sc = scene(sun)
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:passes])
    info = r.kernel_info()
    assert timed_kernel(info), info
    assert info["passes_per_launch"] >= passes, info   # one launch (257: its seeds travel in device memory)
    assert_same(r.read(), oracle_image(sun, passes), f"sun {sun}, {passes} passes")
    r.close()
    loader.close()


@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_two_launches_in_a_row(gpu_instance, sun):
    sc = scene(sun)
    want = oracle(sc, SEEDS[257:257 + 64], first_spp=5, res=oracle_image(sun, 5).copy())
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    r.render_passes(SEEDS[257:257 + 64], first_buffer_spp=5)
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), want, f"sun {sun}: 5 passes, then 64 on top")
    r.close()
    loader.close()


@pytest.mark.parametrize("rank,world,tile", [(1, 3, 0), (2, 5, 7), (7, 8, 0)], ids=["blocks_1_of_3", "runs_of_7_2_of_5", "owns_nothing"])
def test_shards(gpu_instance, rank, world, tile):
    """the rank's pixels are the oracle's, everybody else's stay zero"""
    sc = scene(True)
    own = parallel.owned_gids(N_PIXELS, rank, world, tile, W)
    assert (len(own) == 0) == (rank == 7)   # six blocks of 16 x 16 cover 33 x 17: rank 7 of 8 has none
    want = np.zeros((N_PIXELS, 3), np.float32)
    want[own] = oracle_image(True, 5).reshape(-1, 3)[own]
    loader, r = make(gpu_instance, sc)
    r.set_shard(rank, world, tile)
    r.render_passes(SEEDS[:5])
    if len(own):
        assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), want, f"shard {rank} of {world}, tile {tile}")
    r.close()
    loader.close()


@pytest.mark.parametrize("kind", ["aperture", "pregenerated", "fisheye"])
def test_cameras(gpu_instance, kind):
    """(the plain pinhole camera is every other test of this file)"""
    sc = camera_scene(kind)
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:5])
    assert timed_kernel(r.kernel_info()), r.kernel_info()
    assert_same(r.read(), oracle(sc, SEEDS[:5]), f"camera {kind}")
    # ... and as one shard of pixel runs: the decode's general path with this camera's ray
    own = parallel.owned_gids(N_PIXELS, 2, 5, 7, W)
    r.close()
    loader.close()
    loader, r = make(gpu_instance, sc)
    r.set_shard(2, 5, 7)
    r.render_passes(SEEDS[:5])
    want = np.zeros((N_PIXELS, 3), np.float32)
    want[own] = oracle(sc, SEEDS[:5], gids=own).reshape(-1, 3)[own]
    assert_same(r.read(), want, f"camera {kind}, shard 2 of 5 in runs of 7")
    r.close()
    loader.close()


@pytest.mark.parametrize("variant,tree,pool,sorted_", [(256, 17, 64, True), (1 << 6, -1, 0, False)], ids=["sorted", "no_parked"])
@pytest.mark.parametrize("sun", [True, False], ids=["sun", "no_sun"])
def test_other_plain_instantiations(gpu_instance, sun, variant, tree, pool, sorted_):
    sc = scene(sun)
    loader, r = make(gpu_instance, sc, variant)
    r.render_passes(SEEDS[:64])
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]) == (tree, pool, False, False, sorted_), info
    assert_same(r.read(), oracle_image(sun, 64), f"sun {sun}, OPT_KERNEL {variant}")
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
    sc = scene(True)
    opts = dict(bsdf=1, nee=1)
    loader, r = make(gpu_instance, sc, options=((native.OPT_BSDF, 1), (native.OPT_EMITTER_NEE, 1)))
    r.render_passes(SEEDS[:5])
    info = r.kernel_info()
    assert info["ext"] and info["tree"] == 17 and info["pool"] > 0, info
    port = binding.port()
    with PortExt(port, sc, **opts):
        want = port.render_gids(sc, SEEDS[:5], ALL, threads=THREADS)
    assert_same(r.read(), want, "extended integrator")
    r.close()
    loader.close()
