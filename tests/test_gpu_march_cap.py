"""render_pool ends the march of a ray that runs upwards once it stands at or above hit_top, 1 + the highest cell of any leaf that can
be hit (path_state.hpp march_step): such a trace is the miss it would have been at the world's edge, so every image here is compared
with oracle/port.c bit for bit, 40 x 30 pixels and 4 passes, at the shapes at which the cap can go wrong:

  where the top is      worlds of depth 7 (the timed tree form, 17) whose highest leaf that can be hit ends at y = 1, below the
                        middle, in the world's last row (nothing is capped), is a leaf of level 2, is a full column, or does not
                        exist (hit_top 0: every upward ray ends at its first step); invisible and ANY_TYPE leaves lie above the top
  where the camera is   below the cap, inside the capped region, above the world looking down (the march is entered through the top
                        face), above the floor looking up
  the instantiations    17 plain, 17 sorted, the projected cameras' copy (a fisheye), the generic tree form (-1) with no parked
                        paths and with 32: kernel_info says which ran
  the rays              pre-generated ones with d.y exactly +0, -0, 1e-30 and -1e-30, origins at y = hit_top and one ulp either
                        side of it, origins just below the world going up with d.y = 1e-6 (the cell y = -1), outside a side face,
                        and a NaN component in the origin
  the sun               on the horizon (shadow rays with d.y about 0), below it, off
  the march             draw depths 1, 2 and 256
  the routes            a shard of 16 x 16 blocks (set_shard(1, 2, 0)) and the pixel list
  scene updates         a block-palette change moves hit_top on the loaded scene, and the next launch is the oracle's image"""
import dataclasses
import functools

import numpy as np
import pytest

import march_cap_scenes as mc
from oracle import binding
from oracle.binding import PortOptions

from chunkyclplugin_amd import native, parallel, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, camera_rays

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
W, H = 40, 30
N_PIXELS = W * H
DEPTH = 7
SEEDS = native.java_random_ints(8, seed=4242)[:4]
ALL = np.arange(N_PIXELS, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def scene(kind, where, sun="on"):
    sc, top = mc.world(kind, DEPTH, sun)
    return mc.view(sc, where, top, W, H), top


def oracle(sc, seeds=SEEDS, gids=ALL):
    port = binding.port()
    if sc.projector_type <= 0:
        return port.render_gids(sc, seeds, gids, threads=THREADS)
    res = np.zeros(3 * sc.width * sc.height, np.float32)  # a projected camera: pass by pass on its table of rays
    for i, seed in enumerate(seeds):
        table = dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, sc.width, sc.height, int(seed)),
                                    projector_type=native.PROJ_PREGENERATED)
        port.render_gids(table, np.array([seed], np.int32), gids, first_spp=i, res=res, threads=THREADS)
    return res


@functools.lru_cache(maxsize=None)
def oracle_image(kind, where, sun="on"):
    img = oracle(scene(kind, where, sun)[0])
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


def kernel(info):
    return info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]


TIMED = (17, 64, False, False, False)


@pytest.mark.parametrize("where", ["below", "inside", "down", "up"])
@pytest.mark.parametrize("kind", mc.KINDS)
def test_tops_and_cameras(gpu_instance, kind, where):
    sc, top = scene(kind, where)
    loader, r = make(gpu_instance, sc)
    assert loader.hit_top() == top
    r.render_passes(SEEDS)
    assert kernel(r.kernel_info()) == TIMED, r.kernel_info()
    assert_same(r.read(), oracle_image(kind, where), f"{kind}, camera {where}")
    r.close()
    loader.close()


@pytest.mark.parametrize("where", ["inside", "down"])
@pytest.mark.parametrize("variant,want", [(256, (17, 64, False, False, True)), (1 << 6, (-1, 0, False, False, False)),
                                          (2 << 6, (-1, 32, False, False, False))], ids=["sorted", "generic_no_parked", "generic_32_parked"])
def test_other_instantiations(gpu_instance, variant, want, where):
    for kind in ("middle", "big_leaf"):
        sc, _top = scene(kind, where)
        loader, r = make(gpu_instance, sc, variant)
        r.render_passes(SEEDS)
        assert kernel(r.kernel_info()) == want, r.kernel_info()
        assert_same(r.read(), oracle_image(kind, where), f"{kind}, camera {where}, OPT_KERNEL {variant}")
        r.close()
        loader.close()


@pytest.mark.parametrize("where", ["inside", "down", "up"])
def test_projected_camera(gpu_instance, where):
    """(a projector type above 0 is dispatched to proj::render_pool, the other copy of the kernel's text; kernel_info reports the
    template arguments, which both copies share)"""
    sc, _top = scene("middle", where)
    cam = np.asarray(sc.camera, np.float32)[:15].copy()
    cam[12], cam[13], cam[14] = 0.0, 0.0, 180.0
    sc = dataclasses.replace(sc, camera=cam, projector_type=native.PROJ_FISHEYE)
    for variant, want in ((0, TIMED), (256, (17, 64, False, False, True))):
        loader, r = make(gpu_instance, sc, variant)
        r.render_passes(SEEDS)
        assert kernel(r.kernel_info()) == want, r.kernel_info()
        assert_same(r.read(), oracle(sc), f"fisheye, camera {where}, OPT_KERNEL {variant}")
        r.close()
        loader.close()


@pytest.mark.parametrize("where", ["below", "down"])
@pytest.mark.parametrize("sun", ["horizon", "below", "off"])
def test_suns(gpu_instance, sun, where):
    sc, _top = scene("middle", where, sun)
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    assert kernel(r.kernel_info()) == TIMED, r.kernel_info()
    want = oracle_image("middle", where, sun)
    assert not np.array_equal(bits(want), bits(oracle_image("middle", where))), "the sun changed nothing"
    assert_same(r.read(), want, f"sun {sun}, camera {where}")
    r.close()
    loader.close()


@pytest.mark.parametrize("draw_depth", [1, 2, 256])
def test_draw_depths(gpu_instance, draw_depth):
    for where in ("inside", "down"):
        sc, _top = scene("big_leaf", where)
        loader, r = make(gpu_instance, sc, options=((native.OPT_DRAW_DEPTH, draw_depth),))
        r.render_passes(SEEDS)
        assert kernel(r.kernel_info()) == TIMED, r.kernel_info()
        with PortOptions(binding.port(), draw_depth=draw_depth):
            want = oracle(sc)
        assert_same(r.read(), want, f"draw depth {draw_depth}, camera {where}")
        r.close()
        loader.close()


def test_a_shard_of_blocks(gpu_instance):
    own = parallel.owned_gids(N_PIXELS, 1, 2, 0, W)
    assert 0 < len(own) < N_PIXELS
    want = np.zeros((N_PIXELS, 3), np.float32)
    want[own] = oracle_image("middle", "down").reshape(-1, 3)[own]
    loader, r = make(gpu_instance, scene("middle", "down")[0])
    r.set_shard(1, 2, 0)
    r.render_passes(SEEDS)
    assert kernel(r.kernel_info()) == TIMED, r.kernel_info()
    assert_same(r.read(), want, "shard 1 of 2 in 16 x 16 blocks")
    r.close()
    loader.close()


def test_the_pixel_list(gpu_instance):
    listed = np.random.default_rng(5).permutation(N_PIXELS)[:777].astype(np.int32)
    want = np.zeros((N_PIXELS, 3), np.float32)
    want[listed] = oracle_image("middle", "inside").reshape(-1, 3)[listed]
    loader, r = make(gpu_instance, scene("middle", "inside")[0])
    r.render_list(listed, SEEDS)
    info = r.kernel_info()
    assert info["tree"] == 17 and info["pool"] == 64 and not info["bvh"], info
    assert_same(r.read(), want, "777 listed pixels")
    r.close()
    loader.close()


def hand_made_rays(top, side):
    """[N_PIXELS, 6] origins and directions: the cases of the module's text first, then upward and downward rays from all over"""
    f = np.float32
    below, above = np.nextafter(f(top), f(-np.inf)), np.nextafter(f(top), f(np.inf))
    rays = []
    for dy in (f(0.0), f(-0.0), f(1e-30), f(-1e-30)):
        for oy in (f(top), below, above, f(top - 0.5), f(2.5)):
            for dx, dz in ((1.0, 0.3), (-0.7, 1.0), (0.0, -1.0)):
                rays.append((2.5, oy, 3.5, dx, dy, dz))
    for oy in (-1e-6, -1e-3, -0.5):  # from below the world, hardly rising: the first cell may be y = -1
        for d in ((1.0, 1e-6, 0.2), (1e-3, 1e-6, 0.0), (0.0, 1e-6, 0.0), (0.3, 1e-6, -1.0)):
            rays.append((5.5, oy, 5.5, *d))
    for dy in (0.3, -0.3, 1e-6, 0.0):  # from outside a side face
        rays.append((-3.5, top + 0.5, 5.5, 1.0, dy, 0.1))
        rays.append((side + 2.0, 0.5, side / 2, -1.0, dy, 0.05))
        rays.append((side / 2, top - 0.5, -7.0, 0.02, dy, 1.0))
    nan = float("nan")
    # a NaN component of the origin: the first cell is outside any world.  (Not of the direction: the sky lookup of a miss is fed the
    # direction, and oracle/port.c itself crashes there on a NaN d.x or d.z — there is no reference for such a ray.)
    rays += [(nan, 2.5, 3.5, 1.0, 0.2, 0.1), (2.5, nan, 3.5, 1.0, 0.2, 0.1), (2.5, nan, 3.5, 1.0, -0.2, 0.1), (2.5, top + 1.5, nan, 0.1, 0.2, 1.0)]
    rng = np.random.default_rng(77)
    n = N_PIXELS - len(rays)
    assert n > N_PIXELS // 2
    o = rng.uniform(0.5, side - 0.5, (n, 3))
    o[::3, 1] = rng.uniform(0.5, top + 3.0, len(o[::3]))
    d = rng.normal(size=(n, 3))
    d[::5, 1] = np.abs(d[::5, 1]) * 0.01
    out = np.concatenate([np.array(rays, np.float64), np.concatenate([o, d], axis=1)]).astype(np.float32)
    for k, dy in enumerate((0.0, -0.0, 1e-30, -1e-30)):  # (astype keeps the sign of zero; said again for the reader)
        assert np.signbit(out[15 * k, 4]) == np.signbit(f(dy))
    return out


@pytest.mark.parametrize("variant,want", [(0, TIMED), (256, (17, 64, False, False, True)), (1 << 6, (-1, 0, False, False, False))],
                         ids=["plain", "sorted", "generic"])
@pytest.mark.parametrize("kind", ["middle", "big_leaf", "air"])
def test_hand_made_rays(gpu_instance, kind, variant, want):
    base, top = mc.world(kind, DEPTH)
    rays = hand_made_rays(max(top, 1), float(1 << DEPTH))
    sc = base.with_view(W, H, camera=rays.reshape(-1), projector_type=native.PROJ_PREGENERATED)
    loader, r = make(gpu_instance, sc, variant)
    r.render_passes(SEEDS)
    assert kernel(r.kernel_info()) == want, r.kernel_info()
    assert_same(r.read(), oracle(sc), f"hand-made rays on {kind}, OPT_KERNEL {variant}")
    r.close()
    loader.close()


def test_a_palette_change_moves_the_cap(gpu_instance):
    """the invisible block above everything becomes a cube: hit_top is the world's edge and the image the oracle's; hidden again, the
    cap is back where it was"""
    sc, top = mc.world("middle", DEPTH)
    S = float(1 << DEPTH)
    sc = sc.with_view(W, H, camera=scenes.look_at_camera((12.5, S - 30.0, 11.5), (3.0, S - 1.0, 3.0)), projector_type=0)  # looks up at the invisible blocks
    _sc, cube, _model, ghost = mc.base()
    blocks = np.asarray(sc.block_palette, np.int32)
    raised = blocks.copy()
    raised[2 * ghost:2 * ghost + 2] = blocks[2 * cube:2 * cube + 2]
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    assert loader.hit_top() == top
    for palette, want_top in ((raised, 1 << DEPTH), (blocks, top)):
        a = np.ascontiguousarray(palette, np.int32)
        native.check(native.lib().chunky_scene_set_palette(loader._h, native.PALETTE_BLOCK, native.ptr(a), a.size))
        assert loader.hit_top() == want_top
        r.reset()
        r.render_passes(SEEDS)
        assert kernel(r.kernel_info()) == TIMED, r.kernel_info()
        changed = dataclasses.replace(sc, block_palette=palette)
        want = oracle(changed)
        assert_same(r.read(), want, f"block palette with hit_top {want_top}")
    assert not np.array_equal(bits(oracle(dataclasses.replace(sc, block_palette=raised))), bits(oracle(sc))), "the cube is not in view"
    r.close()
    loader.close()
