"""render_pool keeps a path's state in place across its phases: the phases of the kernel's loop are consecutive ifs that update the state
where it lives, and in the six-word instantiations a block test that ends a trace writes the hit's colour and emittance straight
into the registers of 1/d and the distance marched, where SHADE reads them (path_state.hpp block_phase<SHARE>, pool_kernel.inc).
The hand-over between the block test and SHADE is the one place where that can put a wrong value into a pixel, and the headline
goldens cannot see half of it: the benchmark world has no emitters, so a mishandled emittance register is invisible there.

Three small worlds that still select the timed instantiation, render_pool<17, 64> — an outdoor world with emitters, with and without
the sun's shadow rays, and the indoor room (lamps, no sun) — rendered as 32 passes in one launch and 32 more on top of them, every
pixel against oracle/port.c (`port.render_gids`), bit for bit: by the default kernel, with the block tests sorted (OPT_KERNEL bit 8)
and unsorted (bit 9), by the pool-size rigs (variant bits 6-7: no parked paths, so every hand-over happens in a lane's registers; 32
parked), and as one shard of 16 x 16-pixel blocks.  Between them the scenes reach a cube hit, an alpha-rejected cube followed by a hit
(leaves, plants), slab, post and plant hits, a shadow ray's hit, a trace that ends in the march, a fresh lane and non-zero emittance;
the CPU test below asserts on the oracle's own records that emitted light and model-block hits are in every image."""
import functools

import numpy as np
import pytest

from oracle import binding

from chunkyclplugin_amd import native, parallel, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader

THREADS = binding.usable_threads()
PASSES = 32
SEEDS = native.java_random_ints(2 * PASSES)
SCENES = ("outdoor", "outdoor_no_sun", "indoor")
# OPT_KERNEL value -> (tree, pool, sorted) the launch has to report; None: whatever the scene's own choice is
VARIANTS = {"default": (0, 17, 64, None), "sorted": (256, 17, 64, True), "unsorted": (512, 17, 64, False),
            "no_parked": (1 << 6, -1, 0, False), "parked_32": (2 << 6, -1, 32, False)}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The small worlds fit a depth-6 octree, which the library walks as one dense node (tree form 16): each is put, unmoved, into a
    depth-7 octree — same blocks, same camera, same image — whose form is the timed one, a dense top over one level of 8^3 nodes (17)."""
    if name == "outdoor":
        sc = scenes.outdoor_world(chunks=4, height=64, emitters=0.02, width=96, img_height=64)
    elif name == "outdoor_no_sun":
        sc = scenes.outdoor_world(chunks=4, height=64, emitters=0.02, width=96, img_height=64, sun_flag=False)
    else:
        sc = scenes.indoor_room(size=32, width=96, img_height=64)
    assert sc.octree_depth == 6
    return scenes.embed_deeper(sc, 7)


@functools.lru_cache(maxsize=None)
def oracle_image(name):
    """the image after 32 passes and after 64 (the second launch continues the running mean), computed once and shared"""
    sc = scene(name)
    port = binding.port()
    gids = np.arange(sc.width * sc.height, dtype=np.int32)
    first = port.render_gids(sc, SEEDS[:PASSES], gids, threads=THREADS)
    both = port.render_gids(sc, SEEDS[PASSES:], gids, first_spp=PASSES, res=first.copy(), threads=THREADS)
    first, both = first.reshape(-1, 3), both.reshape(-1, 3)
    first.setflags(write=False)
    both.setflags(write=False)
    return first, both


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    same = (bits(got) == bits(want)).all(axis=1)
    if not same.all():
        i = int(np.argmin(same))
        pytest.fail(f"{what}: {int((~same).sum())} of {len(want)} pixels differ from the oracle; first: pixel {i} got {got[i]!r} want {want[i]!r}")


@pytest.mark.parametrize("name", SCENES)
def test_the_oracle_images_hold_what_the_hand_over_carries(port, name):
    """On the oracle's own records (first pass, every pixel): light emitted by a hit block reaches the image, a model block (slab, post,
    plant) is hit, and — outdoors — some traces end in the march (the sky)."""
    sc = scene(name)
    h = binding.SceneHandle(sc)
    types = np.asarray(sc.block_palette)
    emitted = model_hits = misses = 0
    for gid in range(sc.width * sc.height):
        rec, _rad = port.trace_records(h, int(SEEDS[0]), gid)
        hit = rec["hit"] != 0
        emitted += int(np.count_nonzero(hit & (rec["emittance"] > 0) & (rec["color"][:, :3].max(axis=1) > 0)))
        model_hits += int(np.count_nonzero(hit & np.isin(types[np.clip(rec["material"], 0, len(types) - 1)], (2, 3))))
        misses += int(np.count_nonzero(~hit))
    assert emitted > 0 and model_hits > 0, (emitted, model_hits)
    assert misses > 0 or name == "indoor", name   # (the room is closed: no trace there ends in the march)
    first, both = oracle_image(name)
    assert np.isfinite(both).all() and both.max() > 0 and not np.array_equal(bits(first), bits(both))


def make(gpu_instance, sc, variant):
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    return loader, r


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", SCENES)
def test_two_launches_match_the_oracle(gpu_instance, name, variant):
    sc = scene(name)
    first, both = oracle_image(name)
    bits_, tree, pool, sorted_ = VARIANTS[variant]
    loader, r = make(gpu_instance, sc, bits_)
    r.render_passes(SEEDS[:PASSES])
    info = r.kernel_info()
    assert (info["tree"], info["pool"], info["bvh"], info["ext"]) == (tree, pool, False, False), info
    assert sorted_ is None or info["sorted"] == sorted_, info
    assert info["passes_per_launch"] >= PASSES, info   # one launch
    assert_same(r.read().reshape(-1, 3), first, f"{name}, {variant}: 32 passes")
    r.render_passes(SEEDS[PASSES:], first_buffer_spp=PASSES)
    assert_same(r.read().reshape(-1, 3), both, f"{name}, {variant}: 32 more passes")
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_one_shard_of_blocks(gpu_instance, name):
    """rank 1 of 3, the image's 16 x 16 blocks dealt round-robin: its pixels are the oracle's, everybody else's stay zero"""
    sc = scene(name)
    first, both = oracle_image(name)
    loader, r = make(gpu_instance, sc, 0)
    r.set_shard(1, 3, 0)
    own = parallel.owned_gids(sc.width * sc.height, 1, 3, 0, sc.width)
    mine = np.zeros(sc.width * sc.height, bool)
    mine[own] = True
    for seeds, spp, want, what in ((SEEDS[:PASSES], 0, first, "32 passes"), (SEEDS[PASSES:], PASSES, both, "32 more passes")):
        r.render_passes(seeds, first_buffer_spp=spp)
        info = r.kernel_info()
        assert (info["tree"], info["pool"], info["bvh"], info["ext"]) == (17, 64, False, False), info
        assert_same(r.read().reshape(-1, 3), np.where(mine[:, None], want, np.float32(0)), f"{name}, shard 1 of 3: {what}")
    r.close()
    loader.close()
