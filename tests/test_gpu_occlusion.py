"""chunky_render_occlusion_passes / _read (csrc/occlusion.hip) on the device, bit for bit against the specification restated on the
C restatement of the reference (occlusion_spec.expected_occlusion: records 0 to 2 of the sample, two images folded from them;
tests/test_occlusion_cpu.py shows the restatement means the same on the reference build and that both sample values occur): the
golden scenes whole, radii and the radius boundary on an octree hit and on a triangle hit, every tree form, split calls and the launch
cut, the deep form, a projected camera with a lens, shards, a group, the BVH cull option, a scene update, the isolation from every
other image of the target, and the ABI's errors.  Every comparison is over every pixel named, without tolerance."""
import dataclasses

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from occlusion_spec import IMAGES, WHICH, expected_occlusion, fold_occlusion, occlusion_records
from chunkyclplugin_amd import native
from chunkyclplugin_amd.native import check, ptr
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays
from test_camera_lens_ods_cpu import GPU_LENS, projected

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(gs.N_PASSES)
ALL = np.arange(gs.W * gs.H)
RADIUS = 4.0
WHOLE = ["outdoor", "outdoor_nosun", "entities", "dof", "pregen", "inside", "indoor_sun"]


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


def images(r, gids=None):
    """{"ao", "sun"}: (pixels,) float32 as chunky_render_occlusion_read delivers them"""
    out = {k: r.read_occlusion(WHICH[k]).reshape(-1) for k in IMAGES}
    assert all(v.dtype == np.float32 for v in out.values())
    return out if gids is None else {k: v[gids] for k, v in out.items()}


def assert_same(got, want, gids, what):
    for k in IMAGES:
        same = bits(got[k]) == bits(want[k])
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what}: {k} differs at {int((~same).sum())} of {len(same)} pixels (first gid {int(gids[i])}: "
                        f"{float(got[k][i])!r} against {float(want[k][i])!r})")


@pytest.fixture(scope="module")
def golden(port):
    """The records of the golden scenes' whole images for SEEDS, gathered once per scene and never changed."""
    cache = {}

    def get(name, cull=False):
        if (name, cull) not in cache:
            with binding.PortCull(port, cull):
                rec = occlusion_records(port, gs.make(name), SEEDS, ALL)
            for v in rec.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[name, cull] = rec
        return cache[name, cull]
    return get


def first_pass(rec):
    return {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in rec.items()}


@pytest.mark.parametrize("name", WHOLE)
def test_golden_scene_whole_images(gpu_instance, golden, name):
    """Sun on and off (both RNG orders), the BVH walk, lens draws before the sun draws, pre-generated rays."""
    sc = gs.make(name)
    loader, r = make(gpu_instance, sc)
    r.render_occlusion(SEEDS, RADIUS)
    got = images(r)
    assert_same(got, fold_occlusion(golden(name), RADIUS), ALL, name)
    info = r.occlusion_info()
    assert info["launches"] == 1 and info["bvh"] == (name == "entities"), info
    assert r.occlusion_time()[1] == 1
    assert (got["ao"] < 1).any() and (got["sun"] < 1).any()   # some sample is occluded, some is in shadow
    assert ((got["sun"] >= 0) & (got["sun"] <= 1)).all() and ((got["ao"] >= 0) & (got["ao"] <= 1)).all()
    close(r, loader)


@pytest.mark.parametrize("radius", [0.25, 1.0, 16.0, np.inf], ids=lambda x: f"r{x}")
@pytest.mark.parametrize("name", ["entities", "outdoor"])
def test_radii(gpu_instance, golden, name, radius):
    loader, r = make(gpu_instance, gs.make(name))
    r.render_occlusion(SEEDS, radius)
    got = images(r)
    assert_same(got, fold_occlusion(golden(name), radius), ALL, f"{name}, radius {radius}")
    # SUN does not depend on the radius
    assert bits(got["sun"]).tobytes() == bits(fold_occlusion(golden(name), RADIUS)["sun"]).tobytes()
    close(r, loader)


@pytest.mark.parametrize("radius", [0.25, 1.0, 2.5, 16.0, 5000.0], ids=lambda x: f"r{x}")
@pytest.mark.parametrize("name", ["inside", "indoor_sun", "pregen"])
def test_bounded_bounce_changes_no_bit(gpu_instance, golden, name, radius):
    """Without an entity BVH the bounce record starts at a bound beyond the radius (occlusion.hip bounce_reach; above 4096 at +inf):
    rays from inside the terrain, in a closed room where every bounce hits, and from pre-generated directions, at radii below a block,
    between blocks and beyond the room."""
    loader, r = make(gpu_instance, gs.make(name))
    r.render_occlusion(SEEDS, radius)
    assert not r.occlusion_info()["bvh"]
    assert_same(images(r), fold_occlusion(golden(name), radius), ALL, f"{name}, radius {radius}")
    close(r, loader)


def test_bounded_bounce_far_from_the_origin(gpu_instance, port):
    """... and in a world whose corner is at x = z = 1024, where a float's spacing is 2^-13 and the march's offset rounds coarsely."""
    sc = gs.embedded_offset()
    gids = np.arange(sc.width * sc.height)
    rec = occlusion_records(port, sc, SEEDS, gids)
    loader, r = make(gpu_instance, sc)
    for radius in (0.25, 1.0, 3.0):
        r.reset_occlusion()
        r.render_occlusion(SEEDS, radius)
        assert_same(images(r), fold_occlusion(rec, radius), gids, f"outdoor at 1024, radius {radius}")
    assert (rec["hit"] & rec["b_hit"]).any()
    close(r, loader)


def is_triangle(normal):
    """A normal no block of these worlds has: all three components non-zero (test_radius_boundary asserts that of "outdoor")."""
    return (normal != 0).all(axis=-1)


@pytest.mark.parametrize("name,triangle", [("outdoor", False), ("entities", True)], ids=["octree-hit", "triangle-hit"])
def test_radius_boundary(gpu_instance, golden, name, triangle):
    """A pixel whose bounce record hits at distance D > 0: at ao_distance = D its sample is clear (the compare is strict), at the next
    float it is occluded; the rest of the image follows the specification at both radii."""
    rec = first_pass(golden(name))
    cand = rec["hit"][0] & rec["b_hit"][0] & (rec["b_distance"][0] > 0)
    outdoor = first_pass(golden("outdoor"))
    assert not is_triangle(outdoor["b_normal"][0][outdoor["b_hit"][0]]).any(), "a block's normal passes for a triangle's"
    cand &= is_triangle(rec["b_normal"][0]) if triangle else ~is_triangle(rec["b_normal"][0])
    assert cand.any(), "no pixel of pass 0 has such a bounce hit"
    gid = int(np.flatnonzero(cand)[len(np.flatnonzero(cand)) // 2])
    D = np.float32(rec["b_distance"][0][gid])
    above = np.nextafter(D, np.float32(np.inf))
    loader, r = make(gpu_instance, gs.make(name))
    for radius, value in ((D, 1.0), (above, 0.0)):
        r.reset_occlusion()
        r.render_occlusion(SEEDS[:1], float(radius))
        got = images(r)
        assert got["ao"][gid] == value, (gid, float(D), float(radius), float(got["ao"][gid]))
        assert_same(got, fold_occlusion(rec, radius), ALL, f"{name}, radius {float(radius)!r}")
    close(r, loader)


FORM_CASES = list(gs.form_cases(ragged=True))


@pytest.mark.parametrize("key,build,kernel", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_tree_forms(gpu_instance, port, key, build, kernel):
    """The lookup forms 17 / 18 / 19 / 0 and the entity form 18 with the walk, whole images; the form-19 case at 33 x 17."""
    sc = build()
    loader, r = make(gpu_instance, sc)
    r.render_occlusion(SEEDS, RADIUS)
    info = r.occlusion_info()
    assert (info["tree"], info["bvh"]) == kernel, info
    if (sc.width, sc.height) == gs.RAGGED_VIEW:
        assert info["blocks"] == 6   # 24 claims, one per wave of four-wave workgroups: the grid cap, not the device's size
    gids = np.arange(sc.width * sc.height)
    assert_same(images(r), expected_occlusion(port, sc, SEEDS, gids, RADIUS), gids, key)
    close(r, loader)


def test_two_calls_equal_one(gpu_instance, golden):
    loader, r = make(gpu_instance, gs.make("entities"))
    r.render_occlusion(SEEDS[:2], RADIUS)
    r.render_occlusion(SEEDS[2:], RADIUS, first_buffer_spp=2)
    assert_same(images(r), fold_occlusion(golden("entities"), RADIUS), ALL, "2 + 1 passes")
    close(r, loader)


def test_launch_cut_is_invisible(gpu_instance, port):
    sc = gs.make("outdoor").with_view(8, 8)
    seeds = native.java_random_ints(300)
    gids = np.arange(8 * 8)
    loader, r = make(gpu_instance, sc)
    r.render_occlusion(seeds, RADIUS)
    assert r.occlusion_info()["launches"] == 2  # 256 + 44
    assert r.occlusion_time()[1] == 2
    got = images(r)
    assert_same(got, expected_occlusion(port, sc, seeds, gids, RADIUS), gids, "300 passes")
    r.reset_occlusion()
    r.render_occlusion(seeds[:100], RADIUS)
    r.render_occlusion(seeds[100:], RADIUS, first_buffer_spp=100)
    assert r.occlusion_info()["launches"] == 1
    assert_same(images(r), got, gids, "100 + 200 passes")
    close(r, loader)


def test_deep_form_on_whole_rows(gpu_instance, port):
    sc = gs.make("inside", gs.DEEP_CHUNKS)
    loader, r = make(gpu_instance, sc)
    r.render_occlusion(SEEDS, RADIUS)
    info = r.occlusion_info()
    assert (info["tree"], info["bvh"]) == (17, False), info
    gids = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in (3, 17, 30, 44)])
    want = expected_occlusion(port, sc, SEEDS, gids, RADIUS)
    assert_same(images(r, gids), want, gids, "inside, deep")
    assert 0 < want["ao"].mean() < 1
    close(r, loader)


def test_projected_camera_with_a_lens(gpu_instance, port):
    """A pass of a projected camera is the pass on the table of its rays, with the lens as without."""
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind]
    loader, r = make(gpu_instance, sc, lens)
    r.render_occlusion(SEEDS, RADIUS)
    gids = np.arange(0, sc.width * sc.height, 3)
    want = None
    for i, seed in enumerate(SEEDS):
        table = dataclasses.replace(sc, camera=camera_rays(kind, sc.camera, sc.width, sc.height, int(seed), lens), projector_type=-1)
        want = expected_occlusion(port, table, [seed], gids, RADIUS, first_spp=i, init=want)
    assert_same(images(r, gids), want, gids, "fisheye with a lens")
    assert len(set(want["sun"].tolist())) > 2 and len(set(want["ao"].tolist())) > 2
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
    want = fold_occlusion(golden("entities"), RADIUS)
    for rank in range(3):
        loader, r = make(gpu_instance, sc)
        r.set_shard(rank, 3, tile)
        r.render_occlusion(SEEDS, RADIUS)
        got = images(r)
        mine = owner(sc, 3, tile) == rank
        assert mine.any() and not mine.all()
        assert_same({k: v[mine] for k, v in got.items()}, {k: v[mine] for k, v in want.items()}, ALL[mine], f"rank {rank} of 3, tile {tile}")
        for k in IMAGES:
            assert not bits(got[k][~mine]).any(), k
        close(r, loader)


def test_group_equals_one_context(gpu_instance, golden):
    g = RendererInstance.group([0, 0])
    sc = gs.make("entities")
    lg, rg = make(g, sc)
    rg.render_occlusion(SEEDS[:2], RADIUS)
    rg.render_occlusion(SEEDS[2:], RADIUS, first_buffer_spp=2)
    assert_same(images(rg), fold_occlusion(golden("entities"), RADIUS), ALL, "a two-member group")
    info = rg.occlusion_info()
    assert info["bvh"] and info["launches"] == 1, info
    assert rg.occlusion_time()[1] == 2
    rg.reset_occlusion()
    assert not any(bits(v).any() for v in images(rg).values())
    close(rg, lg, g)


def test_bvh_cull_option(gpu_instance, golden):
    loader, r = make(gpu_instance, gs.make("entities"))
    r.set_option(native.OPT_BVH_CULL_BEHIND, 1)
    r.render_occlusion(SEEDS, RADIUS)
    assert r.occlusion_info()["bvh"]
    assert_same(images(r), fold_occlusion(golden("entities", cull=True), RADIUS), ALL, "entities, BVH cull")
    close(r, loader)


def test_ignored_options_change_nothing(gpu_instance, golden):
    """CHUNKY_OPT_MAX_DEPTH and CHUNKY_OPT_SUN_SAMPLING do not reach the pass: it follows the scene's sun flag."""
    loader, r = make(gpu_instance, gs.make("outdoor"))
    r.set_option(native.OPT_MAX_DEPTH, 1)
    r.set_option(native.OPT_SUN_SAMPLING, 0)
    r.render_occlusion(SEEDS, RADIUS)
    assert_same(images(r), fold_occlusion(golden("outdoor"), RADIUS), ALL, "outdoor, max depth 1, sun sampling off")
    close(r, loader)


def test_set_sun_takes_effect_in_the_next_call(gpu_instance, golden):
    on, off = gs.make("outdoor"), gs.make("outdoor_nosun")
    loader, r = make(gpu_instance, on)
    r.render_occlusion(SEEDS, RADIUS)
    assert_same(images(r), fold_occlusion(golden("outdoor"), RADIUS), ALL, "sun on")
    s = np.ascontiguousarray(off.sun, np.int32)
    check(native.lib().chunky_scene_set_sun(loader._h, ptr(s)))
    r.reset_occlusion()
    r.render_occlusion(SEEDS, RADIUS)
    got = images(r)
    lf, fresh = make(gpu_instance, off)
    fresh.render_occlusion(SEEDS, RADIUS)
    assert_same(got, images(fresh), ALL, "after set_sun, against a fresh upload")
    assert_same(got, fold_occlusion(golden("outdoor_nosun"), RADIUS), ALL, "after set_sun, against the specification")
    close(r, loader, fresh, lf)


def other_state(r):
    """every image of the target the occlusion calls must not touch, as bytes"""
    out = {"beauty": r.read().tobytes()}
    for which in range(native.AOV_BLOCK + 1):
        out[f"aov {which}"] = r.read_aov_ex(which).tobytes()
    ids, counts, other, passes = r.read_matte()
    out.update({"matte ids": ids.tobytes(), "matte counts": counts.tobytes(), "matte other": other.tobytes(), "matte passes": passes})
    return out


def test_isolation(gpu_instance):
    sc = gs.make("entities")
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    r.render_aov_ex(SEEDS)
    r.render_matte(SEEDS)
    before = other_state(r)
    timers = (r.kernel_time()[1], r.aov_kernel_time()[1], r.matte_kernel_time()[1])
    assert min(timers) >= 1
    r.render_occlusion(SEEDS, RADIUS)
    assert other_state(r) == before
    assert (r.kernel_time()[1], r.aov_kernel_time()[1], r.matte_kernel_time()[1]) == (0, 0, 0)   # (drained above: no other timer saw the launch)
    assert r.occlusion_time()[1] == 1
    held = {k: bits(v).tobytes() for k, v in images(r).items()}
    assert any(np.frombuffer(v, np.uint32).any() for v in held.values())
    # chunky_render_aov_reset, _matte_reset and chunky_render_reset leave AO and SUN alone
    r.reset_aov()
    r.reset_matte()
    r.reset()
    assert {k: bits(v).tobytes() for k, v in images(r).items()} == held
    assert not np.frombuffer(r.read_aov_ex(native.AOV_ALPHA).tobytes(), np.uint32).any()
    # render passes after an occlusion pass equal render passes without one
    r.render_passes(SEEDS)
    assert r.read().tobytes() == before["beauty"]
    r.reset_occlusion()
    assert not any(bits(v).any() for v in images(r).values())
    close(r, loader)


def test_abi_errors_on_a_device(gpu_instance):
    L = native.lib()
    sc = gs.make("outdoor")
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    seeds = native.java_random_ints(2)
    n = sc.width * sc.height
    out = np.zeros(n, np.float32)
    assert L.chunky_render_occlusion_passes(r._h, seeds.ctypes.data, 2, 0, 4.0) == native.E_STATE   # before set_camera
    r.set_camera(sc.projector_type, sc.camera)
    for which in (native.AOV_AO, native.AOV_SUN):
        assert L.chunky_render_occlusion_read(r._h, which, out.ctypes.data, n) == native.E_STATE      # before the first pass
    assert L.chunky_render_occlusion_reset(r._h) == 0                                                # (nothing to zero)
    for radius in (0.0, -2.0, float("nan")):
        assert L.chunky_render_occlusion_passes(r._h, seeds.ctypes.data, 2, 0, radius) == native.E_INVALID
    assert L.chunky_render_occlusion_read(r._h, native.AOV_AO, out.ctypes.data, n) == native.E_STATE  # a refused call allocates nothing
    assert L.chunky_render_occlusion_passes(r._h, seeds.ctypes.data, -1, 0, 4.0) == native.E_INVALID
    assert L.chunky_render_occlusion_passes(r._h, None, 2, 0, 4.0) == native.E_INVALID
    assert L.chunky_render_occlusion_passes(r._h, seeds.ctypes.data, 2, -3, 4.0) == native.E_INVALID
    assert L.chunky_render_occlusion_passes(r._h, None, 0, 0, 4.0) == 0                              # n == 0: allocates the images
    assert r.occlusion_info()["launches"] == 0 and r.occlusion_time()[1] == 0
    for which in (native.AOV_AO, native.AOV_SUN):
        out[:] = 1
        assert L.chunky_render_occlusion_read(r._h, which, out.ctypes.data, n) == 0 and not out.any()
    for which in (-1, 0, native.AOV_BLOCK, 9):
        assert L.chunky_render_occlusion_read(r._h, which, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_occlusion_read(r._h, native.AOV_AO, out.ctypes.data, n - 1) == native.E_INVALID
    assert L.chunky_render_occlusion_read(r._h, native.AOV_SUN, out.ctypes.data, 3 * n) == native.E_INVALID
    assert L.chunky_render_occlusion_read(r._h, native.AOV_AO, None, n) == native.E_INVALID
    assert L.chunky_render_occlusion_kernel_info(r._h, None) == native.E_INVALID
    assert L.chunky_render_aov_read_ex(r._h, native.AOV_AO, out.ctypes.data, n) == native.E_INVALID   # the AOV's read does not know them
    r.render_occlusion(seeds, float("inf"))
    held = images(r)
    assert L.chunky_render_occlusion_passes(r._h, None, 0, 2, 4.0) == 0                              # n == 0 changes nothing
    assert all(bits(images(r)[k]).tobytes() == bits(held[k]).tobytes() for k in IMAGES)
    close(r, loader)
