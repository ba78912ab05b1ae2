"""chunky_render_aov_passes_ex / _read_ex (csrc/aov.hip AovExFold) and chunky_filter_frame_alpha on the device, bit for bit
against their specification restated on the C restatement of the reference (aov_ex_spec.expected_aov_ex: record 0 of the sample,
seven images folded from it; tests/test_aov_ex_cpu.py shows the restatement means the same on the reference build): the golden
scenes whole, every tree form, a call split in two, the launch cut, a projected camera with a lens, shards, a group, the BVH cull
option, the timed instantiations on whole rows, the line-up with chunky_render_aov_passes, the untouched beauty buffer, the ABI's errors, and the
tone map's alpha byte."""
import dataclasses

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from aov_ex_spec import IMAGES, WHICH, WORDS, alpha_byte, expected_aov_ex
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipPostProcessingFilter, HipSceneLoader, RendererInstance, camera_rays
from test_aov_ex_cpu import boundary_values
from test_camera_lens_ods_cpu import GPU_LENS, projected

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(gs.N_PASSES)


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
    """{image name: (pixels, words per pixel)} as chunky_render_aov_read_ex delivers them"""
    out = {k: r.read_aov_ex(WHICH[k]).reshape(-1, WORDS[k]) for k in IMAGES}
    assert out["block"].dtype == np.int32 and all(out[k].dtype == np.float32 for k in IMAGES if k != "block")
    return out if gids is None else {k: v[gids] for k, v in out.items()}


def assert_same(got, want, gids, what):
    for k in IMAGES:
        same = (bits(got[k]) == bits(want[k])).all(axis=1)
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what}: {k} differs at {int((~same).sum())} of {len(same)} pixels (first gid {int(gids[i])}: "
                        f"{got[k][i].tolist()} against {want[k][i].tolist()})")


@pytest.fixture(scope="module")
def golden(port):
    """The restatement of the golden scenes' whole images after SEEDS, computed once per scene and never changed."""
    cache = {}

    def get(name, cull=False):
        if (name, cull) not in cache:
            sc = gs.make(name)
            with binding.PortCull(port, cull):
                cache[name, cull] = expected_aov_ex(port, binding.SceneHandle(sc), SEEDS, np.arange(sc.width * sc.height))
        return {k: v.copy() for k, v in cache[name, cull].items()}
    return get


ALL = np.arange(gs.W * gs.H)


@pytest.mark.parametrize("name", gs.NAMES)
def test_golden_scene_whole_images(gpu_instance, golden, name):
    sc = gs.make(name)
    loader, r = make(gpu_instance, sc)
    r.render_aov_ex(SEEDS)
    got = images(r)
    assert_same(got, golden(name), ALL, name)
    assert r.aov_info()["launches"] == 1
    # albedo and normal are those of chunky_render_aov_passes, through either read call
    lp, plain = make(gpu_instance, sc)
    plain.render_aov(SEEDS)
    for k in ("albedo", "normal"):
        want = plain.read_aov(WHICH[k])
        assert bits(r.read_aov(WHICH[k])).tobytes() == bits(want).tobytes() == bits(got[k]).tobytes(), k
    hit = got["alpha"][:, 0] > 0
    assert hit.any() and (got["depth"][hit] > 0).all()
    close(r, loader, plain, lp)


FORM_CASES = list(gs.form_cases(ragged=True))


@pytest.mark.parametrize("key,build,kernel", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_tree_forms(gpu_instance, port, key, build, kernel):
    """The lookup forms 17 / 18 / 19 / 0 and the entity form 18 with the walk, whole images; the form-19 case at 33 x 17."""
    sc = build()
    loader, r = make(gpu_instance, sc)
    r.render_aov_ex(SEEDS)
    info = r.aov_info()
    assert (info["tree"], info["bvh"]) == kernel, info
    if (sc.width, sc.height) == gs.RAGGED_VIEW:
        assert info["blocks"] == 6   # 24 claims, one per wave of four-wave workgroups: the grid cap, not the device's size
    gids = np.arange(sc.width * sc.height)
    assert_same(images(r), expected_aov_ex(port, binding.SceneHandle(sc), SEEDS, gids), gids, key)
    close(r, loader)


def test_two_calls_equal_one(gpu_instance, golden):
    sc = gs.make("entities")
    loader, r = make(gpu_instance, sc)
    r.render_aov_ex(SEEDS[:2])
    r.render_aov_ex(SEEDS[2:], first_buffer_spp=2)
    assert_same(images(r), golden("entities"), ALL, "2 + 1 passes")
    close(r, loader)


def test_launch_cut_is_invisible_and_block_is_the_last_pass(gpu_instance, port):
    sc = gs.make("outdoor").with_view(16, 16)
    seeds = native.java_random_ints(300)
    gids = np.arange(16 * 16)
    loader, r = make(gpu_instance, sc)
    r.render_aov_ex(seeds)
    assert r.aov_info()["launches"] == 2  # 256 + 44
    assert r.aov_kernel_time()[1] == 2
    got = images(r)
    h = binding.SceneHandle(sc)
    want = expected_aov_ex(port, h, seeds, gids)
    assert_same(got, want, gids, "300 passes")
    last = expected_aov_ex(port, h, seeds[299:], gids, first_spp=299)
    np.testing.assert_array_equal(got["block"], last["block"])
    assert (got["block"] == -1).any() and (got["block"] >= 0).any()   # the view has sky and ground in its last pass
    close(r, loader)


def test_projected_camera_with_a_lens(gpu_instance, port):
    """A pass of a projected camera is the pass on the table of its rays, with the lens as without."""
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind]
    loader, r = make(gpu_instance, sc, lens)
    r.render_aov_ex(SEEDS)
    gids = np.arange(0, sc.width * sc.height, 3)
    want = None
    for i, seed in enumerate(SEEDS):
        table = dataclasses.replace(sc, camera=camera_rays(kind, sc.camera, sc.width, sc.height, int(seed), lens), projector_type=-1)
        want = expected_aov_ex(port, binding.SceneHandle(table), [seed], gids, first_spp=i, init=want)
    assert_same(images(r, gids), want, gids, "fisheye with a lens")
    close(r, loader)


def owner(sc, world, tile):
    gid = np.arange(sc.width * sc.height)
    if tile > 0:
        return (gid // tile) % world
    bw = (sc.width + 15) // 16
    return ((gid // sc.width // 16) * bw + (gid % sc.width) // 16) % world


@pytest.mark.parametrize("tile", [0, 7])
def test_shards(gpu_instance, golden, tile):
    """Block shards (tile 0) and run shards of 7 pixels: the rank's pixels are the whole image's, every other word stays 0."""
    sc = gs.make("entities")
    want = golden("entities")
    loader, r = make(gpu_instance, sc)
    r.set_shard(1, 3, tile)
    r.render_aov_ex(SEEDS)
    got = images(r)
    mine = owner(sc, 3, tile) == 1
    assert mine.any() and not mine.all()
    assert_same({k: v[mine] for k, v in got.items()}, {k: v[mine] for k, v in want.items()}, ALL[mine], f"rank 1 of 3, tile {tile}")
    for k in IMAGES:
        assert not bits(got[k][~mine]).any(), k
    close(r, loader)


def test_group_equals_one_context(gpu_instance, golden):
    g = RendererInstance.group([0, 0])
    sc = gs.make("entities")
    lg, rg = make(g, sc)
    rg.render_aov_ex(SEEDS[:2])
    rg.render_aov_ex(SEEDS[2:], first_buffer_spp=2)
    assert_same(images(rg), golden("entities"), ALL, "a two-member group")
    l1, r1 = make(gpu_instance, sc)
    r1.render_aov_ex(SEEDS)
    assert rg.aov_info()["tree"] == r1.aov_info()["tree"] and rg.aov_info()["bvh"]
    rg.reset_aov()
    assert not any(bits(v).any() for v in images(rg).values())
    close(rg, lg, r1, l1, g)


def test_bvh_cull_option(gpu_instance, golden):
    sc = gs.make("entities")
    loader, r = make(gpu_instance, sc)
    r.set_option(native.OPT_BVH_CULL_BEHIND, 1)
    r.render_aov_ex(SEEDS)
    assert r.aov_info()["bvh"]
    assert_same(images(r), golden("entities", cull=True), ALL, "entities, BVH cull")
    close(r, loader)


@pytest.mark.parametrize("name,kernel", [("outdoor", (17, False)), ("entities", (17, True))])
def test_timed_instantiations_on_whole_rows(gpu_instance, port, name, kernel):
    """The outdoor headline view and the entity view at 1920 x 1080: the dense-top forms, which no 64 x 48 scene runs."""
    sc = gs.timed_view(name)
    assert (sc.width, sc.height) == (1920, 1080)
    seeds = SEEDS[:2]
    loader, r = make(gpu_instance, sc)
    r.render_aov_ex(seeds)
    info = r.aov_info()
    assert (info["tree"], info["bvh"]) == kernel, info
    assert info["blocks"] >= 256 and info["launches"] == 1
    gids = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in (411, 799)])
    got = images(r, gids)
    assert_same(got, expected_aov_ex(port, binding.SceneHandle(sc), seeds, gids), gids, name)
    assert got["alpha"].max() == 1 and np.isfinite(got["position"]).all()
    close(r, loader)


def test_beauty_buffer_and_timers_are_untouched(gpu_instance):
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    before, launches, kinfo = r.read().tobytes(), r.kernel_time()[1], r.kernel_info()
    r.render_aov_ex(SEEDS)
    assert r.read().tobytes() == before
    assert r.kernel_time()[1] == 0 and launches >= 1 and r.kernel_info() == kinfo   # (the render timer was drained above)
    ms, n = r.aov_kernel_time()
    assert n == 1 and ms > 0
    # chunky_render_aov_passes leaves the five images alone: they lag behind albedo and normal
    ex = images(r)
    r.render_aov(SEEDS[:1], first_buffer_spp=3)
    after = images(r)
    for k in IMAGES:
        assert (bits(after[k]).tobytes() == bits(ex[k]).tobytes()) == (k not in ("albedo", "normal")), k
    r.reset()   # chunky_render_reset does not touch them, chunky_render_aov_reset zeroes all seven
    assert bits(images(r)["depth"]).tobytes() == bits(ex["depth"]).tobytes()
    r.reset_aov()
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
    out = np.zeros(3 * n, np.float32)
    assert L.chunky_render_aov_passes_ex(r._h, seeds.ctypes.data, 2, 0) == native.E_STATE   # before set_camera
    r.set_camera(sc.projector_type, sc.camera)
    for which in range(7):
        assert L.chunky_render_aov_read_ex(r._h, which, out.ctypes.data, n * native.AOV_WORDS[which]) == native.E_STATE   # nothing rendered
    r.render_aov(seeds)
    assert L.chunky_render_aov_read_ex(r._h, native.AOV_ALBEDO, out.ctypes.data, 3 * n) == 0
    for which in range(2, 7):   # plain AOV passes do not make the five images
        assert L.chunky_render_aov_read_ex(r._h, which, out.ctypes.data, n * native.AOV_WORDS[which]) == native.E_STATE
    assert L.chunky_render_aov_passes_ex(r._h, seeds.ctypes.data, -1, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes_ex(r._h, None, 2, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes_ex(r._h, seeds.ctypes.data, 2, -3) == native.E_INVALID
    assert L.chunky_render_aov_passes_ex(r._h, seeds.ctypes.data, 0, 0) == 0              # allocates the images
    assert L.chunky_render_aov_read_ex(r._h, native.AOV_POSITION, out.ctypes.data, 3 * n) == 0 and not out.any()
    assert L.chunky_render_aov_read_ex(r._h, 7, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_aov_read_ex(r._h, -1, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_aov_read_ex(r._h, native.AOV_DEPTH, out.ctypes.data, 3 * n) == native.E_INVALID
    assert L.chunky_render_aov_read_ex(r._h, native.AOV_POSITION, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_aov_read_ex(r._h, native.AOV_BLOCK, None, n) == native.E_INVALID
    close(r, loader)


# ---- chunky_filter_frame_alpha ------------------------------------------------------------------------------------------------------
def frame(w, h, seed=4):
    rng = np.random.default_rng(seed)
    x = rng.gamma(0.7, 0.6, size=3 * w * h)
    x[::17] = 0.0
    x[5::29] *= 40.0   # beyond white
    return np.ascontiguousarray(x, np.float64)


@pytest.mark.parametrize("size", [(65, 5), (1, 1), (1, 7), (513, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_frame_alpha(gpu_instance, size):
    """RGB byte-identical to chunky_filter_frame for the four curves, the alpha byte the formula's; 513 x 3 takes the kernel's
    whole-tile path and its tail."""
    w, h = size
    x = frame(w, h)
    vals = boundary_values()
    alpha = np.resize(vals, w * h).astype(np.float32) if w * h >= vals.size else vals[[2, 3, 7, 30, 44, 50, 51][:w * h]].copy()
    assert w * h < vals.size or set(bits(vals).tolist()) <= set(bits(alpha).tolist())   # the 65 x 5 image holds every boundary value
    want_alpha = alpha_byte(alpha)
    for fid in ("GAMMA", "TONEMAP1", "TONEMAP2", "TONEMAP3"):
        f = HipPostProcessingFilter(fid, gpu_instance)
        plain = np.zeros(w * h, np.uint32)
        got = np.zeros(w * h, np.uint32)
        f.process_frame(w, h, x, plain, 1.3)
        f.process_frame_alpha(w, h, x, alpha, got, 1.3)
        assert (plain >> 24 == 0xFF).all()
        np.testing.assert_array_equal(got & 0xFFFFFF, plain & 0xFFFFFF, err_msg=fid)
        np.testing.assert_array_equal(got >> 24, want_alpha, err_msg=fid)


def test_filter_frame_alpha_errors(gpu_instance):
    L = native.lib()
    x, a, out = frame(2, 2), np.ones(4, np.float32), np.zeros(4, np.int32)
    h = gpu_instance._h
    assert L.chunky_filter_frame_alpha(h, 2, 2, 1.0, x.ctypes.data, None, out.ctypes.data, 0) == native.E_INVALID
    assert L.chunky_filter_frame_alpha(h, -1, 2, 1.0, x.ctypes.data, a.ctypes.data, out.ctypes.data, 0) == native.E_INVALID
    assert L.chunky_filter_frame_alpha(h, 0, 2, 1.0, None, None, None, 0) == 0   # an empty frame, as chunky_filter_frame
    assert L.chunky_filter_frame_alpha(h, 2, 2, 1.0, x.ctypes.data, a.ctypes.data, out.ctypes.data, 0) == 0
    assert (out.view(np.uint32) >> 24 == 255).all()
