"""Projected cameras (projector types 1-5) on the device.  The equivalence of DESIGN.md section 11: a pass with projected camera k and
seed s is, bit for bit, the pass with seed s on projector type -1 fed the table R_k(s) = chunky_camera_rays(k, ..., s).  So every
image here is checked against the reference build (or the C restatement, where the reference has no counterpart or a whole
1080p image per case would take too long on the host) rendering those tables pass by pass."""
import dataclasses
import math

import numpy as np
import pytest

import golden_scenes as gs
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays
from oracle import binding

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
TYPES = [native.PROJ_PARALLEL, native.PROJ_FISHEYE, native.PROJ_PANORAMIC, native.PROJ_PANORAMIC_SLOT, native.PROJ_STEREOGRAPHIC]
SEEDS = native.java_random_ints(4, seed=97531)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def projected(sc, kind, parallel=(20.0, 48.0)):
    """sc's pinhole camera (position and rotation) as projected camera `kind`."""
    base = np.asarray(sc.camera if sc.projector_type == 0 else gs.make("outdoor").camera, np.float32)[:15].copy()
    base[12] = 0.0
    base[13], base[14] = {native.PROJ_PARALLEL: parallel, native.PROJ_FISHEYE: (0.0, 180.0), native.PROJ_PANORAMIC: (0.0, 240.0),
                          native.PROJ_PANORAMIC_SLOT: (2.0 * math.tan(math.radians(35.0)), 150.0),
                          native.PROJ_STEREOGRAPHIC: (0.0, 2.0 * math.tan(math.radians(160.0) / 4.0))}[kind]
    return dataclasses.replace(sc, camera=base, projector_type=kind)


def table_view(sc, seed):
    """The projector type -1 copy of projected scene sc for the pass of `seed`: R_k(seed)."""
    return dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, sc.width, sc.height, int(seed)), projector_type=-1)


def equivalent(lib, sc, seeds, gids=None, first_spp=0):
    """lib's image of projected scene sc: pass i on R_k(seeds[i]) with bufferSpp first_spp + i."""
    res = np.zeros(3 * sc.width * sc.height, np.float32)
    for i, seed in enumerate(seeds):
        h = binding.SceneHandle(table_view(sc, seed))
        one = np.array([seed], np.int32)
        if gids is None:
            lib.render_passes(h, one, first_spp=first_spp + i, res=res, threads=THREADS)
        else:
            lib.render_gids(h, one, gids, first_spp=first_spp + i, res=res, threads=THREADS)
    return res


def make(instance, sc, variant=0, options=()):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    for k, v in options:
        r.set_option(k, v)
    return loader, r


def close(*xs):
    for x in xs:
        x.close()


def row_gids(sc, rows):
    return np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in rows]).astype(np.int32)


def assert_same(got, want, what):
    same = (bits(got).reshape(-1, 3) == bits(want).reshape(-1, 3)).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} pixels differ (first {int(np.argmin(same))})"


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_set_camera_takes_the_projected_types_and_rejects_bad_settings(gpu_instance):
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    L = native.lib()
    for kind in TYPES:
        s = projected(sc, kind).camera
        r.set_camera(kind, s)
        for i, v in ((12, 0.1), (14, 0.0), (14, -5.0), (3, np.nan), (0, np.inf)):
            bad = s.copy()
            bad[i] = v
            assert L.chunky_render_set_camera(r._h, kind, bad.ctypes.data, 15) == native.E_INVALID
        assert L.chunky_render_set_camera(r._h, kind, s.ctypes.data, 14) == native.E_INVALID
    assert L.chunky_render_set_camera(r._h, 6, s.ctypes.data, 15) == native.E_INVALID
    assert L.chunky_render_set_camera(r._h, 3, np.zeros(15, np.float32).ctypes.data, 15) == native.E_INVALID
    # a refused camera leaves the one before in place: the last accepted (stereographic) still renders its equivalent
    r.render_passes(SEEDS[:1])
    assert_same(r.read(), equivalent(binding.port(), projected(sc, native.PROJ_STEREOGRAPHIC), SEEDS[:1]), "after refusals")
    out = np.zeros(sc.width * sc.height * 6, np.float32)
    assert L.chunky_selftest_camera_rays(r._h, 0, out.ctypes.data, out.size - 1) == native.E_INVALID
    r.set_camera(0, sc.camera)
    assert L.chunky_selftest_camera_rays(r._h, 0, out.ctypes.data, out.size) == native.E_STATE
    close(r, loader)


# ---- the device's rays are the host's table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1920, 1080), (1917, 1075)])
def test_device_rays_equal_the_host_table(gpu_instance, size):
    sc = scenes.tiny_scene(width=size[0], height=size[1])
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, *size)
    for kind in TYPES:
        s = projected(sc, kind, parallel=(30.0, 200.0)).camera
        r.set_camera(kind, s)
        for seed in (0, 1, -1155484576, 2147483647):
            dev = r.camera_rays(seed)
            host = camera_rays(kind, s, size[0], size[1], seed)
            diff = int((bits(dev) != bits(host)).sum())
            assert diff == 0, f"type {kind} seed {seed}: {diff} floats differ"
    close(r, loader)


# ---- whole images of the ten golden scenes against the reference build -----------------------------------------------------------
@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("name", gs.NAMES)
def test_golden_scenes_equal_the_reference_on_the_equivalent_tables(gpu_instance, ref, name, kind):
    sc = projected(gs.make(name), kind)
    seeds = SEEDS[:3]
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    assert_same(r.read(), equivalent(ref, sc, seeds), f"{name} type {kind}")
    np.testing.assert_array_equal(r.preview(), ref.preview(binding.SceneHandle(table_view(sc, 0))))
    # the jitter is fresh every pass: one more pass moves the image
    before = r.read().copy()
    r.render_passes(SEEDS[3:], first_buffer_spp=3)
    assert not np.array_equal(bits(before), bits(r.read()))
    assert_same(r.read(), equivalent(ref, sc, SEEDS), f"{name} type {kind}, 4 passes")
    close(r, loader)


# ---- the timed kernel: 1080p worlds, render_pool<17, 64> --------------------------------------------------------------------------
_TIMED = {}


def timed(kind):
    """fisheye and panoramic on the timed outdoor world at 1920 x 1080, parallel on a ragged 1917 x 1075 view of it"""
    if kind not in _TIMED:
        _TIMED.clear()
        sc = gs.timed_view("outdoor")
        if kind == native.PROJ_PARALLEL:
            sc = sc.with_view(1917, 1075)
        _TIMED[kind] = projected(sc, kind, parallel=(40.0, 260.0))
    return _TIMED[kind]


@pytest.mark.parametrize("kind", [native.PROJ_FISHEYE, native.PROJ_PANORAMIC, native.PROJ_PARALLEL])
def test_timed_kernel_rows_equal_the_restatement(gpu_instance, port, kind):
    sc = timed(kind)
    seeds = SEEDS[:3]
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["tree"] == 17 and info["pool"] == 64 and not info["bvh"] and not info["ext"], info
    gids = row_gids(sc, gs.camera_rows(sc))
    want = equivalent(port, sc, seeds, gids).reshape(-1, 3)[gids]
    assert_same(r.read().reshape(-1, 3)[gids], want, f"timed type {kind}")
    close(r, loader)


def test_timed_kernel_whole_image_equals_the_live_reference(gpu_instance, ref):
    sc = timed(native.PROJ_FISHEYE)
    seeds = SEEDS[:2]
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["tree"] == 17 and info["pool"] == 64, info
    assert_same(r.read(), equivalent(ref, sc, seeds), "timed fisheye, whole image")
    close(r, loader)


def test_entity_view_runs_the_bvh_instantiation(gpu_instance, port):
    _TIMED.clear()
    sc = projected(gs.timed_view("entities"), native.PROJ_PANORAMIC)
    seeds = SEEDS[:2]
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["bvh"] and info["tree"] == 17 and info["pool"] in (16, 32), info
    gids = row_gids(sc, (270, 540, 810))
    want = equivalent(port, sc, seeds, gids).reshape(-1, 3)[gids]
    assert_same(r.read().reshape(-1, 3)[gids], want, "entities panoramic")
    close(r, loader)


# ---- kernel variants, shards, long launches, groups, AOV, the extended integrator ---------------------------------------------------
@pytest.mark.parametrize("kind", [native.PROJ_FISHEYE, native.PROJ_PARALLEL, native.PROJ_STEREOGRAPHIC])
@pytest.mark.parametrize("name", ["outdoor", "entities", "pregen"])
def test_fallback_kernels_give_the_same_images(gpu_instance, port, name, kind):
    """CHUNKY_OPT_KERNEL bit 1 (render_waves) and bit 3 (render_lanes) take the projected camera through primary_ray too."""
    sc = projected(gs.make(name, gs.DEEP_CHUNKS if name != "entities" else 2), kind)
    seeds = SEEDS[:3]
    want = equivalent(port, sc, seeds)
    for variant in (0, 2, 8):
        loader, r = make(gpu_instance, sc, variant)
        r.render_passes(seeds)
        assert_same(r.read(), want, f"{name} type {kind} variant {variant}")
        np.testing.assert_array_equal(r.preview(), port.preview(binding.SceneHandle(table_view(sc, 0))))
        close(r, loader)


def test_block_shards_assemble_the_whole_image(gpu_instance):
    from chunkyclplugin_amd import parallel
    sc = projected(gs.timed_view("outdoor").with_view(333, 211), native.PROJ_PANORAMIC)
    seeds = SEEDS[:2]
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    whole = r.read().copy()
    n = sc.width * sc.height
    assembled = np.zeros((n, 3), np.float32)
    covered = np.zeros(n, np.int32)
    for rank in range(3):
        r.reset()
        r.set_shard(rank, 3, 0)
        r.render_passes(seeds)
        own = parallel.owned_gids(n, rank, 3, 0, sc.width)
        covered[own] += 1
        assembled[own] = r.read().reshape(-1, 3)[own]
    assert (covered == 1).all()
    assert_same(assembled, whole, "16 x 16 block shards")
    close(r, loader)


def test_one_launch_of_300_passes_reads_its_seeds_from_device_memory(gpu_instance, port):
    sc = projected(gs.make("outdoor", gs.DEEP_CHUNKS).with_view(48, 32), native.PROJ_FISHEYE)
    seeds = native.java_random_ints(300, seed=4242)
    loader, r = make(gpu_instance, sc)
    r.kernel_time()
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["passes_per_launch"] > 256 and r.kernel_time()[1] == 1, info
    assert_same(r.read(), equivalent(port, sc, seeds), "300 passes in one launch")
    close(r, loader)


def test_two_member_group_on_one_device(port):
    g = RendererInstance.group([0, 0])
    sc = projected(gs.make("outdoor"), native.PROJ_PANORAMIC_SLOT)
    seeds = SEEDS[:3]
    loader, r = make(g, sc)
    r.render_passes(seeds)
    assert_same(r.read(), equivalent(port, sc, seeds), "group of two")
    np.testing.assert_array_equal(r.preview(), port.preview(binding.SceneHandle(table_view(sc, 0))))
    dev = r.camera_rays(SEEDS[0])
    np.testing.assert_array_equal(bits(dev), bits(camera_rays(sc.projector_type, sc.camera, sc.width, sc.height, int(SEEDS[0]))))
    close(r, loader, g)


@pytest.mark.parametrize("name,kind", [("outdoor", native.PROJ_FISHEYE), ("entities", native.PROJ_PANORAMIC),
                                       ("indoor", native.PROJ_PARALLEL)])
def test_aov_of_a_projected_camera_is_the_aov_of_the_equivalent_tables(gpu_instance, name, kind):
    sc = projected(gs.make(name), kind)
    seeds = SEEDS[:3]
    loader, r = make(gpu_instance, sc)
    r.render_aov(seeds)
    got = [r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL)]
    lt, t = make(gpu_instance, table_view(sc, seeds[0]))
    for i, seed in enumerate(seeds):
        t.set_camera(-1, table_view(sc, seed).camera)
        t.render_aov([seed], first_buffer_spp=i)
    want = [t.read_aov(native.AOV_ALBEDO), t.read_aov(native.AOV_NORMAL)]
    for g, w, what in zip(got, want, ("albedo", "normal")):
        assert_same(g, w, f"{name} type {kind} AOV {what}")
    assert r.aov_info()["tree"] == t.aov_info()["tree"]
    close(r, loader, t, lt)


def test_extended_integrator_equals_the_restatement(gpu_instance, port):
    from oracle.binding import PortExt
    from test_gpu_extensions import with_spec_words
    sc = projected(with_spec_words(gs.make("indoor", gs.DEEP_CHUNKS)), native.PROJ_FISHEYE)
    seeds = SEEDS[:3]
    loader, r = make(gpu_instance, sc, options=((native.OPT_EMITTER_NEE, 1), (native.OPT_BSDF, 1)))
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["ext"] and info["pool"] > 0, info
    with PortExt(port, sc, nee=1, bsdf=1):
        want = equivalent(port, sc, seeds)
    assert_same(r.read(), want, "extended integrator, fisheye")
    assert not np.array_equal(bits(want), bits(equivalent(port, sc, seeds))), "the options changed nothing"
    close(r, loader)
