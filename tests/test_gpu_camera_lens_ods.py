"""The lens (chunky_render_set_lens) and the ODS projector types 7 / 8 on the device.  The equivalence of DESIGN.md section 11 carries
over: a pass with projected camera k, lens L and seed s is, bit for bit, the pass with seed s on projector type -1 fed the table
chunky_camera_rays_lens(k, ..., s, L).  Every image here is checked against the reference build or the C restatement rendering
those tables pass by pass; every comparison is bit for bit.  The cameras are those of tests/test_camera_lens_ods_cpu.py, which
shows on the host that their lens moves more than 99 % of the rays."""
import dataclasses

import numpy as np
import pytest

import golden_scenes as gs
from aov_spec import expected_aov
from chunkyclplugin_amd import native, parallel, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays
from oracle import binding
from test_camera_lens_ods_cpu import GPU_LENS, OLD_TYPES, projected

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
SEEDS = native.java_random_ints(4, seed=86420)
SEEDS_B = native.java_random_ints(3, seed=1357)
ODS, STACKED = native.PROJ_ODS, native.PROJ_ODS_STACKED
# (projector type, with its lens of GPU_LENS or without): a spherical lens, the planar lens, one eye, and both eyes with a lens
CAMERAS = [(native.PROJ_FISHEYE, True), (native.PROJ_PARALLEL, True), (ODS, False), (STACKED, True)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lens_of(kind, on):
    return GPU_LENS[kind] if on else None


def table_view(sc, seed, lens):
    """The projector type -1 copy of projected scene sc with `lens` for the pass of `seed`."""
    return dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, sc.width, sc.height, int(seed), lens), projector_type=-1)


def equivalent(lib, sc, lens, seeds, gids=None, first_spp=0):
    """lib's image of projected scene sc with `lens`: pass i on the table of seeds[i] with bufferSpp first_spp + i."""
    res = np.zeros(3 * sc.width * sc.height, np.float32)
    for i, seed in enumerate(seeds):
        h = binding.SceneHandle(table_view(sc, seed, lens))
        one = np.array([seed], np.int32)
        if gids is None:
            lib.render_passes(h, one, first_spp=first_spp + i, res=res, threads=THREADS)
        else:
            lib.render_gids(h, one, gids, first_spp=first_spp + i, res=res, threads=THREADS)
    return res


def make(instance, sc, lens=None, variant=0, options=()):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    if lens is not None:
        r.set_lens(*lens)
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


# ---- the device's rays are the host's table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 48), (37, 23), (1917, 1075)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_rays_equal_the_host_table(gpu_instance, size):
    """Whole tables, so ODS columns 0 and W - 1 and the stacked rows H/2 - 1 and H/2 are among the rays compared.  The stacked image
    needs an even height: at the two ragged sizes it is compared one row taller (37 x 24, 1917 x 1076: still no multiple of 16)."""
    w, h = size
    cases = [(k, True) for k in OLD_TYPES] + [(ODS, False), (ODS, True), (STACKED, False), (STACKED, True)]
    for height in sorted({h, h + h % 2}):
        sc = scenes.tiny_scene(width=w, height=height)
        loader = HipSceneLoader(gpu_instance)
        loader.load_packed(sc)
        r = HipPathTracingRenderer(loader, w, height)
        for kind, on in cases:
            if height % 2 != 0 if kind == STACKED else height != h:
                continue   # the stacked image on the even height, every other camera on the stated one
            s = projected(sc, kind, (30.0, 200.0) if kind == native.PROJ_PARALLEL else None).camera
            lens = lens_of(kind, on)
            r.set_camera(kind, s)
            if on:
                r.set_lens(*lens)
            for seed in (0, -1155484576) if w > 1000 else (0, 1, -1155484576, 2147483647):
                host = camera_rays(kind, s, w, height, seed, lens)
                diff = int((bits(r.camera_rays(seed)) != bits(host)).sum())
                assert diff == 0, f"type {kind} lens {lens} seed {seed} at {w} x {height}: {diff} floats differ"
            if kind == STACKED and not on:
                t = host.reshape(height, w, 6)
                assert not np.array_equal(bits(t[height // 2 - 1, :, :3]), bits(t[height // 2, :, :3]))   # the eye changes there
        close(r, loader)


def test_device_rays_at_the_fisheye_centre_and_the_basis_tie(gpu_instance):
    """A fisheye so narrow that ax^2 + ay^2 underflows has a == 0 at every pixel: the local direction is (0, 0, 1), the centre
    pixel's branch, and |ld.x| == |ld.y| there, the tie of the lens basis."""
    w, h = 64, 48
    sc = scenes.tiny_scene(width=w, height=h)
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, w, h)
    s = np.concatenate([[1.0, 2.0, 3.0], np.eye(3).reshape(-1), [0.0, 0.0, 1e-30]]).astype(np.float32)
    off = camera_rays(native.PROJ_FISHEYE, s, w, h, 9).reshape(-1, 6)
    assert (off[:, 3:] == np.array([0, 0, 1], np.float32)).all()
    r.set_camera(native.PROJ_FISHEYE, s)
    assert np.array_equal(bits(r.camera_rays(9)), bits(off.reshape(-1)))
    r.set_lens(0.4, 14.0)
    on = camera_rays(native.PROJ_FISHEYE, s, w, h, 9, (0.4, 14.0))
    assert np.array_equal(bits(r.camera_rays(9)), bits(on))
    assert (bits(on).reshape(-1, 6) != bits(off)).any(axis=1).mean() > 0.99
    close(r, loader)


# ---- whole images and previews of golden scenes against the reference build -------------------------------------------------------
@pytest.mark.parametrize("kind,on", CAMERAS + [(native.PROJ_PANORAMIC, True), (native.PROJ_PANORAMIC_SLOT, True), (native.PROJ_STEREOGRAPHIC, True)])
@pytest.mark.parametrize("name", ["outdoor", "indoor_sun", "entities"])
def test_golden_scenes_equal_the_reference_on_the_tables(gpu_instance, ref, name, kind, on):
    sc = projected(gs.make(name), kind)
    lens = lens_of(kind, on)
    loader, r = make(gpu_instance, sc, lens)
    r.render_passes(SEEDS[:3])
    assert_same(r.read(), equivalent(ref, sc, lens, SEEDS[:3]), f"{name} type {kind} lens {lens}")
    np.testing.assert_array_equal(r.preview(), ref.preview(binding.SceneHandle(table_view(sc, 0, lens))))
    r.render_passes(SEEDS[3:], first_buffer_spp=3)
    assert_same(r.read(), equivalent(ref, sc, lens, SEEDS), f"{name} type {kind} lens {lens}, 4 passes")
    # a second seed set into a buffer that already holds samples
    r.reset()
    r.render_passes(SEEDS_B, first_buffer_spp=5)
    assert_same(r.read(), equivalent(ref, sc, lens, SEEDS_B, first_spp=5), f"{name} type {kind} lens {lens}, bufferSpp 5")
    close(r, loader)


# ---- the timed instantiation: the 1080p outdoor world, render_pool<17, 64> ----------------------------------------------------------
TIMED_ROWS = (0, 269, 539, 540, 811, 1079)   # the first and the last row, the two at H/2 where the stacked image changes eye


@pytest.mark.parametrize("kind,on", [(native.PROJ_PANORAMIC, True), (STACKED, False)])
def test_timed_kernel_rows_equal_the_restatement(gpu_instance, port, kind, on):
    sc = projected(gs.timed_view("outdoor"), kind)
    lens = lens_of(kind, on)
    seeds = SEEDS[:2]
    loader, r = make(gpu_instance, sc, lens)
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["tree"] == 17 and info["pool"] == 64 and not info["bvh"] and not info["ext"], info
    gids = row_gids(sc, TIMED_ROWS)
    want = equivalent(port, sc, lens, seeds, gids).reshape(-1, 3)
    assert_same(r.read().reshape(-1, 3)[gids], want[gids], f"timed type {kind} lens {lens}")
    if kind == STACKED:   # ... and on one share of 16 x 16 blocks
        r.reset()
        r.set_shard(5, 8, 0)
        r.render_passes(seeds)
        own = np.intersect1d(parallel.owned_gids(sc.width * sc.height, 5, 8, 0, sc.width), gids)
        assert own.size > 1000
        assert_same(r.read().reshape(-1, 3)[own], want[own], "timed ODS stacked, shard 5 of 8")
    close(r, loader)


# ---- routes ----------------------------------------------------------------------------------------------------------------------
def test_one_launch_of_300_passes_reads_its_seeds_from_device_memory(gpu_instance, port):
    sc = projected(gs.make("outdoor", gs.DEEP_CHUNKS), STACKED)
    lens = GPU_LENS[STACKED]
    seeds = native.java_random_ints(300, seed=2424)
    loader, r = make(gpu_instance, sc, lens)
    r.kernel_time()
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["passes_per_launch"] > 256 and r.kernel_time()[1] == 1, info
    assert_same(r.read(), equivalent(port, sc, lens, seeds), "300 passes in one launch")
    close(r, loader)


@pytest.mark.parametrize("kind,on", CAMERAS)
@pytest.mark.parametrize("name", ["outdoor", "entities"])
def test_fallback_kernels_give_the_same_images(gpu_instance, port, name, kind, on):
    """CHUNKY_OPT_KERNEL bit 1 (render_lanes) and bit 3 (render_waves) reach the lens and ODS through primary_ray_any, as do the
    preview and the record tracer."""
    sc = projected(gs.make(name, gs.DEEP_CHUNKS if name != "entities" else 2), kind)
    lens = lens_of(kind, on)
    seeds = SEEDS[:3]
    want = equivalent(port, sc, lens, seeds)
    gids = gs.RECORD_GIDS[::4]
    lt, t = make(gpu_instance, table_view(sc, seeds[0], lens))
    want_rec = t.trace_records(int(seeds[0]), gids)
    close(t, lt)
    for variant in (0, 2, 8):
        loader, r = make(gpu_instance, sc, lens, variant)
        r.render_passes(seeds)
        info = r.kernel_info()   # render_pool parks paths (pool >= 0); render_waves has lanes per pixel (group >= 1), render_lanes none
        ran = "pool" if info["pool"] >= 0 else ("waves" if info["group"] >= 1 else "lanes")
        assert ran == {0: "pool", 2: "lanes", 8: "waves"}[variant], (variant, info)
        assert_same(r.read(), want, f"{name} type {kind} lens {lens} variant {variant}")
        np.testing.assert_array_equal(r.preview(), port.preview(binding.SceneHandle(table_view(sc, 0, lens))))
        for g, w in zip(r.trace_records(int(seeds[0]), gids), want_rec):
            assert g.tobytes() == w.tobytes(), f"trace_records, variant {variant}"
        close(r, loader)


@pytest.mark.parametrize("kind,on", [(native.PROJ_FISHEYE, True), (STACKED, True), (ODS, False)])
@pytest.mark.parametrize("chunks,tree", [(2, 16), (gs.DEEP_CHUNKS, 17)])
def test_sorted_block_tests_give_the_same_images(gpu_instance, port, chunks, tree, kind, on):
    """CHUNKY_OPT_KERNEL bit 8: proj::render_pool<16 / 17, 64, ..., SORT = true>; with bit 2 its phase-profile (STATS) form, which
    exists for the generic walk (-1) and for form 17 only: the depth-6 world's runs as <-1, 64, true, ..., true>."""
    sc = projected(gs.make("outdoor", chunks), kind)
    lens = lens_of(kind, on)
    seeds = SEEDS[:3]
    want = equivalent(port, sc, lens, seeds)
    for variant in (256, 256 | 4):
        loader, r = make(gpu_instance, sc, lens, variant)
        r.render_passes(seeds)
        info = r.kernel_info()
        want_tree = tree if variant == 256 or tree == 17 else -1
        assert info["sorted"] and info["tree"] == want_tree and info["pool"] == 64 and not info["bvh"] and not info["ext"], (variant, info)
        assert_same(r.read(), want, f"outdoor form {tree} type {kind} lens {lens} variant {variant}")
        close(r, loader)


def test_extended_integrator_equals_the_restatement(gpu_instance, port):
    from oracle.binding import PortExt
    from test_gpu_extensions import with_spec_words
    kind = native.PROJ_FISHEYE
    sc = projected(with_spec_words(gs.make("indoor", gs.DEEP_CHUNKS)), kind)
    lens = GPU_LENS[kind]
    seeds = SEEDS[:3]
    loader, r = make(gpu_instance, sc, lens, options=((native.OPT_EMITTER_NEE, 1), (native.OPT_BSDF, 1)))
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["ext"] and info["pool"] > 0, info
    with PortExt(port, sc, nee=1, bsdf=1):
        want = equivalent(port, sc, lens, seeds)
    assert_same(r.read(), want, "extended integrator, fisheye with a lens")
    assert not np.array_equal(bits(want), bits(equivalent(port, sc, lens, seeds))), "the options changed nothing"
    close(r, loader)


@pytest.mark.parametrize("name,kind,on", [("outdoor", native.PROJ_FISHEYE, True), ("entities", STACKED, True), ("indoor", ODS, False)])
def test_aov_is_record_0_on_the_tables(gpu_instance, port, name, kind, on):
    sc = projected(gs.make(name), kind)
    lens = lens_of(kind, on)
    seeds = SEEDS[:2]
    loader, r = make(gpu_instance, sc, lens)
    r.render_aov(seeds)
    gids = np.arange(0, sc.width * sc.height, 3)   # (a third of the image: the oracle traces one sample per call)
    want = None
    for i, seed in enumerate(seeds):
        want = expected_aov(port, binding.SceneHandle(table_view(sc, seed, lens)), [seed], gids, first_spp=i, init=want)
    for which, w, what in ((native.AOV_ALBEDO, want[0], "albedo"), (native.AOV_NORMAL, want[1], "normal")):
        assert_same(r.read_aov(which).reshape(-1, 3)[gids], w, f"{name} type {kind} lens {lens} AOV {what}")
    close(r, loader)


def test_adaptive_run_equals_the_specification_on_the_tables_samples(gpu_instance, port):
    """The pixel-list route of render_pool: the rounds after the first check render from a list."""
    from test_adaptive_cpu import params
    from test_gpu_adaptive import check_against_samples
    kind = native.PROJ_PANORAMIC
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind]
    seeds = native.java_random_ints(24)
    s = np.stack([equivalent(port, sc, lens, [int(k)]).reshape(sc.height, sc.width, 3) for k in seeds])
    loader, r = make(gpu_instance, sc, lens)
    counts, _ = check_against_samples(r, s, seeds, params(8, 4, 0.1), "panoramic with a lens")
    assert len(np.unique(counts)) >= 2 and (counts < len(seeds)).any() and (counts == len(seeds)).any()
    close(r, loader)


def test_two_member_group_on_one_device(port):
    g = RendererInstance.group([0, 0])
    sc = projected(gs.make("outdoor"), STACKED)
    lens = GPU_LENS[STACKED]
    seeds = SEEDS[:3]
    loader, r = make(g, sc, lens)   # set_lens reaches both members
    r.render_passes(seeds)
    assert_same(r.read(), equivalent(port, sc, lens, seeds), "group of two")
    np.testing.assert_array_equal(r.preview(), port.preview(binding.SceneHandle(table_view(sc, 0, lens))))
    np.testing.assert_array_equal(bits(r.camera_rays(SEEDS[0])), bits(camera_rays(sc.projector_type, sc.camera, sc.width, sc.height, int(SEEDS[0]), lens)))
    close(r, loader, g)


# ---- state -----------------------------------------------------------------------------------------------------------------------
def test_lens_state_and_refusals(gpu_instance, port):
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind]
    seeds = SEEDS[:2]
    L = native.lib()
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    assert L.chunky_render_set_lens(r._h, 0.1, 5.0) == native.E_STATE          # no camera yet
    for typ, cam in ((0, gs.make("outdoor").camera), (-1, gs.make("pregen").camera)):
        r.set_camera(typ, cam)
        assert L.chunky_render_set_lens(r._h, 0.1, 5.0) == native.E_STATE      # they have their own aperture or table
        assert L.chunky_render_set_lens(r._h, 0.0, 0.0) == native.E_STATE
    r.set_camera(kind, sc.camera)
    r.set_lens(*lens)
    want_on = equivalent(port, sc, lens, seeds)
    want_off = equivalent(port, sc, None, seeds)
    assert not np.array_equal(bits(want_on), bits(want_off))
    for bad in ((np.nan, 5.0), (0.1, np.inf), (-0.1, 5.0), (0.1, 0.0), (0.1, -1.0)):
        assert L.chunky_render_set_lens(r._h, *bad) == native.E_INVALID
    r.render_passes(seeds)
    assert_same(r.read(), want_on, "a refused set_lens leaves the lens as it was")
    # refused cameras leave camera and lens in place; an accepted one clears the lens
    bad_cam = sc.camera.copy()
    bad_cam[14] = -1.0
    assert L.chunky_render_set_camera(r._h, kind, bad_cam.ctypes.data, 15) == native.E_INVALID
    assert L.chunky_render_set_camera(r._h, 6, sc.camera.ctypes.data, 15) == native.E_INVALID
    r.reset()
    r.render_passes(seeds)
    assert_same(r.read(), want_on, "refused cameras leave the lens as it was")
    r.set_camera(kind, sc.camera)
    r.reset()
    r.render_passes(seeds)
    assert_same(r.read(), want_off, "set_camera after set_lens renders lens-off")
    r.set_lens(*lens)
    r.set_lens(0.0, 0.0)                                                       # aperture 0 switches it off
    r.reset()
    r.render_passes(seeds)
    assert_same(r.read(), want_off, "aperture 0")
    close(r, loader)


def test_set_lens_ends_a_resumable_adaptive_run(gpu_instance):
    """As set_camera does (tests/test_gpu_adaptive_resume.py test_what_ends_a_state): what a pass renders changes.  A refused call ends nothing."""
    from test_adaptive_cpu import MAX_SPP, SETTINGS, params
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    seeds = native.java_random_ints(MAX_SPP)
    p = params(*SETTINGS[0])
    loader, r = make(gpu_instance, sc, GPU_LENS[kind])
    assert r.render_adaptive_ex(seeds[:12], p)[0]
    assert r.adaptive_state().state.passes == 12
    assert native.lib().chunky_render_set_lens(r._h, -1.0, 5.0) == native.E_INVALID
    assert r.adaptive_state().state.passes == 12
    r.set_lens(*GPU_LENS[kind])   # even the same lens again
    for call in (lambda: r.resume_adaptive(seeds, p), r.adaptive_state):
        with pytest.raises(native.ChunkyHipError) as e:
            call()
        assert e.value.code == native.E_STATE, e.value
    close(r, loader)


def test_ods_settings_are_validated_by_set_camera(gpu_instance, port):
    sc = projected(gs.make("outdoor"), ODS)
    loader, r = make(gpu_instance, sc)
    L = native.lib()
    for kind in (ODS, STACKED):
        s = projected(sc, kind).camera
        for i, v in ((12, 0.1), (14, 0.0), (14, -5.0), (13, np.nan), (3, np.nan), (0, np.inf)):
            bad = s.copy()
            bad[i] = v
            assert L.chunky_render_set_camera(r._h, kind, bad.ctypes.data, 15) == native.E_INVALID
        assert L.chunky_render_set_camera(r._h, kind, s.ctypes.data, 14) == native.E_INVALID
    neg = projected(sc, STACKED).camera
    neg[13] = -0.0345
    assert L.chunky_render_set_camera(r._h, STACKED, neg.ctypes.data, 15) == native.E_INVALID
    assert L.chunky_render_set_camera(r._h, 6, sc.camera.ctypes.data, 15) == native.E_INVALID
    r.render_passes(SEEDS[:1])
    assert_same(r.read(), equivalent(port, sc, None, SEEDS[:1]), "after refusals")
    close(r, loader)
    # an odd height refuses the stacked image, and only that
    odd = sc.with_view(64, 47)
    loader, r = make(gpu_instance, odd)
    assert L.chunky_render_set_camera(r._h, STACKED, projected(odd, STACKED).camera.ctypes.data, 15) == native.E_INVALID
    r.render_passes(SEEDS[:1])
    assert_same(r.read(), equivalent(port, odd, None, SEEDS[:1]), "odd height, single eye")
    close(r, loader)
