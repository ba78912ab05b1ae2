"""Canvas windows (chunky_render_set_canvas, include/chunky_hip.h) on the device.  The rule: a window target
stores, at local index g, exactly what a target of the canvas's size stores at canvas index G — every image, bit for bit.  Checked
against the reference build's committed 64 x 48 goldens (tests/golden/), against the C restatement at the window's canvas gids
(oracle/binding.py port) and, for the passes existing tests already tie to the oracle, against the crop of the same call on a target
of the canvas's size.  Windows (tests/test_window_cpu.py): A = 33 x 17 at (19, 11) — offsets and sizes off the 16 x 16 blocks and the
2 x 2 sub-blocks, 3 x 2 blocks with padded edge blocks —, B the same flush with the right and bottom edges, C the last pixel, D the
identity.  Every comparison is == on the bit patterns."""
import os

import numpy as np
import pytest

import biome_spec as bs
import golden_scenes as gs
from aov_ex_spec import expected_aov_ex
from aov_spec import expected_aov
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays, render_tiled
from oracle import binding
from test_camera_lens_ods_cpu import GPU_LENS, TYPES, projected
from test_window_cpu import CH, CW, WINDOWS, canvas_gids, crop

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
THREADS = binding.usable_threads()
A, B, C_, D = (WINDOWS[k] for k in "ABCD")
SEEDS = native.java_random_ints(5, seed=24680)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ (first at {int(np.argmax(bad))})"


def window_target(loader, sc, window, canvas=(CW, CH), variant=0, lens=None, options=(), camera=None, projector_type=None):
    """A target of the window's size on sc's world with sc's camera, declared the window of the canvas."""
    w, h, x0, y0 = window
    r = HipPathTracingRenderer(loader, w, h)
    r.set_canvas(canvas[0], canvas[1], x0, y0)
    r.set_camera(sc.projector_type if projector_type is None else projector_type, sc.camera if camera is None else camera)
    if lens is not None:
        r.set_lens(*lens)
    r.set_option(native.OPT_KERNEL, variant)
    for k, v in options:
        r.set_option(k, v)
    return r


def full_target(loader, sc, variant=0, lens=None, options=()):
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    if lens is not None:
        r.set_lens(*lens)
    r.set_option(native.OPT_KERNEL, variant)
    for k, v in options:
        r.set_option(k, v)
    return r


def load(instance, sc):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    return loader


def close(*xs):
    for x in xs:
        x.close()


def window_camera(sc, window):
    """sc's camera as a window target takes it: a table of pre-generated rays cropped to the window, anything else as it is."""
    if sc.projector_type != -1:
        return sc.camera
    return crop(sc.camera, window, 6, sc.width, sc.height)


# ---- beauty against the reference build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gs.NAMES)
def test_beauty_is_the_crop_of_the_reference_goldens(gpu_instance, port, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sc = gs.make(name)
    assert gs.input_digest(sc) == str(g["digest"]) and len(g["seeds"]) == gs.N_PASSES
    more = SEEDS[:2]
    handle = binding.SceneHandle(sc)
    loader = load(gpu_instance, sc)
    for key in "ABC":
        win = WINDOWS[key]
        r = window_target(loader, sc, win, camera=window_camera(sc, win))
        assert r.canvas() == (CW, CH, win[2], win[3])
        r.render_passes(g["seeds"], first_buffer_spp=0)
        same(r.read(), crop(g["res"], win, 3), f"{name} window {key}")
        # two more passes into the buffer that holds N_PASSES: the C restatement at the window's canvas gids, continued from the golden
        r.render_passes(more, first_buffer_spp=gs.N_PASSES)
        want = port.render_gids(handle, more, canvas_gids(win), first_spp=gs.N_PASSES, res=np.array(g["res"], np.float32).reshape(-1).copy(), threads=THREADS)
        same(r.read(), crop(want, win, 3), f"{name} window {key}, continued")
        r.close()
    loader.close()


# ---- every beauty route -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def form_scenes():
    return {key: (build(), form) for key, build, form in gs.form_cases()}


@pytest.mark.parametrize("key", [k for k, _, _ in gs.form_cases()])
def test_pool_kernel_in_every_tree_form(gpu_instance, port, form_scenes, key):
    sc, (form, bvh) = form_scenes[key]
    assert (sc.width, sc.height) == (CW, CH)
    loader = load(gpu_instance, sc)
    want = port.render_gids(sc, SEEDS[:3], np.concatenate([canvas_gids(A), canvas_gids(B)]), threads=THREADS)
    for win in (A, B):
        r = window_target(loader, sc, win)
        r.render_passes(SEEDS[:3])
        info = r.kernel_info()
        assert info["pool"] >= 0 and info["tree"] == form and info["bvh"] == bvh and not info["ext"], info
        same(r.read(), crop(want, win, 3), f"{key} form {form} window {win}")
        r.close()
    loader.close()


@pytest.mark.parametrize("variant,what", [(2, "render_lanes"), (8, "render_waves"), (8 | 16, "render_waves, one lane per pixel"), (1, "reference octree layout")])
@pytest.mark.parametrize("name", ["entities", "dof", "pregen"])
def test_fallback_routes(gpu_instance, name, variant, what):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sc = gs.make(name)
    loader = load(gpu_instance, sc)
    for key in "ABC":
        win = WINDOWS[key]
        r = window_target(loader, sc, win, variant=variant, camera=window_camera(sc, win))
        r.render_passes(g["seeds"])
        info = r.kernel_info()
        if variant == 2:
            assert info["pool"] < 0 and info["group"] == 0, info
        elif variant & 8:
            assert info["pool"] < 0 and info["group"] >= 1, info
        else:
            assert info["tree"] == 0, info
        same(r.read(), crop(g["res"], win, 3), f"{name} window {key} on {what}")
        r.close()
    loader.close()


# ---- identity -----------------------------------------------------------------------------------------------------------------------
def test_the_identity_window_is_a_target_without_one(gpu_instance):
    g = np.load(os.path.join(GOLD, "entities.npz"))
    sc = gs.make("entities")
    loader = load(gpu_instance, sc)
    plain = full_target(loader, sc)
    assert plain.canvas() == (CW, CH, 0, 0)
    plain.render_passes(g["seeds"])
    r = window_target(loader, sc, D)
    assert r.canvas() == (CW, CH, 0, 0)
    r.render_passes(g["seeds"])
    same(r.read(), plain.read(), "identity")
    same(r.read(), g["res"], "identity against the golden")
    np.testing.assert_array_equal(r.preview(), plain.preview())
    # a window moved and switched off again is the plain target once more; moving it touches no image
    before = bits(r.read()).copy()
    r2 = window_target(loader, sc, A)
    r2.render_passes(g["seeds"])
    a_img = bits(r2.read()).copy()
    r2.set_canvas(CW, CH, B[2], B[3])
    same(r2.read(), a_img, "set_canvas left the image")
    r2.reset()
    r2.render_passes(g["seeds"])
    same(r2.read(), crop(g["res"], B, 3), "moved to B")
    r2.set_canvas(33, 17, 0, 0)
    r2.reset()
    r2.render_passes(g["seeds"])
    small = full_target(loader, sc.with_view(33, 17))
    small.render_passes(g["seeds"])
    same(r2.read(), small.read(), "window switched off")
    same(r.read(), before, "the other target")
    close(plain, r, r2, small, loader)


def test_set_canvas_refusals_change_nothing(gpu_instance, port):
    sc = gs.make("outdoor")
    loader = load(gpu_instance, sc)
    r = window_target(loader, sc, A)
    L = native.lib()
    for args in ((CW, CH, -1, 0), (CW, CH, 32, 11), (CW, CH, 19, 32), (32, CH, 0, 0), (46341, 46341, 0, 0)):
        assert L.chunky_render_set_canvas(r._h, *args) == native.E_INVALID, args
        assert r.canvas() == (CW, CH, A[2], A[3])
    assert L.chunky_render_set_canvas(r._h, 46340, 46340, 46340 - 33, 46340 - 17) == 0
    assert r.canvas() == (46340, 46340, 46340 - 33, 46340 - 17)
    # the stacked ODS camera: an even CANVAS height, checked by whichever of the two calls comes second
    st = projected(sc, native.PROJ_ODS_STACKED)
    r.set_canvas(CW, CH, A[2], A[3])
    r.set_camera(st.projector_type, st.camera)   # window height 17 is odd: the canvas's 48 counts
    assert L.chunky_render_set_canvas(r._h, CW, CH - 1, A[2], A[3]) == native.E_INVALID
    assert r.canvas() == (CW, CH, A[2], A[3])
    r.set_camera(sc.projector_type, sc.camera)
    r.set_canvas(CW, CH - 1, A[2], A[3])
    assert L.chunky_render_set_camera(r._h, st.projector_type, native.ptr(np.ascontiguousarray(st.camera, np.float32)), 15) == native.E_INVALID
    # the refused camera changed nothing: the target still renders the pinhole window of the 64 x 47 canvas
    r.render_passes(SEEDS[:2])
    want = port.render_gids(sc.with_view(CW, CH - 1), SEEDS[:2], canvas_gids(A), threads=THREADS)
    same(r.read(), crop(want, A, 3, CW, CH - 1), "after the refused set_camera")
    close(r, loader)


# ---- far corner: G passes 2^30 and seed + G wraps -----------------------------------------------------------------------------------
def test_far_corner_of_a_40000_square_canvas(gpu_instance, port):
    cw = ch = 40000
    win = (8, 8, 39990, 39985)
    sc = gs.make("outdoor").with_view(cw, ch)
    assert sc.projector_type == 0
    seeds = np.array([SEEDS[0], -5], np.int32)   # G > 2^30; (uint)-5 + G wraps past 2^32
    gids = canvas_gids(win, cw)
    assert int(gids.min()) > 1 << 30 and (int(np.uint32(seeds[1])) + int(gids.min())) >= 1 << 32
    loader = load(gpu_instance, sc)
    r = window_target(loader, sc, win, canvas=(cw, ch))
    r.render_passes(seeds)
    handle = binding.SceneHandle(sc)
    want = np.zeros((64, 3), np.float32)
    for k, seed in enumerate(seeds):
        rad = np.stack([port.trace_records(handle, int(seed), int(G))[1] for G in gids]).astype(np.float32)
        want = ((want * np.float32(k) + rad) / np.float32(k + 1)).astype(np.float32)   # K/rayTracer.cl:109-112, one rounding per operation
    same(r.read(), want, "far corner")
    rec, cnt, rad = r.trace_records(int(seeds[1]), np.arange(64))
    same(rad, np.stack([port.trace_records(handle, int(seeds[1]), int(G))[1] for G in gids]), "far corner records' radiance")
    close(r, loader)


# ---- preview ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["outdoor", "entities", "pregen", "indoor"])
def test_preview_is_the_crop_of_the_golden_preview(gpu_instance, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sc = gs.make(name)
    loader = load(gpu_instance, sc)
    cross = (11, 11, CW // 2 - 5, CH // 2 - 5)   # centred on (32, 24): the whole crosshair and the pixels about it
    for win in (A, B, cross):
        r = window_target(loader, sc, win, camera=window_camera(sc, win))
        got = r.preview()
        np.testing.assert_array_equal(got, crop(g["preview"], win, 1))
        r.close()
    white = crop(g["preview"], cross, 1).reshape(11, 11) == -1
    assert white[5, :].all() and white[:, 5].all()   # the canvas's crosshair lies where the window shows it
    loader.close()


# ---- other outputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["outdoor", "entities", "pregen"])
def test_trace_records_take_local_gids(gpu_instance, port, name):
    sc = gs.make(name)
    handle = binding.SceneHandle(sc)
    loader = load(gpu_instance, sc)
    r = window_target(loader, sc, A, camera=window_camera(sc, A))
    local = np.arange(0, A[0] * A[1], 7, dtype=np.int32)
    G = canvas_gids(A)[local]
    seed = int(SEEDS[1])
    rec, cnt, rad = r.trace_records(seed, local)
    for i, gid in enumerate(G):
        want, wrad = port.trace_records(handle, seed, int(gid))
        assert int(cnt[i]) == len(want), (name, i)
        got = rec[i, :len(want)]
        for f in ("hit", "material"):
            assert got[f].tolist() == want[f].tolist(), (name, i, f)
        for f in ("distance", "normal", "color", "emittance"):
            same(got[f], want[f], f"{name} local gid {local[i]} {f}")
        hit = want["hit"] == 1
        same(got["point"][hit], want["point"][hit], f"{name} point")
        same(rad[i], wrad, f"{name} radiance")
    assert L_invalid(r, A[0] * A[1])   # a gid of the canvas that is no local index
    close(r, loader)


def L_invalid(r, gid):
    g = np.array([gid], np.int32)
    rec = np.zeros((1, native.MAX_TRACES), native.HIT_DTYPE)
    out = np.zeros(4, np.float32)
    return native.lib().chunky_render_trace_records(r._h, 1, native.ptr(g), 1, native.ptr(rec), native.ptr(out.view(np.int32)), native.ptr(out)) == native.E_INVALID


@pytest.mark.parametrize("name", ["entities", "indoor"])
def test_every_other_pass_is_the_crop_of_the_canvas_targets(gpu_instance, port, name):
    sc = gs.make(name)
    seeds = SEEDS[:3]
    loader = load(gpu_instance, sc)
    full, win = full_target(loader, sc), window_target(loader, sc, A)
    ptrs, world_ent, actor_ent = scenes.emitter_ids(sc)
    mapping = {int(p): 1 + i % 2 for i, p in enumerate(ptrs)}
    if world_ent:
        mapping[native.MATTE_WORLD_ENTITY] = 2
    for r in (full, win):
        r.render_aov(seeds)
        r.render_occlusion(seeds, 6.0)
        r.render_matte(seeds)
        r.set_emitter_groups(mapping, 3)
        r.render_lights(seeds)

    def both(read, words, what):
        same(read(win), crop(read(full), A, words), f"{name} {what}")

    for which, what in ((native.AOV_ALBEDO, "albedo"), (native.AOV_NORMAL, "normal")):
        both(lambda r: r.read_aov(which), 3, "AOV " + what)
    for which, what in ((native.AOV_AO, "AO"), (native.AOV_SUN, "SUN")):
        both(lambda r: r.read_occlusion(which), 1, "occlusion " + what)
    for which in (native.LIGHT_SKY, native.LIGHT_SUN, native.LIGHT_EMITTERS, native.LIGHT_ALL):
        both(lambda r: r.read_light(which), 3, f"light image {which}")
    for grp in range(3):
        both(lambda r: r.read_light_group(grp), 3, f"emitter group {grp}")
    assert win.lights_info()["groups"]
    fm, wm = full.read_matte(), win.read_matte()
    assert wm[3] == fm[3] == len(seeds)
    for k, what in ((0, "matte ids"), (1, "matte counts")):
        for slot in range(native.MATTE_SLOTS):
            same(wm[k][slot], crop(fm[k][slot], A, 1), f"{name} {what} slot {slot}")
    same(wm[2], crop(fm[2], A, 1), f"{name} matte other")
    fr, wr = full.matte_ranks(), win.matte_ranks()
    for k in (0, 1):
        for slot in range(native.MATTE_SLOTS):
            same(wr[k][slot], crop(fr[k][slot], A, 1), f"{name} matte ranks {k} slot {slot}")
    # the AOV-ex images replace the AOV's two on the same buffers: after everything above
    for r in (full, win):
        r.reset_aov()
        r.render_aov_ex(seeds)
    for which in (native.AOV_ALBEDO, native.AOV_NORMAL, native.AOV_ALPHA, native.AOV_DEPTH, native.AOV_POSITION, native.AOV_EMITTANCE, native.AOV_BLOCK):
        both(lambda r: r.read_aov_ex(which), native.AOV_WORDS[which], f"AOV-ex image {which}")
    # ... and albedo, normal and ALPHA once more from the oracle's records at the canvas gids
    G = canvas_gids(A)
    ex = expected_aov_ex(port, sc, seeds, G)
    same(win.read_aov_ex(native.AOV_ALBEDO), ex["albedo"], f"{name} albedo from records")
    same(win.read_aov_ex(native.AOV_NORMAL), ex["normal"], f"{name} normal from records")
    same(win.read_aov_ex(native.AOV_ALPHA), ex["alpha"], f"{name} alpha from records")
    win.reset_aov()
    win.render_aov(seeds)
    want_a, want_n = expected_aov(port, sc, seeds, G)
    same(win.read_aov(native.AOV_ALBEDO), want_a, f"{name} AOV albedo from records")
    same(win.read_aov(native.AOV_NORMAL), want_n, f"{name} AOV normal from records")
    close(full, win, loader)


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [False, True], ids=["no-lens", "lens"])
@pytest.mark.parametrize("kind", TYPES)
def test_projected_cameras(gpu_instance, kind, on):
    """Each projected type on window A: the device's rays are the host twin's table; the pass is the pass on that table fed back as type
    -1 on the same window; and it is the crop of the full target's pass.  The stacked ODS window straddles canvas_height / 2 (rows 11 .. 27)."""
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind] if on else None
    seed = int(SEEDS[2])
    loader = load(gpu_instance, sc)
    full, win = full_target(loader, sc, lens=lens), window_target(loader, sc, A, lens=lens)
    table = native.camera_rays_window(kind, sc.camera, A[0], A[1], CW, CH, A[2], A[3], seed, lens)
    same(win.camera_rays(seed), table, f"type {kind} lens {lens}: device rays")
    same(table, crop(camera_rays(kind, sc.camera, CW, CH, seed, lens), A, 6), "host twin")
    fed = window_target(loader, sc, A, camera=table, projector_type=-1)
    for r in (full, win, fed):
        r.render_passes([seed], first_buffer_spp=2)
    same(win.read(), fed.read(), f"type {kind} lens {lens}: the table fed back")
    same(win.read(), crop(full.read(), A, 3), f"type {kind} lens {lens}: crop of the full target")
    if kind == native.PROJ_ODS_STACKED:
        t = table.reshape(A[1], A[0], 6)
        assert not np.array_equal(bits(t[CH // 2 - A[3] - 1, :, :3]), bits(t[CH // 2 - A[3], :, :3]))   # the eye changes inside the window
    for win2 in (B, C_):
        r = window_target(loader, sc, win2, lens=lens)
        r.render_passes([seed], first_buffer_spp=2)
        same(r.read(), crop(full.read(), win2, 3), f"type {kind} lens {lens}: window {win2}")
        r.close()
    np.testing.assert_array_equal(win.preview(), crop(full.preview(), A, 1))
    close(full, win, fed, loader)


def test_pregenerated_rays_take_a_cropped_table(gpu_instance):
    """The table is the window's (width * height * 6 floats, read at g); the RNG state is still the canvas pixel's."""
    g = np.load(os.path.join(GOLD, "pregen.npz"))
    sc = gs.make("pregen")
    loader = load(gpu_instance, sc)
    r = HipPathTracingRenderer(loader, A[0], A[1])
    r.set_canvas(CW, CH, A[2], A[3])
    with pytest.raises(native.ChunkyHipError) as e:
        r.set_camera(-1, sc.camera)   # a canvas-sized table is refused: the table is per window
    assert e.value.code == native.E_INVALID
    r.set_camera(-1, crop(sc.camera, A, 6))
    r.render_passes(g["seeds"])
    same(r.read(), crop(g["res"], A, 3), "cropped table")
    close(r, loader)


# ---- combinations -------------------------------------------------------------------------------------------------------------------
def test_window_on_a_biome_tinted_scene(gpu_instance, port):
    sc = bs.water_world()
    assert (sc.width, sc.height) == (CW, CH)
    loader = load(gpu_instance, sc)
    r = window_target(loader, sc, A)
    r.render_passes(SEEDS[:3])
    info = r.kernel_info()
    assert info["biome"] and info["pool"] >= 0, info
    want = port.render_gids(bs.expand(sc), SEEDS[:3], canvas_gids(A), threads=THREADS)
    same(r.read(), crop(want, A, 3), "biome window")
    np.testing.assert_array_equal(r.preview(), crop(port.preview(bs.expand(sc)), A, 1))
    close(r, loader)


def test_window_with_emitter_nee(gpu_instance, port):
    from oracle.binding import PortExt
    sc = gs.make("indoor")
    loader = load(gpu_instance, sc)
    r = window_target(loader, sc, A, options=((native.OPT_EMITTER_NEE, 1),))
    r.render_passes(SEEDS[:3])
    info = r.kernel_info()
    assert info["ext"] and info["pool"] >= 0, info
    with PortExt(port, sc, nee=1):
        want = port.render_gids(sc, SEEDS[:3], canvas_gids(A), threads=THREADS)
    same(r.read(), crop(want, A, 3), "emitter NEE window")
    assert not np.array_equal(bits(crop(want, A, 3)), bits(crop(port.render_gids(sc, SEEDS[:3], canvas_gids(A), threads=THREADS), A, 3)))
    close(r, loader)


@pytest.mark.parametrize("rank,world,tile", [(1, 3, 0), (2, 3, 7)])
def test_shares_of_a_window(gpu_instance, rank, world, tile):
    """The shard map is the target's own (16 x 16 blocks and runs of 7 slots of the 33 x 17 WINDOW): on the pixels the device's own map
    gives a rank, its image is the unsharded window's; everywhere else it is as reset left it; the ranks together cover the window."""
    g = np.load(os.path.join(GOLD, "outdoor.npz"))
    sc = gs.make("outdoor")
    w, h = A[0], A[1]
    want = bits(crop(g["res"], A, 3)).reshape(-1, 3)
    loader = load(gpu_instance, sc)
    covered = np.zeros(len(want), np.int32)
    for k in [rank] + [q for q in range(world) if q != rank]:
        rows, view = gpu_instance.selftest_shard_map(w, h, k, world, tile, w * h + 512)
        slots = rows[:view[3], 0]
        mine = np.zeros(len(want), bool)
        mine[slots[(slots >= 0) & (slots < w * h)]] = True
        assert mine.any() and not mine.all(), (k, int(mine.sum()))
        r = window_target(loader, sc, A)
        r.set_shard(k, world, tile)
        r.render_passes(g["seeds"])
        got = bits(r.read()).reshape(-1, 3)
        same(got[mine], want[mine], f"rank {k} of {world}, tile {tile}")
        assert not got[~mine].any(), f"rank {k} of {world}, tile {tile}: pixels outside the share were written"
        covered += mine
        r.close()
    assert (covered == 1).all()
    loader.close()


def test_window_on_a_group_of_two(gpu_instance):
    g = np.load(os.path.join(GOLD, "entities.npz"))
    sc = gs.make("entities")
    grp = RendererInstance.group([0, 0])
    lg, l1 = load(grp, sc), load(gpu_instance, sc)
    rg, r1 = window_target(lg, sc, B), window_target(l1, sc, B)   # set_canvas reaches both members
    assert rg.canvas() == (CW, CH, B[2], B[3])
    for r in (rg, r1):
        r.render_passes(g["seeds"])
    same(rg.read(), r1.read(), "group of two against one context")
    same(rg.read(), crop(g["res"], B, 3), "group of two against the golden")
    np.testing.assert_array_equal(rg.preview(), r1.preview())
    assert native.lib().chunky_render_set_canvas(rg._h, CW, CH, 32, 31) == native.E_INVALID and rg.canvas() == (CW, CH, B[2], B[3])
    close(rg, r1, lg, l1, grp)


def test_adaptive_run_on_a_window(gpu_instance, port):
    """min_spp 2, a check after every pass, at most 6: a pixel that stopped after n_p passes holds render_passes(seeds[0 .. n_p)) of its
    CANVAS pixel (the 3 x 3 activity neighbourhood is the window's: the counts need not be the canvas target's)."""
    sc = gs.make("outdoor")
    seeds = native.java_random_ints(6, seed=97531)
    loader = load(gpu_instance, sc)
    r = window_target(loader, sc, A)
    image, counts, _, summary = r.render_adaptive(seeds, native.adaptive_params(threshold=0.05, min_spp=2, check_interval=1))
    counts = counts.reshape(-1)
    assert counts.min() >= 2 and counts.max() <= 6, np.unique(counts)
    G = canvas_gids(A)
    want = np.zeros((len(G), 3), np.float32)
    for n in np.unique(counts):
        res = port.render_gids(sc, seeds[:int(n)], G[counts == n], threads=THREADS)
        want[counts == n] = crop(res, A, 3).reshape(-1, 3)[counts == n]
    same(image, want, "adaptive window")
    # it ends a run that could have been resumed
    r.set_canvas(CW, CH, B[2], B[3])
    p = native.adaptive_params(threshold=0.05, min_spp=2, check_interval=1)
    summ = native.AdaptiveSummary()
    import ctypes
    s = np.ascontiguousarray(seeds, np.int32)
    assert native.lib().chunky_render_adaptive_resume(r._h, native.ptr(s), s.size, ctypes.byref(p), None, ctypes.byref(summ)) == native.E_STATE
    close(r, loader)


# ---- render_tiled -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in gs.NAMES if n != "pregen"])
def test_render_tiled_reassembles_the_golden(gpu_instance, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    sc = gs.make(name)
    loader = load(gpu_instance, sc)
    frame = render_tiled(loader, CW, CH, CW, CH, g["seeds"], sc.projector_type, sc.camera, x_cuts=[19], y_cuts=[11])
    same(frame, g["res"], f"{name} in four windows")
    loader.close()


def test_render_tiled_on_a_grid_and_with_pregenerated_rays(gpu_instance):
    g = np.load(os.path.join(GOLD, "outdoor.npz"))
    sc = gs.make("outdoor")
    loader = load(gpu_instance, sc)
    same(render_tiled(loader, CW, CH, 24, 20, g["seeds"], sc.projector_type, sc.camera), g["res"], "3 x 3 windows of two sizes each way")
    loader.close()
    # a table of pre-generated rays is per window: four targets by hand
    g = np.load(os.path.join(GOLD, "pregen.npz"))
    sc = gs.make("pregen")
    loader = load(gpu_instance, sc)
    frame = np.zeros((CH, CW, 3), np.float32)
    for y0, y1 in ((0, 11), (11, CH)):
        for x0, x1 in ((0, 19), (19, CW)):
            win = (x1 - x0, y1 - y0, x0, y0)
            r = window_target(loader, sc, win, camera=window_camera(sc, win))
            r.render_passes(g["seeds"])
            frame[y0:y1, x0:x1] = r.read().reshape(y1 - y0, x1 - x0, 3)
            r.close()
    same(frame, g["res"], "pregen in four windows")
    loader.close()
