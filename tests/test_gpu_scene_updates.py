"""Parity after scene updates: every setter against a fresh upload.

One chunky_scene and one render target live across every case of tests/scene_update_cases.py.  After each update the target's
image and preview must be the oracle's of the scene as it stands now, the kernel the launch picked, the addr32 word and the emitter
list must be those of a fresh scene loaded with the same contents, and so must the first-hit outputs that share scene_view (the
seven AOV images, the matte state, trace records).  tests/test_scene_updates_cpu.py shows that every case would tell a stale
derived copy from a rebuilt one.  Further down: another launch order (the emitter list's own flag), two targets on one scene, an
update behind queued passes, a scene in the middle of an update, an incomplete scene, upload orders, tile writes, and a group."""
import numpy as np
import pytest

import golden_scenes as gs
import scene_update_cases as suc
from chunkyclplugin_amd import native, parallel, scenes
from chunkyclplugin_amd.native import check, ptr
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance
from oracle import binding
from oracle.binding import PortExt

pytestmark = pytest.mark.gpu
SEEDS = scenes.java_random_ints(suc.N_PASSES)
CASES = [c.name for c in suc.cases()]
_want = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def oracle(port, sc):
    """(image, preview) of the oracle, once per distinct scene of the module"""
    key = gs.input_digest(sc)
    if key not in _want:
        h = binding.SceneHandle(sc)
        img, pre = port.render_passes(h, SEEDS), port.preview(h)
        img.setflags(write=False)
        pre.setflags(write=False)
        _want[key] = (img, pre)
    return _want[key]


def assert_image(got, want, what, own=None):
    """bit equality with the oracle's image (on the pixels `own` where the target renders a shard)"""
    got, want = np.asarray(got, np.float32).reshape(-1, 3), np.asarray(want, np.float32).reshape(-1, 3)
    if own is not None:
        got, want = got[own], want[own]
    same = (bits(got) == bits(want)).all(axis=1)
    if not same.all():
        i = int(np.argmin(same))
        pytest.fail(f"{what}: {int((~same).sum())} of {len(want)} pixels differ from the oracle; first: pixel {i} got {got[i]!r} want {want[i]!r}")


# ---- uploads through the raw entry points ----
def i32(a):
    return np.ascontiguousarray(a, np.int32)


def upload_piece(loader, sc, piece):
    L, h = native.lib(), loader._h
    if piece == "octree":
        t = i32(sc.octree)
        check(L.chunky_scene_set_octree(h, ptr(t), t.size, int(sc.octree_depth)))
    elif piece in ("blocks", "materials", "aabbs", "quads", "trigs"):
        kind, field = {"blocks": (native.PALETTE_BLOCK, "block_palette"), "materials": (native.PALETTE_MATERIAL, "material_palette"),
                       "aabbs": (native.PALETTE_AABB, "aabb_models"), "quads": (native.PALETTE_QUAD, "quad_models"),
                       "trigs": (native.PALETTE_TRIG, "bvh_trigs")}[piece]
        a = i32(getattr(sc, field))
        check(L.chunky_scene_set_palette(h, kind, ptr(a), a.size))
    elif piece in ("world_bvh", "actor_bvh"):
        a = i32(getattr(sc, piece))
        check(L.chunky_scene_set_bvh(h, native.BVH_WORLD if piece == "world_bvh" else native.BVH_ACTOR, ptr(a), a.size))
    elif piece == "atlas":
        a = np.ascontiguousarray(sc.atlas, np.uint8)
        layers, ah, aw, _ = a.shape
        check(L.chunky_scene_set_atlas(h, ptr(a), aw, ah, layers))
    elif piece == "sky":
        s = np.ascontiguousarray(sc.sky, np.uint8)
        check(L.chunky_scene_set_sky(h, ptr(s), s.shape[1], s.shape[0], float(sc.sky_intensity)))
    elif piece == "sun":
        s = i32(sc.sun)
        check(L.chunky_scene_set_sun(h, ptr(s)))
    else:
        raise KeyError(piece)


def update(loader, r, c, sc):
    """the one update of case `c` that turns the scene object into `sc`"""
    if c.via == "load_packed":
        loader.load_packed(sc)
        r.set_camera(sc.projector_type, sc.camera)
    elif c.via == "load_octree":
        raw, mapping = suc.remapped(sc.octree, len(sc.block_palette) // 2)
        loader.load_octree(raw, int(sc.octree_depth), mapping)
    else:
        for piece in c.pieces():
            upload_piece(loader, sc, piece)


class Rig:
    def __init__(self, instance, sc, shard=None, loader=None):
        self.loader = loader
        if loader is None:
            self.loader = HipSceneLoader(instance)
            self.loader.load_packed(sc)
        self.r = self.target(sc, shard)
        self.shard = shard

    def target(self, sc, shard=None):
        r = HipPathTracingRenderer(self.loader, sc.width, sc.height)
        r.set_camera(sc.projector_type, sc.camera)
        if shard:
            r.set_shard(*shard)
        return r

    def close(self):
        self.r.close()
        self.loader.close()


def first_hits(r):
    """what one AOV pass, one matte pass and the trace records give: name -> array"""
    out = {}
    r.reset_aov()
    r.render_aov_ex(SEEDS[:1])
    for which in range(native.AOV_BLOCK + 1):
        out[f"aov {which}"] = r.read_aov_ex(which)
    r.reset_matte()
    r.render_matte(SEEDS[:1])
    ids, counts, other, passes = r.read_matte()
    out.update({"matte ids": ids, "matte counts": counts, "matte other": other, "matte passes": np.array([passes])})
    rec, cnt, rad = r.trace_records(int(SEEDS[0]), gs.RECORD_GIDS)
    out["record counts"] = cnt
    live = np.arange(rec.shape[1])[None, :] < cnt[:, None]
    for f in rec.dtype.names:
        out[f"record {f}"] = np.ascontiguousarray(rec[f][live])
    out["record radiance"] = rad
    return out


def assert_same_arrays(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {k}"
        bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
        assert len(bad) == 0, f"{what}: {k} differs from the fresh scene's in {len(bad)} bytes, first at {int(bad[0])}"


def assert_kernel(info, sc, what):
    """kernel_info() against what the launch rule fixes for `sc` (scene_update_cases.expected_kernel)"""
    want = dict(suc.expected_kernel(sc))
    assert (info["pool"] >= 0) == want.pop("pool_runs"), f"{what}: kernel family {info}"
    assert not info["ext"], info
    for k, v in want.items():
        assert info[k] == v, f"{what}: kernel_info {k} = {info[k]}, the launch rule gives {v} ({info})"


def check_step(rig, instance, port, sc, what):
    """Everything the updated scene object must have in common with the oracle and with a fresh scene of the same contents."""
    r, loader = rig.r, rig.loader
    fresh = Rig(instance, sc, rig.shard)
    own = parallel.owned_gids(sc.width * sc.height, rig.shard[0], rig.shard[1], rig.shard[2], sc.width) if rig.shard else None
    want_img, want_pre = oracle(port, sc)
    for x in (r, fresh.r):
        x.reset()
        x.render_passes(SEEDS)
    assert_image(r.read(), want_img, f"{what}: image", own)
    info = r.kernel_info()
    assert info == fresh.r.kernel_info(), f"{what}: the kernel of the updated scene is not the fresh scene's"
    assert_kernel(info, sc, what)
    np.testing.assert_array_equal(r.preview(), want_pre, err_msg=f"{what}: preview")
    assert loader.addr32() == fresh.loader.addr32(), f"{what}: addr32"
    # (equal to the fresh scene's is not enough: both run on one library.  These scenes are small and sound, so every form applies)
    assert loader.addr32() == suc.ADDR32_EVERY == native.ADDR32_ATLAS | native.ADDR32_SKY | native.ADDR32_RECORDS, f"{what}: addr32 {loader.addr32()}"
    assert_same_arrays(first_hits(r), first_hits(fresh.r), what)
    np.testing.assert_array_equal(loader.emitters(), fresh.loader.emitters(), err_msg=f"{what}: emitter list")
    if own is not None:   # nobody else's pixels were touched
        rest = np.ones(sc.width * sc.height, bool)
        rest[own] = False
        assert not r.read().reshape(-1, 3)[rest].any(), f"{what}: pixels outside the shard"
    fresh.close()


# ---- every case: one scene object and one render target across the whole chain ----
@pytest.mark.parametrize("name", CASES)
def test_update_matches_the_oracle_and_a_fresh_scene(gpu_instance, port, name):
    c = suc.case(name)
    rig = Rig(gpu_instance, c.chain[0], c.shard)
    check_step(rig, gpu_instance, port, c.chain[0], f"{name}: before")
    for k, sc in enumerate(c.chain[1:], start=1):
        update(rig.loader, rig.r, c, sc)
        check_step(rig, gpu_instance, port, sc, f"{name}: step {k}")
    rig.close()


def test_chains_return_to_their_first_image(gpu_instance, port):
    """The last scene of a chain is its first: after the whole walk the target's image is, bit for bit, the one it began with."""
    c = suc.case("chain_fallback")
    rig = Rig(gpu_instance, c.chain[0])
    rig.r.render_passes(SEEDS)
    first, info = rig.r.read().copy(), rig.r.kernel_info()
    assert info["pool"] == 64 and not info["bvh"], info
    kernels = []
    for sc in c.chain[1:]:
        update(rig.loader, rig.r, c, sc)
        rig.r.reset()
        rig.r.render_passes(SEEDS)
        kernels.append(rig.r.kernel_info())
    assert kernels[0]["pool"] < 0 and kernels[0]["tree"] == 0 and kernels[0]["bvh"], kernels[0]    # the fallback kernel
    assert kernels[1]["pool"] > 0 and kernels[1]["bvh"], kernels[1]                                  # render_pool with BVH phases
    assert kernels[2] == info, (kernels[2], info)
    np.testing.assert_array_equal(bits(rig.r.read()), bits(first))
    rig.close()


# ---- launch order: the first launch after the update needs no emitter list, the second does ----
@pytest.mark.parametrize("name", suc.LAUNCH_ORDER_CASES)
def test_aov_pass_first_then_emitter_sampling(gpu_instance, port, name):
    """The emitter list has a flag of its own: a launch that did not need the list must not mark it clean."""
    c = suc.case(name)
    before, after = PortExt(port, c.before, nee=1), PortExt(port, c.after, nee=1)
    assert before.emitters[:before.n_emitters].tolist() != after.emitters[:after.n_emitters].tolist(), "the update leaves the emitter list as it was"
    rig = Rig(gpu_instance, c.before)
    rig.r.set_option(native.OPT_EMITTER_NEE, 1)
    rig.r.render_passes(SEEDS)     # the emitter list of `before` is built and marked clean
    with before:
        assert_image(rig.r.read(), port.render_passes(c.before, SEEDS), f"{name}: before, with emitter sampling")
    update(rig.loader, rig.r, c, c.after)
    got = first_hits(rig.r)        # scene_view without the emitter list, three times over
    rig.r.reset()
    rig.r.render_passes(SEEDS)
    info = rig.r.kernel_info()
    assert info["ext"] and info["pool"] > 0, info
    with after:
        want = port.render_passes(c.after, SEEDS)
    assert_image(rig.r.read(), want, f"{name}: emitter sampling after first-hit launches")
    assert not np.array_equal(bits(want), bits(oracle(port, c.after)[0])), "the option changed nothing"
    fresh = Rig(gpu_instance, c.after)
    assert_same_arrays(got, first_hits(fresh.r), f"{name}: first-hit launches first")
    np.testing.assert_array_equal(rig.loader.emitters(), fresh.loader.emitters())
    fresh.close()
    rig.close()


# ---- two targets on one scene ----
@pytest.mark.parametrize("name", ["blocks_kinds", "both_bvhs_empty", "chain_tree_forms_distinct"])
def test_two_targets_see_the_update(gpu_instance, port, name):
    c = suc.case(name)
    rig = Rig(gpu_instance, c.before)
    second = rig.target(c.before)
    for r in (rig.r, second):
        r.render_passes(SEEDS)
    for k, sc in enumerate(c.chain[1:], start=1):
        update(rig.loader, rig.r, c, sc)
        if c.via == "load_packed":
            second.set_camera(sc.projector_type, sc.camera)
        want_img, want_pre = oracle(port, sc)
        for which, r in (("first", rig.r), ("second", second)):
            r.reset()
            r.render_passes(SEEDS)
            assert_image(r.read(), want_img, f"{name} step {k}: {which} target")
            np.testing.assert_array_equal(r.preview(), want_pre, err_msg=f"{name} step {k}: {which} target's preview")
        assert rig.r.kernel_info() == second.kernel_info()
    second.close()
    rig.close()


# ---- an update behind queued work ----
@pytest.mark.parametrize("name", suc.QUEUED_CASES)
def test_update_behind_queued_passes(gpu_instance, port, name):
    """Two passes are queued on `before` and not waited for; the update follows at once; the third pass sees `after`.  The queued
    passes finish on the old contents: the image is the oracle's third pass of `after` merged onto its first two of `before`."""
    c = suc.case(name)
    rig = Rig(gpu_instance, c.before)
    rig.r.render_passes(SEEDS[:2], sync=False)
    update(rig.loader, rig.r, c, c.after)
    rig.r.render_passes(SEEDS[2:], first_buffer_spp=2)
    want = port.render_passes(c.after, SEEDS[2:], first_spp=2, res=port.render_passes(c.before, SEEDS[:2]))
    assert_image(rig.r.read(), want, f"{name}: update behind two queued passes")
    rig.close()


# ---- a scene in the middle of an update ----
def test_shorter_triangle_palette_under_the_old_bvhs(gpu_instance, port):
    E, short, done = suc.half_updated()
    rig = Rig(gpu_instance, E)
    rig.r.render_passes(SEEDS)
    assert_image(rig.r.read(), oracle(port, E)[0], "before")
    held = rig.r.read().copy()
    a = i32(short)
    check(native.lib().chunky_scene_set_palette(rig.loader._h, native.PALETTE_TRIG, ptr(a), a.size))
    for call in (lambda: rig.r.render_passes(SEEDS), rig.r.preview, lambda: rig.r.render_aov_ex(SEEDS[:1])):
        with pytest.raises(native.ChunkyHipError) as e:
            call()
        assert e.value.code == native.E_INVALID and "outside its palette" in str(e.value), str(e.value)
    np.testing.assert_array_equal(bits(rig.r.read()), bits(held))
    upload_piece(rig.loader, done, "actor_bvh")
    check_step(rig, gpu_instance, port, done, "after the matching BVH")
    rig.close()


# ---- an incomplete scene ----
def test_incomplete_scene_names_the_missing_piece(gpu_instance, port):
    sc = suc.golden("entities")
    loader = HipSceneLoader(gpu_instance)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    for pieces, missing in suc.INCOMPLETE_STEPS:
        for p in pieces:
            upload_piece(loader, sc, p)
        if missing is None:
            break
        for call in (lambda: r.render_passes(SEEDS), r.preview, lambda: r.render_aov_ex(SEEDS[:1]), loader.addr32):
            with pytest.raises(native.ChunkyHipError) as e:
                call()
            assert e.value.code == native.E_STATE and missing in str(e.value), (missing, str(e.value))
        assert r.kernel_time()[1] == 0 and r.aov_kernel_time()[1] == 0, f"a launch on a scene without its {missing}"
    r.render_passes(SEEDS)
    assert_image(r.read(), oracle(port, sc)[0], "the completed scene")
    np.testing.assert_array_equal(r.preview(), oracle(port, sc)[1])
    r.close()
    loader.close()


# ---- upload order ----
@pytest.mark.parametrize("order", list(suc.UPLOAD_ORDERS))
def test_upload_order_does_not_matter(gpu_instance, port, order):
    sc = suc.golden("entities")
    loader = HipSceneLoader(gpu_instance)
    for piece in suc.UPLOAD_ORDERS[order]:
        upload_piece(loader, sc, piece)
    rig = Rig(gpu_instance, sc, loader=loader)
    check_step(rig, gpu_instance, port, sc, f"upload order {order}")
    rig.close()


# ---- tile writes ----
def test_atlas_tile_writes(gpu_instance, port):
    sc = suc.tile_scene()
    rig = Rig(gpu_instance, sc)
    rig.r.render_passes(SEEDS)
    assert_image(rig.r.read(), oracle(port, sc)[0], "before")
    layers, h, w, _ = sc.atlas.shape
    check(native.lib().chunky_scene_set_atlas(rig.loader._h, None, w, h, layers))
    check_step(rig, gpu_instance, port, suc.zero_atlas(sc), "the zero-filled atlas")
    for x, y, layer, tw, th, rgba in suc.tile_writes(sc.atlas):
        t = np.ascontiguousarray(rgba, np.uint8)
        check(native.lib().chunky_scene_write_atlas_tile(rig.loader._h, x, y, layer, tw, th, ptr(t)))
    check_step(rig, gpu_instance, port, sc, "the atlas written tile by tile")
    rig.close()


# ---- a group: every setter reaches every replica ----
@pytest.fixture(scope="module")
def group3():
    g = RendererInstance.group([0, 0, 0])
    yield g
    g.close()


@pytest.mark.parametrize("name", ["chain_fallback_distinct", "materials_words", "both_bvhs_empty"])
def test_group_scene_follows_updates(group3, port, name):
    c = suc.case(name)
    assert group3.group_size() == 3
    rig = Rig(group3, c.chain[0])
    rig.r.render_passes(SEEDS)
    assert_image(rig.r.read(), oracle(port, c.chain[0])[0], f"{name}: before")
    for k, sc in enumerate(c.chain[1:], start=1):
        update(rig.loader, rig.r, c, sc)
        rig.r.reset()
        rig.r.render_passes(SEEDS)
        assert_image(rig.r.read(), oracle(port, sc)[0], f"{name}: group, step {k}")
        np.testing.assert_array_equal(rig.r.preview(), oracle(port, sc)[1], err_msg=f"{name}: group, step {k}: preview")
    rig.close()
