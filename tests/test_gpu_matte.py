"""The antialiased ID mattes on the device (chunky_render_matte_*, csrc/matte.hip) bit for bit against their specification restated
on the C restatement of the reference (matte_spec.py: the id of a sample from record 0 of trace_records on the scene with and
without its BVHs, then the slot update in numpy; tests/test_matte_cpu.py shows the restatement means the same on the reference build):
the golden scenes whole, every tree form, slot overflow and the launch cut, a call split in two and a restored state, the line-up
with CHUNKY_AOV_BLOCK, the cameras, shards and a group, the ranks and the extract against the host twins, and isolation and errors."""
import dataclasses

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
import matte_spec as ms
from aov_ex_spec import alpha_byte
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipPostProcessingFilter, HipSceneLoader, RendererInstance, camera_rays
from test_camera_lens_ods_cpu import GPU_LENS, projected

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(gs.N_PASSES)
SEEDS300 = native.java_random_ints(300)
ALL = np.arange(gs.W * gs.H)


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


def state(r, gids=None):
    """(ids (6, n), counts (6, n), other (n,)) and the pass count, as chunky_render_matte_read delivers them"""
    ids, counts, other, passes = r.read_matte()
    assert ids.dtype == counts.dtype == other.dtype == np.int32
    st = ids.reshape(ms.SLOTS, -1), counts.reshape(ms.SLOTS, -1), other.reshape(-1)
    return (st if gids is None else (st[0][:, gids], st[1][:, gids], st[2][gids])), passes


def assert_same(got, want, gids, what):
    for g, w, plane in zip(got, want, ("ids", "counts", "other")):
        same = (g == w).reshape(-1, g.shape[-1]).all(axis=0)
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what}: {plane} differ at {int((~same).sum())} of {len(same)} pixels (first gid {int(gids[i])}: "
                        f"{g[..., i].tolist()} against {w[..., i].tolist()})")


_expected = {}


def expected(port, key, sc, seeds, cull=False):
    """The restatement's state of a whole view after `seeds`, computed once per key and never changed."""
    if key not in _expected:
        with binding.PortCull(port, cull):
            ids = ms.expected_ids(port, sc, seeds, np.arange(sc.width * sc.height))
        _expected[key] = (ids, ms.fold(ids))
    return tuple(a.copy() for a in _expected[key][1])


def sample_ids(key):
    return _expected[key][0]


# ---- 1. the golden scenes whole ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gs.NAMES)
def test_golden_scene_whole_state(gpu_instance, port, name):
    sc = gs.make(name)
    want = expected(port, name, sc, SEEDS)
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS)
    got, passes = state(r)
    assert_same(got, want, ALL, name)
    assert passes == 3 and r.matte_info()["launches"] == 1 and r.matte_kernel_time()[1] == 1
    assert (got[1].sum(axis=0) + got[2] == 3).all()
    if name == "entities":
        assert (got[0][got[1] > 0] == ms.WORLD).any() and (got[0][got[1] > 0] == ms.ACTOR).any()
        assert r.matte_info()["bvh"] and r.matte_info()["tree"] == -1   # with an entity BVH this small scene runs the generic walk
    close(r, loader)


# ---- 2. the tree forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,build,kernel", list(gs.form_cases()), ids=[c[0] for c in gs.form_cases()])
def test_tree_forms(gpu_instance, port, key, build, kernel):
    sc = build()
    want = expected(port, key, sc, SEEDS)
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS)
    info = r.matte_info()
    assert (info["tree"], info["bvh"]) == kernel, info
    assert_same(state(r)[0], want, np.arange(sc.width * sc.height), key)
    close(r, loader)


# ---- 3. overflow and the launch cut -----------------------------------------------------------------------------------------------------
def overflow_view():
    return gs.make("outdoor").with_view(4, 3)


def test_overflow_and_the_launch_cut(gpu_instance, port):
    sc = overflow_view()
    want = expected(port, "outdoor-4x3-300", sc, SEEDS300)
    # the fixture exercises rule 3: `other` grows, and some pixel has all six slots occupied
    assert want[2].tolist() == [0, 0, 6, 0, 0, 2, 0, 1, 0, 0, 0, 0]
    assert (want[2] > 0).any() and ((want[1] > 0).sum(axis=0) == ms.SLOTS).any()
    assert max(len(set(col)) for col in sample_ids("outdoor-4x3-300").T) == 9
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS300)
    assert r.matte_info()["launches"] == 2 and r.matte_kernel_time()[1] == 2   # 256 + 44
    got, passes = state(r)
    assert_same(got, want, np.arange(12), "300 passes")
    assert passes == 300
    close(r, loader)


def test_overflow_in_a_single_launch(gpu_instance, port):
    sc = gs.make("outdoor").with_view(8, 6)
    want = expected(port, "outdoor-8x6-64", sc, SEEDS300[:64])
    assert np.flatnonzero(want[2]).tolist() == [13, 18]
    assert ((want[1] > 0).sum(axis=0) > 1).sum() == 38
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS300[:64])
    assert r.matte_info()["launches"] == 1
    assert_same(state(r)[0], want, np.arange(48), "64 passes")
    close(r, loader)


# ---- 4. two calls equal one, and restore ------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_and_restore(gpu_instance, port):
    sc = gs.make("entities")
    want = expected(port, "entities", sc, SEEDS)
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS[:2])
    (ids, counts, other), passes = state(r)
    assert passes == 2
    r.render_matte(SEEDS[2:])
    got, passes = state(r)
    assert_same(got, want, ALL, "2 + 1 passes")
    assert passes == 3
    r.reset_matte()
    empty, passes = state(r)
    assert passes == 0 and not any(a.any() for a in empty)
    r.restore_matte(ids, counts, other, 2)
    r.render_matte(SEEDS[2:])
    got, passes = state(r)
    assert_same(got, want, ALL, "restored after 2 passes, then 1")
    assert passes == 3
    # a malformed state is refused and nothing changes
    L = native.lib()
    bad = got[1].copy()
    bad[0, 100] += 1
    n = sc.width * sc.height
    for i, c, o, p in ((got[0], bad, got[2], 3), (got[0], got[1], got[2], 4)):
        i, c, o = (np.ascontiguousarray(a) for a in (i, c, o))
        assert L.chunky_render_matte_restore(r._h, i.ctypes.data, c.ctypes.data, o.ctypes.data, n, p) == native.E_INVALID
        after, passes = state(r)
        assert_same(after, want, ALL, "after a refused restore")
        assert passes == 3
    close(r, loader)


# ---- 5. the existing device path, no oracle ---------------------------------------------------------------------------------------------
def test_slot_0_is_the_aov_block_image(gpu_instance):
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS)
    r.reset_matte()
    r.render_matte(SEEDS[:1])
    r.render_aov_ex(SEEDS[:1])
    (ids, counts, other), passes = state(r)
    block = r.read_aov_ex(native.AOV_BLOCK).reshape(-1)
    np.testing.assert_array_equal(ids[0], block)
    assert passes == 1 and (counts[0] == 1).all() and not counts[1:].any() and not other.any()
    assert (block == -1).any() and (block >= 0).any()
    close(r, loader)


# ---- 6. cameras -------------------------------------------------------------------------------------------------------------------------
def test_projected_camera_with_a_lens(gpu_instance, port):
    """A pass of a projected camera is the pass on the table of its rays, with the lens as without."""
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    lens = GPU_LENS[kind]
    loader, r = make(gpu_instance, sc, lens)
    r.render_matte(SEEDS)
    gids = np.arange(0, sc.width * sc.height, 3)
    rows = []
    for seed in SEEDS:
        table = dataclasses.replace(sc, camera=camera_rays(kind, sc.camera, sc.width, sc.height, int(seed), lens), projector_type=-1)
        rows.append(ms.expected_ids(port, table, [seed], gids)[0])
    want = ms.fold(np.array(rows))
    assert_same(state(r, gids)[0], want, gids, "fisheye with a lens")
    assert len(np.unique(want[0][want[1] > 0])) > 2
    close(r, loader)


@pytest.mark.parametrize("name", ["dof", "pregen"])
def test_aperture_and_table_cameras(gpu_instance, port, name):
    sc = gs.make(name)
    assert sc.projector_type == (-1 if name == "pregen" else 0)
    want = expected(port, name, sc, SEEDS)
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS[:1])
    r.render_matte(SEEDS[1:])
    assert_same(state(r)[0], want, ALL, name)
    close(r, loader)


# ---- 7. shards and a group --------------------------------------------------------------------------------------------------------------
def owner(sc, world, tile):
    gid = np.arange(sc.width * sc.height)
    if tile > 0:
        return (gid // tile) % world
    bw = (sc.width + 15) // 16
    return ((gid // sc.width // 16) * bw + (gid % sc.width) // 16) % world


@pytest.mark.parametrize("tile", [0, 7])
def test_shards(gpu_instance, port, tile):
    """Block shards (tile 0) and run shards of 7 pixels: the rank's pixels are the whole image's, every other word stays 0."""
    sc = gs.make("entities")
    want = expected(port, "entities", sc, SEEDS)
    loader, r = make(gpu_instance, sc)
    r.set_shard(1, 3, tile)
    r.render_matte(SEEDS)
    got, passes = state(r)
    mine = owner(sc, 3, tile) == 1
    assert mine.any() and not mine.all() and passes == 3
    assert_same(tuple(a[..., mine] for a in got), tuple(a[..., mine] for a in want), ALL[mine], f"rank 1 of 3, tile {tile}")
    assert not any(a[..., ~mine].any() for a in got)
    r_ids, r_cov = r.matte_ranks()
    assert (r_ids.reshape(ms.SLOTS, -1)[:, ~mine] == ms.EMPTY).all() and not bits(r_cov.reshape(ms.SLOTS, -1)[:, ~mine]).any()   # six empty ranks
    # the sharded state is one a resumed render can hand back
    r.restore_matte(*got, 3)
    close(r, loader)


def test_group_equals_one_context(gpu_instance, port):
    g = RendererInstance.group([0, 0])
    sc = gs.make("entities")
    want = expected(port, "entities", sc, SEEDS)
    lg, rg = make(g, sc)
    rg.render_matte(SEEDS[:2])
    rg.render_matte(SEEDS[2:])
    got, passes = state(rg)
    assert_same(got, want, ALL, "a two-member group")
    assert passes == 3 and rg.matte_info()["bvh"] and rg.matte_info()["launches"] == 1
    w_ids, w_cov = native.matte_host_ranks(want[0], want[1], 3)
    g_ids, g_cov = rg.matte_ranks()
    np.testing.assert_array_equal(g_ids.reshape(ms.SLOTS, -1), w_ids)
    np.testing.assert_array_equal(bits(g_cov.reshape(ms.SLOTS, -1)), bits(w_cov))
    rg.reset_matte()
    assert not any(a.any() for a in state(rg)[0])
    close(rg, lg, g)


# ---- 8. ranks and extract ---------------------------------------------------------------------------------------------------------------
def id_sets(ids, counts):
    seen = np.unique(ids[counts > 0])
    rng = np.random.default_rng(3)
    thousand = np.concatenate([seen[::2], seen[::2], rng.integers(-3, 400, 1000)]).astype(np.int32)[:1000]
    assert len(np.unique(thousand)) < 1000 and np.isin(seen[::2], thousand).all()
    return {"sky": [ms.SKY], "entities": [ms.WORLD, ms.ACTOR], "thousand": thousand, "empty": []}


def check_read_outs(r, ids, counts, passes, gpu_instance, w, h):
    w_ids, w_cov = native.matte_host_ranks(ids, counts, passes)
    g_ids, g_cov = r.matte_ranks()
    np.testing.assert_array_equal(g_ids.reshape(ms.SLOTS, -1), w_ids)
    np.testing.assert_array_equal(bits(g_cov.reshape(ms.SLOTS, -1)), bits(w_cov))
    n_ids, n_cov = ms.ranks(ids, counts, passes)   # and the twins equal the numpy restatement on this state
    np.testing.assert_array_equal(w_ids, n_ids)
    np.testing.assert_array_equal(bits(w_cov), bits(n_cov))
    x = np.ascontiguousarray(np.random.default_rng(4).gamma(0.7, 0.6, size=3 * w * h), np.float64)
    f = HipPostProcessingFilter("GAMMA", gpu_instance)
    for name, id_set in id_sets(ids, counts).items():
        want = native.matte_host_extract(ids, counts, passes, id_set)
        got = r.matte_extract(id_set)
        assert got.shape == (h, w) and got.dtype == np.float32
        np.testing.assert_array_equal(bits(got.reshape(-1)), bits(want), err_msg=name)
        np.testing.assert_array_equal(bits(want), bits(ms.extract(ids, counts, passes, id_set)), err_msg=name)
        argb = np.zeros(w * h, np.uint32)
        f.process_frame_alpha(w, h, x, got.reshape(-1), argb, 1.0)
        np.testing.assert_array_equal(argb >> 24, alpha_byte(want), err_msg=name)
        if name == "empty":
            assert not bits(got).any()
        if name == "sky":
            assert got.max() > 0


def test_ranks_and_extract_equal_the_host_twins(gpu_instance, port):
    sc = overflow_view()
    ids, counts, other = expected(port, "outdoor-4x3-300", sc, SEEDS300)
    loader, r = make(gpu_instance, sc)
    r.render_matte(SEEDS300)
    assert_same(state(r)[0], (ids, counts, other), np.arange(12), "300 passes")
    check_read_outs(r, ids, counts, 300, gpu_instance, 4, 3)
    # counts above 2^24: the int -> float conversions round
    passes = 300 * 5000000 + 1001
    big = np.where(counts > 0, counts.astype(np.int64) * 5000000 + np.arange(1, ms.SLOTS + 1)[:, None], 0).astype(np.int32)
    big_other = (passes - big.sum(axis=0)).astype(np.int32)
    assert (big > 2 ** 24).any() and (big[big > 2 ** 24].astype(np.float32).astype(np.int64) != big[big > 2 ** 24]).any()
    assert int(np.float32(passes)) != passes and (big_other > 0).all()
    r.restore_matte(ids, big, big_other, passes)
    got, p = state(r)
    assert_same(got, (ids, big, big_other), np.arange(12), "restored")
    assert p == passes
    check_read_outs(r, ids, big, passes, gpu_instance, 4, 3)
    # one more pass continues the restored state
    r.render_matte(SEEDS300[:1])
    want = ms.fold(sample_ids("outdoor-4x3-300")[:1], (ids, big, big_other))
    got, p = state(r)
    assert_same(got, want, np.arange(12), "restored + 1 pass")
    assert p == passes + 1
    close(r, loader)


# ---- 9. isolation and errors ------------------------------------------------------------------------------------------------------------
def test_isolation(gpu_instance, port):
    sc = gs.make("outdoor")
    want = expected(port, "outdoor", sc, SEEDS)
    loader, r = make(gpu_instance, sc)
    image, ad_counts, ad_noise, _ = r.render_adaptive(native.java_random_ints(8), native.adaptive_params(min_spp=4, check_interval=2))
    r.render_aov_ex(SEEDS)
    before = {"fb": r.read().tobytes(), "counts": ad_counts.tobytes(), "noise": ad_noise.tobytes(),
              "aov": [r.read_aov_ex(which).tobytes() for which in range(7)]}
    r.kernel_time(), r.aov_kernel_time()   # (drained)
    kinfo, ainfo = r.kernel_info(), r.aov_info()
    r.render_matte(SEEDS)
    mine, passes = state(r)
    r.matte_ranks(), r.matte_extract([ms.SKY])
    assert r.read().tobytes() == before["fb"] and r.adaptive_counts().tobytes() == before["counts"] and r.adaptive_noise().tobytes() == before["noise"]
    assert [r.read_aov_ex(which).tobytes() for which in range(7)] == before["aov"]
    assert r.kernel_time()[1] == 0 and r.aov_kernel_time()[1] == 0 and r.kernel_info() == kinfo and r.aov_info() == ainfo
    ms_, n = r.matte_kernel_time()
    assert n == 1 and ms_ > 0
    # ... and theirs leave the planes alone
    r.render_passes(SEEDS)
    r.render_aov_ex(SEEDS, first_buffer_spp=3)
    r.render_aov(SEEDS[:1], first_buffer_spp=6)
    r.denoise()
    r.reset()
    r.reset_aov()
    r.render_adaptive(native.java_random_ints(6), native.adaptive_params(min_spp=4, check_interval=2))
    after, passes_after = state(r)
    assert_same(after, mine, ALL, "after render, AOV, denoise, adaptive and reset calls")
    assert_same(after, want, ALL, "outdoor")
    assert passes_after == passes == 3 and r.matte_info()["launches"] == 1 and r.matte_kernel_time()[1] == 0
    close(r, loader)


def test_bvh_cull_option(gpu_instance, port):
    sc = gs.make("entities")
    want = expected(port, "entities-cull", sc, SEEDS, cull=True)
    loader, r = make(gpu_instance, sc)
    r.set_option(native.OPT_BVH_CULL_BEHIND, 1)
    r.render_matte(SEEDS)
    assert r.matte_info()["bvh"]
    assert_same(state(r)[0], want, ALL, "entities, BVH cull")
    close(r, loader)


def test_abi_errors_on_a_device(gpu_instance):
    L = native.lib()
    sc = gs.make("outdoor")
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    seeds = native.java_random_ints(2)
    n = sc.width * sc.height
    ids, counts, other = np.zeros(6 * n, np.int32), np.zeros(6 * n, np.int32), np.zeros(n, np.int32)
    cov, passes = np.zeros(6 * n, np.float32), native.C.c_int32(-1)
    P = lambda a: a.ctypes.data   # noqa: E731
    assert L.chunky_render_matte_passes(r._h, P(seeds), 2) == native.E_STATE   # before set_camera
    r.set_camera(sc.projector_type, sc.camera)
    assert L.chunky_render_matte_ranks(r._h, P(ids), P(cov), n) == native.E_STATE   # before any pass
    assert L.chunky_render_matte_extract(r._h, P(seeds), 2, P(cov), n) == native.E_STATE
    assert L.chunky_render_matte_read(r._h, P(ids), P(counts), P(other), n, native.C.byref(passes)) == 0 and passes.value == 0   # an empty state
    assert L.chunky_render_matte_passes(r._h, P(seeds), 0) == 0
    assert L.chunky_render_matte_ranks(r._h, P(ids), P(cov), n) == native.E_STATE   # still no pass
    assert L.chunky_render_matte_passes(r._h, P(seeds), -1) == native.E_INVALID
    assert L.chunky_render_matte_passes(r._h, None, 2) == native.E_INVALID
    assert L.chunky_render_matte_passes(r._h, P(seeds), 2) == 0
    assert L.chunky_render_matte_read(r._h, P(ids), P(counts), P(other), n, native.C.byref(passes)) == 0 and passes.value == 2
    for wrong in (n - 1, n + 1, 0, -n, 6 * n):
        assert L.chunky_render_matte_read(r._h, P(ids), P(counts), P(other), wrong, native.C.byref(passes)) == native.E_INVALID
        assert L.chunky_render_matte_restore(r._h, P(ids), P(counts), P(other), wrong, 2) == native.E_INVALID
        assert L.chunky_render_matte_ranks(r._h, P(ids), P(cov), wrong) == native.E_INVALID
        assert L.chunky_render_matte_extract(r._h, P(seeds), 2, P(cov), wrong) == native.E_INVALID
    assert L.chunky_render_matte_read(r._h, None, P(counts), P(other), n, native.C.byref(passes)) == native.E_INVALID
    assert L.chunky_render_matte_read(r._h, P(ids), P(counts), P(other), n, None) == native.E_INVALID
    assert L.chunky_render_matte_restore(r._h, P(ids), None, P(other), n, 2) == native.E_INVALID
    assert L.chunky_render_matte_ranks(r._h, P(ids), None, n) == native.E_INVALID
    assert L.chunky_render_matte_extract(r._h, P(seeds), 2, None, n) == native.E_INVALID
    assert L.chunky_render_matte_extract(r._h, P(seeds), -1, P(cov), n) == native.E_INVALID
    assert L.chunky_render_matte_extract(r._h, None, 2, P(cov), n) == native.E_INVALID
    empty = np.array([4, native.MATTE_EMPTY], np.int32)
    assert L.chunky_render_matte_extract(r._h, P(empty), 2, P(cov), n) == native.E_INVALID
    assert L.chunky_render_matte_kernel_info(r._h, None) == native.E_INVALID
    assert L.chunky_render_matte_extract(r._h, None, 0, P(cov), n) == 0 and not cov[:n].any()
    # the pass count stops at 2^31 - 1: a call that would pass it is refused before any launch
    assert L.chunky_render_matte_restore(r._h, P(ids), P(counts), P(other), n, 2) == 0
    top = 2 ** 31 - 1
    c = counts.copy()
    c[:n] += top - 3
    assert L.chunky_render_matte_restore(r._h, P(ids), P(c), P(other), n, top - 1) == 0
    assert L.chunky_render_matte_passes(r._h, P(seeds), 2) == native.E_INVALID
    assert r.matte_kernel_time()[1] == 1   # (the two passes above; nothing was launched since)
    assert L.chunky_render_matte_passes(r._h, P(seeds), 1) == 0
    assert L.chunky_render_matte_read(r._h, P(ids), P(counts), P(other), n, native.C.byref(passes)) == 0 and passes.value == top
    assert (counts.reshape(6, n).astype(np.int64).sum(axis=0) + other == top).all()
    assert L.chunky_render_matte_passes(r._h, P(seeds), 1) == native.E_INVALID
    close(r, loader)
