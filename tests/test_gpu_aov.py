"""The denoiser's auxiliary images on the device (chunky_render_aov_passes, csrc/aov.hip) against their specification restated on
the oracles (aov_spec.expected_aov: record 0 of the reference's own sample, folded with its running mean), bit for bit: the golden
scenes whole, every tree form, the timed views on whole rows with the instantiation the render kernel runs there, the launch cut, the line-up with
render passes, shards, the BVH cull option, isolation from the render target's own buffers, the ABI's errors and groups."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from aov_spec import expected_aov
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance

pytestmark = pytest.mark.gpu
ROWS = (7, 101, 263, 411, 540, 688, 799, 931, 1003, 1079)  # the rows of tests/test_gpu_timed_kernels.py
AOV_ROWS = ROWS[::3]
A, N = native.AOV_ALBEDO, native.AOV_NORMAL


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(instance, sc):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def images(r):
    return r.read_aov(A).reshape(-1, 3), r.read_aov(N).reshape(-1, 3)


def assert_same(got, want, gids, what):
    for k, kind in enumerate(("albedo", "normal")):
        g, w = bits(got[k]), bits(want[k])
        same = (g == w).all(axis=1)
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what}: {kind} differs at {int((~same).sum())} of {len(same)} pixels (first gid {int(gids[i])}: "
                        f"{got[k][i].tolist()} against {want[k][i].tolist()})")


def whole_image_case(instance, tracer, name):
    sc = gs.make(name)
    seeds = native.java_random_ints(gs.N_PASSES)
    loader, r = make(instance, sc)
    r.render_aov(seeds)
    gids = np.arange(sc.width * sc.height)
    want = expected_aov(tracer, binding.SceneHandle(sc), seeds, gids)
    assert_same(images(r), want, gids, name)
    assert r.aov_info()["launches"] == 1
    r.close()
    loader.close()


@pytest.mark.parametrize("name", gs.NAMES)
def test_golden_scene_whole_images_equal_the_reference(gpu_instance, ref, name):
    whole_image_case(gpu_instance, ref, name)


@pytest.mark.parametrize("name", gs.NAMES)
def test_golden_scene_whole_images_equal_the_port(gpu_instance, port, name):
    whole_image_case(gpu_instance, port, name)


FORM_CASES = list(gs.form_cases(ragged=True))


@pytest.mark.parametrize("key,build,kernel", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_tree_forms(gpu_instance, port, key, build, kernel):
    """The lookup forms 17 / 18 / 19 / 0 and the entity form 18 with the walk, whole images; the form-19 case at 33 x 17."""
    sc = build()
    seeds = native.java_random_ints(gs.N_PASSES)
    loader, r = make(gpu_instance, sc)
    r.render_aov(seeds)
    info = r.aov_info()
    assert (info["tree"], info["bvh"]) == kernel, info
    if (sc.width, sc.height) == gs.RAGGED_VIEW:
        assert info["blocks"] == 6   # 24 claims, one per wave of four-wave workgroups: the grid cap, not the device's size
    gids = np.arange(sc.width * sc.height)
    assert_same(images(r), expected_aov(port, binding.SceneHandle(sc), seeds, gids), gids, key)
    r.close()
    loader.close()


def timed_scene(name):
    return gs.timed_view(name) if name in gs.TIMED_VIEWS else gs.camera_view(name)


@pytest.mark.parametrize("name", gs.TIMED_VIEWS + gs.CAMERA_VIEWS)
def test_timed_views_on_whole_rows(gpu_instance, port, name):
    """The sizes, worlds and cameras bench.py times: the AOV runs the tree form and BVH walk of the render kernel there."""
    sc = timed_scene(name)
    seeds = native.java_random_ints(4)
    loader, r = make(gpu_instance, sc)
    r.render_aov(seeds)
    info = r.aov_info()
    r.render_passes(seeds[:1])
    kinfo = r.kernel_info()
    assert (info["tree"], info["bvh"]) == (kinfo["tree"], kinfo["bvh"]), (info, kinfo)
    assert info["blocks"] >= 256
    rows = sorted({min(y, sc.height - 1) for y in AOV_ROWS})
    gids = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in rows])
    got = tuple(x[gids] for x in images(r))
    h = binding.SceneHandle(sc)
    assert_same(got, expected_aov(port, h, seeds, gids), gids, f"{name} against the port")
    ref = binding.ref()
    if ref is not None:  # the reference build on two of the rows (it traces one sample per call)
        sub = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in rows[1:3]])
        idx = np.searchsorted(gids, sub)
        assert_same(tuple(x[idx] for x in got), expected_aov(ref, h, seeds, sub), sub, f"{name} against the reference")
    assert np.isfinite(got[0]).all() and got[0].max() > 0
    r.close()
    loader.close()


def test_launch_cut_is_invisible(gpu_instance, port):
    sc = gs.make("outdoor")
    seeds = native.java_random_ints(300)
    l1, whole = make(gpu_instance, sc)
    whole.render_aov(seeds)
    assert whole.aov_info()["launches"] == 2  # 256 + 44
    l2, single = make(gpu_instance, sc)
    for k in range(len(seeds)):
        single.render_aov(seeds[k:k + 1], first_buffer_spp=k, sync=False)
    a, b = images(whole), images(single)
    gids = np.arange(sc.width * sc.height)
    assert_same(a, b, gids, "300 passes in one call against 300 calls")
    sub = gids[::7]
    assert_same(tuple(x[sub] for x in a), expected_aov(port, binding.SceneHandle(sc), seeds, sub), sub, "300 passes against the port")
    assert single.aov_kernel_time()[1] == 300
    for x in (whole, single, l1, l2):
        x.close()


@pytest.mark.parametrize("name", ["outdoor", "entities", "dof", "pregen"])
def test_aov_lines_up_with_the_render_pass(gpu_instance, name):
    """One AOV pass (bufferSpp 0: the sample itself) is record 0 of chunky_render_trace_records with the same seed."""
    sc = gs.make(name)
    seed = int(native.java_random_ints(5)[4])
    loader, r = make(gpu_instance, sc)
    r.render_aov([seed])
    albedo, normal = images(r)
    gids = np.arange(3, sc.width * sc.height, 211, dtype=np.int32)
    rec, cnt, rad = r.trace_records(seed, gids)
    assert (cnt >= 1).all()
    hit = rec[:, 0]["hit"] != 0
    assert hit.any()
    want_a = np.where(hit[:, None], rec[:, 0]["color"][:, :3], rad)
    want_n = np.where(hit[:, None], rec[:, 0]["normal"], 0).astype(np.float32)
    np.testing.assert_array_equal(bits(albedo[gids]), bits(want_a))
    np.testing.assert_array_equal(bits(normal[gids]), bits(want_n))
    r.close()
    loader.close()


def owner(sc, world, tile):
    gid = np.arange(sc.width * sc.height)
    if tile > 0:
        return (gid // tile) % world
    bw = (sc.width + 15) // 16
    return ((gid // sc.width // 16) * bw + (gid % sc.width) // 16) % world


@pytest.mark.parametrize("tile", [0, 256])
def test_shards(gpu_instance, tile):
    sc = gs.make("entities")
    seeds = native.java_random_ints(3)
    l0, r0 = make(gpu_instance, sc)
    r0.render_aov(seeds)
    one = images(r0)
    own = owner(sc, 3, tile)
    total = [np.zeros_like(one[0]), np.zeros_like(one[1])]
    for rank in range(3):
        lr, rr = make(gpu_instance, sc)
        rr.set_shard(rank, 3, tile)
        rr.render_aov(seeds)
        part = images(rr)
        mine = own == rank
        for k in range(2):
            np.testing.assert_array_equal(bits(part[k][mine]), bits(one[k][mine]))
            assert (bits(part[k][~mine]) == 0).all()
            total[k] = total[k] + part[k]
        rr.close()
        lr.close()
    for k in range(2):
        np.testing.assert_array_equal(bits(total[k]), bits(one[k]))
    r0.close()
    l0.close()


def test_bvh_cull_option(gpu_instance, port):
    sc = gs.make("entities")
    seeds = native.java_random_ints(3)
    loader, r = make(gpu_instance, sc)
    r.set_option(native.OPT_BVH_CULL_BEHIND, 1)
    r.render_aov(seeds)
    assert r.aov_info()["bvh"]
    gids = np.arange(sc.width * sc.height)
    with binding.PortCull(port, True):
        want = expected_aov(port, binding.SceneHandle(sc), seeds, gids)
    assert_same(images(r), want, gids, "entities, BVH cull")
    r.close()
    loader.close()


def test_render_target_buffers_are_isolated(gpu_instance):
    """AOV calls change nothing render_passes / read / kernel_time / kernel_info see, in either order; reset leaves the AOV alone."""
    sc = gs.make("outdoor")
    seeds = native.java_random_ints(6)
    lp, plain = make(gpu_instance, sc)
    plain.render_passes(seeds)
    want_img, want_launches, want_info = plain.read(), plain.kernel_time()[1], plain.kernel_info()
    la, a = make(gpu_instance, sc)   # render, then AOV
    a.render_passes(seeds)
    a.render_aov(seeds)
    lb, b = make(gpu_instance, sc)   # AOV, then render
    b.render_aov(seeds)
    b.render_passes(seeds)
    for x in (a, b):
        np.testing.assert_array_equal(bits(x.read()), bits(want_img))
        ms, n = x.kernel_time()
        assert n == want_launches and ms > 0
        assert x.kernel_info() == want_info
        aov_ms, aov_n = x.aov_kernel_time()
        assert aov_n == 1 and aov_ms > 0
    before = images(a)
    a.reset()
    after = images(a)
    for k in range(2):
        np.testing.assert_array_equal(bits(after[k]), bits(before[k]))
    assert not (a.read() != 0).any()
    b.reset_aov()
    assert not any((x != 0).any() for x in images(b))
    np.testing.assert_array_equal(bits(b.read()), bits(want_img))
    for x in (plain, a, b, lp, la, lb):
        x.close()


def test_abi_errors_on_a_device(gpu_instance):
    L = native.lib()
    sc = gs.make("outdoor")
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    seeds = native.java_random_ints(2)
    n = sc.width * sc.height * 3
    out = np.zeros(n, np.float32)
    assert L.chunky_render_aov_passes(r._h, seeds.ctypes.data, 2, 0) == native.E_STATE  # before set_camera
    r.set_camera(sc.projector_type, sc.camera)
    assert L.chunky_render_aov_read(r._h, A, out.ctypes.data, n) == native.E_STATE     # before any AOV pass
    assert L.chunky_render_aov_passes(r._h, seeds.ctypes.data, -1, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes(r._h, None, 2, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes(r._h, seeds.ctypes.data, 2, -3) == native.E_INVALID
    assert L.chunky_render_aov_passes(r._h, seeds.ctypes.data, 0, 0) == 0                # allocates the images
    assert L.chunky_render_aov_read(r._h, A, out.ctypes.data, n) == 0                  # allocated, zero
    assert not out.any()
    assert L.chunky_render_aov_read(r._h, 2, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_aov_read(r._h, -1, out.ctypes.data, n) == native.E_INVALID
    assert L.chunky_render_aov_read(r._h, N, out.ctypes.data, n - 1) == native.E_INVALID
    assert L.chunky_render_aov_read(r._h, N, None, n) == native.E_INVALID
    assert L.chunky_render_aov_kernel_info(r._h, None) == native.E_INVALID
    ms, cnt = C.c_float(), C.c_int()
    assert L.chunky_render_aov_kernel_time(r._h, C.byref(ms), C.byref(cnt)) == 0 and cnt.value == 0
    r.close()
    loader.close()


@pytest.fixture(scope="module")
def group3():
    g = RendererInstance.group([0, 0, 0])
    yield g
    g.close()


@pytest.mark.parametrize("name,shard", [("outdoor", None), ("entities", None), ("pregen", (1, 2, 0)), ("indoor", (0, 2, 256))])
def test_group_images_equal_one_context(group3, gpu_instance, name, shard):
    sc = gs.make(name)
    seeds = native.java_random_ints(5)
    lg, rg = make(group3, sc)
    l1, r1 = make(gpu_instance, sc)
    for x in (rg, r1):
        if shard:
            x.set_shard(*shard)
        x.render_aov(seeds[:2])
        x.render_aov(seeds[2:], first_buffer_spp=2)
    a, b = images(rg), images(r1)
    for k in range(2):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]))
    assert rg.aov_info()["tree"] == r1.aov_info()["tree"]
    assert a[0].any()
    for x in (rg, r1, lg, l1):
        x.close()
