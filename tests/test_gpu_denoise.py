"""The denoiser on the device (csrc/denoise.hip) against its specification, chunky_denoise_host (the host loop over the same
csrc/denoise_spec.h, itself held to the numpy restatement by tests/test_denoise_cpu.py), bit for bit: chunky_denoise_frame on the
golden scenes, on the timed outdoor view whole and ragged, on degenerate sizes and on bad values, with both kernel forms;
chunky_render_denoise against chunky_denoise_frame, its isolation from the target's buffers, groups, errors and timing."""
import ctypes as C

import numpy as np
import pytest

import golden_scenes as gs
import denoise_spec as ds
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, denoise_frame

pytestmark = pytest.mark.gpu
A, N = native.AOV_ALBEDO, native.AOV_NORMAL
FORMS = [native.DENOISE_KERNEL_PACKED, native.DENOISE_KERNEL_GATHER]


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def make(instance, sc):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def rendered(instance, sc, passes):
    """(loader, target, colour, albedo, normal) after `passes` render and AOV passes"""
    seeds = native.java_random_ints(passes)
    loader, r = make(instance, sc)
    r.render_passes(seeds)
    r.render_aov(seeds)
    return loader, r, r.read().reshape(sc.height, sc.width, 3), r.read_aov(A), r.read_aov(N)


def assert_frame_equals_host(instance, w, h, c, a, n, what, **kw):
    want = native.denoise_host(w, h, c, a, n, native.denoise_params(**kw))
    for form in FORMS:
        got = denoise_frame(instance, w, h, c, a, n, native.denoise_params(kernel=form, **kw))
        same = bits(got) == bits(want)
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what} {kw} kernel form {form}: {int((~same).sum())} of {same.size} floats differ (first at pixel {i // 3}: "
                        f"{got.reshape(-1)[i]!r} against {want[i]!r})")
    return want


@pytest.mark.parametrize("name", gs.NAMES)
def test_frame_equals_host_on_the_golden_scenes(gpu_instance, name):
    sc = gs.make(name)
    loader, r, c, a, n = rendered(gpu_instance, sc, gs.N_PASSES)
    assert np.isfinite(c).all() and a.any()
    for iterations in range(1, 7):
        for demodulate in (True, False):
            out = assert_frame_equals_host(gpu_instance, sc.width, sc.height, c, a, n, name, iterations=iterations, demodulate=demodulate)
    assert np.isfinite(out).all()
    r.close()
    loader.close()


@pytest.mark.parametrize("size", [(1920, 1080), (1917, 1075)])
def test_frame_equals_host_on_the_headline_view(gpu_instance, size):
    """Whole and ragged: edges of the 64 x 4 blocks, and steps up to 16 pixels against the image edges."""
    sc = gs.timed_view("outdoor").with_view(*size)
    loader, r, c, a, n = rendered(gpu_instance, sc, 4)
    assert_frame_equals_host(gpu_instance, sc.width, sc.height, c, a, n, f"outdoor {size}")
    np.testing.assert_array_equal(bits(r.denoise()), bits(native.denoise_host(sc.width, sc.height, c, a, n)))
    r.close()
    loader.close()


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (7, 1), (3, 2), (65, 5), (130, 9)])
def test_frame_equals_host_on_small_images(gpu_instance, size):
    w, h = size
    c, a, n = ds.synthetic(w, h, 21)
    for iterations in (1, 3, 8):
        for demodulate in (True, False):
            assert_frame_equals_host(gpu_instance, w, h, c, a, n, f"{w}x{h}", iterations=iterations, demodulate=demodulate)


def test_frame_equals_host_on_bad_values(gpu_instance):
    w, h = 150, 70
    c, a, n = ds.synthetic(w, h, 22)
    rng = np.random.default_rng(23)
    for value in (np.nan, np.inf, -np.inf):
        ys, xs = rng.integers(0, h, 12), rng.integers(0, w, 12)
        c[ys, xs, rng.integers(0, 3, 12)] = value
    a[20:40, 30:90] = 0            # zero albedo
    a[5, 5] = np.nan               # bad guides: the pixel drops out as a tap and keeps its own value
    n[6, 6] = np.inf
    a[50:, 100:] = 0
    c[0, 0] = np.nan               # corners
    c[h - 1, w - 1] = np.inf
    bad = ~np.isfinite(c).all(axis=-1)
    for demodulate in (True, False):
        out = assert_frame_equals_host(gpu_instance, w, h, c, a, n, "bad values", demodulate=demodulate).reshape(h, w, 3)
        np.testing.assert_array_equal(bits(out[bad]), bits(c[bad]))      # come back unchanged
        good = ~bad
        good[5, 5] = good[6, 6] = False
        assert np.isfinite(out[good]).all()                               # and nothing spread
    assert_frame_equals_host(gpu_instance, w, h, c, np.zeros_like(a), n, "albedo 0")


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor"])
def test_render_denoise_equals_frame_and_leaves_the_target_alone(gpu_instance, name):
    sc = gs.make(name)
    loader, r, c, a, n = rendered(gpu_instance, sc, 5)
    for form in FORMS:
        for kw in (dict(), dict(iterations=3, demodulate=False), dict(iterations=1), dict(iterations=8, sigma_color=0.5)):
            p = native.denoise_params(kernel=form, **kw)
            got = r.denoise(p)
            np.testing.assert_array_equal(bits(got), bits(denoise_frame(gpu_instance, sc.width, sc.height, c, a, n, p)))
            np.testing.assert_array_equal(bits(got), bits(native.denoise_host(sc.width, sc.height, c, a, n, p)))
    assert r.read().tobytes() == c.tobytes() and r.read_aov(A).tobytes() == a.tobytes() and r.read_aov(N).tobytes() == n.tobytes()
    assert (got != c).any()
    r.close()
    loader.close()


def test_a_group_denoises_like_one_context(gpu_instance):
    g = RendererInstance.group([0, 0])
    sc = gs.make("entities")
    l1, r1, c, a, n = rendered(gpu_instance, sc, 4)
    lg, rg, cg, ag, ng = rendered(g, sc, 4)
    np.testing.assert_array_equal(bits(cg), bits(c))
    got = rg.denoise()
    np.testing.assert_array_equal(bits(got), bits(r1.denoise()))
    np.testing.assert_array_equal(bits(got), bits(native.denoise_host(sc.width, sc.height, c, a, n)))
    assert rg.read().tobytes() == c.tobytes() and rg.read_aov(A).tobytes() == a.tobytes() and rg.read_aov(N).tobytes() == n.tobytes()
    ms, launches = rg.denoise_kernel_time()
    assert launches == 6 and ms > 0
    np.testing.assert_array_equal(bits(denoise_frame(g, sc.width, sc.height, c, a, n)), bits(got))
    for x in (rg, r1, lg, l1):
        x.close()
    g.close()


def test_state_and_argument_errors(gpu_instance):
    L = native.lib()
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    seeds = native.java_random_ints(2)
    n = sc.width * sc.height * 3
    out = np.zeros(n, np.float32)
    p = native.denoise_params()
    r.render_passes(seeds)
    assert L.chunky_render_denoise(r._h, C.byref(p), out.ctypes.data, n) == native.E_STATE      # before any AOV pass
    assert b"AOV" in L.chunky_last_error()
    r.render_aov(seeds)
    assert L.chunky_render_denoise(r._h, C.byref(p), out.ctypes.data, n) == 0
    assert L.chunky_render_denoise(r._h, C.byref(p), out.ctypes.data, n - 1) == native.E_INVALID
    assert L.chunky_render_denoise(r._h, C.byref(p), None, n) == native.E_INVALID
    assert L.chunky_render_denoise(r._h, None, out.ctypes.data, n) == native.E_INVALID
    for field, value in (("iterations", 0), ("iterations", 9), ("sigma_color", 0.0), ("sigma_normal", float("nan")), ("sigma_albedo", float("inf")), ("size", 8),
                         ("flags", 4)):
        q = native.denoise_params()
        setattr(q, field, value)
        assert L.chunky_render_denoise(r._h, C.byref(q), out.ctypes.data, n) == native.E_INVALID, field
        img = np.zeros(12, np.float32)
        assert L.chunky_denoise_frame(gpu_instance._h, 2, 2, img.ctypes.data, img.ctypes.data, img.ctypes.data, C.byref(q), img.ctypes.data) == native.E_INVALID, field
    img = np.zeros(12, np.float32)
    for args in ((0, 2, img, img, img, img), (2, -1, img, img, img, img), (2, 2, None, img, img, img), (2, 2, img, None, img, img), (2, 2, img, img, None, img),
                 (2, 2, img, img, img, None)):
        f = [x if isinstance(x, int) or x is None else x.ctypes.data for x in args]
        assert L.chunky_denoise_frame(gpu_instance._h, f[0], f[1], f[2], f[3], f[4], C.byref(p), f[5]) == native.E_INVALID
    r.set_shard(1, 2, 0)   # half of the image's blocks: the target no longer holds the whole image
    assert L.chunky_render_denoise(r._h, C.byref(p), out.ctypes.data, n) == native.E_STATE
    r.set_shard(0, 1, 0)
    assert L.chunky_render_denoise(r._h, C.byref(p), out.ctypes.data, n) == 0
    r.close()
    loader.close()


def test_kernel_time_reports_launches_and_resets(gpu_instance):
    sc = gs.make("indoor")
    loader, r, c, a, n = rendered(gpu_instance, sc, 3)
    assert r.denoise_kernel_time() == (0.0, 0)
    r.denoise()                                                                     # the demodulation pass + 5 iterations
    r.denoise(native.denoise_params(iterations=3, kernel=native.DENOISE_KERNEL_PACKED))  # the pack pass + 3 iterations
    ms, launches = r.denoise_kernel_time()
    assert launches == 6 + 4 and ms > 0
    assert r.denoise_kernel_time() == (0.0, 0)
    assert r.kernel_time()[1] == 1 and r.aov_kernel_time()[1] == 1   # the render and AOV timers do not see denoise launches
    r.close()
    loader.close()
