"""Firefly-robust accumulation on the device (chunky_render_robust_*, csrc/robust.hip) against its specification, every float and
byte compared bit for bit: the buckets equal chunky_robust_host on the oracle's per-pass samples, the resolved image and the trim
bytes equal chunky_robust_host_resolve, and the beauty image equals the oracle's render of the same seeds.  Also: launch
boundaries, padded tiles, shards, the two kernels on synthetic streams with non-finite values, the denoiser fed with the resolved
image, repeatability, isolation from every other image and timer of the target, and every error of the ABI."""
import ctypes as C

import numpy as np
import pytest

import adaptive_spec as sp
import golden_scenes as gs
import robust_spec as rs
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance
from test_adaptive_cpu import MAX_SPP, samples_of
from test_robust_cpu import BUCKETS, GAINS, MODES, NON_DEGENERATE, trim_shares

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(MAX_SPP)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(instance, sc, options=()):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    for k, v in options:
        r.set_option(k, v)
    return loader, r


def close(*xs):
    for x in xs:
        x.close()


def same(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.size == w.size, (what, g.size, w.size)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        pytest.fail(f"{what}: {bad.size} of {g.size} floats differ (first: index {int(bad[0])}, {np.ravel(got)[bad[0]]!r} against {np.ravel(want)[bad[0]]!r})")


def check_resolves(r, buckets, what):
    """the device's resolve of r's buckets against the host's of `buckets`, every mode and gain; returns the default's trim"""
    default_trim = None
    for mode in MODES:
        for gain in GAINS:
            p = native.robust_params(mode, gain)
            img, trim = r.robust_resolve(p)
            wimg, wtrim = native.robust_host_resolve(buckets, p)
            same(img, wimg, f"{what} resolved image, mode {mode} gain {gain}")
            assert np.array_equal(trim, wtrim), (what, mode, gain, int((trim != wtrim).sum()))
            if mode == native.ROBUST_GINI and gain == 1.0:
                default_trim = trim
    same(r.robust_resolve(trim=False)[0], native.robust_host_resolve(buckets)[0], what + " resolved without the trim map")
    return default_trim


@pytest.mark.parametrize("M", BUCKETS)
@pytest.mark.parametrize("name", ["indoor", "outdoor", "entities"])
def test_golden_scenes_equal_the_host_on_oracle_samples(gpu_instance, port, name, M):
    sc = gs.make(name)
    s = samples_of(name, port)
    loader, r = make(gpu_instance, sc)
    r.robust_begin(M)
    r.robust_passes(SEEDS)
    info = r.kernel_info()
    assert info["pool"] >= 0 and info["bvh"] == (name == "entities"), info
    want = native.robust_host(s, M)
    got = r.robust_buckets(M)
    for b in range(M):
        same(got[b], want[b], f"{name} M={M} bucket {b}")
    assert r.robust_bucket(0)[1] == MAX_SPP
    trim = check_resolves(r, want, f"{name} M={M}")
    same(r.read(), port.render_passes(sc, SEEDS), f"{name} M={M} beauty image")
    if name in NON_DEGENERATE and NON_DEGENERATE[name][0] == M:  # the condition tests/test_robust_cpu.py checks on the oracle
        for share, need in zip(trim_shares(trim, M), NON_DEGENERATE[name][1]):
            assert need is None or share >= need
    close(r, loader)


def test_launch_boundaries_and_first_buffer_spp(gpu_instance, port):
    sc = gs.make("outdoor")
    M = 5
    loader, r = make(gpu_instance, sc)
    r.robust_begin(M)
    r.robust_passes(SEEDS)
    whole, image = r.robust_buckets(M), r.read().copy()
    r.reset()
    r.robust_begin(M)  # a second begin resets the state
    assert r.robust_bucket(0)[1] == 0 and not r.robust_buckets(M).any()
    r.robust_passes(SEEDS[:7], 0)
    r.robust_passes([], 7)  # n = 0 is legal
    r.robust_passes(SEEDS[7:8], 7)
    r.robust_passes(SEEDS[8:], 8)
    same(r.robust_buckets(M), whole, "7 + 1 + 32 passes, buckets")
    same(r.read(), image, "7 + 1 + 32 passes, beauty image")
    assert r.robust_bucket(M - 1)[1] == MAX_SPP
    # first_buffer_spp weights the beauty mean only
    r.reset()
    r.robust_begin(M)
    r.robust_passes(SEEDS, 7)
    same(r.robust_buckets(M), whole, "first_buffer_spp = 7, buckets")
    plain_loader, plain = make(gpu_instance, sc)
    plain.render_passes(SEEDS, 7)
    same(r.read(), plain.read(), "first_buffer_spp = 7, beauty image against render_passes")
    assert not np.array_equal(bits(r.read()), bits(image))
    same(r.read(), port.render_passes(sc, SEEDS, first_spp=7), "first_buffer_spp = 7, beauty image against the oracle")
    close(r, loader, plain, plain_loader)


def device_samples(r, seeds):
    """One-pass renders from a reset target: the sample of every pass (parity of those renders: tests/test_gpu_timed_kernels.py)."""
    out = np.empty((len(seeds), r.height, r.width, 3), np.float32)
    for k, s in enumerate(seeds):
        r.reset()
        r.render_passes([s])
        r.read(out[k].reshape(-1))
    return out


def test_three_hundred_passes_are_two_launches(gpu_instance):
    sc = gs.make("outdoor").with_view(8, 8)
    seeds = native.java_random_ints(300)
    M = 9
    loader, r = make(gpu_instance, sc)
    s = device_samples(r, seeds)
    r.reset()
    r.robust_kernel_time()
    r.robust_begin(M)
    r.robust_passes(seeds)
    ms, launches, _ = r.robust_kernel_time()
    assert launches == 2 and ms > 0
    whole, image = r.robust_buckets(M), r.read().copy()
    same(whole, native.robust_host(s, M), "300 passes against the host fold of the device's own samples")
    check_resolves(r, whole, "300 passes")
    plain_loader, plain = make(gpu_instance, sc)
    plain.render_passes(seeds)
    same(image, plain.read(), "300 passes, beauty image against render_passes")
    r.reset()
    r.robust_begin(M)
    r.robust_passes(seeds[:100], 0)
    r.robust_passes(seeds[100:], 100)
    same(r.robust_buckets(M), whole, "100 + 200 passes, buckets")
    same(r.read(), image, "100 + 200 passes, beauty image")
    close(r, loader, plain, plain_loader)


def padded_cases():
    for key, build, kernel in gs.form_cases(ragged=True):
        if kernel[0] in (17, 19) and not kernel[1]:
            yield pytest.param(build, kernel[0], id=key)


@pytest.mark.parametrize("build,form", list(padded_cases()))
def test_padded_tiles_and_deep_trees(gpu_instance, port, build, form):
    """The ragged 33 x 17 view on the three-level tree (edge tiles padded on both axes) and the form-17 deep scene."""
    sc = build()
    seeds = SEEDS[:11]
    s = sp.oracle_samples(port, sc, seeds)
    loader, r = make(gpu_instance, sc)
    for M in (3, 5):
        r.reset()
        r.robust_begin(M)
        r.robust_passes(seeds)
        assert r.kernel_info()["tree"] == form, r.kernel_info()
        want = native.robust_host(s, M)
        same(r.robust_buckets(M), want, f"form {form} M={M} buckets")
        check_resolves(r, want, f"form {form} M={M}")
        same(r.read(), port.render_passes(sc, seeds), f"form {form} M={M} beauty image")
    close(r, loader)


@pytest.mark.parametrize("tile", [0, 7])
def test_shards_fold_their_own_pixels(gpu_instance, port, tile):
    """Block shards (tile 0) and run shards of 7 pixels at world 3: on every rank the pixels it owns equal the unsharded buckets and
    the others stay zero; the ranks together own every pixel once."""
    sc = gs.make("outdoor")
    M, world = 5, 3
    want = native.robust_host(samples_of("outdoor", port), M)
    image = port.render_passes(sc, SEEDS).reshape(sc.height, sc.width, 3)
    loader, r = make(gpu_instance, sc)
    owned = np.zeros((sc.height, sc.width), np.int32)
    y, x = np.mgrid[0:sc.height, 0:sc.width]
    # the ownership rule of chunky_render_set_shard: runs of `tile` pixel indices, or 16 x 16 blocks, dealt round-robin
    unit = (y * sc.width + x) // tile if tile else (y >> 4) * ((sc.width + 15) >> 4) + (x >> 4)
    for rank in range(world):
        r.set_shard(rank, world, tile)
        r.reset()
        r.robust_begin(M)
        r.robust_passes(SEEDS)
        got = r.robust_buckets(M)
        mine = unit % world == rank
        assert 0 < mine.sum() < mine.size
        same(got[:, mine], want[:, mine], f"rank {rank} own pixels")
        assert not got[:, ~mine].any()
        same(r.read().reshape(sc.height, sc.width, 3)[mine], image[mine], f"rank {rank} beauty image")
        resolved, trim = r.robust_resolve()
        wimg, wtrim = native.robust_host_resolve(got)
        same(resolved, wimg, f"rank {rank} resolve")
        assert np.array_equal(trim, wtrim) and not resolved[~mine].any() and not trim[~mine].any()
        owned += mine
    assert (owned == 1).all()
    close(r, loader)


@pytest.mark.parametrize("stream", sorted(rs.synthetic_streams()))
def test_selftest_kernels_on_synthetic_streams(gpu_instance, stream):
    s = rs.synthetic_streams()[stream]
    n, h, w, _ = s.shape
    L = native.lib()
    for M in native.ROBUST_BUCKETS:
        for first in (0, 7):
            want = native.robust_host(s, M, first)
            for mode in MODES:
                for gain in GAINS:
                    p = native.robust_params(mode, gain)
                    buckets, image, trim = np.empty((M, h, w, 3), np.float32), np.empty((h, w, 3), np.float32), np.empty((h, w), np.uint8)
                    native.check(L.chunky_selftest_robust(gpu_instance._h, w, h, native.ptr(s), n, M, first, C.byref(p), native.ptr(buckets),
                                                          native.ptr(image), native.ptr(trim)))
                    same(buckets, want, f"{stream} M={M} first={first} buckets")
                    wimg, wtrim = native.robust_host_resolve(want, p)
                    same(image, wimg, f"{stream} M={M} first={first} mode {mode} gain {gain} image")
                    assert np.array_equal(trim, wtrim), (stream, M, first, mode, gain)


def test_robust_denoise_equals_the_host_filter_of_the_resolved_image(gpu_instance, port):
    sc = gs.make("indoor")
    loader, r = make(gpu_instance, sc)
    r.robust_begin(9)
    r.robust_passes(SEEDS)
    r.render_aov(SEEDS[:4])
    albedo, normal = r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL)
    beauty = r.read().copy()
    r.denoise_kernel_time()
    for p in (native.robust_params(), native.robust_params(native.ROBUST_MEDIAN)):
        resolved, _ = r.robust_resolve(p)
        got = r.robust_denoise(p)
        same(got, native.denoise_host(sc.width, sc.height, resolved, albedo, normal), f"robust_denoise mode {p.mode}")
    assert not np.array_equal(bits(resolved), bits(beauty))
    assert r.denoise_kernel_time()[1] > 0
    same(r.denoise(), native.denoise_host(sc.width, sc.height, beauty, albedo, normal), "denoise of the beauty image afterwards")
    same(r.read(), beauty, "the framebuffer after the filters")
    close(r, loader)


def all_images(r):
    """every image and map of the target that is not the robust state, as one list of byte strings"""
    out = [r.read().tobytes(), r.read_aov(native.AOV_ALBEDO).tobytes(), r.read_aov(native.AOV_NORMAL).tobytes()]
    out += [a.tobytes() if hasattr(a, "tobytes") else a for a in r.read_matte()]
    out += [r.read_occlusion(native.AOV_AO).tobytes(), r.read_occlusion(native.AOV_SUN).tobytes()]
    out += [r.read_light(k).tobytes() for k in range(4)]
    out += [r.adaptive_counts().tobytes(), r.adaptive_noise().tobytes()]
    return out


def other_timers(r):
    return [r.kernel_time(), r.aov_kernel_time(), r.matte_kernel_time(), r.occlusion_time(), r.lights_time(), r.adaptive_kernel_time(), r.denoise_kernel_time()]


def test_repeatability_and_isolation(gpu_instance, port):
    sc = gs.make("outdoor")
    M = 9
    loader, r = make(gpu_instance, sc)
    # the other images first
    r.render_adaptive(SEEDS[:16], native.adaptive_params(threshold=0.2, floor=0.01, min_spp=8, check_interval=4))
    r.render_aov(SEEDS[:3])
    r.render_matte(SEEDS[:3])
    r.render_occlusion(SEEDS[:3], 8.0)
    r.render_lights(SEEDS[:3])
    r.reset()
    r.render_passes(SEEDS[:5])
    before = all_images(r)
    other_timers(r)
    # robust calls touch none of them but the framebuffer, and none of their timers
    r.robust_begin(M)
    r.robust_passes(SEEDS[:20], 5)
    first = (r.robust_buckets(M).tobytes(), r.robust_resolve()[0].tobytes(), r.robust_resolve()[1].tobytes())
    after = all_images(r)
    assert after[1:] == before[1:]
    same(r.read(), port.render_passes(sc, SEEDS[:5].tolist() + SEEDS[:20].tolist()), "beauty image: 5 plain passes, then 20 robust ones")
    assert [t[1] for t in other_timers(r)] == [0] * 7
    ms, launches, resolve_ms = r.robust_kernel_time()
    assert ms > 0 and launches == 1 and resolve_ms > 0 and r.robust_kernel_time() == (0.0, 0, 0.0)
    # the other calls do not touch the robust state: chunky_render_passes between robust calls adds to the beauty image only
    r.render_passes(SEEDS[20:24], 25)
    r.render_aov(SEEDS[:2])
    r.render_matte(SEEDS[:2])
    r.render_occlusion(SEEDS[:2], 8.0)
    r.render_lights(SEEDS[:2])
    r.denoise()
    assert r.robust_kernel_time() == (0.0, 0, 0.0)
    assert r.robust_buckets(M).tobytes() == first[0] and r.robust_bucket(0)[1] == 20
    r.reset()  # not even the reset of the framebuffer
    assert r.robust_buckets(M).tobytes() == first[0] and r.robust_resolve()[0].tobytes() == first[1]
    r.render_adaptive(SEEDS[:16], native.adaptive_params(threshold=0.2, floor=0.01, min_spp=8, check_interval=4))
    assert r.robust_buckets(M).tobytes() == first[0] and r.robust_bucket(0)[1] == 20
    r.robust_passes(SEEDS[20:], 0)  # ... and the state goes on where it was
    same(r.robust_buckets(M), native.robust_host(samples_of("outdoor", port), M), "the buckets after all 40 samples")
    # two runs give identical bytes
    r.reset()
    r.robust_begin(M)
    r.robust_passes(SEEDS[:20], 5)
    second = (r.robust_buckets(M).tobytes(), r.robust_resolve()[0].tobytes(), r.robust_resolve()[1].tobytes())
    assert second == first
    r.robust_begin(0)  # released
    with pytest.raises(native.ChunkyHipError) as e:
        r.robust_bucket(0)
    assert e.value.code == native.E_STATE
    close(r, loader)


def expect(code, fn):
    with pytest.raises(native.ChunkyHipError) as e:
        fn()
    assert e.value.code == code, e.value


def test_every_abi_error(gpu_instance):
    sc = gs.make("outdoor")
    L = native.lib()
    loader, r = make(gpu_instance, sc)
    np_ = sc.width * sc.height
    out, trim = np.zeros(3 * np_, np.float32), np.zeros(np_, np.uint8)
    ok = native.robust_params()
    # before begin
    expect(native.E_STATE, lambda: r.robust_passes(SEEDS[:4]))
    expect(native.E_STATE, lambda: r.robust_bucket(0))
    expect(native.E_STATE, r.robust_resolve)
    r.render_aov(SEEDS[:1])
    expect(native.E_STATE, r.robust_denoise)
    # bucket counts
    for bad in (1, 2, 4, 8, 16, 17, -3):
        expect(native.E_INVALID, lambda: r.robust_begin(bad))
    expect(native.E_STATE, lambda: r.robust_bucket(0))  # a refused begin left no state
    r.robust_begin(5)
    # fewer than M samples
    r.robust_passes(SEEDS[:4])
    expect(native.E_STATE, r.robust_resolve)
    expect(native.E_STATE, r.robust_denoise)
    r.robust_passes(SEEDS[4:5], 4)
    r.robust_resolve()
    r.robust_denoise()
    # NULL pointers and wrong counts
    h = r._h
    assert L.chunky_render_robust_passes(h, None, 3, 0) == native.E_INVALID
    assert L.chunky_render_robust_passes(h, native.ptr(SEEDS), -1, 0) == native.E_INVALID
    assert L.chunky_render_robust_passes(h, native.ptr(SEEDS), 1, -1) == native.E_INVALID
    assert L.chunky_render_robust_passes(None, native.ptr(SEEDS), 1, 0) == native.E_INVALID
    assert L.chunky_render_robust_begin(None, 3) == native.E_INVALID
    assert L.chunky_render_robust_read_bucket(h, 0, None, out.size, None) == native.E_INVALID
    assert L.chunky_render_robust_read_bucket(h, 0, native.ptr(out), out.size - 3, None) == native.E_INVALID
    assert L.chunky_render_robust_read_bucket(h, 5, native.ptr(out), out.size, None) == native.E_INVALID
    assert L.chunky_render_robust_read_bucket(h, -1, native.ptr(out), out.size, None) == native.E_INVALID
    assert L.chunky_render_robust_read_bucket(h, 4, native.ptr(out), out.size, None) == 0
    assert L.chunky_render_robust_resolve(h, None, native.ptr(out), out.size, None, 0) == native.E_INVALID
    assert L.chunky_render_robust_resolve(h, C.byref(ok), None, out.size, None, 0) == native.E_INVALID
    assert L.chunky_render_robust_resolve(h, C.byref(ok), native.ptr(out), out.size + 1, None, 0) == native.E_INVALID
    assert L.chunky_render_robust_resolve(h, C.byref(ok), native.ptr(out), out.size, native.ptr(trim), np_ - 1) == native.E_INVALID
    assert L.chunky_render_robust_resolve(None, C.byref(ok), native.ptr(out), out.size, None, 0) == native.E_INVALID
    dn = native.denoise_params()
    assert L.chunky_render_robust_denoise(h, None, C.byref(dn), native.ptr(out), out.size) == native.E_INVALID
    assert L.chunky_render_robust_denoise(h, C.byref(ok), None, native.ptr(out), out.size) == native.E_INVALID
    assert L.chunky_render_robust_denoise(h, C.byref(ok), C.byref(dn), None, out.size) == native.E_INVALID
    assert L.chunky_render_robust_denoise(h, C.byref(ok), C.byref(dn), native.ptr(out), out.size - 1) == native.E_INVALID
    assert L.chunky_render_robust_kernel_time(None, None, None, None) == native.E_INVALID
    assert L.chunky_render_robust_kernel_time(h, None, None, None) == 0
    # a bad mode, a negative or NaN gain, a short struct
    for mode, gain in ((3, 1.0), (-1, 1.0), (native.ROBUST_GINI, -0.5), (native.ROBUST_GINI, float("nan")), (native.ROBUST_GINI, float("inf"))):
        expect(native.E_INVALID, lambda: r.robust_resolve(native.robust_params(mode, gain)))
        expect(native.E_INVALID, lambda: r.robust_denoise(native.robust_params(mode, gain)))
    short = native.robust_params()
    short.size = 8
    expect(native.E_INVALID, lambda: r.robust_resolve(short))
    # the self test's arguments
    s = np.zeros((3, 2, 2, 3), np.float32)
    ctx = gpu_instance._h

    def selftest(w=2, h_=2, samples=s, n=3, M=3, first=0, p=ok):
        return L.chunky_selftest_robust(ctx, w, h_, native.ptr(samples) if samples is not None else None, n, M, first, C.byref(p) if p is not None else None,
                                        None, None, None)

    assert selftest() == 0
    for bad in (dict(w=0), dict(h_=-1), dict(samples=None), dict(n=0), dict(n=257), dict(M=4), dict(M=17), dict(first=-1), dict(p=None), dict(p=short)):
        assert selftest(**bad) == native.E_INVALID, bad
    assert L.chunky_selftest_robust(None, 2, 2, native.ptr(s), 3, 3, 0, C.byref(ok), None, None, None) == native.E_INVALID
    # a sharded target resolves its share, but does not denoise it
    r.set_shard(0, 2, 0)
    r.robust_resolve()
    expect(native.E_STATE, r.robust_denoise)
    r.set_shard(0, 1, 256)
    # a fallback-kernel target, by option
    r.set_option(native.OPT_KERNEL, 8)
    expect(native.E_STATE, lambda: r.robust_passes(SEEDS[:2]))
    r.set_option(native.OPT_KERNEL, 0)
    before = r.robust_buckets(5).tobytes()
    # a biome map on the scene
    loader.set_biome_tints(0, 0, np.full((4, 4, 3), 0x40A030, np.int32))
    expect(native.E_STATE, lambda: r.robust_passes(SEEDS[:2]))
    r.set_option(native.OPT_BIOME_TINT, 0)  # ... unless the target does not tint
    r.robust_passes(SEEDS[5:6], 5)
    r.set_option(native.OPT_BIOME_TINT, 1)
    loader.set_biome_tints(0, 0, None)
    assert r.robust_bucket(0)[1] == 6 and r.robust_buckets(5).tobytes() != before  # the refused calls folded nothing, the accepted one did
    close(r, loader)
    # the fallback-only scene of tests/test_gpu_deep_trees.py: entities in an octree without a wide tree
    deep = gs.embedded("entities", 16)
    loader, r = make(gpu_instance, deep)
    r.robust_begin(3)
    expect(native.E_STATE, lambda: r.robust_passes(SEEDS[:3]))
    r.render_passes(SEEDS[:1])
    assert r.kernel_info()["pool"] < 0
    close(r, loader)
    g = RendererInstance.group([0, 0])  # a group's target
    loader, r = make(g, sc)
    expect(native.E_STATE, lambda: r.robust_begin(3))
    expect(native.E_STATE, lambda: r.robust_passes(SEEDS[:3]))
    expect(native.E_STATE, lambda: r.robust_bucket(0))
    expect(native.E_STATE, r.robust_resolve)
    expect(native.E_STATE, r.robust_denoise)
    expect(native.E_STATE, r.robust_kernel_time)
    close(r, loader)
    g.close()
