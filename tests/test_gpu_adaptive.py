"""Adaptive sampling on the device (chunky_render_adaptive, csrc/adaptive.hip) against its specification: counts and (m, M2) equal
chunky_adaptive_host fed with the oracle's per-pass samples, and the image equals, on the pixels of each distinct count n, the
oracle's image after n passes — bit for bit.  Also: the list route of render_pool on its own, larger and ragged views, the entity
BVH / projected / extended instantiations, a caller-owned buffer, repeatability, what follows an adaptive call, and the errors."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding
from oracle.binding import PortExt

import adaptive_spec as sp
import golden_scenes as gs
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, pool_slot_order
from test_adaptive_cpu import CARRIES, MAX_SPP, SETTINGS, params, samples_of

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
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = (g != w).reshape(g.shape[0] * g.shape[1], -1).any(axis=1)
        i = int(np.argmax(bad))
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} pixels differ (first: pixel {i}, {got.reshape(bad.size, -1)[i].tolist()} "
                    f"against {want.reshape(bad.size, -1)[i].tolist()})")


def check_against_samples(r, s, seeds, p, what, image_after=None):
    """The adaptive run of r against chunky_adaptive_host on the samples s; image_after(n) = the expected image after n passes
    (default: the running mean of s)."""
    image, counts, noise, summary = r.render_adaptive(seeds, p)
    wc, wimg, wst = native.adaptive_host(s, p)
    if not np.array_equal(counts, wc):
        pytest.fail(f"{what}: counts differ at {int((counts != wc).sum())} of {wc.size} pixels; device {np.unique(counts).tolist()}, host {np.unique(wc).tolist()}")
    same(noise, wst, what + " (m, M2)")
    for n in np.unique(wc):
        want = (image_after or (lambda k: sp.running_mean(s, k)))(int(n)).reshape(wimg.shape)
        sel = wc == n
        same(image[sel][None], want[sel][None], f"{what} image on the pixels of count {int(n)}")
    same(image, wimg, what + " image against the host's")
    assert summary["samples"] == int(wc.sum()) and summary["passes"] == int(wc.max()), summary
    assert r.kernel_info()["pool"] >= 0, r.kernel_info()  # a render_pool instantiation ran
    return counts, summary


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", gs.NAMES)
def test_golden_scenes_equal_the_specification_on_oracle_samples(gpu_instance, port, name, setting):
    sc = gs.make(name)
    loader, r = make(gpu_instance, sc)
    mn, ci, thr = setting
    counts, summary = check_against_samples(r, samples_of(name, port), SEEDS, params(mn, ci, thr), f"{name} {setting}")
    if setting == SETTINGS[CARRIES[name]]:  # the pair that carries the non-degeneracy condition (tests/test_adaptive_cpu.py)
        assert len(np.unique(counts)) >= 3 and (counts < MAX_SPP).mean() >= 0.1 and summary["active"][-1] >= 0.1 * counts.size, summary
    assert summary["checks"] == len(summary["active"]) and all(a >= b for a, b in zip(summary["active"], summary["active"][1:]))
    close(r, loader)


@pytest.mark.parametrize("name", ["outdoor", "entities"])
def test_render_pool_through_a_hand_made_list(gpu_instance, port, name):
    """The list route on its own: a permuted subset of the pixels (not a multiple of 256: the last tile is padded), every listed pixel
    equals the oracle's, every other pixel keeps the marker it held."""
    sc = gs.make(name)
    seeds = SEEDS[:5]
    loader, r = make(gpu_instance, sc)
    rng = np.random.default_rng(12)
    np_ = sc.width * sc.height
    listed = rng.permutation(np_)[:1337].astype(np.int32)
    import torch
    marker = np.full((np_, 3), 7.25, np.float32)
    fb = torch.full((3 * np_,), 7.25, dtype=torch.float32, device="cuda")  # a caller-owned buffer holding the marker
    torch.cuda.synchronize()
    r.set_device_buffer(fb.data_ptr())
    r.render_list(listed, seeds)
    info = r.kernel_info()
    assert info["pool"] >= 0 and info["bvh"] == (name == "entities"), info
    got = r.read().reshape(np_, 3)
    want = port.render_passes(sc, seeds).reshape(np_, 3)
    assert np.array_equal(bits(got[listed]), bits(want[listed]))
    rest = np.ones(np_, bool)
    rest[listed] = False
    assert np.array_equal(bits(got[rest]), bits(marker[rest]))
    # ... and the whole image in slot order is the image of the block mapping
    r.render_list(pool_slot_order(sc.width, sc.height), seeds)
    assert np.array_equal(bits(r.read()), bits(want.reshape(-1)))
    with pytest.raises(native.ChunkyHipError) as e:  # an entry listed twice
        r.render_list(np.array([3, 4, 3], np.int32), seeds)
    assert e.value.code == native.E_INVALID
    r.set_device_buffer(None)
    close(r, loader)


def device_samples(r, seeds):
    """One-pass renders from a reset target: the sample of every pass (parity of those renders: tests/test_gpu_timed_kernels.py)."""
    out = np.empty((len(seeds), r.height, r.width, 3), np.float32)
    for k, s in enumerate(seeds):
        r.reset()
        r.render_passes([s])
        r.read(out[k].reshape(-1))
    return out


@pytest.mark.parametrize("size", [(1920, 1080), (1917, 1075)])
def test_headline_outdoor_view(gpu_instance, size):
    sc = gs.timed_view("outdoor").with_view(*size)
    seeds = native.java_random_ints(24)
    loader, r = make(gpu_instance, sc)
    s = device_samples(r, seeds)
    p = params(8, 8, SETTINGS[0][2])

    def image_after(n):
        r.reset()
        r.render_passes(seeds[:n])
        return r.read().copy()

    wc = native.adaptive_host(s, p)[0]
    wants = {int(n): image_after(int(n)) for n in np.unique(wc)}
    counts, summary = check_against_samples(r, s, seeds, p, f"outdoor {size}", image_after=lambda n: wants[n])
    assert len(np.unique(counts)) >= 3 and 0 < summary["active"][-1] < counts.size, summary
    close(r, loader)


def test_entity_world_on_a_bvh_instantiation(gpu_instance, port):
    sc = gs.make("entities")
    loader, r = make(gpu_instance, sc)
    check_against_samples(r, samples_of("entities", port), SEEDS, params(*SETTINGS[0]), "entities")
    assert r.kernel_info()["bvh"]
    close(r, loader)


def test_projected_camera(gpu_instance, port):
    from test_gpu_camera_projections import equivalent, projected
    sc = projected(gs.make("outdoor"), native.PROJ_FISHEYE)
    seeds = SEEDS[:24]
    s = np.stack([equivalent(port, sc, [int(k)]).reshape(sc.height, sc.width, 3) for k in seeds])
    loader, r = make(gpu_instance, sc)
    # (threshold 0.1, chosen on the CPU oracle: the fisheye sees mostly sky, and at 0.2 fewer than 10 % of its pixels stay to the end)
    counts, _ = check_against_samples(r, s, seeds, params(8, 4, 0.1), "fisheye")
    assert len(np.unique(counts)) >= 3 and 0.1 <= (counts < len(seeds)).mean() <= 0.9
    close(r, loader)


def test_extended_integrator_options(gpu_instance, port):
    from test_gpu_extensions import with_spec_words
    sc = with_spec_words(gs.make("outdoor"))
    seeds = SEEDS[:24]
    ext = dict(bsdf=1, nee=1)
    with PortExt(port, sc, **ext):
        s = sp.oracle_samples(port, sc, seeds)
    loader, r = make(gpu_instance, sc, [(native.OPT_BSDF, 1), (native.OPT_EMITTER_NEE, 1)])
    counts, _ = check_against_samples(r, s, seeds, params(8, 4, SETTINGS[0][2]), "extended options")
    assert r.kernel_info()["ext"]
    assert len(np.unique(counts)) >= 3 and 0.1 <= (counts < len(seeds)).mean() <= 0.9
    close(r, loader)


def test_caller_owned_device_buffer(gpu_instance, port):
    import torch
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    fb = torch.full((3 * sc.width * sc.height,), 3.5, dtype=torch.float32, device="cuda")
    r.set_device_buffer(fb.data_ptr())
    image, counts, _, _ = r.render_adaptive(SEEDS, params(*SETTINGS[0]))
    wc, wimg, _ = native.adaptive_host(samples_of("outdoor", port), params(*SETTINGS[0]))
    assert np.array_equal(counts, wc)
    torch.cuda.synchronize()
    assert np.array_equal(bits(fb.cpu().numpy()), bits(wimg.reshape(-1))) and np.array_equal(bits(image), bits(wimg))
    r.set_device_buffer(None)
    close(r, loader)


def test_two_runs_give_identical_bytes(gpu_instance):
    sc = gs.timed_view("outdoor").with_view(480, 270)
    seeds = native.java_random_ints(32)
    loader, r = make(gpu_instance, sc)
    a = r.render_adaptive(seeds, params(8, 8, SETTINGS[0][2]))
    b = r.render_adaptive(seeds, params(8, 8, SETTINGS[0][2]))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]
    assert len(np.unique(a[1])) >= 3
    ms, rounds = r.adaptive_kernel_time()
    assert ms > 0 and rounds == 2 * a[3]["rounds"]
    assert r.adaptive_kernel_time() == (0.0, 0)
    close(r, loader)


def test_the_target_afterwards(gpu_instance, port):
    """read, denoise and the AOV images see the adaptive image; the render timer does not see the adaptive launches; a plain reset +
    render_passes afterwards gives the usual image (shard and launch cap untouched)."""
    sc = gs.make("outdoor")
    loader, r = make(gpu_instance, sc)
    r.kernel_time()
    image, counts, _, _ = r.render_adaptive(SEEDS, params(*SETTINGS[0]))
    assert r.kernel_time() == (0.0, 0)
    assert np.array_equal(bits(r.read()), bits(image.reshape(-1)))
    r.render_aov(SEEDS[:4])
    albedo, normal = r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL)
    l2, plain = make(gpu_instance, sc)
    plain.render_aov(SEEDS[:4])
    assert np.array_equal(bits(albedo), bits(plain.read_aov(native.AOV_ALBEDO))) and np.array_equal(bits(normal), bits(plain.read_aov(native.AOV_NORMAL)))
    got = r.denoise()
    assert np.array_equal(bits(got.reshape(-1)), bits(native.denoise_host(sc.width, sc.height, image, albedo, normal)))
    assert np.array_equal(bits(r.read()), bits(image.reshape(-1)))  # the filter left the framebuffer alone
    r.reset()
    r.render_passes(SEEDS[:7])
    assert np.array_equal(bits(r.read()), bits(port.render_passes(sc, SEEDS[:7])))
    assert np.array_equal(r.adaptive_counts(), counts)  # the maps stay readable until the next adaptive run
    close(r, loader, plain, l2)


def expect_state(fn):
    with pytest.raises(native.ChunkyHipError) as e:
        fn()
    assert e.value.code == native.E_STATE, e.value


def test_state_and_argument_errors(gpu_instance):
    sc = gs.make("outdoor")
    p = params(*SETTINGS[0])
    loader, r = make(gpu_instance, sc)
    expect_state(r.adaptive_counts)  # before any adaptive run
    expect_state(r.adaptive_noise)
    r.set_shard(0, 2, 0)  # a sharded target
    expect_state(lambda: r.render_adaptive(SEEDS, p))
    r.set_shard(0, 1, 256)
    r.set_option(native.OPT_KERNEL, 8)  # sent to the fallback kernels by option
    expect_state(lambda: r.render_adaptive(SEEDS, p))
    r.set_option(native.OPT_KERNEL, 0)
    with pytest.raises(native.ChunkyHipError) as e:  # fewer seeds than min_spp
        r.render_adaptive(SEEDS[:4], p)
    assert e.value.code == native.E_INVALID
    expect_state(r.adaptive_counts)  # still none
    r.render_adaptive(SEEDS[:8], p)
    assert (r.adaptive_counts() == 8).all()  # max_spp == min_spp: no check is due
    close(r, loader)
    # the fallback-only scene of tests/test_gpu_deep_trees.py: entities in an octree without a wide tree
    deep = gs.embedded("entities", 16)
    loader, r = make(gpu_instance, deep)
    expect_state(lambda: r.render_adaptive(SEEDS, p))
    r.render_passes(SEEDS[:1])
    assert r.kernel_info()["pool"] < 0
    close(r, loader)
    g = RendererInstance.group([0, 0])  # a group's target
    loader, r = make(g, sc)
    expect_state(lambda: r.render_adaptive(SEEDS, p))
    expect_state(r.adaptive_counts)
    close(r, loader)
    g.close()
