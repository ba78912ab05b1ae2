"""The denoiser without a device: chunky_denoise_host (the loop over csrc/denoise_spec.h that the kernels are held to, bit for bit,
by tests/test_gpu_denoise.py) against the independent numpy restatement of its specification in tests/denoise_spec.py.

The bound of every comparison "within the tolerance" is denoise_spec.tolerance on the inputs at hand: four times the largest
difference between the float32 and the float64 restatement, neither of which is the code under test (two float evaluation orders of
the same sums may differ by a small multiple of each other's rounding error).  Figures on this repository's inputs:
profiles/denoise_tolerance.json and profiles/denoise_quality.json (tools/denoise_quality.py)."""
import ctypes as C
import re

import mpmath
import numpy as np
import pytest

import denoise_spec as ds
from chunkyclplugin_amd import native

ORACLE_SCENES = ["outdoor", "indoor", "entities"]
SPEC = dict(iterations=5, sigma_color=4.0, sigma_normal=0.5, sigma_albedo=0.1)   # the defaults


def host(color, albedo, normal, **kw):
    h, w, _ = np.shape(color)
    return native.denoise_host(w, h, color, albedo, normal, native.denoise_params(**kw)).reshape(h, w, 3)


def assert_within(got, want, bound, what):
    both = np.isfinite(got) & np.isfinite(want)
    assert (np.isfinite(got) == np.isfinite(want)).all(), what
    with np.errstate(invalid="ignore"):
        worst = float(np.abs(got.astype(np.float64) - want)[both].max())
    print(f"{what}: largest difference {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound, f"{what}: {worst:.3e} > {bound:.3e}"


def test_header_declares_and_library_exports_the_denoise_entry_points():
    declared = native.declared_symbols()
    L = native.lib()
    for name in ("chunky_denoise_default_params", "chunky_denoise_host", "chunky_denoise_frame", "chunky_render_denoise",
                 "chunky_render_denoise_kernel_time", "chunky_denoise_exp"):
        assert name in declared and hasattr(L, name), name
    assert re.search(r"#define\s+CHUNKY_DENOISE_DEMODULATE\s+1u", open(native.HEADER).read())
    p = native.denoise_params()
    assert p.size == C.sizeof(native.DenoiseParams) and (p.iterations, p.flags) == (5, native.DENOISE_DEMODULATE)
    assert (p.sigma_color, p.sigma_normal, p.sigma_albedo) == tuple(np.float32(SPEC[k]) for k in ("sigma_color", "sigma_normal", "sigma_albedo"))


# ---- 1. the host function against the float64 restatement
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("demodulate", [True, False])
def test_host_equals_the_restatement_on_random_images_with_step_edges(seed, demodulate):
    C_, A, N = ds.synthetic(96, 64, seed)
    for iterations in (1, 3, 5, 8):
        kw = dict(SPEC, iterations=iterations, demodulate=demodulate)
        measured, bound, want = ds.tolerance(C_, A, N, **kw)
        assert 0 < measured < 1e-4   # (float32 rounding on values of order 1, not something else)
        assert_within(host(C_, A, N, **kw), want, bound, f"synthetic {seed} x{iterations} demodulate={demodulate}")


@pytest.mark.parametrize("name", ORACLE_SCENES)
@pytest.mark.parametrize("demodulate", [True, False])
def test_host_equals_the_restatement_on_oracle_renders(name, demodulate):
    color, albedo, normal = ds.oracle_inputs(name)[:3]
    kw = dict(SPEC, demodulate=demodulate)
    measured, bound, want = ds.tolerance(color, albedo, normal, **kw)
    assert measured > 0
    assert_within(host(color, albedo, normal, **kw), want, bound, f"{name} demodulate={demodulate}")


# ---- 2. dn_exp
def ulp_error(got, x):
    """|got - e^(-x)| in units of the last place of the true value (binary32, subnormals included)."""
    want = mpmath.exp(-mpmath.mpf(float(x)))
    e = mpmath.frexp(want)[1] if want > 0 else -149   # want = m * 2^e, 0.5 <= m < 1
    ulp = mpmath.ldexp(1, max(e - 24, -149))
    return float(abs(mpmath.mpf(float(got)) - want) / ulp)


def test_dn_exp_accuracy_on_a_dense_grid():
    mpmath.mp.prec = 100
    rng = np.random.default_rng(5)
    x = np.concatenate([np.linspace(0, 110, 22001), rng.uniform(0, 110, 8000), rng.uniform(0, 2, 8000), rng.uniform(86, 105, 4000)]).astype(np.float32)
    got = native.denoise_exp(x)
    worst = max(ulp_error(g, v) for g, v in zip(got, x))
    print(f"dn_exp: worst error {worst:.3f} ULP over {x.size} values")
    assert worst <= 3.0


def test_dn_exp_at_every_power_of_two():
    mpmath.mp.prec = 100
    x = np.array([2.0 ** k for k in range(-149, 128)], np.float32)
    got = native.denoise_exp(x)
    assert max(ulp_error(g, v) for g, v in zip(got, x)) <= 3.0
    assert (got[x > 104] == 0).all() and (got[x < 2.0 ** -25] == 1).all()


def test_dn_exp_exact_sign_and_monotone():
    assert native.denoise_exp([0.0])[0] == 1.0
    big = native.denoise_exp(np.array([104.0, 110.0, 128.0, 129.0, 1e6, 3e38, np.inf], np.float32))
    assert (big == 0).all() and not np.signbit(big).any()
    # consecutive floats: around every range-reduction boundary k ln 2 / (the halfway points (k + 1/2) ln 2), and a dense sweep
    runs = [np.float32(j * 0.5 * np.log(2)) for j in range(0, 320)]
    x = np.concatenate([np.frombuffer((np.arange(-256, 257, dtype=np.int64) + int(np.float32(c).view(np.uint32))).clip(0).astype(np.uint32).tobytes(), np.float32)
                        for c in runs] + [np.linspace(0, 110, 400001).astype(np.float32)])
    x = np.unique(x)   # sorted
    y = native.denoise_exp(x)
    assert not np.isnan(y).any() and (y >= 0).all() and not np.signbit(y).any()
    assert (np.diff(y) <= 0).all()


# ---- 3. properties
def test_a_constant_colour_stays_constant_whatever_the_guides():
    _, A, N = ds.synthetic(80, 60, 4)
    color = np.broadcast_to(np.array([0.25, 1.5, 0.7], np.float32), A.shape).copy()
    for demodulate in (True, False):
        kw = dict(SPEC, demodulate=demodulate)
        _, bound, _ = ds.tolerance(color, A, N, **kw)
        got = host(color, A, N, **kw)
        print(f"constant image demodulate={demodulate}: largest change {np.abs(got - color).max():.3e}, bound {bound:.3e}")
        assert np.abs(got.astype(np.float64) - color).max() <= bound


def test_without_demodulation_the_output_stays_within_the_input_range():
    C_, A, N = ds.synthetic(80, 60, 6)
    kw = dict(SPEC, demodulate=False)
    _, bound, _ = ds.tolerance(C_, A, N, **kw)
    got = host(C_, A, N, **kw)
    for k in range(3):
        assert got[..., k].min() >= C_[..., k].min() - bound and got[..., k].max() <= C_[..., k].max() + bound


def test_halves_with_different_normals_do_not_mix():
    rng = np.random.default_rng(8)
    h, w = 48, 64
    A = np.full((h, w, 3), 0.5, np.float32)
    N = np.zeros((h, w, 3), np.float32)
    N[:, :w // 2] = (1, 0, 0)
    N[:, w // 2:] = (0, 1, 0)
    color = np.empty((h, w, 3), np.float32)
    color[:, :w // 2] = rng.uniform(0.0, 1.0, (h, w // 2, 3))
    color[:, w // 2:] = rng.uniform(5.0, 6.0, (h, w - w // 2, 3))
    for demodulate in (False, True):   # (a constant albedo: demodulation scales every pixel alike)
        kw = dict(SPEC, sigma_normal=0.01, demodulate=demodulate)
        _, bound, _ = ds.tolerance(color, A, N, **kw)
        got = host(color, A, N, **kw)
        for half in (np.s_[:, :w // 2], np.s_[:, w // 2:]):
            assert got[half].min() >= color[half].min() - bound and got[half].max() <= color[half].max() + bound


def test_a_horizontal_flip_of_the_inputs_flips_the_output():
    C_, A, N = ds.synthetic(70, 50, 9)
    _, bound, _ = ds.tolerance(C_, A, N, **SPEC)
    a = host(C_, A, N, **SPEC)
    b = host(C_[:, ::-1].copy(), A[:, ::-1].copy(), N[:, ::-1].copy(), **SPEC)
    print(f"flip: largest difference {np.abs(a - b[:, ::-1]).max():.3e}, bound {bound:.3e}")
    assert np.abs(a.astype(np.float64) - b[:, ::-1]).max() <= bound


@pytest.mark.parametrize("demodulate", [True, False])
def test_bad_pixels_come_back_unchanged_and_do_not_spread(demodulate):
    C_, A, N = ds.synthetic(64, 48, 10)
    C_[10, 20, 1] = np.nan
    C_[30, 40] = np.inf
    got = host(C_, A, N, **dict(SPEC, demodulate=demodulate))
    np.testing.assert_array_equal(got[10, 20].view(np.uint32), C_[10, 20].view(np.uint32))
    np.testing.assert_array_equal(got[30, 40].view(np.uint32), C_[30, 40].view(np.uint32))
    mask = np.ones((48, 64), bool)
    mask[10, 20] = mask[30, 40] = False
    assert np.isfinite(got[mask]).all()
    _, bound, want = ds.tolerance(C_, A, N, **dict(SPEC, demodulate=demodulate))
    assert_within(got, want, bound, "with a NaN and an inf pixel")


def test_zero_albedo_yields_finite_output():
    C_, A, N = ds.synthetic(64, 48, 11)
    got = host(C_, np.zeros_like(A), N, **SPEC)
    assert np.isfinite(got).all()
    _, bound, want = ds.tolerance(C_, np.zeros_like(A), N, **SPEC)
    assert_within(got, want, bound, "albedo 0")


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 3)])
def test_degenerate_sizes_are_legal(shape):
    h, w = shape
    C_, A, N = ds.synthetic(w, h, 12)
    _, bound, want = ds.tolerance(C_, A, N, **SPEC)
    assert_within(host(C_, A, N, **SPEC), want, max(bound, 0.0), f"{w}x{h}")


# ---- 4. validation
def call_host(w, h, c, a, n, p, o):
    f = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    return native.lib().chunky_denoise_host(w, h, f(c), f(a), f(n), None if p is None else C.byref(p), f(o))


def test_invalid_arguments_are_refused():
    L = native.lib()
    img = np.zeros(3 * 4 * 3, np.float32)
    out = np.zeros_like(img)
    ok = native.denoise_params()
    assert call_host(4, 3, img, img, img, ok, out) == 0
    assert L.chunky_denoise_default_params(None) == native.E_INVALID
    for args in [(4, 3, None, img, img, ok, out), (4, 3, img, None, img, ok, out), (4, 3, img, img, None, ok, out), (4, 3, img, img, img, None, out),
                 (4, 3, img, img, img, ok, None), (0, 3, img, img, img, ok, out), (4, 0, img, img, img, ok, out), (-1, 3, img, img, img, ok, out)]:
        assert call_host(*args) == native.E_INVALID, args[:2]
        assert L.chunky_last_error()
    for field, values in [("iterations", (0, -1, 9)), ("sigma_color", (0.0, -1.0, np.nan, np.inf)), ("sigma_normal", (0.0, -2.0, np.nan, np.inf)),
                          ("sigma_albedo", (0.0, -0.5, np.nan, -np.inf))]:
        for v in values:
            p = native.denoise_params()
            setattr(p, field, v)
            assert call_host(4, 3, img, img, img, p, out) == native.E_INVALID, (field, v)
    p = native.denoise_params()
    p.size = native.DenoiseParams.flags.offset + 4 - 1   # one byte short of the first version of the struct (which ends with `flags`)
    assert call_host(4, 3, img, img, img, p, out) == native.E_INVALID
    p.size = 0
    assert call_host(4, 3, img, img, img, p, out) == native.E_INVALID
    # the device entry points validate before they look for a device
    assert L.chunky_denoise_frame(None, 4, 3, img.ctypes.data, img.ctypes.data, img.ctypes.data, C.byref(ok), out.ctypes.data) == native.E_INVALID
    assert L.chunky_render_denoise(None, C.byref(ok), out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_denoise_kernel_time(None, None, None) == native.E_INVALID
    assert L.chunky_denoise_exp(None, 3, out.ctypes.data) == native.E_INVALID


def test_a_larger_struct_is_accepted_and_only_the_known_part_is_read():
    class Bigger(C.Structure):
        _fields_ = [("known", native.DenoiseParams), ("later", C.c_float * 6)]
    C_, A, N = ds.synthetic(24, 16, 13)
    want = host(C_, A, N, **SPEC)
    big = Bigger()
    big.known = native.denoise_params(**SPEC)
    big.known.size = C.sizeof(Bigger)
    for fill in (0.0, np.nan, -7.0):
        for i in range(6):
            big.later[i] = fill
        out = np.zeros(C_.size, np.float32)
        f = lambda x: np.ascontiguousarray(x, np.float32).ctypes.data  # noqa: E731
        rc = native.lib().chunky_denoise_host(24, 16, f(C_), f(A), f(N), C.cast(C.byref(big), C.POINTER(native.DenoiseParams)), out.ctypes.data)
        assert rc == 0
        np.testing.assert_array_equal(out.view(np.uint32), want.reshape(-1).view(np.uint32))


# ---- 5. it denoises
@pytest.mark.parametrize("name", ["outdoor", "indoor"])
def test_the_default_parameters_reduce_the_error_of_an_8_pass_render(name):
    few, many = ds.QUALITY_PASSES
    color, albedo, normal, reference = ds.oracle_inputs(name, reference_passes=many)
    w, h = ds.QUALITY_SIZE
    out = native.denoise_host(w, h, color, albedo, normal).reshape(h, w, 3)
    before, after = ds.rmse(color, reference), ds.rmse(out, reference)
    print(f"{name}: RMSE against {many} passes: {few}-pass {before:.4f}, denoised {after:.4f}, ratio {after / before:.3f}")
    # the reference must itself be far below the 8-pass noise: its error is about sqrt(few / many) of it (independent samples)
    assert (few / many) ** 0.5 <= 0.125
    assert after < before
