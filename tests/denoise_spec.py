"""The denoiser's specification (include/chunky_hip.h, chunky_denoise_host) restated in numpy, independently of csrc/denoise_spec.h:
an edge-avoiding A-Trous filter over colour C guided by albedo A and normal N, evaluated in float64 or, with dtype=np.float32, in
float32 with one rounding per operation.  A plain helper module for the denoise tests and tools (not a conftest).

The difference between the two evaluations, on given inputs, is what float arithmetic costs there; four times it is the bound the
tests hold chunky_denoise_host to (`tolerance`)."""
import numpy as np

EPS = np.float32(2.0 ** -10)
K1D = (0.375, 0.25, 0.0625)


def coefficients(iterations, sigma_color, sigma_normal, sigma_albedo):
    """(c_i for each iteration, c_n, c_a), computed in float32 as the host computes them once per call."""
    one = np.float32(1)
    sc, sn, sa = np.float32(sigma_color), np.float32(sigma_normal), np.float32(sigma_albedo)
    c_i = [np.float32(4 ** i) / (sc * sc) for i in range(iterations)]
    return c_i, one / (sn * sn), one / (sa * sa)


def _finite3(a):
    return np.isfinite(a).all(axis=-1)


def denoise(color, albedo, normal, iterations=5, sigma_color=1.0, sigma_normal=1.0, sigma_albedo=1.0, demodulate=True, dtype=np.float64):
    """color / albedo / normal: (H, W, 3).  Returns (H, W, 3) of `dtype`."""
    C = np.asarray(color, np.float32).astype(dtype)
    A = np.asarray(albedo, np.float32).astype(dtype)
    N = np.asarray(normal, np.float32).astype(dtype)
    H, W, _ = C.shape
    c_i, c_n, c_a = coefficients(iterations, sigma_color, sigma_normal, sigma_albedo)
    c_n, c_a = dtype(c_n), dtype(c_a)
    with np.errstate(all="ignore"):
        m = np.where(A >= dtype(EPS), A, dtype(EPS))   # max(A, eps); a NaN albedo counts as eps
        D = C / m if demodulate else C.copy()
        for i in range(iterations):
            s = 1 << i
            ci = dtype(c_i[i])
            sw = np.zeros((H, W), dtype)
            acc = np.zeros((H, W, 3), dtype)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = s * dy, s * dx
                    y0, y1 = max(0, -oy), min(H, H - oy)
                    x0, x1 = max(0, -ox), min(W, W - ox)
                    if y0 >= y1 or x0 >= x1:
                        continue   # every such tap lies outside the image
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                    h = dtype(K1D[abs(dx)] * K1D[abs(dy)])
                    e, f, g = D[Q] - D[P], N[Q] - N[P], A[Q] - A[P]
                    dc = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
                    dn = (f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2]
                    da = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
                    x = (dc * ci + dn * c_n) + da * c_a
                    ok = _finite3(D[Q]) & np.isfinite(x)
                    w = np.where(ok, h * np.exp(-np.where(ok, x, 0)), 0).astype(dtype)
                    sw[P] = sw[P] + w
                    acc[P] = acc[P] + np.where(ok[..., None], w[..., None] * np.where(ok[..., None], D[Q], 0), 0).astype(dtype)
            keep = ~_finite3(D) | ~(sw > 0)
            D = np.where(keep[..., None], D, acc / np.where(keep, 1, sw)[..., None]).astype(dtype)
        out = D * m if demodulate else D
        out = np.where(_finite3(C)[..., None], out, C)   # a pixel whose input colour is not finite comes back as it went in
    return out.astype(dtype)


def tolerance(color, albedo, normal, **params):
    """(measured, bound, reference): measured = the largest difference between the float32 and the float64 restatement on these
    inputs (over outputs finite in both), bound = 4 * measured, reference = the float64 result."""
    r64 = denoise(color, albedo, normal, dtype=np.float64, **params)
    r32 = denoise(color, albedo, normal, dtype=np.float32, **params)
    both = np.isfinite(r64) & np.isfinite(r32)
    with np.errstate(invalid="ignore"):
        measured = float(np.abs(r32.astype(np.float64) - r64)[both].max()) if both.any() else 0.0
    return measured, 4.0 * measured, r64


def synthetic(width, height, seed, noise=0.3):
    """Seeded random colour over guides with step edges: albedo and normal are piecewise constant over a few rectangles."""
    rng = np.random.default_rng(seed)
    A = np.empty((height, width, 3), np.float32)
    N = np.empty((height, width, 3), np.float32)
    A[:] = rng.uniform(0.1, 0.9, 3)
    N[:] = (0, 1, 0)
    for _ in range(5):
        y0, x0 = int(rng.integers(0, height)), int(rng.integers(0, width))
        y1, x1 = int(rng.integers(y0, height)) + 1, int(rng.integers(x0, width)) + 1
        A[y0:y1, x0:x1] = rng.uniform(0.05, 1.0, 3)
        n = rng.normal(size=3)
        N[y0:y1, x0:x1] = n / np.linalg.norm(n)
    light = rng.uniform(0.5, 2.0, 3).astype(np.float32)
    C = (A * light * (1 + noise * rng.standard_normal((height, width, 3)))).astype(np.float32)
    return np.abs(C), A, N


QUALITY_SIZE = (128, 96)
QUALITY_PASSES = (8, 512)
_oracle_cache = {}


def oracle_inputs(name, width=QUALITY_SIZE[0], height=QUALITY_SIZE[1], passes=QUALITY_PASSES[0], reference_passes=None):
    """A golden scene rendered on the CPU oracle (oracle/port.c): colour after `passes` passes, albedo and normal of the same passes
    (aov_spec.expected_aov), each (height, width, 3); with reference_passes also the colour after that many passes."""
    key = (name, width, height, passes, reference_passes)
    if key not in _oracle_cache:
        from oracle import binding
        import golden_scenes as gs
        from aov_spec import expected_aov
        from chunkyclplugin_amd import native
        sc = gs.make(name).with_view(width, height)
        h = binding.SceneHandle(sc)
        port = binding.port()
        seeds = native.java_random_ints(max(passes, reference_passes or 0))
        shape = (height, width, 3)
        color = port.render_passes(h, seeds[:passes]).reshape(shape).copy()
        albedo, normal = expected_aov(port, h, seeds[:passes], np.arange(width * height))
        out = [color, albedo.reshape(shape), normal.reshape(shape)]
        if reference_passes:
            out.append(port.render_passes(h, seeds[:reference_passes]).reshape(shape).copy())
        _oracle_cache[key] = tuple(out)
    return _oracle_cache[key]


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
