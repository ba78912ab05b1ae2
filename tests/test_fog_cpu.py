"""The ground-fog layer without a GPU: the CPU specification (tests/fog_port.c over csrc/fog_spec.h) against the
oracle with the layer off, known answers and error bounds of the header's functions, two analytic images (absorption, the white
furnace), and the device-free part of the C API (chunky_fog_check, plan_fog, octree2.fog_settings)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import fog_spec
import golden_scenes as gs
from chunkyclplugin_amd import native, octree2, scenes
from oracle.binding import PortExt

INF = np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def fog():
    return fog_spec.lib()


# ---- 1. with the layer off the copied loop is the oracle's integrator ----
@pytest.mark.parametrize("name", ["outdoor", "indoor", "entities"])
@pytest.mark.parametrize("ext", [{}, dict(bsdf=1, nee=1, sun_sampling=1)], ids=["defaults", "bsdf-nee-sun"])
def test_fog_off_is_the_oracle(port, fog, name, ext):
    sc = gs.make(name).with_view(96, 64)
    seeds = scenes.java_random_ints(4)
    with PortExt(port, sc, **ext):
        want = port.render_passes(sc, seeds)
    with PortExt(fog, sc, **ext):
        got = fog.fog_render_passes(sc, seeds)
        gids = np.arange(0, 96 * 64, 7, dtype=np.int32)
        listed = fog.fog_render_gids(sc, seeds, gids)
    np.testing.assert_array_equal(bits(got), bits(want))
    np.testing.assert_array_equal(bits(listed.reshape(-1, 3)[gids]), bits(want.reshape(-1, 3)[gids]))
    assert want.max() > 0


# ---- 2. the interval ----
# (o.y, d, t_end) over the slab [10, 20) -> (non-empty, ta, tb, |d|); ta / tb are only pinned for a non-empty interval
INTERVALS = [
    ("parallel inside", 15.0, (1, 0, 0), INF, (1, 0.0, INF, 1.0)),
    ("parallel inside, a hit", 15.0, (0, 0, 1), 7.0, (1, 0.0, 7.0, 1.0)),
    ("parallel inside, d.y = -0", 15.0, (1, -0.0, 0), 3.0, (1, 0.0, 3.0, 1.0)),
    ("parallel on y_min (inside)", 10.0, (1, 0, 0), INF, (1, 0.0, INF, 1.0)),
    ("parallel outside", 25.0, (1, 0, 0), INF, (0, None, None, 1.0)),
    ("parallel exactly on y_max (outside)", 20.0, (1, 0, 0), INF, (0, None, None, 1.0)),
    ("entering from above", 30.0, (0, -1, 0), INF, (1, 10.0, 20.0, 1.0)),
    ("entering from below", 4.0, (0, 2, 0), INF, (1, 3.0, 8.0, 2.0)),
    ("starting inside, downwards", 15.0, (0, -1, 0), INF, (1, 0.0, 5.0, 1.0)),
    ("starting inside, upwards", 15.0, (0, 1, 0), INF, (1, 0.0, 5.0, 1.0)),
    ("leaving before a hit", 15.0, (0, 1, 0), 8.0, (1, 0.0, 5.0, 1.0)),
    ("a hit inside the slab", 30.0, (0, -1, 0), 13.0, (1, 10.0, 13.0, 1.0)),
    ("a hit before the slab", 30.0, (0, -1, 0), 4.0, (0, None, None, 1.0)),
    ("a hit exactly where the slab begins", 30.0, (0, -1, 0), 10.0, (0, None, None, 1.0)),
    ("pointing away", 30.0, (0, 1, 0), INF, (0, None, None, 1.0)),
    ("non-unit d", 30.0, (3, -4, 0), INF, (1, 2.5, 5.0, 5.0)),
    ("non-unit d, short", 30.0, (0, -0.25, 0), INF, (1, 40.0, 80.0, 0.25)),
    ("d = 0", 15.0, (0, 0, 0), INF, (0, None, None, 0.0)),
]


def test_interval_known_answers(fog):
    rows = np.array([[oy, *d, t_end, 10.0, 20.0, 0.0] for _, oy, d, t_end, _ in INTERVALS], np.float32)
    out = fog.helpers_fog(0, rows)
    for (what, *_ignored, want), got in zip(INTERVALS, out):
        assert int(got[0]) == want[0], what
        assert got[3] == np.float32(want[3]), what
        if want[0]:
            assert (got[1], got[2]) == (np.float32(want[1]), np.float32(want[2])), what


# ---- 3. the transmittance ----
def ulps(a, b):
    """distance in binary32 steps between non-negative floats"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def test_transmittance_within_one_ulp_of_exp(fog):
    tau = np.exp2(np.linspace(-20.0, np.log2(200.0), 20001)).astype(np.float32)
    tau[-1] = 200.0
    got = fog.helpers_fog(1, tau.reshape(-1, 1))[:, 0]
    want = np.exp(-tau.astype(np.float64)).astype(np.float32)
    worst = int(ulps(got, want).max())
    print("fog_transmittance against float64 exp: worst", worst, "ulp over", tau.size, "optical depths")
    assert worst <= 1
    assert not np.isnan(got).any() and got.min() >= 0 and got.max() <= 1


def test_transmittance_is_total(fog):
    special = np.array([0.0, -0.0, -1.0, INF, -INF, np.nan, 1e-45, 3.4e38], np.float32)
    got = fog.helpers_fog(1, special.reshape(-1, 1))[:, 0]
    assert not np.isnan(got).any()
    assert got[0] == 1 and got[1] == 1 and got[2] == 1 and got[3] == 0 and got[4] == 1 and got[6] == 1 and got[7] == 0
    # an empty interval: exactly 1; an infinite one (a horizontal ray inside the slab, to infinity): exactly 0
    rows = np.array([[25.0, 1, 0, 0, INF, 10, 20, 0.5], [30.0, 0, -1, 0, 4.0, 10, 20, 0.5], [15.0, 1, 0, 0, INF, 10, 20, 0.5],
                     [15.0, 0, 0, 0, INF, 10, 20, 0.5]], np.float32)
    seg = fog.helpers_fog(2, rows)[:, 0]
    assert list(seg) == [1.0, 1.0, 0.0, 1.0]
    # every combination of zeros, ones, huge values and infinities for the origin, the direction and the end: never a NaN
    vals = np.array([0.0, -0.0, 1.0, -1.0, 15.0, 3e38, -3e38, INF, -INF, 1e-45], np.float32)
    grid = np.array(np.meshgrid(vals, vals, vals, vals, [0.0, 1.0, 7.0, 3e38, INF]), np.float32).reshape(5, -1).T   # o.y, d.x, d.y, d.z, t_end
    rows = np.zeros((len(grid), 8), np.float32)
    rows[:, :5], rows[:, 5], rows[:, 6], rows[:, 7] = grid, 10.0, 20.0, 0.25
    seg = fog.helpers_fog(2, rows)[:, 0]
    assert not np.isnan(seg).any() and seg.min() >= 0 and seg.max() <= 1
    itv = fog.helpers_fog(0, rows)
    assert not np.isnan(itv[itv[:, 0] == 1][:, 1:3]).any()


def test_free_flight_and_sphere(fog):
    u = (np.arange(0, 1 << 24, 4099, dtype=np.int64) / float(1 << 24)).astype(np.float32)   # draws of rt_pcg_float: multiples of 2^-24
    u = np.append(u, np.float32((2 ** 24 - 1) / 2 ** 24))
    s = fog.helpers_fog(3, np.stack([u, np.full_like(u, 0.125)], axis=1))[:, 0]
    want = -np.log1p(-u.astype(np.float64)) / 0.125
    assert s[0] == 0 and np.isfinite(s).all() and (s >= 0).all()
    # rt_log2_d is good to 2^-44 absolute (rt_math.h) — 2^-43 generously, on the natural logarithm — and two binary32 roundings follow
    assert (np.abs(s.astype(np.float64) - want) <= 2.0 ** -43 / 0.125 + 2 * np.spacing(want.astype(np.float32)).astype(np.float64)).all()
    assert int(ulps(s[u > 0.01], want.astype(np.float32)[u > 0.01]).max()) <= 2
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1 << 24, (4096, 2)).astype(np.float32) / np.float32(1 << 24)
    d = fog.helpers_fog(4, x)[:, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    assert np.abs(d.mean(axis=0)).max() < 5 / np.sqrt(3 * 4096)   # uniform on the sphere: each component has variance 1/3
    np.testing.assert_allclose(d[:, 2], 1 - 2 * x[:, 0].astype(np.float64), atol=1e-7)


# ---- 4. / 5. analytic images: an empty world under a constant white sky, vertical rays through a slab of optical depth 1 ----
W, H, PASSES = 64, 48, 8
SLAB = (4.0, 12.0)          # 8 blocks thick
SIGMA = 0.125               # optical depth 1 across it
SKY_SLACK = 2.0 ** -21      # a white sky's four bilinear weights sum to 1 within four binary32 steps: a sample that sees it is 1 +- this


def empty_world():
    """Nothing but air in a 16^3 octree, a uniform white sky of radiance 1, no sun; every pixel looks straight down through the slab from
    above it, half of them along a direction of length 2."""
    pal = scenes.Palettes()
    pal.block_invisible()
    b, m, a, q = pal.arrays()
    rays = np.zeros((W * H, 6), np.float32)
    rays[:, :3] = (8.0, 30.0, 8.0)
    rays[:, 4] = -1.0
    rays[1::2, 4] = -2.0
    return scenes.PackedScene(octree=scenes.build_octree(np.zeros((16, 16, 16), np.int32), 4), octree_depth=4, block_palette=b,
                              material_palette=m, aabb_models=a, quad_models=q, world_bvh=scenes.empty_bvh(), actor_bvh=scenes.empty_bvh(),
                              bvh_trigs=np.zeros(1, np.int32), atlas=np.zeros((1, 16, 16, 4), np.uint8), sky=np.full((8, 8, 4), 255, np.uint8),
                              sky_intensity=1.0, sun=scenes.pack_sun(0.6, 1.2, 1.0, False), camera=rays.reshape(-1), projector_type=-1,
                              width=W, height=H, name="empty")


def per_pass(sc, fog_layer, max_depth):
    """one sample per pixel and pass: (PASSES, W * H), the channels agree"""
    out = []
    for s in scenes.java_random_ints(PASSES):
        img = fog_spec.render(sc, [s], fog_layer, max_depth=max_depth).reshape(-1, 3)
        assert (img[:, 0] == img[:, 1]).all() and (img[:, 0] == img[:, 2]).all()
        out.append(img[:, 0].copy())
    return np.stack(out)


def test_absorbing_fog_is_beer_lambert():
    x = per_pass(empty_world(), (SIGMA, *SLAB, (0, 0, 0)), 5).astype(np.float64)
    assert ((x == 0) | (np.abs(x - 1) <= SKY_SLACK)).all()   # absorbed, or the sky at full weight: no transmittance factor
    n, t = x.size, np.exp(-1.0)
    se = np.sqrt(t * (1 - t) / n)
    print(f"absorbing fog: mean {x.mean():.6f}, exp(-1) {t:.6f}, standard error {se:.6f}, N {n}")
    assert abs(x.mean() - t) <= 5 * se
    for half in (x[:, 0::2], x[:, 1::2]):   # directions of length 1 and of length 2: the same physical slab
        assert abs(half.mean() - t) <= 5 * np.sqrt(t * (1 - t) / half.size)


def test_white_fog_furnace_conserves_energy():
    sc = empty_world()
    x = per_pass(sc, (SIGMA, *SLAB, (1, 1, 1)), 64).astype(np.float64)
    assert ((x == 0) | (np.abs(x - 1) <= SKY_SLACK)).all()
    se = x.std(ddof=1) / np.sqrt(x.size)
    print(f"furnace: mean {x.mean():.8f}, standard error of the samples {se:.3g}, samples at 0: {(x == 0).sum()} of {x.size}")
    assert abs(x.mean() - 1) <= 5 * se + SKY_SLACK
    # max depth 1: the unscattered fraction only — a scattered path ends at its first medium vertex, having seen nothing — which is,
    # bit for bit, the absorbing layer's image: the same draws decide, and black fog adds exact zeros afterwards
    one = per_pass(sc, (SIGMA, *SLAB, (1, 1, 1)), 1)
    black = per_pass(sc, (SIGMA, *SLAB, (0, 0, 0)), 5)
    np.testing.assert_array_equal(bits(one), bits(black))
    t = np.exp(-1.0)
    assert abs(one.astype(np.float64).mean() - t) <= 5 * np.sqrt(t * (1 - t) / one.size)


def test_census_counts_what_the_samples_met():
    sc = empty_world()
    _, c = fog_spec.render(sc, scenes.java_random_ints(2), (SIGMA, *SLAB, (1, 1, 1)), max_depth=3, census=True)
    assert c["segments"] >= 2 * W * H and 0 < c["medium"] < c["segments"], c
    assert c["medium_sun"] == 0 and c["surface_sun"] == 0 and c["emitter"] == 0 and c["parallel"] == 0, c
    _, c = fog_spec.render(sc, scenes.java_random_ints(2), (SIGMA, *SLAB, (1, 1, 1)), ext=dict(sun_sampling=1), max_depth=3, census=True)
    assert c["medium_sun"] == c["medium"] > 0, c
    _, off = fog_spec.render(sc, scenes.java_random_ints(1), (0.0, 0.0, 1.0, (1, 1, 1)), census=True)
    assert not any(off.values()), off


# ---- 6. the device-free C API ----
def test_fog_check_accepts_and_refuses():
    ok = native.fog_struct(0.05, 0.0, 64.0, (0.5, 0.6, 1.0))
    assert native.fog_check(ok) == 0
    assert native.fog_check(None) == 0                                  # NULL: off
    assert native.fog_check(native.fog_struct(0.0, 5.0, 1.0, (2, 2, 2))) == native.E_INVALID   # density 0 is "off", but a bad struct is still one
    assert native.fog_check(native.fog_struct(0.0, 0.0, 1.0)) == 0
    bad = [native.fog_struct(-0.1, 0, 64), native.fog_struct(np.nan, 0, 64), native.fog_struct(np.inf, 0, 64), native.fog_struct(0.1, 64, 64),
           native.fog_struct(0.1, 65, 64), native.fog_struct(0.1, -np.inf, 64), native.fog_struct(0.1, 0, np.inf), native.fog_struct(0.1, np.nan, 64),
           native.fog_struct(0.1, 0, 64, (1.01, 0, 0)), native.fog_struct(0.1, 0, 64, (0, -0.01, 0)), native.fog_struct(0.1, 0, 64, (0, 0, np.nan))]
    for f in bad:
        assert native.fog_check(f) == native.E_INVALID
        assert native.lib().chunky_last_error()
    # the size member: smaller than the first version is refused; larger is taken when the bytes this library does not know are zero
    small = native.fog_struct(0.05, 0, 64)
    small.size = C.sizeof(native.Fog) - 4
    assert native.fog_check(small) == native.E_INVALID
    zero = native.fog_struct(0.05, 0, 64)
    zero.size = 0
    assert native.fog_check(zero) == native.E_INVALID

    class Bigger(C.Structure):
        _fields_ = [("fog", native.Fog), ("later", C.c_float * 4)]

    big = Bigger()
    big.fog = native.fog_struct(0.05, 0, 64)
    big.fog.size = C.sizeof(Bigger)
    check = native.lib().chunky_fog_check
    assert check(C.cast(C.pointer(big), C.POINTER(native.Fog))) == 0
    big.later[2] = 1.0
    assert check(C.cast(C.pointer(big), C.POINTER(native.Fog))) == native.E_INVALID
    huge = native.fog_struct(0.05, 0, 64)
    huge.size = 1 << 20
    assert native.fog_check(huge) == native.E_INVALID


def test_plan_fog_names_the_six_kernels_and_refuses_the_rest():
    #        kernel word, projector, max depth, wide, bvh, records, biome, wide levels
    ok = [[0, 0, 5, 1, 0, 1, 0, 2], [0, -1, 5, 1, 0, 1, 0, 3], [0, 0, 254, 1, 0, 1, 0, 1], [0, 0, 5, 1, 0, 1, 0, 4], [0, 0, 5, 1, 0, 1, 0, 5],
          [0, 0, 5, 1, 1, 1, 0, 2], [0, -1, 5, 1, 1, 1, 0, 3], [0, 0, 5, 1, 1, 1, 0, 1], [64, 0, 5, 1, 0, 1, 0, 2], [256, 0, 5, 1, 0, 1, 0, 2]]
    out, text = native.plan_fog(ok)
    want_tree = [17, 18, -1, -1, -1, 17, 18, -1, 17, 17]
    for row, o, t, tree in zip(ok, out, text, want_tree):
        assert (o[0], o[1], t) == (0, 0, ""), (row, o, t)
        assert o[2] == tree and o[3] == (native.FOG_POOL_BVH_PARK if row[4] else native.FOG_POOL_PARK) and o[4] == row[4] and o[5] == 1 and o[6] == 0, (row, o)
        assert tree in native.FOG_POOL_FORMS
    refused = {"biome": ([0, 0, 5, 1, 0, 1, 1, 2], "biome map"), "stats": ([4, 0, 5, 1, 0, 1, 0, 2], "phase-statistics"),
               "rig_bits": ([2, 0, 5, 1, 0, 1, 0, 2], "default kernel"), "projected": ([0, 3, 5, 1, 0, 1, 0, 2], "projected cameras"),
               "max_depth": ([0, 0, 255, 1, 0, 1, 0, 2], "max depth <= 254"), "wide_tree": ([0, 0, 5, 0, 0, 1, 0, 0], "wide re-layout"),
               "bvh_records": ([0, 0, 5, 1, 1, 0, 0, 2], "entity BVHs")}
    out, text = native.plan_fog([r for r, _ in refused.values()])
    for (name, (row, words)), o, t in zip(refused.items(), out, text):
        assert native.FOG_REFUSALS[o[1]] == name, (row, o, t)
        assert t.startswith("fog: ") and words in t, (name, t)
    for word in (1, 8, 1 | 4):   # the other rig bits that pick another walk or kernel
        out, _ = native.plan_fog([[word, 0, 5, 1, 0, 1, 0, 2]])
        assert native.FOG_REFUSALS[out[0][1]] in ("rig_bits", "stats")


def test_host_file_is_plain_cpp_and_in_the_build():
    for src in ("fog_host.cpp", "capi_fog.hip", "render_pool_fog.hip", "render_pool_fog_bvh.hip"):
        assert src in native.SOURCES
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
           os.path.join(native.CSRC, "fog_host.cpp")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    # the header is C99: the specification compiles it as C, the kernels as HIP
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-x", "c", os.path.join(native.CSRC, "fog_spec.h")]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]


def test_fog_host_under_asan_ubsan(tmp_path):
    """chunky_fog_check over structs in heap blocks of exactly their declared size and plan_fog over every combination of its inputs, in a
    stand-alone program (tests/sanitize/fog_host_fuzz.cpp) under AddressSanitizer + UBSan."""
    exe = str(tmp_path / "fog_host_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "fog_host_fuzz.cpp"), os.path.join(native.CSRC, "fog_host.cpp"),
           os.path.join(native.CSRC, "launch_plan.cpp"), os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0 and out["accepted"] > 0 and out["refused"] > out["accepted"] and 0 < out["planned"] < out["plans"], out


# ---- 7. the scene JSON ----
def test_fog_settings_of_the_benchmark_scene():
    js = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "benchmark_OpenCL_test_fog.json")))
    f = octree2.fog_settings(js, 10)
    assert f["density"] == 0.0                                           # the benchmark scene has fogDensity 0: off
    assert (f["y_min"], f["y_max"]) == (0.0, 1024.0)
    assert f["color"] == (js["fogColor"]["red"], js["fogColor"]["green"], js["fogColor"]["blue"])
    g = octree2.fog_settings(dict(js, fogDensity=0.5), 8)
    assert g["density"] == 0.5 * octree2.FOG_EXTINCTION_FACTOR and g["y_max"] == 256.0
    assert native.fog_check(native.fog_struct(g["density"], g["y_min"], g["y_max"], g["color"])) == 0
    assert octree2.fog_settings({}, 6)["density"] == 0.0
