"""Adaptive sampling without a device: chunky_adaptive_host (the specification as code, csrc/adaptive_spec.h) against its numpy
restatement (tests/adaptive_spec.py) on the oracle's per-pass samples, bit for bit; the specification's properties on synthetic
streams; the parameter errors; and the non-degeneracy of the settings tests/test_gpu_adaptive.py uses."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import binding

import adaptive_spec as sp
import golden_scenes as gs
from chunkyclplugin_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SPP = 40
# (min_spp, check_interval, threshold): what tests/test_gpu_adaptive.py runs on the golden scenes, chosen on the CPU oracle
# (profiles/adaptive_spec_check.json).  One threshold does not fit an open landscape and a closed room, so every scene names the
# setting that carries the non-degeneracy condition for it (CARRIES); under the other two a scene may be an edge case — nearly
# everything leaves at the first checks, or nearly nothing leaves — which the parity tests still run and the record lists as such.
SETTINGS = [(8, 4, 0.2), (4, 12, 0.5), (6, 5, 0.75)]
CARRIES = {"outdoor": 0, "outdoor_nosun": 0, "entities": 0, "dof": 0, "pregen": 0, "atlas_layers": 0, "water": 0,
           "inside": 1, "indoor_sun": 1, "indoor": 2}
FLOOR = 0.01


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(mn, ci, thr, floor=FLOOR):
    return native.adaptive_params(threshold=thr, floor=floor, min_spp=mn, check_interval=ci)


_samples = {}


def samples_of(name, tracer=None):
    if name not in _samples:
        _samples[name] = sp.oracle_samples(tracer or binding.port(), gs.make(name), native.java_random_ints(MAX_SPP))
    return _samples[name]


def assert_host_equals_restatement(s, mn, ci, thr, floor=FLOOR):
    c, img, st = native.adaptive_host(s, params(mn, ci, thr, floor))
    wc, wimg, wst = sp.adaptive(s, thr, floor, mn, ci)
    assert np.array_equal(c, wc)
    assert np.array_equal(bits(img), bits(wimg))
    assert np.array_equal(bits(st), bits(wst))
    return c, img, st


@pytest.mark.parametrize("name", gs.NAMES)
def test_host_equals_the_restatement_on_oracle_samples(port, name):
    s = samples_of(name, port)
    for mn, ci, thr in SETTINGS + [(8, 4, 0.0)]:
        c, img, _ = assert_host_equals_restatement(s, mn, ci, thr)
        for n in np.unique(c):  # the image is the running mean after each pixel's own count
            assert np.array_equal(bits(img)[c == n], bits(sp.running_mean(s, int(n)))[c == n])


@pytest.mark.parametrize("name", ["outdoor", "indoor", "entities"])
def test_port_samples_equal_the_reference_build(port, ref, name):
    sc = gs.make(name)
    seeds = native.java_random_ints(6)
    assert np.array_equal(bits(sp.oracle_samples(port, sc, seeds)), bits(sp.oracle_samples(ref, sc, seeds)))


def non_degenerate(s, mn, ci, thr):
    trace = []
    c, _, _ = sp.adaptive(s, thr, FLOOR, mn, ci, trace)
    early = float((c < s.shape[0]).mean())
    last = trace[-1] / c.size
    return {"early": round(early, 4), "active_at_last_check": round(last, 4), "distinct_counts": int(len(np.unique(c)))}


def is_ok(d):
    return d["early"] >= 0.10 and d["active_at_last_check"] >= 0.10 and d["distinct_counts"] >= 3


def test_gpu_settings_are_not_degenerate(port):
    """For every golden scene under the setting that carries the condition for it (CARRIES): >= 10 % of the pixels leave before
    max_spp, >= 10 % are still active at the last check, and the counts take at least three values.  The record in profiles/ holds
    every (scene, setting) pair with its role and says what this run finds."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "adaptive_spec_check.json")))
    assert rec["max_spp"] == MAX_SPP and [tuple(x) for x in rec["settings"]] == SETTINGS and rec["carries"] == CARRIES
    assert sorted(CARRIES) == sorted(gs.NAMES) and set(CARRIES.values()) == {0, 1, 2}  # every setting carries it somewhere
    for name in gs.NAMES:
        s = samples_of(name, port)
        rows = [dict(non_degenerate(s, *st), role="condition" if k == CARRIES[name] else "edge case") for k, st in enumerate(SETTINGS)]
        assert rows == rec["scenes"][name], (name, rows)
        assert is_ok(rows[CARRIES[name]]), (name, rows)


def stream(n, h, w, rng, base=0.5, noise=0.0):
    s = np.full((n, h, w, 3), base, np.float32)
    if noise:
        s += rng.normal(0, noise, size=s.shape).astype(np.float32)
    return s


def test_threshold_zero_renders_every_pass():
    rng = np.random.default_rng(1)
    s = np.abs(stream(24, 9, 11, rng, 0.5, 0.2))
    c, _, _ = assert_host_equals_restatement(s, 4, 3, 0.0)
    assert (c == 24).all()
    c, _, _ = assert_host_equals_restatement(samples_of("outdoor")[:, :16, :16], 8, 4, 0.0)
    m2 = native.adaptive_host(samples_of("outdoor")[:, :16, :16], params(8, 4, 0.0))[2][..., 1]
    assert (c[m2 > 0] == MAX_SPP).all()


def test_constant_stream_leaves_at_min_spp():
    s = stream(20, 6, 7, None, 0.25)
    for thr in (0.0, 0.1):
        c, img, st = assert_host_equals_restatement(s, 5, 4, thr)
        assert (c == 5).all() and (st[..., 1] == 0).all()
        assert np.array_equal(bits(img), bits(sp.running_mean(s, 5)))


def test_counts_take_only_check_points_or_max_spp():
    s = samples_of("outdoor")
    for mn, ci, thr in SETTINGS:
        c, _, _ = native.adaptive_host(s, params(mn, ci, thr))
        allowed = set(range(mn, MAX_SPP, ci)) | {MAX_SPP}
        assert set(np.unique(c).tolist()) <= allowed


def test_appending_passes_leaves_inactive_pixels_alone():
    s = samples_of("outdoor")
    mn, ci, thr = SETTINGS[0]
    c0, i0, st0 = native.adaptive_host(s[:24], params(mn, ci, thr))
    c1, i1, st1 = native.adaptive_host(s, params(mn, ci, thr))
    gone = c0 < 24  # inactive before the shorter run's last pass
    assert gone.any() and np.array_equal(c0[gone], c1[gone])
    assert np.array_equal(bits(i0)[gone], bits(i1)[gone]) and np.array_equal(bits(st0)[gone], bits(st1)[gone])


def test_neighbour_of_an_unconverged_pixel_stays_active():
    rng = np.random.default_rng(3)
    s = stream(16, 9, 9, None, 0.5)
    s[:, 4, 4] = np.abs(rng.normal(0.5, 0.5, size=(16, 3))).astype(np.float32)  # one noisy pixel in a constant image
    c, _, _ = assert_host_equals_restatement(s, 4, 4, 0.01)
    assert (c[3:6, 3:6] == 16).all()  # its 3 x 3 neighbourhood stays with it to the end
    rest = np.ones((9, 9), bool)
    rest[3:6, 3:6] = False
    assert (c[rest] == 4).all()
    s[:, 0, 0] = s[:, 4, 4]  # and at a corner the neighbourhood is clipped to the image
    c, _, _ = assert_host_equals_restatement(s, 4, 4, 0.01)
    assert (c[:2, :2] == 16).all() and c[2, 2] == 4 and c[0, 2] == 4


def test_non_finite_samples_count_as_converged():
    rng = np.random.default_rng(4)
    s = np.abs(stream(12, 5, 5, rng, 0.5, 0.3))
    s[2, 1, 1, 0] = np.nan
    s[1, 3, 3, 2] = np.inf
    c, _, st = assert_host_equals_restatement(s, 4, 4, 0.0)
    assert not np.isfinite(st[1, 1]).all() and not np.isfinite(st[3, 3]).all()
    assert (c == 12).all()  # their finite neighbours are unconverged at threshold 0 and keep them active
    alone = stream(12, 5, 5, None, 0.5)
    alone[2, 2, 2, 1] = np.nan
    c, _, _ = assert_host_equals_restatement(alone, 4, 4, 0.0)
    assert (c == 4).all()  # a bad pixel among converged ones does not hold the frame


def test_parameter_errors():
    L = native.lib()
    s = np.zeros((8, 2, 2, 3), np.float32)
    out = np.zeros(4, np.int32)

    def rc(p, n=8):
        return L.chunky_adaptive_host(2, 2, native.ptr(s), n, C.byref(p), native.ptr(out), None, None)

    assert rc(params(4, 2, 0.1)) == 0
    small = params(4, 2, 0.1)
    small.size = native.AdaptiveParams.flags.offset  # cuts the first version short
    assert rc(small) == native.E_INVALID
    for bad in (dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(floor=0.0), dict(floor=float("inf")),
                dict(floor=float("nan")), dict(min_spp=1), dict(check_interval=0)):
        assert rc(native.adaptive_params(**{**dict(min_spp=4, check_interval=2), **bad})) == native.E_INVALID, bad
    flagged = params(4, 2, 0.1)
    flagged.flags = 1
    assert rc(flagged) == native.E_INVALID
    assert rc(params(9, 2, 0.1)) == native.E_INVALID  # max_spp < min_spp
    assert L.chunky_adaptive_default_params(None) == native.E_INVALID
    d = native.adaptive_params()
    assert d.size == C.sizeof(native.AdaptiveParams) and d.min_spp >= 2 and d.check_interval >= 1 and d.threshold >= 0 and d.floor > 0
