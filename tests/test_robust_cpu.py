"""Firefly-robust accumulation without a device: chunky_robust_host and chunky_robust_host_resolve (the specification as code,
csrc/robust_spec.h) against the numpy restatement (tests/robust_spec.py) on the oracle's per-pass samples and on synthetic streams,
bit for bit; the specification's properties; the parameter and argument errors; and the non-degeneracy of the settings
tests/test_gpu_robust.py uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import robust_spec as rs
from chunkyclplugin_amd import native
from test_adaptive_cpu import MAX_SPP, samples_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUCKETS = (3, 5, 9, 15)
MODES = (native.ROBUST_MEAN, native.ROBUST_MEDIAN, native.ROBUST_GINI)
GAINS = (0.0, 0.5, 1.0, 3.7)
HOST_ONLY = ["robust_host.cpp"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_resolve_equals_restatement(buckets, what):
    """every mode and gain; returns {(mode, gain): (image, trim)} of the host"""
    got = {}
    for mode in MODES:
        for gain in GAINS:
            img, trim = native.robust_host_resolve(buckets, native.robust_params(mode, gain))
            wimg, wtrim = rs.resolve(buckets, mode, gain)
            assert np.array_equal(bits(img), bits(wimg)), (what, mode, gain, int((bits(img) != bits(wimg)).sum()))
            assert np.array_equal(trim, wtrim), (what, mode, gain)
            got[(mode, gain)] = (img, trim)
    return got


def assert_fold_equals_restatement(s, M, first, what):
    b = native.robust_host(s, M, first)
    assert np.array_equal(bits(b), bits(rs.fold(s, M, first))), (what, M, first)
    return b


@pytest.mark.parametrize("name", ["indoor", "outdoor", "entities", "inside"])
def test_host_equals_the_restatement_on_oracle_samples(port, name):
    s = samples_of(name, port)
    assert s.shape == (MAX_SPP, 48, 64, 3)
    for M in BUCKETS:
        for first in (0, 7):
            b = assert_fold_equals_restatement(s, M, first, name)
            assert_resolve_equals_restatement(b, (name, M, first))
        # a fold continued at sample 7 is the fold of all the samples
        head = native.robust_host(s[:7], M, 0)
        assert np.array_equal(bits(native.robust_host(s[7:], M, 7, head)), bits(native.robust_host(s, M, 0)))


@pytest.mark.parametrize("stream", sorted(rs.synthetic_streams()))
def test_host_equals_the_restatement_on_synthetic_streams(stream):
    s = rs.synthetic_streams()[stream]
    for M in native.ROBUST_BUCKETS:
        for first in (0, 7):
            b = assert_fold_equals_restatement(s, M, first, stream)
            assert_resolve_equals_restatement(b, (stream, M, first))


def test_the_streams_hold_what_they_are_named_for():
    st = rs.synthetic_streams()
    assert np.isnan(st["nan"]).any() and np.isposinf(st["inf"]).any() and np.isneginf(st["inf"]).any()
    assert (st["zeros"][:, 0] == 0).all() and np.signbit(st["zeros"]).any() and (st["huge"] >= 1e30).any()
    tiny = np.abs(st["denormal"])
    assert ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).any()
    b = native.robust_host(st["nan"], 5)
    assert np.isnan(b).any() and np.isnan(native.robust_host_resolve(b)[0]).any()  # a NaN is not hidden: it reaches the image
    z = native.robust_host(st["zeros"], 9)
    img, trim = native.robust_host_resolve(z)
    assert (img[0] == 0).all() and (trim[0] == 0).all()  # S = 0: no trim, the value 0
    big = native.robust_host(st["huge"], 3)
    assert np.isinf(big.sum(axis=0, dtype=np.float32)).any()  # S = inf is reached


def test_equal_buckets_give_that_value_untrimmed():
    """t = 0 whatever the value (W = 0 exactly or to rounding, and p stays under 1).  The value itself comes back exactly where the
    sum of M copies is exact — values of few significant bits: up to 15 copies need 4 more — and otherwise within the rounding of
    M - 1 additions and one division, each at most 2^-24 relative: (M + 1) 2^-24 with room for the second-order terms."""
    for M in native.ROBUST_BUCKETS:
        for v in (0.25, 0.375, 7.0, 1536.0, 2.0 ** 100, 2.0 ** -100):
            b = np.full((M, 4, 3), v, np.float32)
            img, trim = native.robust_host_resolve(b, native.robust_params(native.ROBUST_GINI, 3.7))
            assert (trim == 0).all() and np.array_equal(bits(img), bits(np.full((4, 3), v, np.float32))), (M, v)
        for v in (1e-3, 0.1, 1e30, 123.456):
            b = np.full((M, 4, 3), v, np.float32)
            img, trim = native.robust_host_resolve(b, native.robust_params(native.ROBUST_GINI, 1.0))
            v32 = float(np.float32(v))
            assert (trim == 0).all() and (np.abs(img.astype(np.float64) - v32) <= (M + 1) * 2.0 ** -24 * v32).all(), (M, v)


def test_one_firefly_in_ninety_samples_is_trimmed_away():
    s = np.full((90, 1, 1, 3), 0.5, np.float32)
    s[41] = 1e4
    assert s.mean(axis=0, dtype=np.float64).min() > 100
    b = native.robust_host(s, 9)
    assert native.robust_host_resolve(b, native.robust_params(native.ROBUST_MEAN))[0].min() > 100  # the plain mean of the buckets keeps it
    img, trim = native.robust_host_resolve(b, native.robust_params(native.ROBUST_GINI, 1.0))
    assert np.array_equal(bits(img), bits(np.full((1, 1, 3), 0.5, np.float32))) and trim.min() >= 1
    assert np.array_equal(bits(native.robust_host_resolve(b, native.robust_params(native.ROBUST_MEDIAN))[0]), bits(img))


def test_the_resolve_does_not_depend_on_the_bucket_order():
    rng = np.random.default_rng(5)
    for M in native.ROBUST_BUCKETS:
        b = np.abs(rng.normal(0.5, 0.5, size=(M, 64, 3))).astype(np.float32)
        b[:, :8] = np.round(b[:, :8] * 4) / 4  # ties among them
        want = assert_resolve_equals_restatement(b, M)
        for _ in range(3):
            shuffled = b[rng.permutation(M)]
            for (mode, gain), (img, trim) in want.items():
                got, gtrim = native.robust_host_resolve(shuffled, native.robust_params(mode, gain))
                assert np.array_equal(bits(got), bits(img)) and np.array_equal(gtrim, trim), (M, mode, gain)


def test_mean_of_whole_rounds_of_a_constant_is_the_constant():
    """(constants of few significant bits: every product v * k, every sum and every quotient on the way is then exact)"""
    for M in native.ROBUST_BUCKETS:
        for q in (1, 2, 7):
            for v in (0.25, 0.375, 96.0):
                s = np.full((M * q, 2, 2, 3), v, np.float32)
                img, trim = native.robust_host_resolve(native.robust_host(s, M), native.robust_params(native.ROBUST_MEAN))
                assert (trim == 0).all() and np.array_equal(bits(img), bits(np.full((2, 2, 3), v, np.float32))), (M, q, v)


def test_trim_bounds_and_modes():
    rng = np.random.default_rng(6)
    for M in native.ROBUST_BUCKETS:
        h = (M - 1) // 2
        b = np.abs(rng.normal(0.2, 1.0, size=(M, 256, 3))).astype(np.float32) ** 3
        assert (native.robust_host_resolve(b, native.robust_params(native.ROBUST_MEAN, 2.0))[1] == 0).all()
        img, trim = native.robust_host_resolve(b, native.robust_params(native.ROBUST_MEDIAN, 2.0))
        assert (trim == h).all() and np.array_equal(bits(img), bits(np.sort(b, axis=0)[h]))
        assert (native.robust_host_resolve(b, native.robust_params(native.ROBUST_GINI, 0.0))[1] == 0).all()
        trims = [native.robust_host_resolve(b, native.robust_params(native.ROBUST_GINI, g))[1] for g in (0.5, 1.0, 3.7, 1e30)]
        assert all((a <= c).all() for a, c in zip(trims, trims[1:])) and trims[-1].max() == h and all(t.max() <= h for t in trims)


def test_parameter_and_argument_errors():
    L = native.lib()
    s = np.zeros((6, 2, 2, 3), np.float32)
    b = np.zeros((3, 2, 2, 3), np.float32)
    out, trim = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2), np.uint8)
    ok = native.robust_params()
    assert ok.size == C.sizeof(native.RobustParams) == 12 and ok.mode == native.ROBUST_GINI and ok.gain == 1.0
    assert L.chunky_robust_default_params(None) == native.E_INVALID

    def fold(w=2, h=2, samples=s, n=6, M=3, first=0, buckets=b):
        return L.chunky_robust_host(w, h, native.ptr(samples) if samples is not None else None, n, M, first, native.ptr(buckets) if buckets is not None else None)

    assert fold() == 0 and fold(n=0, samples=None) == 0
    for bad in (dict(M=0), dict(M=1), dict(M=4), dict(M=8), dict(M=17), dict(M=-3), dict(w=0), dict(h=-1), dict(n=-1), dict(first=-1),
                dict(first=2 ** 31 - 3), dict(samples=None), dict(buckets=None)):
        assert fold(**bad) == native.E_INVALID, bad

    def resolve(M=3, n=4, buckets=b, p=ok, o=out, t=trim):
        return L.chunky_robust_host_resolve(M, n, native.ptr(buckets) if buckets is not None else None, C.byref(p) if p is not None else None,
                                            native.ptr(o) if o is not None else None, native.ptr(t) if t is not None else None)

    assert resolve() == 0 and resolve(t=None) == 0
    for bad in (dict(M=2), dict(M=17), dict(n=0), dict(n=-4), dict(buckets=None), dict(o=None), dict(p=None)):
        assert resolve(**bad) == native.E_INVALID, bad
    for mode, gain in ((3, 1.0), (-1, 1.0), (native.ROBUST_GINI, -0.5), (native.ROBUST_GINI, float("nan")), (native.ROBUST_GINI, float("inf")),
                       (native.ROBUST_MEAN, -1.0)):
        assert resolve(p=native.robust_params(mode, gain)) == native.E_INVALID, (mode, gain)
    short = native.robust_params()
    short.size = 8  # cuts the first version short
    assert resolve(p=short) == native.E_INVALID
    longer = native.robust_params()
    longer.size = 64  # a newer caller: the members known here are read
    assert resolve(p=longer) == 0


def test_host_file_is_plain_cpp_and_in_the_build():
    for src in HOST_ONLY + ["robust.hip", "capi_robust.hip"]:
        assert src in native.SOURCES
    for src in HOST_ONLY:
        cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
               os.path.join(native.CSRC, src)]
        assert not any("rocm" in a.lower() for a in cmd)
        proc = subprocess.run(cmd, capture_output=True, text=True)
        assert proc.returncode == 0, (src, proc.stderr[-3000:])
    text = open(os.path.join(native.CSRC, "robust_spec.h")).read() + open(os.path.join(ROOT, "PAPERS.md")).read()
    assert text.count("own specification") >= 2  # the header and PAPERS.md say whose formulas these are


# scene -> (M, the least share of the pixels in each trim class: t = 0, 0 < t < h, t = h; None = not required)
NON_DEGENERATE = {"indoor": (5, (0.10, 0.10, 0.10)), "entities": (9, (0.10, 0.10, None)), "outdoor": (15, (0.10, 0.10, None))}


def trim_shares(trim, M):
    h = (M - 1) // 2
    return float((trim == 0).mean()), float(((trim > 0) & (trim < h)).mean()), float((trim == h).mean())


@pytest.mark.parametrize("name", sorted(NON_DEGENERATE))
def test_gpu_settings_are_not_degenerate(port, name):
    """At 40 passes, gain 1, first index 0, the golden scenes tests/test_gpu_robust.py resolves put at least 10 % of their pixels
    into each trim class required of them, and `indoor` reaches the S = 0 branch with pixels that are zero in every bucket."""
    M, least = NON_DEGENERATE[name]
    b = native.robust_host(samples_of(name, port), M)
    _, trim = native.robust_host_resolve(b)
    shares = trim_shares(trim, M)
    print(name, M, [round(100 * x, 1) for x in shares])
    for share, need in zip(shares, least):
        assert need is None or share >= need, (name, M, shares)
    if name == "indoor":
        assert (b == 0).all(axis=(0, 3)).sum() >= 1
