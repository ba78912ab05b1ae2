"""The short forms of `1.0f / x`, `sqrtf(x)` and `x / constant` (csrc/rt_short_forms.h) against the operations they stand for, for every
float there is.  The kernels use the reciprocal (rcp_exact, rcp3); the root and the division by a constant are held exact here all the
same (EXPERIMENTS 7.3 has why the kernels do not use them).

  sweeps     math_selftest_kernel's sweep numbers evaluate a short form and the compiled IEEE operation side by side on the device and
             compare the bits, NaNs included; one launch covers all 2^32 patterns (2^20 threads, 4096 patterns each).  0 mismatches is
             the only result a form may ship with.  -(1 / x) is no form of its own (a negation of rcp_exact's result, exact), and rcp3
             is rcp_exact's core with a merged test: its pointwise number is checked below.
  host tie   the compiled operation is itself no axiom: on 2^16 patterns — the edges of every range the forms test, the extremes of
             mantissa and exponent, zeros, infinities, NaNs, and random patterns — the device's compiled operations AND the short forms
             (pointwise numbers 20-28) are compared bit for bit with numpy float32 `1 / x`, `sqrt(x)` and `x / c` (IEEE on the host)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_THREADS = 1 << 20
TWO_PI = np.float32(3.14159274101257) * np.float32(2)        # RT_PI_F * 2, as sky_fetch spells it
DISC_WIDTH = np.float32(0.03) * np.float32(4) * np.float32(2)  # width2 of the sun disc
SWEEPS = {40: "rcp_exact(x) against 1.0f / x", 41: "rt_sqrt_short(x) against __builtin_sqrtf(x)",
          42: "x / (2 pi), short against compiled", 43: "x / 0.24 (the sun disc's width2), short against compiled"}


def sweep(gpu_instance, which, first=0, count=(1 << 32) // N_THREADS):
    a = np.zeros(N_THREADS, np.uint32)
    b = np.zeros(N_THREADS, np.uint32)
    a[0], b[0] = first, count
    out = gpu_instance.selftest_math(which, a.view(np.float32), b.view(np.float32)).view(np.uint32)
    return int(out[0]), [f"0x{int(u):08x}" for u in out[2:2 + min(int(out[1]), 60)]]


@pytest.mark.parametrize("which", sorted(SWEEPS))
def test_sweep_of_all_patterns(gpu_instance, which):
    bad, first = sweep(gpu_instance, which)
    print(f"sweep {which} ({SWEEPS[which]}): {bad} mismatches of 2^32 {first}")
    assert bad == 0, f"{SWEEPS[which]}: {bad} of 2^32 patterns differ; some of them: {first}"


def test_sweep_counts_what_it_is_given(gpu_instance):
    """the sweep's plumbing: a run that is not the whole space (first pattern, count), and a form that must fail — the bare hardware
    estimate (50), which is within 1 ulp of 1.0f / x and not equal to it: a sweep that finds nothing there finds nothing anywhere"""
    assert sweep(gpu_instance, 40, first=0x3F800000, count=4) == (0, [])
    bad, first = sweep(gpu_instance, 50)
    print(f"the bare estimate: {bad} mismatches, e.g. {first[:8]}")
    assert bad > 1 << 20 and len(first) == 60
    # every recorded pattern is in the fast range (outside it the form IS the compiled division)
    x = np.array([int(f, 16) for f in first], np.uint32).view(np.float32)
    assert ((np.abs(x) >= np.float32(2.0 ** -126)) & (np.abs(x) < np.float32(2.0 ** 126))).all()
    bad, first = sweep(gpu_instance, 50, first=0x7F800000, count=1)   # 2^20 patterns from +inf on: NaNs, all on the slow path
    assert (bad, first) == (0, [])


def patterns():
    """2^16 bit patterns"""
    u = []
    for sign in (0, 0x80000000):
        u += [sign | v for v in (0, 1, 2, 0x007FFFFF, 0x007FFFFE, 0x00400000)]                 # zeros, denormals
        for e in (1, 2, 26, 27, 28, 30, 31, 32, 126, 127, 128, 226, 227, 228, 252, 253, 254):  # 2^(e-127) and its neighbours
            base = e << 23
            u += [sign | (base + d) & 0xFFFFFFFF for d in (-2, -1, 0, 1, 2)]
        for e in range(1, 255, 3):                                                             # mantissas of all zeros / all ones
            u += [sign | (e << 23), sign | (e << 23) | 0x7FFFFF, sign | (e << 23) | 0x7FFFFE, sign | (e << 23) | 0x400000]
        u += [sign | 0x7F800000, sign | 0x7FC00000, sign | 0x7FC12345, sign | 0x7F800001, sign | 0x7FA00000, sign | 0x7FFFFFFF]
    u = np.array(u, np.uint32)
    rng = np.random.default_rng(7301)
    rest = rng.integers(0, 1 << 32, (1 << 16) - len(u), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([u, rest])


def same_bits(dev, host, x, what):
    """bit for bit, NaN results included — payload and quieting too.  One bit is left out, in one case: the sign of a NaN that the
    operation MAKES from an operand that is no NaN (sqrt of a negative number): x86 makes 0xFFC00000 there and the device 0x7FC00000,
    before this change as after it.  A NaN operand's own sign is compared."""
    d, h = dev.view(np.uint32), host.view(np.uint32)
    made_nan = np.isnan(dev) & np.isnan(host) & ~np.isnan(x)
    mask = np.where(made_nan, np.uint32(0x7FFFFFFF), np.uint32(0xFFFFFFFF))
    bad = (d & mask) != (h & mask)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(x)} differ; first x = 0x{int(x.view(np.uint32)[np.argmax(bad)]):08x}: device 0x{int(d[np.argmax(bad)]):08x} host 0x{int(h[np.argmax(bad)]):08x}"


def test_host_tie(gpu_instance):
    x = patterns().view(np.float32)
    assert x.size == 1 << 16
    with np.errstate(all="ignore"):
        want = {"1 / x": np.float32(1) / x, "sqrt(x)": np.sqrt(x), "x / 2pi": x / TWO_PI, "x / width2": x / DISC_WIDTH}
    for (short, compiled), key in (((20, 21), "1 / x"), ((22, 23), "sqrt(x)"), ((24, 25), "x / 2pi"), ((26, 27), "x / width2")):
        same_bits(gpu_instance.selftest_math(compiled, x, x), want[key], x, f"compiled {key} against numpy")
        same_bits(gpu_instance.selftest_math(short, x, x), want[key], x, f"short form of {key} against numpy")
    # rcp3: even rows 1 / a, odd rows 1 / b, the three components tested together (a wave holds every mixture of lanes here)
    y = np.roll(x, 12345)
    with np.errstate(all="ignore"):
        want3 = np.where(np.arange(x.size) & 1, np.float32(1) / y, np.float32(1) / x).astype(np.float32)
    same_bits(gpu_instance.selftest_math(28, x, y), want3, x, "rcp3 against numpy")
