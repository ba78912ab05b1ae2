"""Firefly-robust accumulation restated in numpy float32 from the text of include/chunky_hip.h ("firefly-robust accumulation"),
independently of csrc/robust_spec.h: the checker of chunky_robust_host and chunky_robust_host_resolve, and with them of the device.
Every operation is one float32 operation; the sort is the header's network, compare by compare, because that is what decides where a
NaN ends up."""
import numpy as np

f32 = np.float32
MEAN, MEDIAN, GINI = 0, 1, 2


def fold(samples, n_buckets, first_index=0, buckets=None):
    """(M, ..., 3) bucket means after the samples (n, ..., 3) taken as robust samples first_index .., from `buckets` (default zero)."""
    s = np.ascontiguousarray(samples, f32)
    M = int(n_buckets)
    b = np.zeros((M,) + s.shape[1:], f32) if buckets is None else np.array(buckets, f32)
    with np.errstate(all="ignore"):
        for k in range(s.shape[0]):
            j = first_index + k
            q = j // M
            b[j % M] = (b[j % M] * f32(q) + s[k]) / f32(q + 1)
    return b


def sort_network(x):
    """x: (M, ...) -> sorted copy by the odd-even transposition network; a pair swaps iff x[i + 1] < x[i]."""
    x = [np.array(v, f32) for v in x]
    M = len(x)
    with np.errstate(invalid="ignore"):
        for r in range(M):
            for i in range(r & 1, M - 1, 2):
                swap = x[i + 1] < x[i]
                x[i], x[i + 1] = np.where(swap, x[i + 1], x[i]), np.where(swap, x[i], x[i + 1])
    return x


def resolve(buckets, mode=GINI, gain=1.0):
    """(image (..., 3) float32, trim (...) uint8) of bucket means (M, ..., 3)."""
    b = np.ascontiguousarray(buckets, f32)
    M = b.shape[0]
    h = (M - 1) // 2
    g = f32(gain)
    with np.errstate(all="ignore"):
        x = sort_network(list(b))
        S = x[0].copy()
        W = f32(1 - M) * x[0]
        for i in range(1, M):
            S = S + x[i]
            W = W + f32(2 * i - M + 1) * x[i]
        ok = (S > 0) & (S < np.inf)
        G = np.where(ok, W / (f32(M) * S), f32(0)).astype(f32)
        if mode == MEAN:
            t = np.zeros(S.shape, np.int32)
        elif mode == MEDIAN:
            t = np.full(S.shape, h, np.int32)
        else:
            p = ((G * f32(h + 1)).astype(f32) * g).astype(f32)
            inside = (p > 0) & ~(p >= f32(h))
            t = np.where(~(p > 0), 0, np.where(p >= f32(h), h, np.where(inside, p, 0).astype(np.int32))).astype(np.int32)
        out = np.zeros(S.shape, f32)
        for tv in range(h + 1):
            acc = x[tv].copy()
            for i in range(tv + 1, M - tv):
                acc = acc + x[i]
            out = np.where(t == tv, acc / f32(M - 2 * tv), out)
    return out.astype(f32), t.max(axis=-1).astype(np.uint8)


def synthetic_streams():
    """Named per-pass sample streams (n, h, w, 3) float32 that hold the values a renderer can produce at its worst: NaN, +-inf, -0,
    ties, all-zero pixels (S = 0), 1e30 and denormals, each among ordinary values.  n = 47: not a multiple of any bucket count."""
    rng = np.random.default_rng(20)
    n, h, w = 47, 5, 7
    base = np.abs(rng.normal(0.5, 0.3, size=(n, h, w, 3))).astype(f32)
    out = {}
    s = base.copy()
    s[3, 1, 1, 0] = np.nan
    s[10, 2, 3, :] = np.nan
    s[[4, 5, 6], 4, 6, 1] = np.nan
    out["nan"] = s
    s = base.copy()
    s[2, 0, 0, 0] = np.inf
    s[7, 1, 2, 1] = -np.inf
    s[9, 3, 3, 2] = np.inf
    s[12, 3, 3, 2] = -np.inf  # inf and -inf in different buckets of one pixel
    s[5, 4, 0, :] = np.inf
    s[5 + 15, 4, 0, :] = -np.inf
    out["inf"] = s
    s = base.copy()
    s[:, 0, :, :] = 0.0
    s[::2, 0, 1, :] = -0.0
    s[:, 1, 0, :] = -0.0
    s[:, 2, 2, 1] = -base[:, 2, 2, 1]  # a negative channel: S < 0
    out["zeros"] = s
    s = base.copy()
    s[:, 1, :, :] = f32(0.25)  # every bucket equal
    s[:, 2, :, :] = np.where((np.arange(n) % 2 == 0)[:, None, None], f32(0.5), f32(1.0))  # two values only
    s[:, 3, 3, :] = np.round(base[:, 3, 3, :] * 4) / 4  # a few values, many ties
    out["ties"] = s
    s = base.copy()
    s[11, 1, 1, :] = f32(1e30)
    s[13, 2, 2, 0] = f32(1e30)
    s[14, 2, 2, 0] = f32(3e38)
    s[:, 3, 1, :] = f32(3e38)  # S overflows to inf
    out["huge"] = s
    s = base.copy()
    s[:, 0, 0, :] = f32(1e-45)
    s[:, 1, 1, :] = (base[:, 1, 1, :] * f32(1e-40)).astype(f32)
    s[::3, 2, 2, :] = f32(1e-41)
    out["denormal"] = s
    s = np.full((n, h, w, 3), 0.5, f32)  # one firefly in a constant pixel
    s[17, 2, 2, :] = f32(1e4)
    out["firefly"] = s
    return out
