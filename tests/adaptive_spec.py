"""Adaptive sampling restated in numpy float32 from the text of include/chunky_hip.h ("adaptive sampling"), independently of
csrc/adaptive_spec.h: the checker of chunky_adaptive_host, and with it of the device.  Every operation is one float32 operation."""
import numpy as np

f32 = np.float32


def oracle_samples(tracer, sc, seeds):
    """(n, h, w, 3): the sample of every pass — one render_passes call per pass from a zero buffer (bufferSpp 0 returns the sample)."""
    from oracle import binding
    h = binding.SceneHandle(sc)
    return np.stack([tracer.render_passes(h, [int(s)]).reshape(sc.height, sc.width, 3) for s in seeds]).astype(np.float32)


def running_mean(samples, n):
    """The image after the first n passes (K/rayTracer.cl:109-112), (h, w, 3)."""
    mean = np.zeros(samples.shape[1:], f32)
    for k in range(n):
        mean = (mean * f32(k) + samples[k]) / f32(k + 1)
    return mean


def adaptive(samples, threshold, floor, min_spp, check_interval, trace=None):
    """(counts (h, w) int32, image (h, w, 3), stat (h, w, 2)) for per-pass samples (n, h, w, 3); n is max_spp.  `trace`: a list that
    receives the number of active pixels after each check."""
    s = np.ascontiguousarray(samples, f32)
    n, h, w, _ = s.shape
    t2 = f32(threshold) * f32(threshold)
    fl = f32(floor)
    mean = np.zeros((h, w, 3), f32)
    m = np.zeros((h, w), f32)
    M2 = np.zeros((h, w), f32)
    active = np.ones((h, w), bool)
    count = np.zeros((h, w), np.int32)
    done = 0
    with np.errstate(all="ignore"):
        while done < n and active.any():
            c = s[done]
            k = done
            y = (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)
            d = y - m
            m_new = m + d / f32(k + 1)
            M2_new = M2 + d * (y - m_new)
            mean_new = (mean * f32(k) + c) / f32(k + 1)
            m = np.where(active, m_new, m)
            M2 = np.where(active, M2_new, M2)
            mean = np.where(active[..., None], mean_new, mean)
            done += 1
            if done < min_spp or done >= n or (done - min_spp) % check_interval:
                continue
            b = np.where(m > fl, m, fl)
            lim = ((t2 * (f32(done) * f32(done - 1))) * b) * b
            unconv = active & np.isfinite(m) & np.isfinite(M2) & (M2 > lim)
            pad = np.zeros((h + 2, w + 2), bool)
            pad[1:-1, 1:-1] = unconv
            near = np.zeros((h, w), bool)
            for dy in range(3):
                for dx in range(3):
                    near |= pad[dy:dy + h, dx:dx + w]
            leave = active & ~near
            count[leave] = done
            active &= near
            if trace is not None:
                trace.append(int(active.sum()))
    count[active] = done
    return count, mean, np.stack([m, M2], axis=-1)
