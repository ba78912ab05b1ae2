#!/usr/bin/env python3
"""What the denoiser's tests rest on, measured on the CPU oracle (no device): writes profiles/denoise_tolerance.json — for each test
input, the largest difference between the float32 and the float64 numpy restatement (tests/denoise_spec.py), the bound asserted
(4 x that) and the largest difference of chunky_denoise_host from the float64 restatement — and profiles/denoise_quality.json — for
the outdoor and indoor golden scenes at 128 x 96, the RMSE against a 512-pass render of the 8-pass render and of its denoised
image with the default parameters (the ratio the defaults were chosen by), and the noise of the 512-pass image itself, estimated
from its two independent halves."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_spec as ds  # noqa: E402
from chunkyclplugin_amd import native  # noqa: E402


def host(c, a, n, **kw):
    h, w, _ = c.shape
    return native.denoise_host(w, h, c, a, n, native.denoise_params(**kw)).reshape(h, w, 3)


def main():
    p = native.denoise_params()
    spec = dict(iterations=p.iterations, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo)
    rows = []
    inputs = [(f"synthetic seed {s}", ds.synthetic(96, 64, s)) for s in (1, 2, 3)] + [(f"oracle {n}", ds.oracle_inputs(n)[:3]) for n in ("outdoor", "indoor", "entities")]
    for what, (c, a, n) in inputs:
        for demodulate in (True, False):
            kw = dict(spec, demodulate=demodulate)
            measured, bound, want = ds.tolerance(c, a, n, **kw)
            rows.append({"input": what, "demodulate": demodulate, "float32_vs_float64_restatement": measured, "asserted_bound": bound,
                         "host_vs_float64_restatement": float(np.abs(host(c, a, n, **kw) - want).max())})
    json.dump({"parameters": spec, "rows": rows}, open(os.path.join(ROOT, "profiles", "denoise_tolerance.json"), "w"), indent=1)
    from oracle import binding
    import golden_scenes as gs
    few, many = ds.QUALITY_PASSES
    w, h = ds.QUALITY_SIZE
    out = []
    for name in ("outdoor", "indoor"):
        c, a, n, ref = ds.oracle_inputs(name, reference_passes=many)
        den = host(c, a, n)
        sc = binding.SceneHandle(gs.make(name).with_view(w, h))
        seeds = native.java_random_ints(many)
        halves = [binding.port().render_passes(sc, seeds[k * many // 2:(k + 1) * many // 2]).reshape(h, w, 3) for k in range(2)]
        before, after = ds.rmse(c, ref), ds.rmse(den, ref)
        out.append({"scene": name, "size": [w, h], "passes": few, "reference_passes": many, "rmse_noisy": before, "rmse_denoised": after, "ratio": after / before,
                    "reference_noise_estimate": 0.5 * ds.rmse(halves[0], halves[1])})
    json.dump({"parameters": dict(spec, demodulate=True), "scenes": out}, open(os.path.join(ROOT, "profiles", "denoise_quality.json"), "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
