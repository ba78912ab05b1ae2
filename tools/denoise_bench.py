#!/usr/bin/env python3
"""The denoiser (chunky_render_denoise, csrc/denoise.hip) on one MI355X, on two of the views bench.py / tools/config_bench.py time:

  outdoor      32x32-chunk world, 1920x1080 (bench.py's headline view)
  entities4k   the outdoor world + 100 000 world / 5 000 actor triangles at 3840x2160

Per view: 8 render and AOV passes, then for each kernel form (gather: the default and the yardstick; packed) and for 5 iterations and 1
iteration one warm-up call and three timed ones; kernel time from the library's HIP events (chunky_render_denoise_kernel_time), median
of the three.  The time per iteration is (t5 - t1) / 4: the pack / demodulation pass and the last iteration's output pass cancel.
Beside them: the render kernel's time for ONE pass of the same view (median of three launches of 8 passes, over 8), so that the
denoise reads as "costs as much as N passes"; chunky_denoise_host on the same input with this box's CPUs; and the unique-bytes floor
of an iteration (gather: 36 bytes read and 12 written per pixel; packed: 48 and 16) at 8 TB/s.  One JSON line per view.

    python tools/denoise_bench.py [names...] > profiles/denoise_bench.jsonl"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chunkyclplugin_amd import native, scenes  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402

VIEWS = ["outdoor", "entities4k"]
FORMS = {"gather": native.DENOISE_KERNEL_GATHER, "packed": native.DENOISE_KERNEL_PACKED}
BYTES_PER_PIXEL = {"gather": 48, "packed": 64}  # unique bytes read + written per pixel per iteration
PASSES, REPEATS = 8, 3


def view(name):
    """The scenes of tests/golden_scenes.py timed_view, built the same way."""
    if name == "outdoor":
        return scenes.cached_outdoor_world(chunks=32, height=256)
    if name == "entities4k":
        sc = scenes.add_entities(scenes.cached_outdoor_world(chunks=32, height=256), 100000, seed=11, actor_tris=5000,
                                 region=((40, 90, 40), (470, 170, 470)))
        return sc.with_view(3840, 2160)
    raise KeyError(name)


def timed(r, params):
    r.denoise(params)  # warm-up
    r.denoise_kernel_time()
    ms = []
    for _ in range(REPEATS):
        out = r.denoise(params)
        ms.append(r.denoise_kernel_time()[0])
    return statistics.median(ms), ms, out


def main():
    inst = RendererInstance.get(0)
    for name in sys.argv[1:] or VIEWS:
        sc = view(name)
        loader = HipSceneLoader(inst)
        loader.load_packed(sc)
        r = HipPathTracingRenderer(loader, sc.width, sc.height)
        r.set_camera(sc.projector_type, sc.camera)
        seeds = native.java_random_ints(PASSES)
        r.render_passes(seeds)  # warm-up
        r.kernel_time()
        render_ms = []
        for k in range(REPEATS):
            r.reset()
            r.render_passes(seeds)
            render_ms.append(r.kernel_time()[0] / PASSES)
        r.render_aov(seeds)
        pass_ms = statistics.median(render_ms)
        n_pixels = sc.width * sc.height
        row = {"view": name, "width": sc.width, "height": sc.height, "device": inst.device_name(), "passes": PASSES,
               "render_ms_per_pass": pass_ms, "render_ms_per_pass_all": render_ms,
               "forms": {}}
        results = {}
        for form, code in FORMS.items():
            t5, all5, out = timed(r, native.denoise_params(iterations=5, kernel=code))
            t1, all1, _ = timed(r, native.denoise_params(iterations=1, kernel=code))
            results[form] = out
            row["forms"][form] = {"ms_5_iterations": t5, "ms_5_iterations_all": all5, "ms_1_iteration": t1, "ms_per_iteration": (t5 - t1) / 4,
                                  "floor_bytes_per_pixel": BYTES_PER_PIXEL[form], "floor_us_per_iteration": n_pixels * BYTES_PER_PIXEL[form] / 8e12 * 1e6,
                                  "render_passes_equivalent": t5 / pass_ms}
        row["forms_bit_identical"] = bool(np.array_equal(results["packed"].view(np.uint32), results["gather"].view(np.uint32)))
        c, a, n = r.read(), r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL)
        host_s = []
        for _ in range(2):
            t = time.perf_counter()
            want = native.denoise_host(sc.width, sc.height, c, a, n)
            host_s.append(time.perf_counter() - t)
        row["host_ms_5_iterations"] = min(host_s) * 1e3
        row["host_threads"] = min(16, os.cpu_count() or 1)
        row["device_equals_host"] = bool(np.array_equal(results["gather"].reshape(-1).view(np.uint32), want.view(np.uint32)))
        print(json.dumps(row), flush=True)
        r.close()
        loader.close()


if __name__ == "__main__":
    main()
