#!/usr/bin/env python3
"""ID-matte passes (chunky_render_matte_passes) against AOV passes (chunky_render_aov_passes) on the same target,
one MI355X (GPU box), on three of the views tools/aov_bench.py times:

  outdoor      32x32-chunk world, 1920x1080 (bench.py's headline view)
  city         the reference's benchmark/OpenCL_test scene, 1920x1080
  entities     the outdoor world + 100 000 world / 5 000 actor triangles, 1920x1080

For N = 16 and 256 passes per call: one warm-up call of each kind, then three alternating repeats (AOV, matte); kernel time from the
library's HIP-event accessors (chunky_render_aov_kernel_time / chunky_render_matte_kernel_time).  One JSON line per view and N: the
Msamples/s of each kernel (median of the repeats, and all three), matte / AOV, the spread of the repeats, both instantiations, and the
wall time of one chunky_render_matte_ranks and one chunky_render_matte_extract call (device work plus the copy to the host).

    python tools/matte_bench.py [names...] > profiles/matte_bench.jsonl"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aov_bench import view  # noqa: E402
from chunkyclplugin_amd import native  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402

VIEWS = ["outdoor", "city", "entities"]
PASSES = (16, 256)
REPEATS = 3


def spread(xs):
    """(max - min) / median of the repeats"""
    return float((max(xs) - min(xs)) / np.median(xs))


def bench(name, sc, r, n):
    seeds = native.java_random_ints(n)
    samples = sc.width * sc.height * n
    r.reset_matte()
    r.render_aov(seeds)  # warm-up
    r.render_matte(seeds)
    r.aov_kernel_time()
    r.matte_kernel_time()
    aov_ms, matte_ms = [], []
    for k in range(REPEATS):
        r.render_aov(seeds, first_buffer_spp=n * (k + 1))
        aov_ms.append(r.aov_kernel_time()[0])
        r.render_matte(seeds)
        matte_ms.append(r.matte_kernel_time()[0])
    t0 = time.perf_counter()
    r.matte_ranks()
    t1 = time.perf_counter()
    r.matte_extract([native.MATTE_SKY, native.MATTE_WORLD_ENTITY, native.MATTE_ACTOR_ENTITY])
    t2 = time.perf_counter()
    other = r.read_matte()[2]
    rate = lambda ms: samples / (ms * 1e3)  # noqa: E731  (Msamples/s)
    aov_rate, matte_rate = [rate(ms) for ms in aov_ms], [rate(ms) for ms in matte_ms]
    ai, mi = r.aov_info(), r.matte_info()
    return {"view": name, "width": sc.width, "height": sc.height, "passes": n,
            "aov_msamples_s": float(np.median(aov_rate)), "matte_msamples_s": float(np.median(matte_rate)),
            "matte_over_aov": float(np.median(matte_rate) / np.median(aov_rate)),
            "aov_spread": round(spread(aov_rate), 4), "matte_spread": round(spread(matte_rate), 4),
            "aov_msamples_s_runs": [round(x, 1) for x in aov_rate], "matte_msamples_s_runs": [round(x, 1) for x in matte_rate],
            "aov_ms_runs": [round(x, 3) for x in aov_ms], "matte_ms_runs": [round(x, 3) for x in matte_ms],
            "ranks_call_ms": round((t1 - t0) * 1e3, 3), "extract_call_ms": round((t2 - t1) * 1e3, 3),
            "pixels_with_other": int((other > 0).sum()),
            "aov_kernel": {"tree": ai["tree"], "bvh": ai["bvh"], "workgroups": ai["blocks"], "launches": ai["launches"]},
            "matte_kernel": {"tree": mi["tree"], "bvh": mi["bvh"], "workgroups": mi["blocks"], "launches": mi["launches"]},
            "device": RendererInstance.get(0).device_name()}


def main(names):
    for name in names:
        sc = view(name)
        loader = HipSceneLoader(RendererInstance.get(0))
        loader.load_packed(sc)
        r = HipPathTracingRenderer(loader, sc.width, sc.height)
        r.set_camera(sc.projector_type, sc.camera)
        for n in PASSES:
            print(json.dumps(bench(name, sc, r, n)), flush=True)
        r.close()
        loader.close()


if __name__ == "__main__":
    main(sys.argv[1:] or VIEWS)
