#!/usr/bin/env python3
"""AOV passes (chunky_render_aov_passes: albedo + normal of the first hit) against render passes on the same target, on the views
bench.py / tools/config_bench.py time, one MI355X (GPU box):

  outdoor      32x32-chunk world, 1920x1080 (bench.py's headline view)
  city         the reference's benchmark/OpenCL_test scene, 1920x1080
  indoor       emitter-lit room, 1920x1080
  entities     the outdoor world + 100 000 world / 5 000 actor triangles, 1920x1080
  entities4k   the same at 3840x2160 (the whole image on one GPU)

For N = 16 and 256 passes per call: one warm-up call of each kind, then three alternating repeats (render, AOV); kernel time from
the library's HIP-event accessors (chunky_render_kernel_time / chunky_render_aov_kernel_time).  One JSON line per view and N:
Msamples/s of each kernel (median of the repeats, and all three), their ratio and both instantiations.

    python tools/aov_bench.py [names...] > profiles/aov_bench.jsonl

With --ex the two kinds are chunky_render_aov_passes and chunky_render_aov_passes_ex (all seven first-hit images from the same trace,
DESIGN.md section 14) instead, alternating in the same way; one JSON line per view and N with both rates and ex / plain:

    python tools/aov_bench.py --ex [names...] > profiles/aov_ex_bench.jsonl"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chunkyclplugin_amd import native, octree2, scenes  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402

VIEWS = ["outdoor", "city", "indoor", "entities", "entities4k"]
PASSES = (16, 256)
REPEATS = 3


def view(name):
    """The scenes of tests/golden_scenes.py timed_view, built the same way."""
    if name == "outdoor":
        return scenes.cached_outdoor_world(chunks=32, height=256)
    if name == "city":
        return octree2.cached_benchmark_scene(1920, 1080)
    if name == "indoor":
        return scenes.indoor_room(size=64, width=1920, img_height=1080)
    if name in ("entities", "entities4k"):
        sc = scenes.add_entities(scenes.cached_outdoor_world(chunks=32, height=256), 100000, seed=11, actor_tris=5000,
                                 region=((40, 90, 40), (470, 170, 470)))
        return sc.with_view(3840, 2160) if name == "entities4k" else sc
    raise KeyError(name)


def bench(name, sc, r, n):
    seeds = native.java_random_ints(n)
    samples = sc.width * sc.height * n
    r.render_passes(seeds)  # warm-up
    r.render_aov(seeds)
    r.kernel_time()
    r.aov_kernel_time()
    render_ms, aov_ms = [], []
    for k in range(REPEATS):
        r.render_passes(seeds, first_buffer_spp=n * (k + 1))
        ms, launches = r.kernel_time()
        render_ms.append(ms)
        r.render_aov(seeds, first_buffer_spp=n * (k + 1))
        ms, launches = r.aov_kernel_time()
        aov_ms.append(ms)
    rate = lambda ms: samples / (ms * 1e3)  # noqa: E731  (Msamples/s)
    render_rate = [rate(ms) for ms in render_ms]
    aov_rate = [rate(ms) for ms in aov_ms]
    ri, ai = r.kernel_info(), r.aov_info()
    return {"view": name, "width": sc.width, "height": sc.height, "passes": n,
            "render_msamples_s": float(np.median(render_rate)), "aov_msamples_s": float(np.median(aov_rate)),
            "aov_over_render": float(np.median(aov_rate) / np.median(render_rate)),
            "render_msamples_s_runs": [round(x, 1) for x in render_rate], "aov_msamples_s_runs": [round(x, 1) for x in aov_rate],
            "render_ms_runs": [round(x, 3) for x in render_ms], "aov_ms_runs": [round(x, 3) for x in aov_ms],
            "aov_kernel": {"tree": ai["tree"], "bvh": ai["bvh"], "workgroups": ai["blocks"], "launches": ai["launches"]},
            "render_kernel": {"tree": ri["tree"], "bvh": ri["bvh"], "workgroups": ri["blocks"], "pool": ri["pool"], "sorted": ri["sorted"]},
            "device": RendererInstance.get(0).device_name()}


def bench_ex(name, sc, r, n):
    seeds = native.java_random_ints(n)
    samples = sc.width * sc.height * n
    r.render_aov(seeds)  # warm-up
    r.render_aov_ex(seeds)
    r.aov_kernel_time()
    plain_ms, ex_ms = [], []
    info = {}
    for k in range(REPEATS):
        for kind, call, ms_list in (("aov_kernel", r.render_aov, plain_ms), ("ex_kernel", r.render_aov_ex, ex_ms)):
            call(seeds, first_buffer_spp=n * (k + 1))
            ms_list.append(r.aov_kernel_time()[0])
            ai = r.aov_info()
            info[kind] = {"tree": ai["tree"], "bvh": ai["bvh"], "workgroups": ai["blocks"], "launches": ai["launches"]}
    rate = lambda ms: samples / (ms * 1e3)  # noqa: E731  (Msamples/s)
    plain_rate, ex_rate = [rate(ms) for ms in plain_ms], [rate(ms) for ms in ex_ms]
    return {"view": name, "width": sc.width, "height": sc.height, "passes": n,
            "aov_msamples_s": float(np.median(plain_rate)), "ex_msamples_s": float(np.median(ex_rate)),
            "ex_over_aov": float(np.median(ex_rate) / np.median(plain_rate)),
            "aov_msamples_s_runs": [round(x, 1) for x in plain_rate], "ex_msamples_s_runs": [round(x, 1) for x in ex_rate],
            "aov_ms_runs": [round(x, 3) for x in plain_ms], "ex_ms_runs": [round(x, 3) for x in ex_ms],
            **info, "device": RendererInstance.get(0).device_name()}


def main(names):
    ex = "--ex" in names
    names = [n for n in names if n != "--ex"] or VIEWS
    for name in names:
        sc = view(name)
        loader = HipSceneLoader(RendererInstance.get(0))
        loader.load_packed(sc)
        r = HipPathTracingRenderer(loader, sc.width, sc.height)
        r.set_camera(sc.projector_type, sc.camera)
        for n in PASSES:
            print(json.dumps((bench_ex if ex else bench)(name, sc, r, n)), flush=True)
        r.close()
        loader.close()


if __name__ == "__main__":
    main(sys.argv[1:] or VIEWS)
