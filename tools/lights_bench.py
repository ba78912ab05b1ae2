#!/usr/bin/env python3
"""Light-group passes (chunky_render_light_passes: the sky's, the sun's and the emitters' share of the beauty image, DESIGN.md section
17) against chunky_render_passes — the unchanged render_pool — on the same target, in the same run, on bench.py's headline view (the
32x32-chunk outdoor world at 1920x1080), one MI355X (GPU box).

For N = 16 and 64 passes per call: one warm-up call of each kind, then three alternating repeats (beauty, light groups, light groups
with the scene's sun flag off); kernel time from the library's HIP-event accessors (chunky_render_kernel_time /
chunky_render_light_kernel_time).  The three group images cost three beauty renders without this pass, so the figure is light-group
time / beauty time against 3.  With the sun flag off a path has no sun traces: (sun on - sun off) is what they cost.

    python tools/lights_bench.py [out.json]     (default profiles/lights_bench.json)"""
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chunkyclplugin_amd import native, scenes  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402

PASSES = (16, 64)
REPEATS = 3


def target(inst, sc):
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def bench(r, r_nosun, n):
    seeds = native.java_random_ints(n)
    kinds = {"beauty": (lambda spp: r.render_passes(seeds, first_buffer_spp=spp), r.kernel_time),
             "lights": (lambda spp: r.render_lights(seeds, first_buffer_spp=spp), r.lights_time),
             "beauty_sun_off": (lambda spp: r_nosun.render_passes(seeds, first_buffer_spp=spp), r_nosun.kernel_time),
             "lights_sun_off": (lambda spp: r_nosun.render_lights(seeds, first_buffer_spp=spp), r_nosun.lights_time)}
    for call, timer in kinds.values():  # warm-up
        call(0)
        timer()
    ms = {k: [] for k in kinds}
    for rep in range(REPEATS):
        for k, (call, timer) in kinds.items():
            call(n * (rep + 1))
            ms[k].append(timer()[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    li, bi = r.lights_info(), r.kernel_info()
    return {"passes": n, "ms": {k: round(v, 3) for k, v in med.items()}, "ms_runs": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "lights_over_beauty": med["lights"] / med["beauty"], "sun_off_lights_over_beauty": med["lights_sun_off"] / med["beauty_sun_off"],
            "share_of_lights_time": {"main traces, shading and folds (sun off)": med["lights_sun_off"] / med["lights"],
                                     "sun traces (sun on - sun off)": (med["lights"] - med["lights_sun_off"]) / med["lights"]},
            "light_kernel": {"tree": li["tree"], "bvh": li["bvh"], "workgroups": li["blocks"], "launches": li["launches"]},
            "beauty_kernel": {"tree": bi["tree"], "bvh": bi["bvh"], "workgroups": bi["blocks"], "pool": bi["pool"], "passes_per_launch": bi["passes_per_launch"]}}


def main(path):
    sc = scenes.cached_outdoor_world(chunks=32, height=256)
    sun = np.array(sc.sun, np.int32)
    assert sun[0] & 1, "the headline view has its sun flag set"
    sun[0] &= ~1
    inst = RendererInstance.get(0)
    loader, r = target(inst, sc)
    loader_off, r_off = target(inst, dataclasses.replace(sc, sun=sun))
    # the two kernels render the same image: ALL against the beauty image, bit for bit, before anything is timed
    check = native.java_random_ints(2)
    r.render_passes(check)
    r.render_lights(check)
    same = bool(r.read().tobytes() == r.read_light(native.LIGHT_ALL).tobytes())
    r.reset()
    r.reset_lights()
    r.kernel_time(), r.lights_time()
    res = {"view": "outdoor", "width": sc.width, "height": sc.height, "all_equals_beauty": same, "device": inst.device_name(),
           "runs": [bench(r, r_off, n) for n in PASSES],
           "note": "measured once on one GPU; kernel time from HIP events; median of three alternating repeats; three is what the same images cost as beauty renders"}
    for x in (r, loader, r_off, loader_off):
        x.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lights_bench.json"))
