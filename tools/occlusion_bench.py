#!/usr/bin/env python3
"""Occlusion passes (chunky_render_occlusion_passes: the sun-shadow and ambient-occlusion images) against
chunky_render_aov_passes_ex passes on the same target, in the same run, on bench.py's headline view (the 32x32-chunk outdoor world at
1920x1080), one MI355X (GPU box).

For N = 16 and 64 passes per call: one warm-up call of each kind, then three alternating repeats (AOV-ex, occlusion at radius 4,
occlusion with the scene's sun flag off); kernel time from the library's HIP-event accessors (chunky_render_aov_kernel_time /
chunky_render_occlusion_kernel_time).  An occlusion sample is up to three traces where an AOV-ex sample is one: the ratio would be 3 if
each cost what a primary trace costs and every first trace hit.  With the sun flag off the sample has no sun trace, so
(sun on - sun off) is what the sun traces cost and (sun off - AOV-ex) what the bounce traces cost.

    python tools/occlusion_bench.py [out.json]     (default profiles/occlusion_bench.json)"""
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
RADIUS = 4.0


def target(inst, sc):
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def bench(r, r_nosun, n):
    seeds = native.java_random_ints(n)
    kinds = {"aov_ex": (lambda spp: r.render_aov_ex(seeds, first_buffer_spp=spp), r.aov_kernel_time),
             "occlusion": (lambda spp: r.render_occlusion(seeds, RADIUS, first_buffer_spp=spp), r.occlusion_time),
             "occlusion_sun_off": (lambda spp: r_nosun.render_occlusion(seeds, RADIUS, first_buffer_spp=spp), r_nosun.occlusion_time)}
    for call, timer in kinds.values():  # warm-up
        call(0)
        timer()
    ms = {k: [] for k in kinds}
    for rep in range(REPEATS):
        for k, (call, timer) in kinds.items():
            call(n * (rep + 1))
            ms[k].append(timer()[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    oi, ai = r.occlusion_info(), r.aov_info()
    return {"passes": n, "ms": {k: round(v, 3) for k, v in med.items()}, "ms_runs": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "occlusion_over_aov_ex": med["occlusion"] / med["aov_ex"], "sun_off_over_aov_ex": med["occlusion_sun_off"] / med["aov_ex"],
            "share_of_occlusion_time": {"primary (the AOV-ex time)": med["aov_ex"] / med["occlusion"],
                                        "bounce (sun off - AOV-ex)": (med["occlusion_sun_off"] - med["aov_ex"]) / med["occlusion"],
                                        "sun (sun on - sun off)": (med["occlusion"] - med["occlusion_sun_off"]) / med["occlusion"]},
            "occlusion_kernel": {"tree": oi["tree"], "bvh": oi["bvh"], "workgroups": oi["blocks"], "launches": oi["launches"]},
            "aov_ex_kernel": {"tree": ai["tree"], "bvh": ai["bvh"], "workgroups": ai["blocks"], "launches": ai["launches"]}}


def main(path):
    sc = scenes.cached_outdoor_world(chunks=32, height=256)
    sun = np.array(sc.sun, np.int32)
    assert sun[0] & 1, "the headline view has its sun flag set"
    sun[0] &= ~1
    inst = RendererInstance.get(0)
    loader, r = target(inst, sc)
    loader_off, r_off = target(inst, dataclasses.replace(sc, sun=sun))
    r.render_aov_ex(native.java_random_ints(4))
    alpha = float(r.read_aov_ex(native.AOV_ALPHA).mean())
    r.reset_aov()
    res = {"view": "outdoor", "width": sc.width, "height": sc.height, "ao_distance": RADIUS, "first_traces_that_hit": alpha,
           "device": inst.device_name(), "runs": [bench(r, r_off, n) for n in PASSES],
           "note": "measured once on one GPU; kernel time from HIP events; median of three alternating repeats"}
    for x in (r, loader, r_off, loader_off):
        x.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "occlusion_bench.json"))
