#!/usr/bin/env python3
"""The ground-fog layer (chunky_render_set_fog): what it costs on bench.py's headline view (the 32x32-chunk outdoor
world at 1920x1080), one MI355X (GPU box).

One target.  Every leg runs the EXTENDED family — CHUNKY_OPT_SUN_SAMPLING at 1, which on this world (its sun is on) is the transport of
the default — so that what is compared is the fog instantiation render_pool<17, 32, ext> (CHUNKY_FOG) against the plain
render_pool<17, 32, ext>: fog off, then a layer over y in [0, 128) at optical depths 0.1, 1 and 4 across it.  For N = 16 passes per
call: one warm-up call of each leg, then three repeats in which the legs alternate; kernel time from the library's HIP-event accessor
(chunky_render_kernel_time), the median of the three.  Medium vertices per sample come from the CPU specification (tests/fog_port.c,
its census) on sixteen whole rows of the view, two passes.  Before anything is timed: with the layer off again the image is the
image of a target that never had one, bit for bit.  No threshold: nobody has measured any of this before.

    python tools/fog_bench.py [out.json]     (default profiles/fog_bench.json)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chunkyclplugin_amd import native, scenes  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402

PASSES = 16
REPEATS = 3
SLAB = (0.0, 128.0)
DEPTHS = (0.0, 0.1, 1.0, 4.0)  # optical depth across the slab; 0: off
COLOR = (0.8, 0.85, 1.0)
CENSUS_PASSES = 2


def layer(tau):
    return (tau / (SLAB[1] - SLAB[0]), SLAB[0], SLAB[1], COLOR)


def set_layer(r, tau):
    if tau == 0.0:
        r.set_fog(0.0)
    else:
        r.set_fog(*layer(tau))


def census(sc, tau):
    """medium vertices, fog segments and sun rays per sample, by the CPU specification on sixteen rows"""
    import fog_spec
    import golden_scenes as gs
    from oracle import binding
    L = fog_spec.lib()
    gids = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width, dtype=np.int32) for y in gs.timed_rows(sc)])
    L.census(enable=True, reset=True)
    with binding.PortExt(L, sc, sun_sampling=1), fog_spec.Fog(L, *layer(tau)):
        L.fog_render_gids(sc, native.java_random_ints(CENSUS_PASSES), gids, threads=binding.usable_threads())
    c = L.census(enable=False, reset=True)
    n = float(gids.size * CENSUS_PASSES)
    return {"samples": int(n), "medium_vertices_per_sample": c["medium"] / n, "fog_segments_per_sample": c["segments"] / n,
            "medium_sun_rays_per_sample": c["medium_sun"] / n, "dimmed_surface_sun_rays_per_sample": c["surface_sun"] / n}


def main(path):
    sc = scenes.cached_outdoor_world(chunks=32, height=256)
    inst = RendererInstance.get(0)
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_SUN_SAMPLING, 1)
    # the guard: a layer set and taken away again leaves the image of a target that never had one
    check = native.java_random_ints(2)
    r.render_passes(check)
    want = r.read().copy()
    set_layer(r, 1.0)
    r.reset()
    r.render_passes(check)
    changed = int((r.read().view(np.uint32) != want.view(np.uint32)).sum())
    set_layer(r, 0.0)
    r.reset()
    r.render_passes(check)
    if r.read().tobytes() != want.tobytes():
        raise SystemExit("fog_bench: with the layer off again the image differs from the image before it was set: nothing timed")
    r.reset()
    r.kernel_time()
    seeds = native.java_random_ints(PASSES)
    ms, info = {t: [] for t in DEPTHS}, {}
    for tau in DEPTHS:  # warm-up of each leg
        set_layer(r, tau)
        r.render_passes(seeds)
        r.kernel_time()
    for rep in range(REPEATS):
        for tau in DEPTHS:
            set_layer(r, tau)
            r.render_passes(seeds, first_buffer_spp=PASSES * (rep + 1))
            ms[tau].append(r.kernel_time()[0])
            info[tau] = r.kernel_info()
    samples = sc.width * sc.height * PASSES
    legs = []
    for tau in DEPTHS:
        med = float(np.median(ms[tau]))
        leg = {"optical_depth": tau, "density": layer(tau)[0], "ms": round(med, 3), "ms_runs": [round(x, 3) for x in ms[tau]],
               "msamples_per_s": samples / med / 1e3, "over_fog_off": med / float(np.median(ms[0.0])),
               "kernel": {k: info[tau][k] for k in ("tree", "pool", "bvh", "ext", "fog", "blocks")}}
        if tau > 0:
            leg.update(census(sc, tau))
        legs.append(leg)
    res = {"view": "outdoor", "width": sc.width, "height": sc.height, "device": inst.device_name(), "passes_per_call": PASSES, "slab": list(SLAB),
           "color": list(COLOR), "options": {"sun_sampling": 1}, "floats_changed_by_the_layer_at_depth_1": changed, "of_floats": int(want.size),
           "off_again_equals_never_set": True, "legs": legs,
           "note": "measured once on one GPU; kernel time from HIP events; median of three repeats in which the legs alternate on one target; "
                   "fog off = the plain extended instantiation; per-sample counts from the CPU specification on sixteen rows"}
    for x in (r, loader):
        x.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "fog_bench.json"))
