#!/usr/bin/env python3
"""Translucent blocks (chunky_render_set_translucency): what they cost on bench.py's headline view (the 32x32-chunk
outdoor world at 1920x1080), one MI355X (GPU box).

Every leg runs the EXTENDED family — CHUNKY_OPT_SUN_SAMPLING at 1, which on this world (its sun is on) is the transport of the default —
so that what is compared is the glass instantiation render_pool<17, 32, ext> (CHUNKY_GLASS) against the plain render_pool<17, 32, ext>:
  off          the headline world, the feature off;
  on_opaque    the same world, the feature on: nothing in it is translucent, so this is the cost of the hook and the wider parked record alone
               (and, checked before anything is timed, the same image bit for bit);
  water_off    outdoor_world(water=True, water_alpha=0xB0), the feature off: the lakes are painted lids;
  water_on     the same world, the feature on: the lakebeds are seen.
For N = 16 passes per call: one warm-up call of each leg, then three repeats in which the legs alternate; kernel time from the library's
HIP-event accessor (chunky_render_kernel_time), the median of the three.  Crossings per sample come from the CPU specification
(tests/glass_port.c, its census) on sixteen whole rows of the water view, two passes.  No threshold: nobody has measured any of this before.

    python tools/glass_bench.py [out.json]     (default profiles/glass_bench.json)"""
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
WATER_ALPHA = 0xB0
CENSUS_PASSES = 2
LEGS = (("off", "plain", False), ("on_opaque", "plain", True), ("water_off", "water", False), ("water_on", "water", True))


def census(sc):
    """crossings per sample on the water view, by the CPU specification on sixteen rows"""
    import glass_spec
    import golden_scenes as gs
    from oracle import binding
    L = glass_spec.lib()
    gids = np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width, dtype=np.int32) for y in gs.timed_rows(sc)])
    L.census(enable=True, reset=True)
    with binding.PortExt(L, sc, sun_sampling=1), glass_spec.Glass(L):
        L.glass_render_gids(sc, native.java_random_ints(CENSUS_PASSES), gids, threads=binding.usable_threads())
    c = L.census(enable=False, reset=True)
    n = float(gids.size * CENSUS_PASSES)
    return {"samples": int(n), **{k + "_per_sample": v / n for k, v in c.items()}}


def main(path):
    worlds = {"plain": scenes.cached_outdoor_world(chunks=32, height=256),
              "water": scenes.cached_outdoor_world(chunks=32, height=256, water=True, water_alpha=WATER_ALPHA)}
    inst = RendererInstance.get(0)
    targets = {}
    for name, sc in worlds.items():
        loader = HipSceneLoader(inst)
        loader.load_packed(sc)
        r = HipPathTracingRenderer(loader, sc.width, sc.height)
        r.set_camera(sc.projector_type, sc.camera)
        r.set_option(native.OPT_SUN_SAMPLING, 1)
        targets[name] = (loader, r)
    # the guards: on the plain world the feature changes no bit; on the water world it does
    check = native.java_random_ints(2)
    changed = {}
    for name, (_, r) in targets.items():
        r.render_passes(check)
        want = r.read().copy()
        r.set_translucency()
        r.reset()
        r.render_passes(check)
        changed[name] = int((r.read().view(np.uint32) != want.view(np.uint32)).sum())
        r.set_translucency(None)
        r.reset()
        r.kernel_time()
    if changed["plain"] != 0:
        raise SystemExit("glass_bench: the feature changed the image of a world with nothing translucent in it: nothing timed")
    if changed["water"] == 0:
        raise SystemExit("glass_bench: the feature changed nothing on the water world: nothing timed")
    seeds = native.java_random_ints(PASSES)
    ms, info = {leg[0]: [] for leg in LEGS}, {}

    def run(leg, first):
        name, world, on = leg
        r = targets[world][1]
        r.set_translucency(0.99 if on else None)
        r.render_passes(seeds, first_buffer_spp=first)
        t = r.kernel_time()[0]
        info[name] = r.kernel_info()
        return t

    for leg in LEGS:  # warm-up of each leg
        run(leg, 0)
    for rep in range(REPEATS):
        for leg in LEGS:
            ms[leg[0]].append(run(leg, PASSES * (rep + 1)))
    sc = worlds["plain"]
    samples = sc.width * sc.height * PASSES
    legs = []
    for name, world, on in LEGS:
        med = float(np.median(ms[name]))
        base = float(np.median(ms["off" if world == "plain" else "water_off"]))
        legs.append({"leg": name, "world": world, "translucency": on, "ms": round(med, 3), "ms_runs": [round(x, 3) for x in ms[name]],
                     "msamples_per_s": samples / med / 1e3, "over_its_off_leg": med / base,
                     "kernel": {k: info[name][k] for k in ("tree", "pool", "bvh", "ext", "glass", "blocks")}})
    res = {"view": "outdoor", "width": sc.width, "height": sc.height, "device": inst.device_name(), "passes_per_call": PASSES,
           "water_alpha": WATER_ALPHA, "options": {"sun_sampling": 1}, "floats_changed_by_the_feature": changed, "of_floats": int(3 * sc.width * sc.height),
           "legs": legs, "water_view_census": census(worlds["water"]),
           "note": "measured once on one GPU; kernel time from HIP events; median of three repeats in which the legs alternate; "
                   "off = the plain extended instantiation; per-sample counts from the CPU specification on sixteen rows"}
    for loader, r in targets.values():
        r.close()
        loader.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "glass_bench.json"))
