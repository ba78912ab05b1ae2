#!/usr/bin/env python3
"""Biome tints by block position (chunky_scene_set_biome_tints): what the feature costs on bench.py's headline view
(the 32x32-chunk outdoor world at 1920x1080: tint-2 grass everywhere, tint-1 leaves), one MI355X (GPU box).

One target on a scene with a 512 x 512 map of 8-cell patches.  For N = 16 and 64 passes per call: one warm-up call of each kind, then
three alternating repeats with CHUNKY_OPT_BIOME_TINT at 0 — the unchanged render_pool<17, 64> — and at 1 — its biome instantiation;
kernel time from the library's HIP-event accessor (chunky_render_kernel_time), the median of the three.  The figure is on / off.
Before anything is timed: with the option at 0 the target's image is the image of a target on a scene without a map, bit for bit.

    python tools/biome_bench.py [out.json]     (default profiles/biome_bench.json)"""
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
MAP = (0, 0, 512, 512, 8)  # origin x, z; size x, z; patch


def target(inst, sc):
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def bench(r, n):
    seeds = native.java_random_ints(n)
    ms, info = {0: [], 1: []}, {}
    for on in (0, 1):  # warm-up of each kind
        r.set_option(native.OPT_BIOME_TINT, on)
        r.render_passes(seeds)
        r.kernel_time()
    for rep in range(REPEATS):
        for on in (0, 1):
            r.set_option(native.OPT_BIOME_TINT, on)
            r.render_passes(seeds, first_buffer_spp=n * (rep + 1))
            ms[on].append(r.kernel_time()[0])
            info[on] = r.kernel_info()
    med = {on: float(np.median(v)) for on, v in ms.items()}
    samples = r.width * r.height * n
    return {"passes": n, "ms_off": round(med[0], 3), "ms_on": round(med[1], 3), "on_over_off": med[1] / med[0],
            "msamples_per_s_off": samples / med[0] / 1e3, "msamples_per_s_on": samples / med[1] / 1e3,
            "ms_runs_off": [round(x, 3) for x in ms[0]], "ms_runs_on": [round(x, 3) for x in ms[1]],
            "kernel_off": {k: info[0][k] for k in ("tree", "pool", "bvh", "biome", "sorted", "blocks")},
            "kernel_on": {k: info[1][k] for k in ("tree", "pool", "bvh", "biome", "sorted", "blocks")}}


def main(path):
    plain = scenes.cached_outdoor_world(chunks=32, height=256)
    x0, z0, sx, sz, patch = MAP
    sc = dataclasses.replace(plain, biome=(x0, z0, scenes.biome_patches(sx, sz, patch, seed=1)))
    inst = RendererInstance.get(0)
    loader, r = target(inst, sc)
    # the guard: option off is a scene without a map, bit for bit; and the map is seen with it on
    check = native.java_random_ints(2)
    lp, rp = target(inst, plain)
    rp.render_passes(check)
    want = rp.read()
    for x in (rp, lp):
        x.close()
    r.set_option(native.OPT_BIOME_TINT, 0)
    r.render_passes(check)
    off_is_plain = bool(r.read().tobytes() == want.tobytes())
    r.set_option(native.OPT_BIOME_TINT, 1)
    r.reset()
    r.render_passes(check)
    floats_changed = int((r.read().view(np.uint32) != want.view(np.uint32)).sum())
    r.reset()
    r.kernel_time()
    if not off_is_plain:
        raise SystemExit("biome_bench: with the option at 0 the image differs from a scene without a map: nothing timed")
    res = {"view": "outdoor", "width": sc.width, "height": sc.height, "device": inst.device_name(), "map": {"origin": [x0, z0], "size": [sx, sz], "patch": patch,
           "layout": "three packed int32 per cell (12 bytes); the 16-byte layout was not measured"}, "option_off_equals_no_map": off_is_plain,
           "floats_changed_by_the_map": floats_changed, "of_floats": int(want.size), "runs": [bench(r, n) for n in PASSES],
           "note": "measured once on one GPU; kernel time from HIP events; median of three alternating repeats on one target; off = the unchanged render_pool<17, 64>"}
    for x in (r, loader):
        x.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "biome_bench.json"))
