#!/usr/bin/env python3
"""Light-group passes (chunky_render_light_passes: the sky's, the sun's and the emitters' share of the beauty image, DESIGN.md section
17) against chunky_render_passes — the unchanged render_pool — on the same target, in the same run, on bench.py's headline view (the
32x32-chunk outdoor world at 1920x1080), one MI355X (GPU box).

For N = 16 and 64 passes per call: one warm-up call of each kind, then three alternating repeats (beauty, light groups, light groups
with the scene's sun flag off); kernel time from the library's HIP-event accessors (chunky_render_kernel_time /
chunky_render_light_kernel_time).  The three group images cost three beauty renders without this pass, so the figure is light-group
time / beauty time against 3.  With the sun flag off a path has no sun traces: (sun on - sun off) is what they cost.

    python tools/lights_bench.py [out.json]     (default profiles/lights_bench.json)

--groups: the emitter groups (chunky_render_light_set_emitter_groups).  On ONE target, for N = 16 and 64: one warm-up of each kind, then
three alternating repeats of the beauty passes, the ungrouped light passes and the light passes with G = 1, 4 and 8 groups (the view's
emissive block pointers dealt round-robin into the groups; the groups are set between the timed calls).  Before anything is timed the
grouped call's four images are compared with the ungrouped call's.  One grouped walk delivers sky, sun and G group images, which cost
G + 2 beauty renders with darkened scenes: the walk wins where grouped time / beauty time < G + 2.

    python tools/lights_bench.py --groups [out.json]     (default profiles/lights_groups_bench.json)"""
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


GROUPS = (1, 4, 8)


def deal(ids, g):
    """the ids dealt round-robin into g groups"""
    return {int(i): k % g for k, i in enumerate(ids)}


def bench_groups(r, ids, n):
    seeds = native.java_random_ints(n)

    def grouped(g):
        def call(spp):
            r.set_emitter_groups(deal(ids, g), g)
            r.render_lights(seeds, first_buffer_spp=spp)
        return call

    def ungrouped(spp):
        r.set_emitter_groups({})
        r.render_lights(seeds, first_buffer_spp=spp)
    kinds = {"beauty": (lambda spp: r.render_passes(seeds, first_buffer_spp=spp), r.kernel_time), "lights": (ungrouped, r.lights_time)}
    kinds.update({f"lights_g{g}": (grouped(g), r.lights_time) for g in GROUPS})
    for call, timer in kinds.values():  # warm-up
        call(0)
        timer()
    ms = {k: [] for k in kinds}
    carried = {}
    for rep in range(REPEATS):
        for k, (call, timer) in kinds.items():
            call(n * (rep + 1))
            ms[k].append(timer()[0])
            if k != "beauty":
                carried[k] = r.lights_info()["groups"]
    assert carried == {"lights": False, **{f"lights_g{g}": True for g in GROUPS}}, carried
    med = {k: float(np.median(v)) for k, v in ms.items()}
    over_beauty = {g: med[f"lights_g{g}"] / med["beauty"] for g in GROUPS}
    wins = [g for g in GROUPS if over_beauty[g] < g + 2]
    # grouped time / beauty time as a line through G = 1 and G = 8, against G + 2
    slope = (over_beauty[GROUPS[-1]] - over_beauty[GROUPS[0]]) / (GROUPS[-1] - GROUPS[0])
    at0 = over_beauty[GROUPS[0]] - slope * GROUPS[0]
    return {"passes": n, "ms": {k: round(v, 3) for k, v in med.items()}, "ms_runs": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "grouped_over_ungrouped": {str(g): med[f"lights_g{g}"] / med["lights"] for g in GROUPS},
            "grouped_over_beauty": {str(g): over_beauty[g] for g in GROUPS}, "lights_over_beauty": med["lights"] / med["beauty"],
            "renders_replaced": {str(g): g + 2 for g in GROUPS}, "smallest_measured_G_that_wins": wins[0] if wins else None,
            "break_even_G_on_the_line_through_G1_and_G8": (at0 - 2) / (1 - slope) if slope < 1 else None}


def view_groups(inst, name, sc):
    """`name`: "outdoor", bench.py's headline view, which holds no emitter (every block pointer is dealt into the groups: what the walk
    pays there is the fold of G more images), or "outdoor_emitters", the same world with 2 % of its surface cells glowing (one
    emissive block pointer: the hit term, the table read and the per-sample sums run too)."""
    ids = [int(p) for p in scenes.emitter_ids(sc)[0]]
    emissive = len(ids)
    if not ids:
        ids = list(range(0, len(np.asarray(sc.block_palette)) - 1, 2))
    loader, r = target(inst, sc)
    # the grouped kernel folds the four images the ungrouped kernel folds, bit for bit, before anything is timed
    check = native.java_random_ints(2)
    r.render_lights(check)
    plain = [r.read_light(w).tobytes() for w in range(4)]
    same = True
    for g in GROUPS:
        r.set_emitter_groups(deal(ids, g), g)
        r.reset_lights()
        r.render_lights(check)
        assert r.lights_info()["groups"]
        same = same and [r.read_light(w).tobytes() for w in range(4)] == plain
    lit = [bool(r.read_light_group(g).any()) for g in range(GROUPS[-1])]
    r.set_emitter_groups({})
    r.reset()
    r.reset_lights()
    r.kernel_time(), r.lights_time()
    res = {"view": name, "width": sc.width, "height": sc.height, "four_images_equal_ungrouped": same, "emissive_block_pointers": emissive,
           "groups_lit_at_G8": lit, "runs": [bench_groups(r, ids, n) for n in PASSES]}
    for x in (r, loader):
        x.close()
    assert same, "the grouped call's four images differ from the ungrouped call's"
    return res


def main_groups(path):
    inst = RendererInstance.get(0)
    views = [view_groups(inst, "outdoor", scenes.cached_outdoor_world(chunks=32, height=256)),
             view_groups(inst, "outdoor_emitters", scenes.cached_outdoor_world(chunks=32, height=256, emitters=0.02))]
    res = {"device": inst.device_name(), "views": views,
           "note": "measured once on one GPU; kernel time from HIP events; median of three alternating repeats on one target; "
                   "G + 2 is what sky, sun and G group images cost as beauty renders"}
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--groups"]
    if "--groups" in sys.argv[1:]:
        main_groups(args[0] if args else os.path.join(ROOT, "profiles", "lights_groups_bench.json"))
    else:
        main(args[0] if args else os.path.join(ROOT, "profiles", "lights_bench.json"))
