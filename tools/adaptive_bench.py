#!/usr/bin/env python3
"""tools/adaptive_bench.py [--views outdoor,city,indoor] [--max-spp 256] [--out profiles/adaptive_bench.jsonl]

The numbers of DESIGN.md section 13, one JSON line each (one warm-up, median of three, variants alternated inside one session,
kernel time from HIP events):
  overhead   threshold 0 at max_spp against chunky_render_passes of the same seeds
  list       the list of all pixels in slot order (chunky_selftest_render_list) against the block mapping, 16 passes
  buys       per view and threshold: samples rendered as a share of W * H * max_spp, wall and kernel time, RMSE against a long uniform
             render (4 x max_spp passes of other seeds), and the uniform render's time and RMSE at the pass count of equal samples
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_scenes as gs  # noqa: E402
from chunkyclplugin_amd import native  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, pool_slot_order  # noqa: E402


def timed(fn, kernel_time):
    kernel_time()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3, kernel_time()[0]


def median3(variants):
    """{name: (fn, kernel_time)} -> {name: (wall ms, kernel ms)}: one warm-up of each, then three alternated rounds."""
    for fn, kt in variants.values():
        timed(fn, kt)
    runs = {k: [] for k in variants}
    for _ in range(3):
        for k, (fn, kt) in variants.items():
            runs[k].append(timed(fn, kt))
    return {k: (statistics.median(w for w, _ in v), statistics.median(g for _, g in v)) for k, v in runs.items()}


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)) ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="outdoor,city,indoor")
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--thresholds", default="0.02,0.05,0.1,0.2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_bench.jsonl"))
    a = ap.parse_args()
    inst = RendererInstance.get(0)
    out = open(a.out, "w")

    def emit(row):
        row["device"] = inst.device_name()
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(json.dumps(row))

    all_seeds = native.java_random_ints(5 * a.max_spp)
    seeds, long_seeds = all_seeds[:a.max_spp], all_seeds[a.max_spp:]
    for view in a.views.split(","):
        sc = gs.timed_view(view)
        loader = HipSceneLoader(inst)
        loader.load_packed(sc)
        r = HipPathTracingRenderer(loader, sc.width, sc.height)
        r.set_camera(sc.projector_type, sc.camera)
        n_px = sc.width * sc.height

        def uniform(s=seeds):
            r.reset()
            r.render_passes(s)

        if view == a.views.split(",")[0]:
            p0 = native.adaptive_params(threshold=0.0)

            def adaptive_t0():  # the call alone: no read-back, like `uniform`
                native.check(native.lib().chunky_render_adaptive(r._h, native.ptr(seeds), seeds.size, ctypes.byref(p0), None))

            m = median3({"adaptive_t0": (adaptive_t0, r.adaptive_kernel_time), "uniform": (uniform, r.kernel_time)})
            emit({"what": "overhead", "view": view, "max_spp": a.max_spp, "min_spp": p0.min_spp, "check_interval": p0.check_interval,
                  "adaptive_t0_wall_ms": m["adaptive_t0"][0], "adaptive_t0_kernel_ms": m["adaptive_t0"][1],
                  "uniform_wall_ms": m["uniform"][0], "uniform_kernel_ms": m["uniform"][1]})
            order = pool_slot_order(sc.width, sc.height)
            m = median3({"list": (lambda: r.render_list(order, seeds[:16]), r.adaptive_kernel_time), "blocks": (lambda: uniform(seeds[:16]), r.kernel_time)})
            emit({"what": "list", "view": view, "passes": 16, "list_wall_ms": m["list"][0], "list_kernel_ms": m["list"][1],
                  "blocks_wall_ms": m["blocks"][0], "blocks_kernel_ms": m["blocks"][1]})
        uniform(long_seeds)
        truth = r.read().copy()
        for thr in [float(t) for t in a.thresholds.split(",")]:
            p = native.adaptive_params(threshold=thr)
            res = {}

            def adaptive():
                res["out"] = r.render_adaptive(seeds, p)

            adaptive()  # fixes the pass count of the uniform render that costs the same samples
            image, counts, _, summary = res["out"]
            share = summary["samples"] / (n_px * a.max_spp)
            equal = max(1, int(round(summary["samples"] / n_px)))
            m = median3({"adaptive": (adaptive, r.adaptive_kernel_time), "uniform": (lambda: uniform(seeds[:equal]), r.kernel_time)})
            uimage = r.read().copy()  # (the uniform variant ran last)
            emit({"what": "buys", "view": view, "max_spp": a.max_spp, "threshold": thr, "min_spp": p.min_spp, "check_interval": p.check_interval,
                  "floor": p.floor, "samples_share": share, "rounds": summary["rounds"], "active_after_checks": summary["active"],
                  "wall_ms": m["adaptive"][0], "kernel_ms": m["adaptive"][1], "rmse": rmse(image, truth),
                  "uniform_equal_passes": equal, "uniform_wall_ms": m["uniform"][0], "uniform_kernel_ms": m["uniform"][1],
                  "uniform_rmse": rmse(uimage, truth)})
        uniform(seeds)
        emit({"what": "uniform_full", "view": view, "max_spp": a.max_spp, "rmse": rmse(r.read(), truth)})
        r.close()
        loader.close()


if __name__ == "__main__":
    main()
