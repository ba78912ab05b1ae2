#!/usr/bin/env python3
"""tools/adaptive_bench.py [--views outdoor,city,indoor] [--max-spp 256] [--out profiles/adaptive_bench.jsonl]

The numbers of DESIGN.md section 13, one JSON line each (one warm-up, median of three, variants alternated inside one session,
kernel time from HIP events):
  overhead   threshold 0 at max_spp against chunky_render_passes of the same seeds
  list       the list of all pixels in slot order (chunky_selftest_render_list) against the block mapping, 16 passes
  buys       per view and threshold: samples rendered as a share of W * H * max_spp, wall and kernel time, RMSE against a long uniform
             render (4 x max_spp passes of other seeds), and the uniform render's time and RMSE at the pass count of equal samples

tools/adaptive_bench.py --resume-legs --parent-lib PATH [--size 1920x1080] [--max-spp 64] [--out profiles/adaptive_resume.json]

The cost of the loop chunky_render_adaptive shares with chunky_render_adaptive_resume, on the `outdoor` timed view with the default
parameters (one warm-up, median of three, builds / variants alternated; wall clock and chunky_render_adaptive_kernel_time):
  single_call   chunky_render_adaptive under the library of the parent commit (PATH, built from a checkout of it) against this
                commit's: one child process per build and repetition, alternated.  Accepted within 3 %.
  four_resumes  on this commit: the same render as chunky_render_adaptive_ex to a quarter of max_spp and three
                chunky_render_adaptive_resume calls, against the single call.  Reported, not gated.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
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


def outdoor_target(inst, size):
    sc = gs.timed_view("outdoor").with_view(*size)
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def resume_child(a):
    """One build's share of `single_call`: a warm-up and one timed chunky_render_adaptive; one JSON line."""
    inst = RendererInstance.get(0)
    loader, r = outdoor_target(inst, a.size)
    seeds = native.java_random_ints(a.max_spp)
    p = native.adaptive_params()
    summ = native.AdaptiveSummary()

    def single():
        native.check(native.lib().chunky_render_adaptive(r._h, native.ptr(seeds), seeds.size, ctypes.byref(p), ctypes.byref(summ)))

    timed(single, r.adaptive_kernel_time)
    wall, kernel = timed(single, r.adaptive_kernel_time)
    print(json.dumps({"wall_ms": wall, "kernel_ms": kernel, "samples": summ.samples, "rounds": summ.rounds, "device": inst.device_name()}))
    r.close()
    loader.close()


def resume_legs(a):
    rows = {"view": "outdoor", "size": list(a.size), "max_spp": a.max_spp, "method": "one warm-up, median of three, alternated"}
    # leg 1: the parent commit's library against this one's, a child process each (one library per process)
    runs = {"parent": [], "this": []}
    for _ in range(3):
        for build, lib_path in (("parent", os.path.abspath(a.parent_lib)), ("this", native.LIB_PATH)):
            env = dict(os.environ, CHUNKY_HIP_LIB=lib_path)
            if build == "parent":
                env["CHUNKY_HIP_LIB_EARLIER"] = "1"  # (native.lib: the entry points that build lacks stay unbound)
            cmd = [sys.executable, os.path.abspath(__file__), "--resume-child", "--size", "%dx%d" % a.size, "--max-spp", str(a.max_spp)]
            proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if proc.returncode != 0:
                raise RuntimeError(f"the {build} build's run failed ({proc.returncode}):\n" + proc.stderr[-2000:])
            runs[build].append(json.loads(proc.stdout.strip().splitlines()[-1]))
    leg = {}
    for build, v in runs.items():
        assert v[0]["samples"] == runs["parent"][0]["samples"], "the two builds rendered different sample counts"
        leg[build] = {"wall_ms": statistics.median(x["wall_ms"] for x in v), "kernel_ms": statistics.median(x["kernel_ms"] for x in v),
                      "wall_ms_runs": [x["wall_ms"] for x in v], "kernel_ms_runs": [x["kernel_ms"] for x in v]}
    leg["samples"], leg["rounds"], rows["device"] = runs["this"][0]["samples"], runs["this"][0]["rounds"], runs["this"][0]["device"]
    leg["kernel_ratio_this_over_parent"] = leg["this"]["kernel_ms"] / leg["parent"]["kernel_ms"]
    leg["wall_ratio_this_over_parent"] = leg["this"]["wall_ms"] / leg["parent"]["wall_ms"]
    leg["accepted_within"] = 0.03
    leg["accepted"] = bool(leg["kernel_ratio_this_over_parent"] <= 1.03 and leg["wall_ratio_this_over_parent"] <= 1.03)
    rows["single_call"] = leg
    # leg 2: this commit, the render split into four calls against the single call
    inst = RendererInstance.get(0)
    loader, r = outdoor_target(inst, a.size)
    seeds = native.java_random_ints(a.max_spp)
    p = native.adaptive_params()
    cuts = [a.max_spp * k // 4 for k in (1, 2, 3, 4)]
    res = {}

    def single():
        res["single"] = r.render_adaptive_ex(seeds, p)[1]

    def split():
        r.render_adaptive_ex(seeds[:cuts[0]], p)
        for c in cuts[1:]:
            res["split"] = r.resume_adaptive(seeds[:c], p)[1]

    m = median3({"single": (single, r.adaptive_kernel_time), "four_resumes": (split, r.adaptive_kernel_time)})
    assert res["single"]["samples"] == res["split"]["samples"] and res["single"]["active"] == res["split"]["active"], (res["single"], res["split"])
    rows["four_resumes"] = {"cuts": cuts, "min_spp": p.min_spp, "check_interval": p.check_interval, "threshold": p.threshold,
                            "single_wall_ms": m["single"][0], "single_kernel_ms": m["single"][1],
                            "split_wall_ms": m["four_resumes"][0], "split_kernel_ms": m["four_resumes"][1],
                            "rounds_single": res["single"]["rounds"], "rounds_split": res["split"]["rounds"], "samples": res["single"]["samples"],
                            "gated": False}
    r.close()
    loader.close()
    json.dump(rows, open(a.out, "w"), indent=1)
    print(json.dumps(rows))
    if not leg["accepted"]:
        sys.exit("single_call: this build is outside 3 %% of the parent's (kernel x%.4f, wall x%.4f)"
                 % (leg["kernel_ratio_this_over_parent"], leg["wall_ratio_this_over_parent"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resume-legs", action="store_true")
    ap.add_argument("--resume-child", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--size", default="1920x1080", type=lambda s: tuple(int(x) for x in s.split("x")))
    ap.add_argument("--views", default="outdoor,city,indoor")
    ap.add_argument("--max-spp", type=int, default=None, help="default: 256, and 64 for --resume-legs")
    ap.add_argument("--thresholds", default="0.02,0.05,0.1,0.2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_bench.jsonl"))
    a = ap.parse_args()
    if a.max_spp is None:
        a.max_spp = 64 if a.resume_legs or a.resume_child else 256
    if a.resume_child:
        return resume_child(a)
    if a.resume_legs:
        if not a.parent_lib:
            ap.error("--resume-legs needs --parent-lib, the library built from the parent commit")
        if a.out == ap.get_default("out"):
            a.out = os.path.join(ROOT, "profiles", "adaptive_resume.json")
        return resume_legs(a)
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
