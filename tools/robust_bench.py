#!/usr/bin/env python3
"""tools/robust_bench.py [--size 1920 1080] [--passes 64] [--buckets 9] [--repeats 3] [--out profiles/robust_bench.json]

What the bucket fold costs on the headline view (the outdoor timed view at 1920 x 1080): the device time of
chunky_render_robust_passes (render_pool + fold_buckets_kernel<M>) against chunky_render_passes (render_pool + fold_kernel: the
kernels as they were) for the same N passes, and the device time of one resolve.  One warm-up of each, then `repeats` alternating
pairs; the medians and their ratio are reported, with every single timing beside them.  The times are the library's own HIP-event
brackets (chunky_render_kernel_time / chunky_render_robust_kernel_time).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_scenes as gs  # noqa: E402
from chunkyclplugin_amd import native  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--passes", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_bench.json"))
    a = ap.parse_args()
    sc = gs.timed_view("outdoor").with_view(*a.size)
    seeds = native.java_random_ints(a.passes)
    inst = RendererInstance.get(0)
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)

    def plain():
        r.reset()
        r.kernel_time()
        r.render_passes(seeds)
        ms, launches = r.kernel_time()
        return ms, launches, r.read().copy()

    def robust():
        r.reset()
        r.robust_begin(a.buckets)
        r.robust_kernel_time()
        r.robust_passes(seeds)
        ms, launches, _ = r.robust_kernel_time()
        image = r.read().copy()
        r.robust_resolve()
        return ms, launches, image, r.robust_kernel_time()[2]

    plain()
    robust()  # warm-up: allocations, code objects
    rows = []
    for _ in range(a.repeats):
        p = plain()
        q = robust()
        if p[2].tobytes() != q[2].tobytes():
            raise SystemExit("robust_bench: the beauty image of robust_passes differs from render_passes")
        rows.append({"passes_ms": p[0], "passes_launches": p[1], "robust_passes_ms": q[0], "robust_passes_launches": q[1], "resolve_ms": q[3]})
    med = {k: statistics.median(row[k] for row in rows) for k in ("passes_ms", "robust_passes_ms", "resolve_ms")}
    res = {"view": "outdoor (timed view)", "size": list(a.size), "passes": a.passes, "buckets": a.buckets, "device": inst.device_name(),
           "kernel": r.kernel_info(), "median": med, "ratio_robust_over_plain": med["robust_passes_ms"] / med["passes_ms"],
           "beauty_image_identical": True, "repeats": rows,
           "method": "one warm-up of each, then alternating pairs; HIP-event brackets around each launch (render kernel + fold), summed per call"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("size", "passes", "buckets", "median", "ratio_robust_over_plain")}))
    r.close()
    loader.close()


if __name__ == "__main__":
    main()
