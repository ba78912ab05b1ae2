#!/usr/bin/env python3
"""Projected cameras against the pinhole and pre-generated (-1) cameras on bench.py's headline view (the 32x32-chunk outdoor world,
1920x1080), one MI355X (GPU box):

  pinhole    projector type 0, the view's own camera
  pregen     projector type -1, the fisheye table R_2(s) of chunky_camera_rays uploaded once
  fisheye    projector type 2, fov 180
  panoramic  projector type 3, fov 240
  fisheye_lens, panoramic_lens   the same two with a lens (chunky_render_set_lens: aperture 0.4, focus 60)
  ods        projector type 7, the right eye (offset 0.0345), vertical fov 180
  ods_stacked  projector type 8, both eyes, offset 0.0345, vertical fov 180

For N = 16 and 256 passes per call: one warm-up call per camera, then three repeats that alternate between the cameras; kernel time
from chunky_render_kernel_time (HIP events).  One JSON line per camera and N: Msamples/s (median of the repeats, and all three) and
the instantiation that ran.  Then one line with the host time of building and uploading one -1 table (chunky_camera_rays +
chunky_render_set_camera(-1), median of three), which the projected types do not pay per table, and one with the host time of one
lens table (chunky_camera_rays_lens), which a lens user paid per regeneration before the kernels had the lens.

    python tools/camera_bench.py [--out profiles/camera_bench.jsonl] [--append] [--cameras a,b,...] [--passes 16,256] [--no-host]

--cameras picks from the list above (default: all); --append adds the lines to the file instead of replacing it; --no-host leaves
out the two host lines.  A library of an earlier commit (CHUNKY_HIP_LIB with CHUNKY_HIP_LIB_EARLIER=1) runs the cameras it has."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chunkyclplugin_amd import native, scenes  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays  # noqa: E402

PASSES = (16, 256)
REPEATS = 3
LENS = (0.4, 60.0)
ALL = ("pinhole", "pregen", "fisheye", "panoramic", "fisheye_lens", "panoramic_lens", "ods", "ods_stacked")


def projected(sc, kind, fov, s13=0.0):
    s = np.asarray(sc.camera, np.float32)[:15].copy()
    s[12], s[13], s[14] = 0.0, s13, fov
    return s


def main(out_path, names=ALL, passes=PASSES, append=False, host=True):
    sc = scenes.cached_outdoor_world(chunks=32, height=256)
    W, H = sc.width, sc.height
    fish, pano = projected(sc, native.PROJ_FISHEYE, 180.0), projected(sc, native.PROJ_PANORAMIC, 240.0)
    cams = {"pinhole": (0, sc.camera, None), "pregen": (-1, None, None),
            "fisheye": (native.PROJ_FISHEYE, fish, None), "panoramic": (native.PROJ_PANORAMIC, pano, None),
            "fisheye_lens": (native.PROJ_FISHEYE, fish, LENS), "panoramic_lens": (native.PROJ_PANORAMIC, pano, LENS),
            "ods": (native.PROJ_ODS, projected(sc, native.PROJ_ODS, 180.0, 0.0345), None),
            "ods_stacked": (native.PROJ_ODS_STACKED, projected(sc, native.PROJ_ODS_STACKED, 180.0, 0.0345), None)}
    cams = {name: cams[name] for name in names}
    inst = RendererInstance.get(0)
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    targets = {}
    for name, (kind, settings, lens) in cams.items():
        r = HipPathTracingRenderer(loader, W, H)
        r.set_camera(kind, camera_rays(native.PROJ_FISHEYE, fish, W, H, 1) if kind == -1 else settings)
        if lens is not None:
            r.set_lens(*lens)
        targets[name] = r
    lines = []
    for n in passes:
        seeds = native.java_random_ints(n)
        for r in targets.values():   # warm-up
            r.render_passes(seeds)
            r.kernel_time()
        ms = {name: [] for name in targets}
        for k in range(REPEATS):
            for name, r in targets.items():
                r.render_passes(seeds, first_buffer_spp=n * (k + 1))
                ms[name].append(r.kernel_time()[0])
        for name, r in targets.items():
            rates = [W * H * n / (m * 1e3) for m in ms[name]]
            info = r.kernel_info()
            lines.append({"view": "outdoor", "camera": name, "projector_type": cams[name][0], **({"lens": list(cams[name][2])} if cams[name][2] else {}),
                          "width": W, "height": H, "passes": n,
                          "msamples_s": float(np.median(rates)), "msamples_s_runs": [round(x, 1) for x in rates],
                          "kernel_ms_runs": [round(x, 3) for x in ms[name]],
                          "kernel": {"tree": info["tree"], "pool": info["pool"], "sorted": info["sorted"], "workgroups": info["blocks"]},
                          "device": inst.device_name()})
            print(json.dumps(lines[-1]), flush=True)
    # the host side of one pre-generated table: build it, upload it
    r = targets.get("pregen") if host else None
    build_s, upload_s, lens_s = [], [], []
    for k in range(REPEATS if r is not None else 0):
        t0 = time.perf_counter()
        table = camera_rays(native.PROJ_FISHEYE, fish, W, H, 100 + k)
        t1 = time.perf_counter()
        r.set_camera(-1, table)
        t2 = time.perf_counter()
        build_s.append(t1 - t0)
        upload_s.append(t2 - t1)
    if r is not None:
        lines.append({"view": "outdoor", "what": "one -1 table: chunky_camera_rays + set_camera(-1)", "width": W, "height": H,
                      "table_mb": round(W * H * 6 * 4 / 1e6, 1), "build_ms": round(1e3 * float(np.median(build_s)), 2),
                      "upload_ms": round(1e3 * float(np.median(upload_s)), 2), "build_ms_runs": [round(1e3 * x, 2) for x in build_s],
                      "upload_ms_runs": [round(1e3 * x, 2) for x in upload_s]})
        print(json.dumps(lines[-1]), flush=True)
    if host and hasattr(native.lib(), "chunky_camera_rays_lens"):   # one lens table on the host (no device involved)
        for k in range(REPEATS):
            t0 = time.perf_counter()
            camera_rays(native.PROJ_FISHEYE, fish, W, H, 200 + k, LENS)
            lens_s.append(time.perf_counter() - t0)
        lines.append({"view": "outdoor", "what": "one lens table on the host: chunky_camera_rays_lens (fisheye)", "lens": list(LENS), "width": W,
                      "height": H, "table_mb": round(W * H * 6 * 4 / 1e6, 1), "build_ms": round(1e3 * float(np.median(lens_s)), 2),
                      "build_ms_runs": [round(1e3 * x, 2) for x in lens_s]})
        print(json.dumps(lines[-1]), flush=True)
    for r in targets.values():
        r.close()
    loader.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a" if append else "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "camera_bench.jsonl"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--cameras", default=",".join(ALL))
    ap.add_argument("--passes", default=",".join(str(n) for n in PASSES))
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    main(a.out, tuple(a.cameras.split(",")), tuple(int(n) for n in a.passes.split(",")), a.append, not a.no_host)
