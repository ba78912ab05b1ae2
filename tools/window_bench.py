#!/usr/bin/env python3
"""Canvas windows (chunky_render_set_canvas): what cutting a frame into windows costs on bench.py's headline world
(the 32x32-chunk outdoor world).  Needs a GPU.

A 3840 x 2160 canvas rendered as one launch on a target of that size, and as its four 1920 x 1080 quadrant windows on one target
moved from quadrant to quadrant (reset in between, as render_tiled does), N = 8 passes per call.  One warm-up of each kind, then three
alternating repeats; kernel time from the library's HIP-event accessor (chunky_render_kernel_time), the median of the three; the
four windows' times are summed.  The figure is windows / whole: a ratio, not a threshold.  Before anything is timed the four windows,
assembled, are the whole target's image bit for bit.

    python tools/window_bench.py [out.json] [--headline FILE]     (default profiles/window_bench.json)

--headline FILE: the output of tools/headline_ab.py (bench.py's headline on the parent commit's library and on this tree's,
alternating on one GPU), stored under "headline" beside the ratio: what the change of the kernels' instructions was measured by."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chunkyclplugin_amd import native, scenes  # noqa: E402
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance  # noqa: E402

CANVAS = (3840, 2160)
PASSES = 8
REPEATS = 3


def quadrants():
    w, h = CANVAS[0] // 2, CANVAS[1] // 2
    return [(x0, y0) for y0 in (0, h) for x0 in (0, w)]


def main(path, headline):
    sc = scenes.cached_outdoor_world(chunks=32, height=256).with_view(*CANVAS)
    inst = RendererInstance.get(0)
    loader = HipSceneLoader(inst)
    loader.load_packed(sc)
    whole = HipPathTracingRenderer(loader, *CANVAS)
    whole.set_camera(sc.projector_type, sc.camera)
    w, h = CANVAS[0] // 2, CANVAS[1] // 2
    win = HipPathTracingRenderer(loader, w, h)
    win.set_canvas(CANVAS[0], CANVAS[1], 0, 0)
    win.set_camera(sc.projector_type, sc.camera)
    seeds = native.java_random_ints(PASSES)

    def run_whole():
        whole.reset()
        whole.kernel_time()
        whole.render_passes(seeds)
        return whole.kernel_time()[0]

    def run_windows(frame=None):
        ms = []
        for x0, y0 in quadrants():
            win.set_canvas(CANVAS[0], CANVAS[1], x0, y0)
            win.reset()
            win.kernel_time()
            win.render_passes(seeds)
            ms.append(win.kernel_time()[0])
            if frame is not None:
                frame[y0:y0 + h, x0:x0 + w] = win.read().reshape(h, w, 3)
        return ms

    # the guard (and the warm-up of each kind): the assembled windows are the whole frame
    run_whole()
    frame = np.zeros((CANVAS[1], CANVAS[0], 3), np.float32)
    run_windows(frame)
    equal = bool(frame.tobytes() == whole.read().tobytes())
    if not equal:
        raise SystemExit("window_bench: the four windows do not assemble the whole target's image: nothing timed")
    t_whole, t_win = [], []
    for _ in range(REPEATS):
        t_whole.append(run_whole())
        t_win.append(run_windows())
    med_whole = float(np.median(t_whole))
    med_win = float(np.median([sum(q) for q in t_win]))
    res = {"view": "outdoor", "canvas": list(CANVAS), "window": [w, h], "passes": PASSES, "device": inst.device_name(),
           "windows_assemble_the_whole_image": equal, "ms_whole": round(med_whole, 3), "ms_four_windows": round(med_win, 3),
           "windows_over_whole": med_win / med_whole, "ms_runs_whole": [round(x, 3) for x in t_whole],
           "ms_runs_windows": [[round(x, 3) for x in q] for q in t_win],
           "kernel_whole": {k: whole.kernel_info()[k] for k in ("tree", "pool", "bvh", "sorted", "blocks")},
           "kernel_window": {k: win.kernel_info()[k] for k in ("tree", "pool", "bvh", "sorted", "blocks")},
           "note": "measured once on one GPU; kernel time from HIP events; median of three alternating repeats; the four windows' times summed"}
    if headline:
        with open(headline) as f:
            res["headline"] = json.load(f)
    for x in (whole, win, loader):
        x.close()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    args = sys.argv[1:]
    headline = None
    if "--headline" in args:
        i = args.index("--headline")
        headline = args[i + 1]
        del args[i:i + 2]
    main(args[0] if args else os.path.join(ROOT, "profiles", "window_bench.json"), headline)
