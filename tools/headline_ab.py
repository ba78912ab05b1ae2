#!/usr/bin/env python3
"""The headline of bench.py on an earlier commit's library and on this tree's, alternating on one GPU: what a change to the
instructions of existing kernels is measured by when tools/isa_same.py cannot call them identical.

    python tools/headline_ab.py EARLIER_LIB [out.json] [--runs N]     (default out: headline_ab.json beside bench_detail.json, N = 2)

EARLIER_LIB: libchunky_hip.so built from the earlier commit (a checkout of it, native.build(), the file copied out).  Each run is a
child process `bench.py --gpus 1 --steps 8 --warmup 2`, the earlier library first; its child loads it through CHUNKY_HIP_LIB with
CHUNKY_HIP_LIB_EARLIER=1, so that entry points the earlier library lacks stay unbound.  The result holds every run's value, each
side's spread (max - min), and whether this tree's mean trails the earlier one's by no more than the earlier side's own spread.
tools/window_bench.py --headline takes the file."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["--gpus", "1", "--steps", "8", "--warmup", "2"]


def one(lib, detail):
    env = dict(os.environ)
    env.pop("CHUNKY_HIP_LIB", None)
    env.pop("CHUNKY_HIP_LIB_EARLIER", None)
    if lib:
        env["CHUNKY_HIP_LIB"] = os.path.abspath(lib)
        env["CHUNKY_HIP_LIB_EARLIER"] = "1"
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *BENCH, "--detail", detail], env=env, capture_output=True, text=True, timeout=300)
    if proc.returncode != 0:
        raise SystemExit(f"headline_ab: bench.py failed ({proc.returncode}) on {lib or 'this tree'}:\n" + proc.stderr[-2000:])
    line = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main(args):
    runs = 2
    if "--runs" in args:
        i = args.index("--runs")
        runs = int(args[i + 1])
        del args[i:i + 2]
    if not args:
        raise SystemExit(__doc__)
    earlier = args[0]
    out = args[1] if len(args) > 1 else os.path.join(ROOT, "headline_ab.json")
    detail = out + ".detail"
    res = {"command": "bench.py " + " ".join(BENCH) + ", the earlier library and this tree's alternating on one GPU, the earlier one first", "earlier": [], "this": []}
    for _ in range(runs):
        for key, lib in (("earlier", earlier), ("this", None)):
            d = one(lib, detail)
            res[key].append(d["value"])
            res["metric"], res["unit"] = d.get("metric"), d.get("unit")
            print(key, d["value"], flush=True)
    if os.path.exists(detail):
        os.remove(detail)
    spread = max(res["earlier"]) - min(res["earlier"])
    mean = {k: sum(res[k]) / len(res[k]) for k in ("earlier", "this")}
    res["earlier_spread"] = spread
    res["this_spread"] = max(res["this"]) - min(res["this"])
    res["this_mean_minus_earlier_mean"] = mean["this"] - mean["earlier"]
    res["within_the_earlier_spread"] = bool(mean["this"] >= mean["earlier"] - spread)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
