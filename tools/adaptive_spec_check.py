#!/usr/bin/env python3
"""tools/adaptive_spec_check.py — writes profiles/adaptive_spec_check.json: for every golden scene and every setting the GPU tests of
adaptive sampling use, the share of pixels that leave early, the share still active at the last check and the number of distinct
counts, from the numpy restatement on the CPU oracle's samples.  CPU only; tests/test_adaptive_cpu.py asserts the record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_scenes as gs  # noqa: E402
import test_adaptive_cpu as t  # noqa: E402

rec = {"max_spp": t.MAX_SPP, "floor": t.FLOOR, "settings": [list(s) for s in t.SETTINGS], "columns": "(min_spp, check_interval, threshold)",
       "carries": t.CARRIES,
       "scenes": {name: [dict(t.non_degenerate(t.samples_of(name), *s), role="condition" if k == t.CARRIES[name] else "edge case")
                         for k, s in enumerate(t.SETTINGS)] for name in gs.NAMES}}
path = os.path.join(ROOT, "profiles", "adaptive_spec_check.json")
json.dump(rec, open(path, "w"), indent=1)
print(path)
for name, rows in rec["scenes"].items():
    print(name, [(d["role"], "ok" if t.is_ok(d) else "degenerate") for d in rows])
