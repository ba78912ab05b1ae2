"""The exhibit of tests/ext_scenes.py on the CPU: the census that keeps it honest — the restatement's own rays, under the options
the GPU tests use (tests/test_gpu_ext_exhibit.py), must reach every class of event of the extended path (oracle/port.c
trace_sample_ext) at least 64 times — the emitter list's levels, and the two mutations of the expectation that the findings of
DESIGN.md section 3 call for: an emitter list without its level bits, and an emitter sample that reads its texture with tu and tv
swapped, must each change the image.

profiles/ext_census.json holds the census; the test compares what it counts with that file (EXT_CENSUS_WRITE=1 rewrites it)."""
import json
import os

import numpy as np

import ext_scenes as es
from oracle import binding
from oracle.binding import PortExt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS = os.path.join(ROOT, "profiles", "ext_census.json")
MIN_EVENTS = 64   # per class, in at least one run: the routes' own threshold (tests/test_routes_cpu.py)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def count(port, name, opts):
    """(the extended path's counters, the image) of variant `name` under `opts`: every pixel, the seeds of the GPU tests."""
    port.counters(enable=True, reset=True)
    port.counters(reset=True)
    try:
        img = es.expected(port, name, opts)
    finally:
        c = port.counters(enable=False, reset=True)
    return {k: c[k] for k in binding.EXT_COUNTER_NAMES}, img


def test_emitter_levels_of_the_exhibit(port):
    for name, broken in (("exhibit", False), ("exhibit_d11", False), ("exhibit_entities", False), ("exhibit_broken", True)):
        with PortExt(port, es.make(name)) as e:
            levels = (e.emitters[:e.n_emitters, 3] >> 25) & 15
        want = es.expected_levels(broken)
        assert {k: int((levels == k).sum()) for k in range(3)} == want and len(levels) == sum(want.values()), (name, levels)
    with PortExt(port, es.make("exhibit")) as e:
        kinds = set((e.emitters[:e.n_emitters, 3] & es.LEVEL_MASK).tolist())
    B = es.blocks()
    assert kinds == {B["glow"], B["quadrants"], B["ember"]}   # no model block, no emittance texture, and not the twin no leaf holds


def test_census_every_class_is_reached(port):
    runs = {}
    for key, (name, opts) in es.OPTION_SETS.items():
        for variant in (name, name + "_entities"):
            runs[f"{key}@{variant}"], _img = count(port, variant, opts)
    found = {"threshold": MIN_EVENTS, "pixels": es.W * es.H, "seeds": es.N_PASSES, "exempt": list(es.CENSUS_EXEMPT), "runs": runs,
             "most": {k: max(r[k] for r in runs.values()) for k in binding.EXT_COUNTER_NAMES}}
    assert set(es.CENSUS_CLASSES) | set(es.CENSUS_EXEMPT) == set(binding.EXT_COUNTER_NAMES)
    for k in es.CENSUS_CLASSES:
        print(k, found["most"][k])
        assert found["most"][k] >= MIN_EVENTS, (k, found["most"][k])
    if os.environ.get("EXT_CENSUS_WRITE"):
        with open(CENSUS, "w") as f:
            json.dump(found, f, indent=1, sort_keys=True)
            f.write("\n")
    assert json.load(open(CENSUS)) == json.loads(json.dumps(found)), "profiles/ext_census.json is not what the census counts (EXT_CENSUS_WRITE=1 rewrites it)"


def test_counters_change_no_float(port):
    for key in ("nee_bsdf", "sun0"):
        name, opts = es.OPTION_SETS[key]
        _c, counted = count(port, name + "_entities", opts)
        plain = es.expected(port, name + "_entities", opts)
        np.testing.assert_array_equal(bits(counted), bits(plain))


def test_mutated_expectations_differ(port):
    """What would have caught the findings: with the level bits of the emitter list masked off, and with tu / tv swapped at the
    emitter sample (the list's `quadrants` entries pointing at a twin block with the texture transposed, which no leaf holds, so
    that nothing but the emitter sample reads it), the expected image is another one.  The inputs are mutated, never the library."""
    name, opts = es.OPTION_SETS["nee"]
    real = es.expected(port, name, opts)
    with PortExt(port, es.make(name)) as e:
        listed = e.emitters[:e.n_emitters].copy()
    np.testing.assert_array_equal(bits(es.expected(port, name, opts, emitters=listed)), bits(real))   # the copy itself changes nothing
    flat = listed.copy()
    flat[:, 3] &= es.LEVEL_MASK
    assert (flat[:, 3] != listed[:, 3]).sum() == 4
    assert not np.array_equal(bits(es.expected(port, name, opts, emitters=flat)), bits(real))
    twin, n = es.transposed_twin(listed)
    assert n == 5
    assert not np.array_equal(bits(es.expected(port, name, opts, emitters=twin)), bits(real))
