"""chunky_render_occlusion_passes without a device: the header declares the calls and the library exports them, NULL handles and a
bad radius are errors, the specification in occlusion_spec.py means the same on the C restatement (oracle/port.c) as on the
reference build, and its samples are what the GPU tests lean on — 0 with the sun flag off, monotone in the radius, and not trivial."""
import re

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from occlusion_spec import IMAGES, expected_occlusion, fold_occlusion, occlusion_records, sample_values
from chunkyclplugin_amd import native

FUNCTIONS = ["chunky_render_occlusion_passes", "chunky_render_occlusion_read", "chunky_render_occlusion_reset",
             "chunky_render_occlusion_kernel_time", "chunky_render_occlusion_kernel_info"]
GIDS = np.arange(0, gs.W * gs.H, 7, dtype=np.int32)   # every 7th pixel, from sky to foreground
SEEDS = native.java_random_ints(3)
RADII = (0.25, 1.0, 4.0, 16.0, np.inf)
_records = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def records(name, passes=3):
    """the port's records of a golden scene at GIDS, gathered once and never changed"""
    if name not in _records:
        rec = occlusion_records(binding.port(), gs.make(name), SEEDS, GIDS)
        for v in rec.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _records[name] = rec
    rec = _records[name]
    return {k: (v[:passes] if isinstance(v, np.ndarray) else v) for k, v in rec.items()}


def test_header_declares_and_library_exports_the_entry_points():
    text = open(native.HEADER).read()
    for name, value in (("AO", 7), ("SUN", 8)):
        assert re.search(rf"#define\s+CHUNKY_AOV_{name}\s+{value}\b", text), name
        assert getattr(native, "AOV_" + name) == value
    declared = native.declared_symbols()
    L = native.lib()
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    for src in ("occlusion.hip", "capi_occlusion.hip"):
        assert src in native.SOURCES


def test_null_handles_and_bad_radii_are_errors():
    L = native.lib()
    seeds = np.zeros(2, np.int32)
    out = np.zeros(12, np.float32)
    info = np.zeros(4, np.int32)
    assert L.chunky_render_occlusion_passes(None, seeds.ctypes.data, 2, 0, 4.0) == native.E_INVALID
    assert b"NULL" in L.chunky_last_error()
    assert L.chunky_render_occlusion_read(None, native.AOV_AO, out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_occlusion_reset(None) == native.E_INVALID
    assert L.chunky_render_occlusion_kernel_info(None, info.ctypes.data) == native.E_INVALID
    for radius in (0.0, -0.0, -1.0, float("nan"), -float("inf")):
        assert L.chunky_render_occlusion_passes(None, seeds.ctypes.data, 2, 0, radius) == native.E_INVALID
        assert b"ao_distance" in L.chunky_last_error(), radius
    assert L.chunky_render_occlusion_passes(None, seeds.ctypes.data, -1, 0, 4.0) == native.E_INVALID
    assert L.chunky_render_occlusion_passes(None, None, 2, 0, 4.0) == native.E_INVALID
    assert L.chunky_render_occlusion_passes(None, seeds.ctypes.data, 2, -1, 4.0) == native.E_INVALID


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun"])
def test_port_spec_is_the_reference_spec(name):
    ref = binding.ref()
    if ref is None:
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    on_port = fold_occlusion(records(name), 4.0)
    on_ref = expected_occlusion(ref, gs.make(name), SEEDS, GIDS, 4.0)
    for k in IMAGES:
        np.testing.assert_array_equal(bits(on_port[k]), bits(on_ref[k]), err_msg=k)


def test_expected_occlusion_is_records_then_fold_and_continues():
    """One call equals records + fold, and 2 + 1 passes continued from `init` equal 3."""
    port = binding.port()
    sc = gs.make("entities")
    gids = GIDS[::9]
    whole = expected_occlusion(port, sc, SEEDS, gids, 4.0, first_spp=5)
    part = expected_occlusion(port, binding.SceneHandle(sc), SEEDS[:2], gids, 4.0, first_spp=5)
    part = expected_occlusion(port, sc, SEEDS[2:], gids, 4.0, first_spp=7, init=part)
    rec = records("entities")
    again = fold_occlusion({k: (v[:, ::9] if isinstance(v, np.ndarray) else v) for k, v in rec.items()}, 4.0, first_spp=5)
    for k in IMAGES:
        np.testing.assert_array_equal(bits(whole[k]), bits(part[k]), err_msg=k)
        np.testing.assert_array_equal(bits(whole[k]), bits(again[k]), err_msg=k)


def test_sun_is_zero_exactly_where_alpha_is_one_with_the_flag_off():
    port = binding.port()
    sc = gs.make("outdoor_nosun")
    rec = occlusion_records(port, sc, SEEDS, GIDS)
    assert not rec["sun"] and not rec["sun_hit"].any()
    img = fold_occlusion(rec, 4.0)
    alpha = rec["hit"].astype(np.float32).mean(axis=0)   # (coverage over three passes: 0, 1/3, 2/3 or 1)
    np.testing.assert_array_equal(img["sun"] == 0, alpha == 1)
    assert (alpha == 1).any() and (alpha == 0).any()
    assert (img["sun"][alpha == 0] == 1).all()
    # the flag on changes the bounce's draws: the sun sample takes two first
    on = records("outdoor")
    both = rec["hit"][0] & rec["b_hit"][0] & on["b_hit"][0]
    assert both.any() and (bits(rec["b_distance"][0][both]) != bits(on["b_distance"][0][both])).any()


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun"])
def test_ao_is_non_increasing_in_the_radius(name):
    rec = records(name)
    before = None
    for radius in RADII:
        ao = fold_occlusion(rec, radius)["ao"]
        v_ao, _ = sample_values(rec, radius)
        if before is not None:
            assert (v_ao <= before[0]).all() and (ao <= before[1]).all(), radius
        before = (v_ao, ao)
    at_inf, _ = sample_values(rec, np.inf)
    np.testing.assert_array_equal(at_inf == 0, rec["hit"] & rec["b_hit"] & ~np.isnan(rec["b_distance"]))


def test_nan_and_negative_distances_follow_the_one_compare():
    rec = {"sun": False, "hit": np.ones((1, 4), bool), "sun_hit": np.zeros((1, 4), bool), "b_hit": np.array([[True, True, True, False]]),
           "b_distance": np.array([[np.nan, -1e-4, 4.0, 1.0]], np.float32), "b_normal": np.zeros((1, 4, 3), np.float32)}
    v_ao, v_sun = sample_values(rec, 4.0)
    assert v_ao.tolist() == [[1.0, 0.0, 1.0, 1.0]]   # NaN clear, negative occluded, the radius itself clear (strict), no hit clear
    assert v_sun.tolist() == [[0.0] * 4]
    assert sample_values(rec, np.nextafter(np.float32(4.0), np.float32(np.inf)))[0].tolist() == [[1.0, 0.0, 0.0, 1.0]]


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun", "pregen"])
def test_both_sample_values_occur(name):
    """What the GPU tests lean on: among first-hit pixels of pass 0, SUN and AO at radius 4 each take both values."""
    rec = records(name, passes=1)
    hit = rec["hit"][0]
    v_ao, v_sun = sample_values(rec, 4.0)
    assert rec["sun"] and hit.any()
    assert set(v_sun[0][hit].tolist()) == {0.0, 1.0}, name
    assert set(v_ao[0][hit].tolist()) == {0.0, 1.0}, name
    # the bounce rays are not all short: some hit beyond the radius, so the compare decides something
    far = hit & rec["b_hit"][0] & (rec["b_distance"][0] >= 4)
    assert far.any(), name


def test_measured_counts_of_the_golden_subset():
    """Pass 0, every 7th gid, on the C restatement: SUN clear / first hits, bounce hits (of those nearer than 4)."""
    want = {"outdoor": (108, 265, 120, 103), "entities": (99, 362, 302, 262), "indoor_sun": (55, 439, 439, 58), "pregen": (48, 113, 48, 45)}
    for name, counts in want.items():
        rec = records(name, passes=1)
        hit, b = rec["hit"][0], rec["hit"][0] & rec["b_hit"][0]
        got = (int((hit & ~rec["sun_hit"][0]).sum()), int(hit.sum()), int(b.sum()), int((b & (rec["b_distance"][0] < 4)).sum()))
        assert got == counts, (name, got)
