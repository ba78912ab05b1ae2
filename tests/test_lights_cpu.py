"""chunky_render_light_passes without a device: the header declares the calls and the library exports them, NULL handles and bad
arguments are errors, and the specification in lights_spec.py — a group image is the oracle's image with the other two scalars at zero
— has the properties the GPU tests and the documentation lean on: ALL is the untouched image, the restatement and the reference build
agree on it, every group is non-trivial where its light exists and zero where it does not, the groups sum to ALL to rounding, and a
doubled scalar doubles its group bit for bit."""
import dataclasses
import re

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from lights_spec import IMAGES, WHICH, expected_lights, group_scene
from chunkyclplugin_amd import native
from chunkyclplugin_amd.scenes import f2i

FUNCTIONS = ["chunky_render_light_passes", "chunky_render_light_read", "chunky_render_light_mix", "chunky_render_light_reset",
             "chunky_render_light_kernel_time", "chunky_render_light_kernel_info"]
SEEDS = native.java_random_ints(3)
MAX_DEPTH = 5
_images = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lights(name, passes=1):
    """the four images of a golden scene on the port after `passes` passes, computed once and never changed"""
    if (name, passes) not in _images:
        img = expected_lights(binding.port(), gs.make(name), SEEDS[:passes])
        for v in img.values():
            v.setflags(write=False)
        _images[name, passes] = img
    return _images[name, passes]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(native.HEADER).read()
    for name, value in (("SKY", 0), ("SUN", 1), ("EMITTERS", 2), ("ALL", 3)):
        assert re.search(rf"#define\s+CHUNKY_LIGHT_{name}\s+{value}\b", text), name
        assert getattr(native, "LIGHT_" + name) == value
    declared = native.declared_symbols()
    L = native.lib()
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    for src in ("lights.hip", "capi_lights.hip"):
        assert src in native.SOURCES


def test_null_handles_and_bad_arguments_are_errors():
    L = native.lib()
    seeds = np.zeros(2, np.int32)
    out = np.zeros(12, np.float32)
    info = np.zeros(4, np.int32)
    w = np.ones(3, np.float32)
    assert L.chunky_render_light_passes(None, seeds.ctypes.data, 2, 0) == native.E_INVALID
    assert b"NULL" in L.chunky_last_error()
    assert L.chunky_render_light_passes(None, seeds.ctypes.data, -1, 0) == native.E_INVALID
    assert b"bad arguments" in L.chunky_last_error()
    assert L.chunky_render_light_passes(None, None, 2, 0) == native.E_INVALID
    assert L.chunky_render_light_passes(None, seeds.ctypes.data, 2, -1) == native.E_INVALID
    for which in (native.LIGHT_SKY, native.LIGHT_ALL, -1, 4):
        assert L.chunky_render_light_read(None, which, out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_light_read(None, native.LIGHT_SKY, None, 0) == native.E_INVALID
    assert L.chunky_render_light_mix(None, w.ctypes.data, out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_light_mix(None, None, out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_light_reset(None) == native.E_INVALID
    assert L.chunky_render_light_kernel_info(None, info.ctypes.data) == native.E_INVALID
    assert L.chunky_render_light_kernel_time(None, None, None) == native.E_INVALID


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun"])
def test_all_is_the_untouched_image(name):
    port = binding.port()
    sc = gs.make(name)
    same = group_scene(sc, "all", 13.0)
    assert same[1] == 13.0 and same[0].sky_intensity == sc.sky_intensity and (np.asarray(same[0].sun) == np.asarray(sc.sun)).all()
    np.testing.assert_array_equal(bits(lights(name, 3)["all"]), bits(port.render_passes(sc, SEEDS)))


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun"])
def test_port_spec_is_the_reference_spec(name):
    """EMITTERS and ALL need no option the reference build lacks: its emitter scale is the fixed 13."""
    ref = binding.ref()
    if ref is None:
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    sc = gs.make(name)
    for g in ("emitters", "all"):
        scene, scale = group_scene(sc, g, 13.0)
        assert scale == 13.0
        np.testing.assert_array_equal(bits(lights(name, 3)[g]), bits(ref.render_passes(scene, SEEDS)), err_msg=g)


# non-zero channel values of (sky, sun, emitters) among the 64 * 48 * 3 of pass 0, measured on the C restatement
NONZERO = {"outdoor": (9135, 3810, 315), "indoor_sun": (6276, 6276, 1017), "entities": (7848, 5223, 2250), "water": (9078, 3609, 366)}


@pytest.mark.parametrize("name", sorted(NONZERO))
def test_every_group_has_light(name):
    img = lights(name)
    got = tuple(int(np.count_nonzero(img[g])) for g in ("sky", "sun", "emitters"))
    assert min(got) > 0, (name, got)
    assert got == NONZERO[name], (name, got)
    for g in IMAGES:
        assert np.isfinite(img[g]).all() and (img[g] >= 0).all(), g


def test_sun_is_all_zero_with_the_flag_off():
    img = lights("outdoor_nosun", 3)
    assert not bits(img["sun"]).any()
    assert img["sky"].any() and img["emitters"].any()


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor_sun", "water"])
def test_groups_sum_to_all_within_the_rounding_bound(name):
    """One pass, first_spp 0: every term is non-negative; a group's sum and the reference's sum take at most 2 * max_depth + 1
    additions each, recombining takes two more: |SKY + SUN + EMITTERS - ALL| <= 4 * (2 * max_depth + 3) * 2^-24 * ALL per float."""
    img = lights(name)
    total = (img["sky"].astype(np.float64) + img["sun"]) + img["emitters"]
    bound = 4 * (2 * MAX_DEPTH + 3) * 2.0 ** -24
    err = np.abs(total - img["all"].astype(np.float64))
    worst = float((err / np.maximum(img["all"], np.float32(1e-30))).max())
    print(f"{name}: worst relative error {worst:.3g} (bound {bound:.3g})")
    assert (err <= bound * img["all"].astype(np.float64)).all(), worst


def test_a_doubled_scalar_doubles_its_group():
    port = binding.port()
    sc = gs.make("outdoor")
    base = lights("outdoor", 3)
    sun = np.array(sc.sun, np.int32)
    sun[3] = f2i(float(np.float32(2) * np.array([sc.sun[3]], np.int32).view(np.float32)[0]))
    doubled = {"sky": (dataclasses.replace(sc, sky_intensity=2 * sc.sky_intensity), 13.0), "sun": (dataclasses.replace(sc, sun=sun), 13.0),
               "emitters": (sc, 26.0)}
    for g, (scene, scale) in doubled.items():
        got = expected_lights(port, scene, SEEDS, emitter_scale=scale, groups=(g,))[g]
        assert base[g].any()
        np.testing.assert_array_equal(bits(got), bits(base[g] * np.float32(2)), err_msg=g)


def test_which_follows_the_table():
    assert [WHICH[g] for g in IMAGES] == [0, 1, 2, 3]
