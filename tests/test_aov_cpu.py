"""The AOV entry points without a device: the header declares them and the library exports them, NULL handles are errors, and
the specification in aov_spec.py means the same on the C restatement (oracle/port.c) as on the reference build."""
import os
import re

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from aov_spec import expected_aov
from chunkyclplugin_amd import native

AOV_FUNCTIONS = ["chunky_render_aov_passes", "chunky_render_aov_read", "chunky_render_aov_reset", "chunky_render_aov_kernel_time",
                 "chunky_render_aov_kernel_info"]
GIDS = np.arange(5, gs.W * gs.H, 97, dtype=np.int32)  # 32 pixels from sky to foreground


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_header_declares_and_library_exports_the_aov_entry_points():
    text = open(native.HEADER).read()
    assert re.search(r"#define\s+CHUNKY_AOV_ALBEDO\s+0\b", text) and re.search(r"#define\s+CHUNKY_AOV_NORMAL\s+1\b", text)
    assert (native.AOV_ALBEDO, native.AOV_NORMAL) == (0, 1)
    declared = native.declared_symbols()
    L = native.lib()
    for name in AOV_FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.chunky_version().startswith(b"chunky-hip 0.6 ")


def test_null_handles_are_errors():
    L = native.lib()
    seeds = np.zeros(2, np.int32)
    out = np.zeros(12, np.float32)
    assert L.chunky_render_aov_passes(None, seeds.ctypes.data, 2, 0) == native.E_INVALID
    assert L.chunky_render_aov_read(None, native.AOV_ALBEDO, out.ctypes.data, out.size) == native.E_INVALID
    assert L.chunky_render_aov_reset(None) == native.E_INVALID
    assert L.chunky_render_aov_kernel_time(None, None, None) == native.E_INVALID
    assert L.chunky_render_aov_kernel_info(None, None) == native.E_INVALID
    assert b"NULL" in L.chunky_last_error()
    # bad counts fail before the handle is looked at
    assert L.chunky_render_aov_passes(None, seeds.ctypes.data, -1, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes(None, None, 2, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes(None, seeds.ctypes.data, 2, -1) == native.E_INVALID


@pytest.mark.parametrize("name", gs.NAMES)
def test_port_spec_is_the_reference_spec(name):
    ref = binding.ref()
    if ref is None:
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    h = binding.SceneHandle(gs.make(name))
    seeds = native.java_random_ints(3)
    a_port, n_port = expected_aov(binding.port(), h, seeds, GIDS)
    a_ref, n_ref = expected_aov(ref, h, seeds, GIDS)
    np.testing.assert_array_equal(bits(a_port), bits(a_ref))
    np.testing.assert_array_equal(bits(n_port), bits(n_ref))


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor"])
def test_spec_values(name):
    """What the images hold: normals of single-sample hits are unit vectors, misses leave the normal 0 and the albedo the sky."""
    port = binding.port()
    h = binding.SceneHandle(gs.make(name))
    seed = int(native.java_random_ints(1)[0])
    gids = np.arange(0, gs.W * gs.H, 13, dtype=np.int32)
    albedo, normal = expected_aov(port, h, [seed], gids)
    hits = np.array([bool(port.trace_records(h, seed, int(g))[0][0]["hit"]) for g in gids])
    assert hits.any()
    assert np.allclose(np.linalg.norm(normal[hits], axis=1), 1.0, atol=1e-5)
    assert (normal[~hits] == 0).all()
    assert np.isfinite(albedo).all() and (albedo >= 0).all()
    if (~hits).any():
        _, rad = port.trace_records(h, seed, int(gids[~hits][0]))
        np.testing.assert_array_equal(bits(albedo[~hits][0]), bits(rad))


def test_fold_is_invariant_to_the_launch_cut():
    """300 passes folded at once equal 256 and then 44 more from bufferSpp 256 (the cut of chunky_render_aov_passes)."""
    port = binding.port()
    h = binding.SceneHandle(gs.make("outdoor"))
    seeds = native.java_random_ints(300)
    gids = np.array([0, 777, 1555, 2333, 3071], np.int32)
    whole = expected_aov(port, h, seeds, gids)
    part = expected_aov(port, h, seeds[:256], gids)
    part = expected_aov(port, h, seeds[256:], gids, first_spp=256, init=part)
    np.testing.assert_array_equal(bits(whole[0]), bits(part[0]))
    np.testing.assert_array_equal(bits(whole[1]), bits(part[1]))
