"""chunky_render_aov_passes_ex / _read_ex and chunky_filter_frame_alpha without a device: the header declares them and the library
exports them, NULL handles are errors, the specification in aov_ex_spec.py means the same on the C restatement (oracle/port.c) as on
the reference build, its albedo and normal are aov_spec's, and the alpha byte the kernel compiles equals the formula."""
import re

import numpy as np
import pytest

from oracle import binding

import golden_scenes as gs
from aov_ex_spec import IMAGES, alpha_byte, expected_aov_ex
from aov_spec import expected_aov
from chunkyclplugin_amd import native

EX_FUNCTIONS = ["chunky_render_aov_passes_ex", "chunky_render_aov_read_ex", "chunky_filter_frame_alpha", "chunky_filter_alpha_bytes"]
GIDS = np.arange(5, gs.W * gs.H, 97, dtype=np.int32)  # 32 pixels from sky to foreground (tests/test_aov_cpu.py)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def boundary_values():
    """0, 1, 0.5, the floats around a few byte boundaries ((k - 0.5) / 255: where alpha * 255 + 0.5 reaches k), negatives, values
    above 1, infinities and NaNs."""
    vals = [0.0, -0.0, 1.0, 0.5]
    for k in (1, 2, 3, 64, 127, 128, 129, 200, 254, 255):
        f = np.float32((k - 0.5) / 255.0)
        vals += [np.nextafter(f, np.float32(-1)), f, np.nextafter(f, np.float32(2))]
    vals += [np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), 1.5, 2.0, 1e30, np.inf]
    vals += [-1e-30, -0.25, -1.0, -3e38, -np.inf, 1e-45, 1e-30, np.nan, -np.nan]
    out = np.array(vals, np.float32)
    return np.concatenate([out, np.array([0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32).view(np.float32)])   # more NaN payloads


def test_header_declares_and_library_exports_the_entry_points():
    text = open(native.HEADER).read()
    for name, value in (("ALPHA", 2), ("DEPTH", 3), ("POSITION", 4), ("EMITTANCE", 5), ("BLOCK", 6)):
        assert re.search(rf"#define\s+CHUNKY_AOV_{name}\s+{value}\b", text), name
        assert getattr(native, "AOV_" + name) == value
    assert native.AOV_WORDS == {0: 3, 1: 3, 2: 1, 3: 1, 4: 3, 5: 1, 6: 1}
    declared = native.declared_symbols()
    L = native.lib()
    for name in EX_FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name


def test_null_handles_are_errors():
    L = native.lib()
    seeds = np.zeros(2, np.int32)
    out = np.zeros(12, np.float32)
    assert L.chunky_render_aov_passes_ex(None, seeds.ctypes.data, 2, 0) == native.E_INVALID
    assert L.chunky_render_aov_read_ex(None, native.AOV_DEPTH, out.ctypes.data, out.size) == native.E_INVALID
    assert b"NULL" in L.chunky_last_error()
    assert L.chunky_render_aov_passes_ex(None, seeds.ctypes.data, -1, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes_ex(None, None, 2, 0) == native.E_INVALID
    assert L.chunky_render_aov_passes_ex(None, seeds.ctypes.data, 2, -1) == native.E_INVALID
    x = np.zeros(3, np.float64)
    a = np.zeros(1, np.float32)
    argb = np.zeros(1, np.int32)
    assert L.chunky_filter_frame_alpha(None, 1, 1, 1.0, x.ctypes.data, a.ctypes.data, argb.ctypes.data, 0) == native.E_INVALID


@pytest.mark.parametrize("name", gs.NAMES)
def test_port_spec_is_the_reference_spec(name):
    ref = binding.ref()
    if ref is None:
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    h = binding.SceneHandle(gs.make(name))
    seeds = native.java_random_ints(3)
    on_port = expected_aov_ex(binding.port(), h, seeds, GIDS)
    on_ref = expected_aov_ex(ref, h, seeds, GIDS)
    for k in IMAGES:
        np.testing.assert_array_equal(bits(on_port[k]), bits(on_ref[k]), err_msg=k)
    assert on_port["alpha"].max() > 0, "no sample of these pixels hits anything"


@pytest.mark.parametrize("name", ["outdoor", "entities", "pregen", "indoor"])
def test_albedo_and_normal_are_the_aov_specs(name):
    port = binding.port()
    h = binding.SceneHandle(gs.make(name))
    seeds = native.java_random_ints(3)
    ex = expected_aov_ex(port, h, seeds, GIDS, first_spp=2)
    albedo, normal = expected_aov(port, h, seeds, GIDS, first_spp=2)
    np.testing.assert_array_equal(bits(ex["albedo"]), bits(albedo))
    np.testing.assert_array_equal(bits(ex["normal"]), bits(normal))


@pytest.mark.parametrize("name", ["outdoor", "entities", "indoor"])
def test_spec_values(name):
    """One pass: a hit has alpha 1, a positive distance, the point o + d * (distance - OFFSET) of its ray's record and a block id >= 0;
    a miss alpha 0, depth 0, position 0, emittance 0 and block -1."""
    port = binding.port()
    h = binding.SceneHandle(gs.make(name))
    seed = int(native.java_random_ints(1)[0])
    gids = np.arange(0, gs.W * gs.H, 13, dtype=np.int32)
    img = expected_aov_ex(port, h, [seed], gids)
    hit = img["alpha"][:, 0] == 1
    assert hit.any() and ((img["alpha"][:, 0] == 0) | hit).all()
    assert (img["depth"][hit] > 0).all() and np.isfinite(img["depth"]).all() and np.isfinite(img["position"]).all()
    assert (img["block"][hit] >= 0).all() and (img["emittance"] >= 0).all()
    for k in ("depth", "position", "emittance", "normal"):
        assert not img[k][~hit].any(), k
    assert (img["block"][~hit] == -1).all()
    for i in np.flatnonzero(hit)[:8]:
        rec = port.trace_records(h, seed, int(gids[i]))[0][0]
        np.testing.assert_array_equal(bits(img["position"][i]), bits(np.asarray(rec["point"], np.float32)))
        assert bits(img["depth"][i])[0] == bits(np.float32(rec["distance"]))
        assert img["block"][i, 0] == rec["material"]


def test_fold_is_invariant_to_the_launch_cut_and_block_is_the_last_pass():
    """300 passes folded at once equal 256 and then 44 more from bufferSpp 256; the block id is pass 299's alone."""
    port = binding.port()
    h = binding.SceneHandle(gs.make("outdoor"))
    seeds = native.java_random_ints(300)
    gids = np.array([0, 777, 1555, 2333, 3071], np.int32)
    whole = expected_aov_ex(port, h, seeds, gids)
    part = expected_aov_ex(port, h, seeds[:256], gids)
    part = expected_aov_ex(port, h, seeds[256:], gids, first_spp=256, init=part)
    for k in IMAGES:
        np.testing.assert_array_equal(bits(whole[k]), bits(part[k]), err_msg=k)
    last = expected_aov_ex(port, h, seeds[299:], gids, first_spp=299)
    np.testing.assert_array_equal(whole["block"], last["block"])


def test_alpha_byte_rule():
    vals = boundary_values()
    want = alpha_byte(vals)
    got = native.filter_alpha_bytes(vals)
    np.testing.assert_array_equal(got.astype(np.uint32), want)
    # the formula's own landmarks: 0 -> 0, 1 -> 255, 0.5 -> (uint)128.0 = 128, negatives and NaN -> 0, above 1 -> 255
    assert want[0] == 0 and want[1] == 0 and want[2] == 255 and want[3] == 128
    assert (want[np.isnan(vals)] == 0).all() and np.isnan(vals).sum() == 5
    assert (want[vals < 0] == 0).all() and (want[vals > 1] == 255).all()
    # the three floats around (k - 0.5) / 255 give k - 1 or k, in order (which side each falls on is the two float roundings'
    # business: the library has to agree with the formula, above), and a little further out the byte is certain
    for j, k in enumerate((1, 2, 3, 64, 127, 128, 129, 200, 254, 255)):
        trio = want[4 + 3 * j:7 + 3 * j]
        assert set(trio) <= {k - 1, k} and trio[0] <= trio[1] <= trio[2], (k, trio)
        f = np.float32((k - 0.5) / 255.0)
        around = np.array([f - np.float32(1e-4), f + np.float32(1e-4)], np.float32)
        assert alpha_byte(around).tolist() == [k - 1, k] and native.filter_alpha_bytes(around).tolist() == [k - 1, k]
    # monotone over a dense sweep of [0, 1], and onto 0 .. 255
    sweep = np.linspace(0, 1, 100001).astype(np.float32)
    b = native.filter_alpha_bytes(sweep)
    np.testing.assert_array_equal(b.astype(np.uint32), alpha_byte(sweep))
    assert (np.diff(b) >= 0).all() and set(np.unique(b)) == set(range(256))
