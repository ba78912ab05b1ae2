"""Canvas windows (chunky_render_set_canvas, include/chunky_hip.h) without a device: the host twin of the
projected cameras on a window is the crop of the canvas's table, bit for bit; the device-free checker refuses what the header says
set_canvas refuses; and a stand-alone program (tests/sanitize/window_fuzz.cpp) holds the checker and the (g, px, py) -> (G, X, Y)
helper of csrc/canvas_window.h to 64-bit arithmetic under AddressSanitizer + UBSan.  Nothing is loaded into Python under a sanitizer."""
import json
import os
import subprocess

import numpy as np
import pytest

from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import camera_rays
from test_camera_lens_ods_cpu import LENS, TYPES, settings_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CW, CH = 64, 48   # the goldens' canvas
# (width, height, x0, y0): A = RAGGED_VIEW off the 16 x 16 and 2 x 2 grids, B the same flush with the right and bottom edges, C the
# last pixel, D the identity
WINDOWS = {"A": (33, 17, 19, 11), "B": (33, 17, 31, 31), "C": (1, 1, 63, 47), "D": (64, 48, 0, 0)}
SEEDS = [77, -1155484576]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def crop(image, window, words, cw=CW, ch=CH):
    """The window's pixels of a canvas image of `words` values per pixel, flat."""
    w, h, x0, y0 = window
    return np.ascontiguousarray(np.asarray(image).reshape(ch, cw, words)[y0:y0 + h, x0:x0 + w]).reshape(-1)


def canvas_gids(window, cw=CW):
    w, h, x0, y0 = window
    return ((y0 + np.arange(h))[:, None] * cw + x0 + np.arange(w)[None, :]).reshape(-1).astype(np.int32)


@pytest.mark.parametrize("lens", [None, LENS], ids=["no-lens", "lens"])
@pytest.mark.parametrize("kind", TYPES)
def test_window_table_is_the_crop_of_the_canvas_table(kind, lens):
    s = settings_for(kind)
    for seed in SEEDS:
        full = camera_rays(kind, s, CW, CH, seed, lens)
        for key in "ABC":
            w, h, x0, y0 = WINDOWS[key]
            got = native.camera_rays_window(kind, s, w, h, CW, CH, x0, y0, seed, lens)
            assert np.array_equal(bits(got), bits(crop(full, WINDOWS[key], 6))), (kind, lens, seed, key)
        # canvas == window: the bytes of chunky_camera_rays / chunky_camera_rays_lens
        assert np.array_equal(bits(native.camera_rays_window(kind, s, CW, CH, CW, CH, 0, 0, seed, lens)), bits(full)), (kind, lens, seed)


def test_stacked_ods_window_straddles_the_canvas_middle_not_its_own():
    """Rows 11 .. 27 of the 48-row canvas: the eye changes between the window's rows 12 and 13 (canvas rows 23 and 24), not at 17 / 2."""
    kind = native.PROJ_ODS_STACKED
    s = settings_for(kind)
    w, h, x0, y0 = WINDOWS["A"]
    t = native.camera_rays_window(kind, s, w, h, CW, CH, x0, y0, 5).reshape(h, w, 6)
    own = camera_rays(kind, s, w, h + 1, 5).reshape(h + 1, w, 6)   # (an even height of its own: its eye changes at row 9)
    assert np.array_equal(bits(t), bits(crop(camera_rays(kind, s, CW, CH, 5), WINDOWS["A"], 6)).reshape(h, w, 6))
    assert not np.array_equal(bits(t[:, :, :3]), bits(own[:h, :, :3]))


def test_the_helper_gives_the_canvas_pixel():
    for key, (w, h, x0, y0) in WINDOWS.items():
        gids = canvas_gids(WINDOWS[key])
        for g in sorted({0, w - 1, (h - 1) * w, w * h - 1, (h // 2) * w + w // 2}):
            G, X, Y = native.canvas_pixel(w, h, CW, CH, x0, y0, g)
            assert (G, X, Y) == (int(gids[g]), x0 + g % w, y0 + g // w), (key, g)
    assert native.canvas_pixel(8, 8, 40000, 40000, 39990, 39985, 63) == (39992 * 40000 + 39997, 39997, 39992)
    assert native.lib().chunky_selftest_canvas_pixel(8, 8, 64, 48, 0, 0, 64, native.ptr(np.zeros(3, np.int32))) == native.E_INVALID


def test_what_set_canvas_refuses():
    ok = native.canvas_check
    for w, h, x0, y0 in WINDOWS.values():
        assert ok(w, h, CW, CH, x0, y0) == 0
    assert ok(33, 17, CW, CH, -1, 11) == native.E_INVALID          # a negative offset
    assert ok(33, 17, CW, CH, 19, -1) == native.E_INVALID
    assert "negative offset" in native.lib().chunky_last_error().decode()
    assert ok(33, 17, CW, CH, 32, 31) == native.E_INVALID          # one column past the right edge
    assert ok(33, 17, CW, CH, 31, 32) == native.E_INVALID          # one row past the bottom edge
    assert "inside" in native.lib().chunky_last_error().decode()
    assert ok(65, 48, CW, CH, 0, 0) == native.E_INVALID            # a window larger than its canvas
    assert ok(33, 17, CW, CH, 2 ** 31 - 1, 0) == native.E_INVALID  # x0 + width leaves an int: refused, not wrapped
    assert ok(33, 17, 2 ** 31 - 1, 1, 0, 0) == native.E_INVALID    # (the window is taller than that canvas)
    assert ok(33, 1, 2 ** 31 - 1, 1, 2 ** 31 - 34, 0) == 0         # a canvas of exactly INT32_MAX pixels, its last window
    assert ok(33, 17, 0, CH, 0, 0) == native.E_INVALID and ok(33, 17, CW, -3, 0, 0) == native.E_INVALID
    # G is an int: 46340^2 = 2 147 395 600 fits, 46341^2 = 2 147 488 281 does not
    assert ok(8, 8, 46341, 46341, 0, 0) == native.E_INVALID
    assert "2^31" in native.lib().chunky_last_error().decode()
    assert ok(8, 8, 46340, 46340, 46332, 46332) == 0
    assert ok(8, 8, 65536, 32768, 0, 0) == native.E_INVALID        # 2^31 exactly
    # the stacked ODS image changes eye at canvas_height / 2: an even CANVAS height, whatever the window's
    assert ok(33, 17, CW, CH, 19, 11, native.PROJ_ODS_STACKED) == 0
    assert ok(33, 16, CW, CH - 1, 19, 11, native.PROJ_ODS_STACKED) == native.E_INVALID
    assert "even canvas height" in native.lib().chunky_last_error().decode()
    assert ok(33, 16, CW, CH - 1, 19, 11, native.PROJ_ODS) == 0


def test_the_window_table_refuses_what_the_checker_and_the_cameras_refuse():
    s = settings_for(native.PROJ_FISHEYE)
    with pytest.raises(native.ChunkyHipError) as e:
        native.camera_rays_window(native.PROJ_FISHEYE, s, 33, 17, CW, CH, 32, 11, 1)
    assert e.value.code == native.E_INVALID
    with pytest.raises(native.ChunkyHipError) as e:   # an odd canvas height under the stacked camera, an even window
        native.camera_rays_window(native.PROJ_ODS_STACKED, settings_for(native.PROJ_ODS_STACKED), 16, 16, CW, CH - 1, 0, 0, 1)
    assert e.value.code == native.E_INVALID
    with pytest.raises(native.ChunkyHipError) as e:   # types 0 and -1 have no table of this kind
        native.camera_rays_window(0, s, 33, 17, CW, CH, 19, 11, 1)
    assert e.value.code == native.E_INVALID
    with pytest.raises(native.ChunkyHipError) as e:
        native.camera_rays_window(native.PROJ_FISHEYE, s, 33, 17, CW, CH, 19, 11, 1, (-1.0, 2.0))
    assert e.value.code == native.E_INVALID


def test_the_new_calls_are_declared_and_exported():
    names = {"chunky_render_set_canvas", "chunky_render_canvas", "chunky_camera_rays_window", "chunky_canvas_check", "chunky_selftest_canvas_pixel"}
    assert names <= set(native.declared_symbols())
    assert all(hasattr(native.lib(), n) for n in names)


def test_checker_and_helper_under_asan_ubsan(tmp_path):
    """The build step also holds canvas_host.cpp to its promise: plain C++, warnings as errors, no ROCm include path."""
    exe = str(tmp_path / "window_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-ffp-contract=off", os.path.join(ROOT, "tests", "sanitize", "window_fuzz.cpp"), os.path.join(native.CSRC, "canvas_host.cpp"),
           os.path.join(native.CSRC, "capi_error.cpp"), "-o", exe]
    assert not any("rocm" in a.lower() for a in cmd)
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-500:], proc.stderr[-3000:])
    out = json.loads(proc.stdout.strip().splitlines()[-1])
    assert out["failures"] == 0
    # of the 200 000 windows built to fit, only a stacked ODS camera (one type in six) on an odd canvas height is refused; nearly all
    # of the 200 000 with random and extreme arguments are; an accepted window of at most 2^30 pixels has 17 pixels compared
    assert out["accepted"] >= 160000 and out["refused"] >= 150000 and out["pixels"] >= 17 * 100000
