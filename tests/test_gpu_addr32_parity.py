"""render_pool's plain, sorted and proj:: instantiations read the atlas, the sky and the box and quad records as a scalar base +
a 32-bit byte offset (csrc/rt_device.hpp load_at; csrc/addr32.h).  On the world of tests/addr32_scenes.py — an 80 x 48 x 4 atlas whose
last tile (last column, row and layer) is a colour and an emittance texture, model blocks of five boxes and five quads, a 96 x 72 sky,
a view into the sun disc — every kernel form gives oracle/port.c's image, 33 x 17 pixels and 4 passes, bit for bit (and the reference
build's, where it is built), and kernel_info says which kernel that was.

Every case runs a second time with the 64-bit path forced: a child process on the -DCHUNKY_TUNING build with CHUNKY_ADDR32_MASK=0,
which makes the scene's word (chunky_scene_addr32) say what it says for a scene too large for 32-bit offsets.  Which form a kernel has
is fixed when it is compiled — there is no branch inside it — so the library then has to start kernels that have the 64-bit forms
(the fallback kernels) for the same image; the test asserts that it does.

The AOV kernel and the fallback kernels keep the 64-bit forms in every build: their cases pin that the shared device code still
renders this world."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import addr32_scenes as a32
from aov_spec import expected_aov
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import camera_rays
from oracle import binding

pytestmark = pytest.mark.gpu
THREADS = binding.usable_threads()
SEEDS = scenes.java_random_ints(a32.N_PASSES)
ALL = np.arange(a32.W * a32.H, dtype=np.int32)
EVERY = native.ADDR32_ATLAS | native.ADDR32_SKY | native.ADDR32_RECORDS
_ORACLE = {}


def oracle_image(view, tracer=None, which="port"):
    """the oracle's image of a view: computed once, shared, read-only"""
    if (view, which) not in _ORACLE:
        tracer = tracer or binding.port()
        sc = a32.scene(view)
        if sc.projector_type <= 0:
            img = tracer.render_passes(sc, SEEDS, threads=THREADS)
        else:   # a projected camera is, pass by pass, the table of its rays (tests/test_gpu_camera_projections.py)
            img = np.zeros(3 * len(ALL), np.float32)
            for i, seed in enumerate(SEEDS):
                table = dataclasses.replace(sc, camera=camera_rays(sc.projector_type, sc.camera, a32.W, a32.H, int(seed)), projector_type=native.PROJ_PREGENERATED)
                tracer.render_passes(table, np.array([seed], np.int32), first_spp=i, res=img, threads=THREADS)
        img.setflags(write=False)
        _ORACLE[(view, which)] = img
    return _ORACLE[(view, which)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1, 3)


def assert_same(got, want, what):
    same = (bits(got) == bits(want)).all(axis=1)
    if not same.all():
        i = int(np.argmin(same))
        pytest.fail(f"{what}: {int((~same).sum())} of {len(same)} pixels differ from the oracle; first: pixel {i} got {bits(got)[i]!r} want {bits(want)[i]!r}")


def test_the_world_is_what_the_cases_need():
    sc, ramp = a32.world()
    layers, h, w, _ = sc.atlas.shape
    assert (w, h) == (80, 48) and layers >= 4
    assert ramp == ((a32.TILES_X - 1) << 22) | ((a32.TILES_Y - 1) << 13) | (layers - 1)      # the last tile of the last layer
    assert sc.atlas[layers - 1, -1, -1, 3] == 255 and sc.atlas[layers - 1, -16, -16, 3] == 0  # ... holds the ramp, its last texel in the array's last word
    assert sc.sky.shape[:2] == (72, 96)
    mats = np.asarray(sc.material_palette).reshape(-1, 6)
    assert ((mats[:, 0] & 2) != 0).any() and (mats[mats[:, 0] & 2 != 0, 4] == ramp).all()      # flags & 2: the emittance texel is the ramp's
    assert sc.aabb_models[0] == 5 and 5 in [int(sc.quad_models[0])]                            # >= 3 boxes / quads: record offsets beyond the first
    # the sun view looks into the disc: without the disc's texture the image is another
    sun = a32.scene("sun")
    no_disc = dataclasses.replace(sun, sun=scenes.pack_sun(a32.ALT, a32.AZI, a32.INTENSITY, False))
    lit = binding.port().render_passes(no_disc, SEEDS[:1], threads=THREADS)
    with_disc = binding.port().render_passes(sun, SEEDS[:1], threads=THREADS)
    assert (bits(lit) != bits(with_disc)).any(axis=1).sum() >= 20
    # ... and the exhibits view meets the last tile: an atlas whose last tile is blank renders another image
    blank = sc.atlas.copy()
    blank[layers - 1, -16:, -16:] = 0
    ex = a32.scene("exhibits")
    other = binding.port().render_passes(dataclasses.replace(ex, atlas=blank), SEEDS[:1], threads=THREADS)
    assert (bits(other) != bits(binding.port().render_passes(ex, SEEDS[:1], threads=THREADS))).any(axis=1).sum() >= 10


@pytest.mark.parametrize("name", list(a32.CASES))
def test_offsets_32(gpu_instance, name):
    view, _variant, want_info = a32.CASES[name]
    img, info, word = a32.render_case(gpu_instance, name, SEEDS)
    assert word == EVERY, word
    for k, v in want_info.items():
        assert (info[k] < 0) if (k == "pool" and v < 0) else (info[k] == v), (k, info)
    assert not info["bvh"] and not info["ext"], info
    assert_same(img, oracle_image(view), f"{name} against oracle/port.c")
    ref = binding.ref()
    if ref is not None:
        assert_same(img, oracle_image(view, ref, "ref"), f"{name} against the reference build")


def test_aov_kernel(gpu_instance):
    (albedo, normal), info = a32.render_aov(gpu_instance, SEEDS)
    assert info["tree"] == 17 and not info["bvh"], info
    want = expected_aov(binding.port(), binding.SceneHandle(a32.scene(a32.AOV_VIEW)), SEEDS, ALL)
    assert_same(albedo, want[0], "albedo")
    assert_same(normal, want[1], "normal")
    _ORACLE["aov"] = want


def test_every_case_with_64_bit_addresses_forced(tmp_path):
    """One child process for all cases (a library is bound once per process)."""
    out = str(tmp_path / "images.npz")
    env = dict(os.environ, CHUNKY_HIP_LIB=native.build_tuning(), CHUNKY_ADDR32_MASK="0")
    p = subprocess.run([sys.executable, os.path.join(a32.HERE, "addr32_scenes.py"), out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    said = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert said["library"] == "libchunky_hip_tuning.so", said
    images = np.load(out)
    for name, (view, _variant, _info) in a32.CASES.items():
        assert said["word"][name] == 0, said
        info = said["kernel"][name]
        assert info["pool"] < 0 and not info["sorted"], (name, info)   # no kernel with 32-bit forms ran: a fallback kernel did
        assert_same(images[name], oracle_image(view), f"{name}, 64-bit addresses forced")
    want = _ORACLE.get("aov") or expected_aov(binding.port(), binding.SceneHandle(a32.scene(a32.AOV_VIEW)), SEEDS, ALL)
    assert_same(images["aov_albedo"], want[0], "albedo, 64-bit addresses forced")
    assert_same(images["aov_normal"], want[1], "normal, 64-bit addresses forced")
