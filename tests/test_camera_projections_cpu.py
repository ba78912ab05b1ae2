"""Projected cameras (projector types 1-5, include/chunky_hip.h) on the host: chunky_camera_rays against an
independent float64 restatement of the specification, analytic properties of each projection, the jitter stream against the
reference RNG, validation, and the reference build rendering the equivalent ray tables.  No device needed."""
import math

import numpy as np
import pytest

import golden_scenes as gs
from chunkyclplugin_amd import native, octree2, renderer
from oracle import binding

TYPES = [native.PROJ_PARALLEL, native.PROJ_FISHEYE, native.PROJ_PANORAMIC, native.PROJ_PANORAMIC_SLOT, native.PROJ_STEREOGRAPHIC]
SIZES = [(64, 48), (33, 17)]
SEEDS = [0, 1, -1155484576, 2147483647]
KEY = 0x9E3779B9


def rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return ry @ rx @ rz


def settings_for(kind, pos=(3.5, 70.25, -12.0), m=None, s13=None, s14=None):
    m = rotation(0.7, 1.1, 0.2) if m is None else np.asarray(m, np.float64)
    default = {native.PROJ_PARALLEL: (12.5, 30.0), native.PROJ_FISHEYE: (0.0, 180.0), native.PROJ_PANORAMIC: (0.0, 200.0),
               native.PROJ_PANORAMIC_SLOT: (2.0 * math.tan(math.radians(35.0)), 120.0),
               native.PROJ_STEREOGRAPHIC: (0.0, 2.0 * math.tan(math.radians(150.0) / 4.0))}[kind]
    s13 = default[0] if s13 is None else s13
    s14 = default[1] if s14 is None else s14
    return np.concatenate([np.asarray(pos, np.float64), m.reshape(-1), [0.0, s13, s14]]).astype(np.float32)


def pcg_next(s):
    """K/randomness.h Random_nextState on uint32 numpy arrays."""
    s = (s * np.uint32(47796405) + np.uint32(2891336453)).astype(np.uint32)
    s = (((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)).astype(np.uint32)
    return ((s >> np.uint32(22)) ^ s).astype(np.uint32)


def jitter(seed, n):
    j = (np.uint32(np.int64(seed) & 0xFFFFFFFF) ^ np.uint32(KEY)) + np.arange(n, dtype=np.uint32)
    j = pcg_next(j.astype(np.uint32))
    ox = (j >> np.uint32(8)).astype(np.float64) / 16777216.0
    j = pcg_next(j)
    oy = (j >> np.uint32(8)).astype(np.float64) / 16777216.0
    return ox, oy


def image_xy(seed, width, height):
    """x, y of every pixel in float64 (the float32 constants of set_camera)."""
    n = width * height
    ox, oy = jitter(seed, n)
    px, py = np.arange(n) % width, np.arange(n) // width
    hw, ih = float(np.float32(width / (2.0 * height))), float(np.float32(1.0 / height))
    return -hw + (px + ox) * ih, -0.5 + (py + oy) * ih


def restated_rays(kind, s, width, height, seed):
    """The specification in float64, independent of camera_proj.h."""
    s = np.asarray(s, np.float64)
    x, y = image_xy(seed, width, height)
    n = x.size
    o = np.zeros((n, 3))
    s13, s14 = s[13], s[14]
    rad = math.pi / 180.0
    if kind == native.PROJ_PARALLEL:
        o = np.stack([s14 * x, s14 * y, np.full(n, -s13)], 1)
        d = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif kind == native.PROJ_FISHEYE:
        ax, ay = x * s14 * rad, y * s14 * rad
        a = np.sqrt(ax * ax + ay * ay)
        safe = np.where(a == 0, 1.0, a)
        d = np.where((a == 0)[:, None], [0.0, 0.0, 1.0], np.stack([np.sin(a) * ax / safe, np.sin(a) * ay / safe, np.cos(a)], 1))
    elif kind == native.PROJ_PANORAMIC:
        ax, ay = x * s14 * rad, y * s14 * rad
        d = np.stack([np.cos(ay) * np.sin(ax), np.sin(ay), np.cos(ay) * np.cos(ax)], 1)
    elif kind == native.PROJ_PANORAMIC_SLOT:
        ax = x * s14 * rad
        d = np.stack([np.sin(ax), s13 * y, np.cos(ax)], 1)
    else:
        X, Y = s14 * x, s14 * y
        r2 = X * X + Y * Y
        d = np.stack([2 * X, 2 * Y, 1 - r2], 1) / (1 + r2)[:, None]
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    m = s[3:12].reshape(3, 3)
    return o @ m.T + s[:3], d @ m.T


@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("kind", TYPES)
def test_host_table_matches_the_float64_restatement(kind, width, height):
    s = settings_for(kind)
    for seed in SEEDS:
        got = renderer.camera_rays(kind, s, width, height, seed).reshape(-1, 6).astype(np.float64)
        o, d = restated_rays(kind, s, width, height, seed)
        scale_o = max(1.0, float(np.abs(o).max()))
        np.testing.assert_allclose(got[:, :3], o, rtol=1e-5, atol=1e-5 * scale_o)
        np.testing.assert_allclose(got[:, 3:], d, rtol=1e-5, atol=1e-5)


def local_rays(kind, s14, s13=0.0, width=64, height=48, seed=77):
    s = settings_for(kind, pos=(0.0, 0.0, 0.0), m=np.eye(3), s13=s13, s14=s14)
    t = renderer.camera_rays(kind, s, width, height, seed).reshape(-1, 6).astype(np.float64)
    x, y = image_xy(seed, width, height)
    return t[:, :3], t[:, 3:], x, y


def test_fisheye_angle_to_the_axis_is_fov_times_the_radius():
    for fov in (90.0, 180.0, 210.0):   # (corner radius 0.83: every angle below pi)
        _, d, x, y = local_rays(native.PROJ_FISHEYE, fov)
        angle = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2])
        np.testing.assert_allclose(angle, np.radians(fov * np.hypot(x, y)), atol=2e-6)


def test_panoramic_yaw_and_pitch_are_linear_in_x_and_y():
    for fov in (60.0, 160.0):
        _, d, x, y = local_rays(native.PROJ_PANORAMIC, fov)
        np.testing.assert_allclose(np.arctan2(d[:, 0], d[:, 2]), np.radians(fov * x), atol=2e-6)
        np.testing.assert_allclose(np.arcsin(np.clip(d[:, 1], -1, 1)), np.radians(fov * y), atol=2e-5)


def test_parallel_directions_are_equal_and_origins_lie_on_a_plane():
    s = settings_for(native.PROJ_PARALLEL)
    t = renderer.camera_rays(native.PROJ_PARALLEL, s, 64, 48, 5).reshape(-1, 6)
    assert (t[:, 3:].view(np.uint32) == t[0, 3:].view(np.uint32)).all()
    axis = s[3:12].reshape(3, 3).astype(np.float64) @ [0.0, 0.0, 1.0]
    np.testing.assert_allclose(t[0, 3:], axis, atol=1e-6)
    height = (t[:, :3].astype(np.float64) - s[:3]) @ axis
    np.testing.assert_allclose(height, -12.5, atol=1e-4)   # the back-off b, along the view axis
    assert np.ptp(t[:, 0]) > 1.0 and np.ptp(t[:, 1]) > 1.0   # and spread across it


@pytest.mark.parametrize("kind", TYPES)
def test_every_direction_is_unit_length(kind):
    for width, height in SIZES:
        d = renderer.camera_rays(kind, settings_for(kind), width, height, 123).reshape(-1, 6)[:, 3:].astype(np.float64)
        np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)


def test_jitter_stream_is_the_pcg_of_the_seed_key():
    """x, y of a parallel camera with w = 1 at the origin are the jitter itself: (seed ^ 0x9E3779B9) + gid, two draws."""
    width, height = 33, 17
    s = settings_for(native.PROJ_PARALLEL, pos=(0, 0, 0), m=np.eye(3), s13=0.0, s14=1.0)
    for seed in SEEDS:
        t = renderer.camera_rays(native.PROJ_PARALLEL, s, width, height, seed).reshape(-1, 6)
        n = width * height
        ox, oy = jitter(seed, n)
        px, py = np.arange(n) % width, np.arange(n) // width
        hw, ih = np.float32(width / (2.0 * height)), np.float32(1.0 / height)
        x = -hw + (px.astype(np.float32) + ox.astype(np.float32)) * ih
        y = (-0.5 + ((py.astype(np.float32) + oy.astype(np.float32)) * ih).astype(np.float64)).astype(np.float32)
        np.testing.assert_array_equal(t[:, 0], x)
        np.testing.assert_array_equal(t[:, 1], y)


def test_jitter_draws_equal_the_reference_rng(ref):
    for seed in SEEDS:
        for gid in (0, 1, 2021, 1920 * 1080 - 1):
            state = ((seed & 0xFFFFFFFF) ^ KEY) + gid
            _, f = ref.pcg_stream(state & 0xFFFFFFFF, 2)
            ox, oy = jitter(seed, gid + 1)
            assert (f[0], f[1]) == (np.float32(ox[gid]), np.float32(oy[gid]))


def test_invalid_settings_are_rejected():
    s = settings_for(native.PROJ_FISHEYE)

    def rejected(kind, settings, width=16, height=8):
        with pytest.raises(native.ChunkyHipError) as e:
            renderer.camera_rays(kind, settings, width, height, 1)
        assert e.value.code == native.E_INVALID

    for kind in TYPES:
        bad = settings_for(kind)
        bad[12] = 0.05
        rejected(kind, bad)                      # aperture: depth of field stays pinhole-only
        for fov in (0.0, -30.0):
            bad = settings_for(kind)
            bad[14] = fov
            rejected(kind, bad)                  # settings[14] <= 0
        for i in (0, 5, 13, 14):
            bad = settings_for(kind)
            bad[i] = np.nan
            rejected(kind, bad)
        bad = settings_for(kind)
        bad[2] = np.inf
        rejected(kind, bad)
        rejected(kind, settings_for(kind)[:14])  # a wrong length
        rejected(kind, np.concatenate([settings_for(kind), [0.0]]))
        rejected(kind, settings_for(kind), width=0)
    for kind in (native.PROJ_FISHEYE, native.PROJ_PANORAMIC, native.PROJ_STEREOGRAPHIC):
        bad = settings_for(kind)
        bad[13] = 1.0
        rejected(kind, bad)                      # settings[13] must be 0 for these
    for kind in (native.PROJ_PINHOLE, native.PROJ_PREGENERATED, 6, -2):
        rejected(kind, s)
    rejected(native.PROJ_PANORAMIC, np.zeros(15, np.float32))   # the zeros test_gpu_parity's edge case hands set_camera(3, ...)


def test_camera_settings_maps_chunky_projection_modes():
    cam = {"position": {"x": 10.0, "y": 80.0, "z": -4.0}, "orientation": {"yaw": 0.4, "pitch": -1.3, "roll": 0.0}, "fov": 120.0}
    kind, s = octree2.camera_settings(cam, (2.0, 0.0, 0.0))
    assert kind == 0 and np.array_equal(s, octree2.camera_from_json(cam, (2.0, 0.0, 0.0)))
    for mode, want in (("PARALLEL", 1), ("FISHEYE", 2), ("PANORAMIC", 3), ("PANORAMIC_SLOT", 4), ("STEREOGRAPHIC", 5)):
        kind, s = octree2.camera_settings(dict(cam, projectionMode=mode), (2.0, 0.0, 0.0), world_width=512.0)
        assert kind == want and s.dtype == np.float32 and s.size == 15
        np.testing.assert_array_equal(s[:12], octree2.camera_from_json(cam, (2.0, 0.0, 0.0))[:12])
        assert s[12] == 0.0
        renderer.camera_rays(kind, s, 8, 4, 0)   # accepted as it is
    assert octree2.camera_settings(dict(cam, projectionMode="PARALLEL"), world_width=512.0)[1][13] == 512.0
    assert octree2.camera_settings(dict(cam, projectionMode="PANORAMIC_SLOT"))[1][13] == np.float32(2.0 * math.tan(math.radians(60.0)))
    for mode in ("ODS", "ODS_STACKED", "SOMETHING_NEW"):
        assert octree2.camera_settings(dict(cam, projectionMode=mode)) == (-1, None)
    assert octree2.camera_settings(dict(cam, projectionMode="FISHEYE", dof=40.0)) == (-1, None)   # depth of field off pinhole
    assert octree2.camera_settings(dict(cam, projectionMode="PINHOLE", dof=40.0))[0] == 0


@pytest.mark.parametrize("kind", TYPES)
def test_reference_build_renders_the_equivalent_tables(ref, kind):
    """The equivalence's right-hand side exists: the reference kernel on projector type -1 fed R_k(s) gives a finite image that
    changes with s (fresh jitter every pass)."""
    import dataclasses
    sc = gs.make("outdoor")
    s = sc.camera[:15].copy()
    s[12:15] = settings_for(kind)[12:15]
    if kind == native.PROJ_PARALLEL:
        s[13], s[14] = 20.0, 40.0
    imgs = []
    for seed in (11, 12):
        rays = renderer.camera_rays(kind, s, sc.width, sc.height, seed)
        view = dataclasses.replace(sc, camera=rays, projector_type=-1)
        imgs.append(ref.render_passes(binding.SceneHandle(view), np.array([seed], np.int32), threads=binding.usable_threads()))
    assert all(np.isfinite(im).all() and im.max() > 0 for im in imgs)
    assert not np.array_equal(imgs[0], imgs[1])
