"""The lens (depth of field) of the projected cameras and the ODS projector types 7 / 8 (include/chunky_hip.h, DESIGN.md section 11,
"Lens and ODS") on the host: chunky_camera_rays_lens against an independent float64 restatement, the two new draws against the
reference RNG, analytic properties of the lens and of both ODS types, validation, the scene-JSON mapping, and the reference build
rendering the lens table.  No device needed.  The cameras the device tests render (tests/test_gpu_camera_lens_ods.py) are defined
here, so that the "not hollow" checks below are made on exactly those."""
import dataclasses
import math

import numpy as np
import pytest

import golden_scenes as gs
from chunkyclplugin_amd import native, octree2, renderer
from oracle import binding

OLD_TYPES = [native.PROJ_PARALLEL, native.PROJ_FISHEYE, native.PROJ_PANORAMIC, native.PROJ_PANORAMIC_SLOT, native.PROJ_STEREOGRAPHIC]
ODS_TYPES = [native.PROJ_ODS, native.PROJ_ODS_STACKED]
TYPES = OLD_TYPES + ODS_TYPES
SIZES = [(64, 48), (33, 17), (37, 22)]   # the sizes of test_camera_projections_cpu.py and a ragged one (stacked ODS: the height even)
SEEDS = [0, 1, -1155484576, 2147483647]
KEY = 0x9E3779B9
LENS = (0.35, 9.0)


def size_for(kind, width, height):
    return (width, height + 1) if kind == native.PROJ_ODS_STACKED and height % 2 else (width, height)


# ---- the cameras of the device tests ---------------------------------------------------------------------------------------------
GPU_LENS = {native.PROJ_PARALLEL: (0.6, 30.0), native.PROJ_FISHEYE: (0.4, 14.0), native.PROJ_PANORAMIC: (0.4, 14.0),
            native.PROJ_PANORAMIC_SLOT: (0.3, 10.0), native.PROJ_STEREOGRAPHIC: (0.5, 20.0), native.PROJ_ODS: (0.25, 8.0),
            native.PROJ_ODS_STACKED: (0.4, 14.0)}
GPU_S13_S14 = {native.PROJ_PARALLEL: (20.0, 48.0), native.PROJ_FISHEYE: (0.0, 180.0), native.PROJ_PANORAMIC: (0.0, 240.0),
               native.PROJ_PANORAMIC_SLOT: (2.0 * math.tan(math.radians(35.0)), 150.0),
               native.PROJ_STEREOGRAPHIC: (0.0, 2.0 * math.tan(math.radians(160.0) / 4.0)),
               native.PROJ_ODS: (-0.0345, 180.0), native.PROJ_ODS_STACKED: (0.0345, 180.0)}


def projected(sc, kind, s13_s14=None):
    """sc's pinhole camera (position and rotation) as projected camera `kind`, as the device tests set it."""
    base = np.asarray(sc.camera if sc.projector_type == 0 else gs.make("outdoor").camera, np.float32)[:15].copy()
    base[12] = 0.0
    base[13], base[14] = GPU_S13_S14[kind] if s13_s14 is None else s13_s14
    return dataclasses.replace(sc, camera=base, projector_type=kind)


# ---- the specification once more, in float64 -------------------------------------------------------------------------------------
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
               native.PROJ_STEREOGRAPHIC: (0.0, 2.0 * math.tan(math.radians(150.0) / 4.0)),
               native.PROJ_ODS: (-0.4, 180.0), native.PROJ_ODS_STACKED: (0.4, 150.0)}[kind]
    s13 = default[0] if s13 is None else s13
    s14 = default[1] if s14 is None else s14
    return np.concatenate([np.asarray(pos, np.float64), m.reshape(-1), [0.0, s13, s14]]).astype(np.float32)


def pcg_next(s):
    """K/randomness.h Random_nextState on uint32 numpy arrays."""
    s = (s * np.uint32(47796405) + np.uint32(2891336453)).astype(np.uint32)
    s = (((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)).astype(np.uint32)
    return ((s >> np.uint32(22)) ^ s).astype(np.uint32)


def draws(seed, n, count=4):
    """The first `count` floats of the jitter stream (seed ^ KEY) + gid of every pixel, as float64."""
    j = ((np.uint32(np.int64(seed) & 0xFFFFFFFF) ^ np.uint32(KEY)) + np.arange(n, dtype=np.uint32)).astype(np.uint32)
    out = []
    for _ in range(count):
        j = pcg_next(j)
        out.append((j >> np.uint32(8)).astype(np.float64) / 16777216.0)
    return out


def image_xy(seed, width, height):
    n = width * height
    ox, oy = draws(seed, n, 2)
    px, py = np.arange(n) % width, np.arange(n) // width
    hw, ih = float(np.float32(width / (2.0 * height))), float(np.float32(1.0 / height))
    return -hw + (px + ox) * ih, -0.5 + (py + oy) * ih, hw


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def local_projection(kind, s13, s14, width, height, seed):
    """lo, ld of the specification: the local origin and the normalised local direction, before the lens and the rotation."""
    x, y, hw = image_xy(seed, width, height)
    n = x.size
    lo = np.zeros((n, 3))
    rad = math.pi / 180.0
    if kind == native.PROJ_PARALLEL:
        lo = np.stack([s14 * x, s14 * y, np.full(n, -s13)], 1)
        ld = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif kind == native.PROJ_FISHEYE:
        ax, ay = x * s14 * rad, y * s14 * rad
        a = np.hypot(ax, ay)
        safe = np.where(a == 0, 1.0, a)
        ld = np.where((a == 0)[:, None], [0.0, 0.0, 1.0], np.stack([np.sin(a) * ax / safe, np.sin(a) * ay / safe, np.cos(a)], 1))
    elif kind == native.PROJ_PANORAMIC:
        ax, ay = x * s14 * rad, y * s14 * rad
        ld = np.stack([np.cos(ay) * np.sin(ax), np.sin(ay), np.cos(ay) * np.cos(ax)], 1)
    elif kind == native.PROJ_PANORAMIC_SLOT:
        ax = x * s14 * rad
        ld = np.stack([np.sin(ax), s13 * y, np.cos(ax)], 1)
    elif kind == native.PROJ_STEREOGRAPHIC:
        X, Y = s14 * x, s14 * y
        r2 = X * X + Y * Y
        ld = np.stack([2 * X, 2 * Y, 1 - r2], 1) / (1 + r2)[:, None]
    else:
        th = x * (math.pi / hw)
        y2, eye = y, np.full(n, s13)
        if kind == native.PROJ_ODS_STACKED:
            top = (np.arange(n) // width) < height // 2
            y2 = np.where(top, 2 * y + 0.5, 2 * y - 0.5)
            eye = np.where(top, -s13, s13)
        ph = y2 * s14 * rad
        ld = np.stack([np.cos(ph) * np.sin(th), np.sin(ph), np.cos(ph) * np.cos(th)], 1)
        lo = np.stack([eye * np.cos(th), np.zeros(n), -eye * np.sin(th)], 1)
    return lo, unit(ld)


def restated_rays(kind, s, width, height, seed, lens=None):
    """The specification in float64, independent of camera_proj.h: world-space origins and directions."""
    s = np.asarray(s, np.float64)
    lo, ld = local_projection(kind, s[13], s[14], width, height, seed)
    if lens is not None and lens[0] > 0:
        aperture, focus = lens
        u1, u2 = draws(seed, width * height, 4)[2:]
        r = np.sqrt(u1) * aperture
        theta = 2.0 * math.pi * u2
        rx, ry = np.cos(theta) * r, np.sin(theta) * r
        if kind == native.PROJ_PARALLEL:
            off = np.stack([rx, ry, np.zeros_like(rx)], 1)
            t = np.array([0.0, 0.0, focus]) - off
        else:
            wide = np.abs(ld[:, 0]) > np.abs(ld[:, 1])
            zero = np.zeros(len(ld))
            U = unit(np.where(wide[:, None], np.stack([-ld[:, 2], zero, ld[:, 0]], 1), np.stack([zero, ld[:, 2], -ld[:, 1]], 1)))
            V = np.cross(ld, U)
            off = U * rx[:, None] + V * ry[:, None]
            t = ld * focus - off
        lo, ld = lo + off, unit(t)
    m = s[3:12].reshape(3, 3)
    return lo @ m.T + s[:3], ld @ m.T


def table(kind, s, width, height, seed, lens=None):
    return renderer.camera_rays(kind, s, width, height, seed, lens).reshape(-1, 6)


@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("lens", [None, LENS], ids=["no_lens", "lens"])
@pytest.mark.parametrize("kind", TYPES)
def test_host_table_matches_the_float64_restatement(kind, lens, width, height):
    width, height = size_for(kind, width, height)
    s = settings_for(kind)
    for seed in SEEDS:
        got = table(kind, s, width, height, seed, lens).astype(np.float64)
        o, d = restated_rays(kind, s, width, height, seed, lens)
        scale_o = max(1.0, float(np.abs(o).max()))
        np.testing.assert_allclose(got[:, :3], o, rtol=1e-5, atol=1e-5 * scale_o)
        np.testing.assert_allclose(got[:, 3:], d, rtol=1e-5, atol=1e-5)


# ---- the two new draws -------------------------------------------------------------------------------------------------------------
def test_lens_draws_are_draws_3_and_4_of_the_jitter_stream(ref):
    """A parallel camera with w = 1, b = 0 at the origin: origin - (x, y, 0) is the lens offset (cos, sin)(theta) * sqrt(u1) * aperture,
    so u1 = |off|^2 / aperture^2 and u2 = angle / 2 pi come back out of the table; they are the reference RNG's draws 3 and 4."""
    width, height, aperture = 33, 17, 0.75
    s = settings_for(native.PROJ_PARALLEL, pos=(0, 0, 0), m=np.eye(3), s13=0.0, s14=1.0)
    n = width * height
    for seed in SEEDS:
        off = (table(native.PROJ_PARALLEL, s, width, height, seed, (aperture, 5.0))[:, :3].astype(np.float64)
               - table(native.PROJ_PARALLEL, s, width, height, seed)[:, :3])
        assert (off[:, 2] == 0).all()
        u1, u2 = draws(seed, n, 4)[2:]
        np.testing.assert_allclose((off[:, 0] ** 2 + off[:, 1] ** 2) / aperture ** 2, u1, atol=2e-6)
        turn = np.mod(np.arctan2(off[:, 1], off[:, 0]) / (2 * math.pi), 1.0)
        far = u1 > 1e-3   # (the angle of a short offset is badly conditioned)
        wrap = np.abs(turn - u2)
        assert np.minimum(wrap, 1.0 - wrap)[far].max() < 2e-5
        for gid in (0, 1, 2021 % n, n - 1):
            state = (((seed & 0xFFFFFFFF) ^ KEY) + gid) & 0xFFFFFFFF
            _, f = ref.pcg_stream(state, 4)
            assert (f[2], f[3]) == (np.float32(u1[gid]), np.float32(u2[gid]))


# ---- analytic properties, at identity rotation and zero position ------------------------------------------------------------------
def local_tables(kind, lens, s13=None, s14=None, width=64, height=48, seed=77):
    s = settings_for(kind, pos=(0.0, 0.0, 0.0), m=np.eye(3), s13=s13, s14=s14)
    off, on = table(kind, s, width, height, seed).astype(np.float64), table(kind, s, width, height, seed, lens).astype(np.float64)
    return off[:, :3], off[:, 3:], on[:, :3], on[:, 3:]


@pytest.mark.parametrize("kind", TYPES)
def test_every_lens_ray_passes_through_its_focus_point(kind):
    for aperture, focus in ((0.35, 9.0), (1.5, 40.0), (0.01, 0.5)):
        # the planar lens lies in the origins' plane; with back-off 0 that is local z = 0 and the focal plane local z = focus
        o0, d0, o, d = local_tables(kind, (aperture, focus), s13=0.0 if kind == native.PROJ_PARALLEL else None)
        point = o0 + d0 * focus
        if kind == native.PROJ_PARALLEL:
            np.testing.assert_allclose(point[:, 2], focus, atol=1e-6 * focus)
        to = point - o
        miss = np.linalg.norm(to - d * np.sum(to * d, axis=1, keepdims=True), axis=1)
        assert miss.max() < 1e-4 * focus, (kind, aperture, focus, miss.max())
        assert (np.sum(to * d, axis=1) > 0).all()          # in front of the lens, not behind it
        np.testing.assert_allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)


def test_the_planar_focal_plane_moves_with_the_back_off():
    o0, d0, o, d = local_tables(native.PROJ_PARALLEL, (0.5, 25.0), s13=12.5)
    to = o0 + d0 * 25.0 - o
    assert np.linalg.norm(to - d * np.sum(to * d, axis=1, keepdims=True), axis=1).max() < 25e-4
    assert (o[:, 2] == -12.5).all()


@pytest.mark.parametrize("kind", TYPES)
def test_origin_offsets_fill_a_disc_across_the_lens_off_direction(kind):
    aperture = 0.35
    o0, d0, o, _ = local_tables(kind, (aperture, 9.0))
    off = o - o0
    r = np.linalg.norm(off, axis=1)
    assert r.max() <= aperture * (1 + 1e-5)
    if kind == native.PROJ_PARALLEL:
        assert (off[:, 2] == 0).all()
    else:
        assert np.abs(np.sum(off * d0, axis=1)).max() < 1e-5 * max(1.0, np.abs(o0).max())
    # uniform over the disc: (r / aperture)^2 is uniform on [0, 1]; 5 sigma of its mean over 3 072 pixels (sigma 0.2887 / sqrt(3072))
    assert abs(np.mean((r / aperture) ** 2) - 0.5) < 0.026


def test_ods_yaw_is_linear_in_x_and_spans_the_full_turn():
    for e in (-0.4, 0.25):
        o, d, _, _ = local_tables(native.PROJ_ODS, None, s13=e, s14=180.0)
        x, y, hw = image_xy(77, 64, 48)
        th = x * (math.pi / hw)
        wrap = np.mod(np.arctan2(d[:, 0], d[:, 2]) - th + math.pi, 2 * math.pi) - math.pi
        assert np.abs(wrap).max() < 2e-6
        assert th.min() < -math.pi * (1 - 1 / 64) and th.max() > math.pi * (1 - 1 / 64)   # columns 0 and W - 1 reach both ends
        np.testing.assert_allclose(np.arcsin(np.clip(d[:, 1], -1, 1)), np.radians(180.0 * y), atol=2e-5)
        np.testing.assert_allclose(np.linalg.norm(o, axis=1), abs(e), rtol=1e-6)
        look = np.stack([np.sin(th), np.zeros_like(th), np.cos(th)], 1)
        assert np.abs(np.sum(o * look, axis=1)).max() < 1e-6
        # e > 0 is the right eye: the origin lies to the right (+x at th = 0) of the direction it looks in
        side = np.sum(o * np.stack([np.cos(th), np.zeros_like(th), -np.sin(th)], 1), axis=1)
        np.testing.assert_allclose(side, e, rtol=1e-5)


def test_ods_stacked_is_the_two_single_eye_images():
    width, height, e, fov = 64, 48, 0.3, 150.0
    s = settings_for(native.PROJ_ODS_STACKED, s13=e, s14=fov)
    half = width * (height // 2)
    for seed in SEEDS:
        both = table(native.PROJ_ODS_STACKED, s, width, height, seed).astype(np.float64)
        # the lower half's pixels have gid + half: the single image whose stream starts there
        lower_seed = ((((seed & 0xFFFFFFFF) ^ KEY) + half) & 0xFFFFFFFF) ^ KEY
        for part, eye, sd in ((both[:half], -e, seed), (both[half:], e, lower_seed)):
            one = table(native.PROJ_ODS, settings_for(native.PROJ_ODS, s13=eye, s14=fov), width, height // 2, sd).astype(np.float64)
            np.testing.assert_allclose(part[:, :3], one[:, :3], rtol=1e-5, atol=1e-5 * max(1.0, np.abs(one[:, :3]).max()))
            np.testing.assert_allclose(part[:, 3:], one[:, 3:], rtol=1e-5, atol=1e-5)
    with_lens = table(native.PROJ_ODS_STACKED, s, width, height, 5, LENS)
    assert not np.array_equal(with_lens[:half], with_lens[half:])


def test_ods_without_an_offset_is_the_panorama_of_the_full_turn():
    width, height = 64, 48
    hw = float(np.float32(width / (2.0 * height)))
    fov = 180.0 / hw
    for seed in SEEDS:
        ods = table(native.PROJ_ODS, settings_for(native.PROJ_ODS, s13=0.0, s14=fov), width, height, seed).astype(np.float64)
        pan = table(native.PROJ_PANORAMIC, settings_for(native.PROJ_PANORAMIC, s14=fov), width, height, seed).astype(np.float64)
        np.testing.assert_allclose(ods, pan, rtol=0, atol=2e-6 * max(1.0, np.abs(pan[:, :3]).max()))
        np.testing.assert_allclose(ods[:, 3:], pan[:, 3:], rtol=0, atol=2e-6)


@pytest.mark.parametrize("kind", TYPES)
def test_aperture_zero_gives_the_lens_off_bytes(kind):
    for width, height in SIZES:
        width, height = size_for(kind, width, height)
        s = settings_for(kind)
        want = table(kind, s, width, height, 123)
        for focus in (0.0, 7.0, -3.0):
            assert np.array_equal(table(kind, s, width, height, 123, (0.0, focus)).view(np.uint32), want.view(np.uint32))


# ---- validation --------------------------------------------------------------------------------------------------------------------
def rejected(kind, settings, width=16, height=8, lens=None):
    with pytest.raises(native.ChunkyHipError) as e:
        renderer.camera_rays(kind, settings, width, height, 1, lens)
    assert e.value.code == native.E_INVALID


def test_invalid_lenses_are_rejected():
    for kind in TYPES:
        s = settings_for(kind)
        for lens in ((np.nan, 5.0), (0.1, np.nan), (np.inf, 5.0), (0.1, np.inf), (-0.1, 5.0), (0.1, 0.0), (0.1, -2.0), (0.0, np.nan)):
            rejected(kind, s, lens=lens)
        renderer.camera_rays(kind, s, 16, 8, 1, (0.1, 5.0))
        renderer.camera_rays(kind, s, 16, 8, 1, (0.0, -1.0))     # no aperture: the focus is not looked at
        bad = s.copy()
        bad[12] = 0.05
        rejected(kind, bad, lens=(0.1, 5.0))                     # settings[12] stays 0: the lens has its own arguments
    for kind in (native.PROJ_PINHOLE, native.PROJ_PREGENERATED, 6, 9, -2):
        rejected(kind, settings_for(native.PROJ_FISHEYE), lens=(0.1, 5.0))
        rejected(kind, settings_for(native.PROJ_FISHEYE))


def test_invalid_ods_settings_are_rejected():
    for kind in ODS_TYPES:
        for i, v in ((12, 0.05), (14, 0.0), (14, -90.0), (13, np.nan), (13, np.inf), (14, np.nan), (0, np.nan), (7, np.inf)):
            bad = settings_for(kind)
            bad[i] = v
            rejected(kind, bad)
        rejected(kind, settings_for(kind)[:14])
        rejected(kind, np.concatenate([settings_for(kind), [0.0]]))
        rejected(kind, settings_for(kind), width=0)
    renderer.camera_rays(native.PROJ_ODS, settings_for(native.PROJ_ODS, s13=0.4), 16, 7, 1)      # either sign, any height
    renderer.camera_rays(native.PROJ_ODS, settings_for(native.PROJ_ODS, s13=-0.4), 16, 7, 1)
    renderer.camera_rays(native.PROJ_ODS_STACKED, settings_for(native.PROJ_ODS_STACKED, s13=0.0), 16, 8, 1)
    rejected(native.PROJ_ODS_STACKED, settings_for(native.PROJ_ODS_STACKED, s13=-0.4))          # the stacked offset is >= 0
    rejected(native.PROJ_ODS_STACKED, settings_for(native.PROJ_ODS_STACKED), height=7)          # and its height even
    rejected(native.PROJ_ODS_STACKED, settings_for(native.PROJ_ODS_STACKED), height=7, lens=(0.1, 5.0))
    rejected(6, settings_for(native.PROJ_ODS))                                                  # 6 stays unassigned


def test_the_new_calls_are_declared_and_exported():
    assert {"chunky_render_set_lens", "chunky_camera_rays_lens"} <= set(native.declared_symbols())
    L = native.lib()
    assert L.chunky_render_set_lens and L.chunky_camera_rays_lens
    assert L.chunky_render_set_lens(None, 0.1, 5.0) == native.E_INVALID   # (a NULL target)


# ---- the scene JSON mapping ----------------------------------------------------------------------------------------------------------
def test_camera_settings_lens_maps_the_ods_modes_and_depth_of_field():
    cam = {"position": {"x": 10.0, "y": 80.0, "z": -4.0}, "orientation": {"yaw": 0.4, "pitch": -1.3, "roll": 0.0}, "fov": 120.0}
    origin = (2.0, 0.0, 0.0)
    base = octree2.camera_from_json(cam, origin)
    kind, s, lens = octree2.camera_settings_lens(cam, origin)
    assert kind == 0 and lens is None and np.array_equal(s, base)
    kind, s, lens = octree2.camera_settings_lens(dict(cam, dof=40.0, focalOffset=8.0), origin)
    assert kind == 0 and lens is None and s[12] == np.float32(8.0 / 40.0)       # the pinhole camera carries its own aperture
    for mode, want, e in (("ODS_LEFT", 7, -0.0345), ("ODS_RIGHT", 7, 0.0345), ("ODS_STACKED", 8, 0.0345)):
        kind, s, lens = octree2.camera_settings_lens(dict(cam, projectionMode=mode), origin)
        assert kind == want and lens is None and s.dtype == np.float32 and s.size == 15
        np.testing.assert_array_equal(s[:12], base[:12])
        assert (s[12], s[13], s[14]) == (0.0, np.float32(e), 180.0)
        renderer.camera_rays(kind, s, 8, 4, 0)
        kind, s2, lens = octree2.camera_settings_lens(dict(cam, projectionMode=mode, dof=50.0, focalOffset=10.0), origin)
        assert kind == want and np.array_equal(s2, s) and lens == pytest.approx((10.0 / 50.0, 10.0))
        renderer.camera_rays(kind, s2, 8, 4, 0, lens)
    for mode, want in (("PARALLEL", 1), ("FISHEYE", 2), ("PANORAMIC", 3), ("PANORAMIC_SLOT", 4), ("STEREOGRAPHIC", 5)):
        plain = octree2.camera_settings(dict(cam, projectionMode=mode), origin, world_width=512.0)
        kind, s, lens = octree2.camera_settings_lens(dict(cam, projectionMode=mode), origin, world_width=512.0)
        assert kind == want == plain[0] and lens is None and np.array_equal(s, plain[1])
        kind, s, lens = octree2.camera_settings_lens(dict(cam, projectionMode=mode, dof=40.0, focalOffset=8.0), origin, world_width=512.0)
        assert kind == want and np.array_equal(s, plain[1]) and lens == pytest.approx((8.0 / 40.0, 8.0))
        assert s[12] == 0.0
        renderer.camera_rays(kind, s, 8, 4, 0, lens)
        kind, s, lens = octree2.camera_settings_lens(dict(cam, projectionMode=mode, dof="Infinity"), origin, world_width=512.0)
        assert kind == want and lens is None
    assert octree2.camera_settings_lens(dict(cam, projectionMode="SOMETHING_NEW")) == (-1, None, None)
    # camera_settings itself is as it was: the host-table route for both
    for mode in ("ODS_LEFT", "ODS_RIGHT", "ODS_STACKED", "ODS", "SOMETHING_NEW"):
        assert octree2.camera_settings(dict(cam, projectionMode=mode)) == (-1, None)
    assert octree2.camera_settings(dict(cam, projectionMode="FISHEYE", dof=40.0)) == (-1, None)
    assert octree2.camera_settings(dict(cam, projectionMode="PINHOLE", dof=40.0))[0] == 0


# ---- not hollow ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", TYPES)
def test_the_lens_of_the_device_tests_moves_nearly_every_ray(kind):
    sc = projected(gs.make("outdoor"), kind)
    for seed in SEEDS[:2]:
        off = table(kind, sc.camera, sc.width, sc.height, seed)
        on = table(kind, sc.camera, sc.width, sc.height, seed, GPU_LENS[kind])
        moved = (off.view(np.uint32) != on.view(np.uint32)).any(axis=1)
        assert moved.mean() > 0.99, (kind, moved.mean())


def test_the_ods_eyes_of_the_device_tests_differ():
    sc = projected(gs.make("outdoor"), native.PROJ_ODS_STACKED)
    t = table(native.PROJ_ODS_STACKED, sc.camera, sc.width, sc.height, 3)
    half = sc.width * sc.height // 2
    assert np.abs(t[:half, :3] - t[half:, :3]).max() > 0.03


def test_reference_build_sees_the_lens(ref):
    """The equivalence's right-hand side changes with the lens: the reference kernel on the lens table against the lens-off table."""
    kind = native.PROJ_FISHEYE
    sc = projected(gs.make("outdoor"), kind)
    seeds = np.array([11], np.int32)
    imgs = []
    for lens in (None, GPU_LENS[kind]):
        rays = renderer.camera_rays(kind, sc.camera, sc.width, sc.height, 11, lens)
        view = dataclasses.replace(sc, camera=rays, projector_type=-1)
        imgs.append(ref.render_passes(binding.SceneHandle(view), seeds, threads=binding.usable_threads()).reshape(-1, 3))
    assert all(np.isfinite(im).all() and im.max() > 0 for im in imgs)
    changed = (imgs[0].view(np.uint32) != imgs[1].view(np.uint32)).any(axis=1)
    assert changed.mean() >= 0.10, changed.mean()
