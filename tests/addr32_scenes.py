"""Scenes and cases of tests/test_gpu_addr32_parity.py (a plain helper module, not a conftest), and — run as a program — the child
process that renders the same cases on the -DCHUNKY_TUNING build with CHUNKY_ADDR32_MASK=0: the library then treats the scene as one
too large for 32-bit offsets and has to pick kernels with 64-bit addresses.

The world is built so that a wrong byte offset shows in the image:

  atlas    80 x 48 texels (5 x 3 tiles: not square, no power of two) in four layers, every tile taken.  The texture `ramp` (alpha
           0 ... 255) is the LAST tile: last column, last row, last layer — the far corner of the array, and with the clamps of
           K/textureAtlas.h:18-28 at work on its last texel.  It is a colour texture, an emittance texture (material flag 2) and both.
  models   a pyramid of five boxes and a tent of five quads on the aligned records (offsets beyond the first record), a second
           pyramid behind it in the record array, and a tent whose material has flag 2 (it stays on the packed palettes)
  sky      96 x 72 texels (no power of two); the view `sun` looks into the sun disc, whose texel is SHADE's atlas read"""
import dataclasses
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":   # (as the child process: the package lies beside tests/)
    sys.path.insert(0, os.path.dirname(HERE))
from chunkyclplugin_amd import native, scenes  # noqa: E402

W, H = 33, 17
N_PASSES = 4
TEX16 = (16 << 16) | 16
TILES_X, TILES_Y = 5, 3
ALT, AZI, INTENSITY = 0.6, 1.2, 1.25


def _material(pal, flags, tint, size, color, ne, spec=0):
    ptr = len(pal.materials)
    pal.materials += [flags, tint, size, color, ne, spec]
    return ptr


def _tent(mat, height=0.7, top_mat=None):
    h = height
    uv = (0.0, 1.0, 0.0, 1.0)
    return [((0.1, h, 0.1), (0, 0, 0.8), (0.8, 0, 0), uv, mat if top_mat is None else top_mat, 1),
            ((0.1, 0, 0.1), (0, h, 0), (0.8, 0, 0), uv, mat, 1),
            ((0.1, 0, 0.9), (0.8, 0, 0), (0, h, 0), uv, mat, 1),
            ((0.1, 0, 0.1), (0, 0, 0.8), (0, h, 0), uv, mat, 1),
            ((0.9, 0, 0.1), (0, h, 0), (0, 0, 0.8), uv, mat, 1)]


def _pyramid(n, mats):
    boxes = []
    for i in range(n):
        s = i / (2.5 * n)
        flags = (((i * 5) & 7) << 4) | (((i * 3) & 7) << 8) | (((i * 7) & 7) << 12) | ((i & 7) << 16) | ((i & 3) << 20)
        boxes.append(((s, 1 - s, i / n, (i + 1) / n, s, 1 - s), flags, tuple(mats[(i + k) % len(mats)] for k in range(6))))
    return boxes


@functools.lru_cache(maxsize=None)
def world():
    """(the depth-5 scene, the atlas location of `ramp`)"""
    rng = np.random.default_rng(20261019)
    ab = scenes.AtlasBuilder(TILES_X, TILES_Y)
    # seven 32 x 32 textures: two fit a layer of 5 x 3 tiles, so they open four layers; 32 textures of 16 x 16 take every tile left
    big = [ab.add(scenes.noise_texture(rng, (255 - 20 * i, 250 - 10 * i, 230), 4, size=32)) for i in range(7)]
    small = [ab.add(scenes.noise_texture(rng, (60 + 6 * i, 200 - 5 * i, 90 + 4 * (i % 9)), 14)) for i in range(31)]
    ramp = scenes.noise_texture(rng, (230, 120, 40), 20)
    ramp[..., 3] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    ramp_id = ab.add(ramp)   # the last texture of its size: the placement rule gives it the last free tile
    atlas, recs = ab.build()
    loc = lambda i: recs[i][1]

    pal = scenes.Palettes()
    m = {"stone": _material(pal, 4, 0, TEX16, loc(small[0]), 0),
         "plank": _material(pal, 4, 0, TEX16, loc(small[17]), 0),
         "far": _material(pal, 4, 0, TEX16, loc(small[30]), 0),
         "edge": _material(pal, 4, 0, TEX16, loc(ramp_id), 40),                 # the colour out of the last tile
         "emit2": _material(pal, 2, 0, TEX16, 0xFFE0A060, loc(ramp_id), 0),     # the emittance out of it
         "emit6": _material(pal, 6, 0, TEX16, loc(ramp_id), loc(ramp_id), 0)}   # both
    B = {"air": pal.block_invisible()}
    for k in ("stone", "edge", "emit2", "emit6"):
        B[k] = pal.block_cube(m[k])
    faces = (m["plank"], m["stone"], m["edge"], m["far"], m["plank"])
    B["pyramid"] = pal.block_aabbs(_pyramid(5, faces))
    B["pyramid2"] = pal.block_aabbs(_pyramid(3, faces[::-1]))
    B["tent"] = pal.block_quads(_tent(m["plank"], top_mat=m["edge"]))
    B["tent2"] = pal.block_quads(_tent(m["far"], 0.5, top_mat=m["stone"])[:3])
    B["emit_tent"] = pal.block_quads(_tent(m["emit6"]))
    depth, S, y = 5, 32, 2
    t = np.zeros((S, S, S), np.int32)
    t[:, :y, :] = B["stone"]
    for slot, name in enumerate(["edge", "emit2", "emit6", "pyramid", "tent", "pyramid2", "tent2", "emit_tent"]):
        x0, z0 = 3 + 7 * (slot % 4), 3 + 7 * (slot // 4)
        for i in range(3):
            for j in range(3):
                t[x0 + 2 * i, y, z0 + 2 * j] = B[name]
    blocks, mats, aabbs, quads = pal.arrays()
    sky = np.ascontiguousarray(scenes.bake_sky(96, scenes.sun_direction(ALT, AZI))[12:84])   # 72 rows of 96 texels
    sc = scenes.PackedScene(octree=scenes.build_octree(t, depth), octree_depth=depth, block_palette=blocks, material_palette=mats,
                            aabb_models=aabbs, quad_models=quads, world_bvh=scenes.empty_bvh(), actor_bvh=scenes.empty_bvh(),
                            bvh_trigs=np.zeros(1, np.int32), atlas=atlas, sky=sky, sky_intensity=INTENSITY,
                            sun=scenes.pack_sun(ALT, AZI, INTENSITY, True, recs[big[6]]),
                            camera=scenes.look_at_camera((15.0, 19.0, -6.0), (15.0, 2.0, 9.0), 60.0), width=W, height=H, name="addr32")
    return sc, loc(ramp_id)


@functools.lru_cache(maxsize=None)
def scene(view="exhibits"):
    """The world inside a depth-7 octree (tree form 17: the timed instantiation) under one of the views."""
    sc = scenes.embed_deeper(world()[0], 7)
    if view == "sun":       # into the sun disc from above the exhibits: sky, disc texel, nothing else
        pos = np.array([15.0, 6.0, 9.0])
        return dataclasses.replace(sc, camera=scenes.look_at_camera(pos, pos + 50.0 * scenes.sun_direction(ALT, AZI), 24.0))
    if view == "fisheye":   # the same position and rotation under a 180-degree fisheye: proj::render_pool
        cam = np.asarray(sc.camera, np.float32)[:15].copy()
        cam[12], cam[13], cam[14] = 0.0, 0.0, 180.0
        return dataclasses.replace(sc, camera=cam, projector_type=native.PROJ_FISHEYE)
    return sc


# case -> (view, OPT_KERNEL variant, what kernel_info has to say on the library as it ships)
CASES = {
    "plain": ("exhibits", 512, {"tree": 17, "pool": 64, "sorted": False}),
    "sorted": ("exhibits", 256, {"tree": 17, "pool": 64, "sorted": True}),
    "default": ("exhibits", 0, {"tree": 17, "pool": 64}),
    "sun": ("sun", 512, {"tree": 17, "pool": 64, "sorted": False}),
    "fisheye": ("fisheye", 512, {"tree": 17, "pool": 64, "sorted": False}),
    "render_waves": ("exhibits", 8, {"pool": -1}),
}
AOV_VIEW = "exhibits"


def render_case(instance, name, seeds):
    """(image, kernel_info, the scene's addr32 word) of a case on `instance`"""
    from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader
    view, variant, _ = CASES[name]
    sc = scene(view)
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    r.render_passes(seeds)
    out = (r.read(), r.kernel_info(), loader.addr32())
    r.close()
    loader.close()
    return out


def render_aov(instance, seeds):
    """((albedo, normal), aov_info) of the AOV kernel on the exhibits"""
    from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader
    sc = scene(AOV_VIEW)
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.render_aov(seeds)
    out = ((r.read_aov(native.AOV_ALBEDO).reshape(-1, 3), r.read_aov(native.AOV_NORMAL).reshape(-1, 3)), r.aov_info())
    r.close()
    loader.close()
    return out


def main(out_path):
    from chunkyclplugin_amd.renderer import RendererInstance
    seeds = scenes.java_random_ints(N_PASSES)
    inst = RendererInstance.get(0)
    arrays, said = {}, {"library": os.path.basename(native.LIB_PATH), "kernel": {}, "word": {}}
    for name in CASES:
        img, info, word = render_case(inst, name, seeds)
        arrays[name] = img
        said["kernel"][name] = info
        said["word"][name] = word
    (albedo, normal), info = render_aov(inst, seeds)
    arrays["aov_albedo"], arrays["aov_normal"] = albedo, normal
    said["kernel"]["aov"] = info
    np.savez(out_path, **arrays)
    print(json.dumps(said))


if __name__ == "__main__":
    main(sys.argv[1])
