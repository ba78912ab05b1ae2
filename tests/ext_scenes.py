"""An exhibit world for the extended integrator (oracle/port.c trace_sample_ext is its specification), and the
small rooms of the analytic tests of its after_nee rule (tests/test_extensions.py).

Found by coverage of oracle/port.c over the extended fixtures: no emitter of any of them is a merged leaf, the
material gate of the emitter sample never fails, their emitter textures are near-uniform, and no emitter the list cannot hold (a
model block, a cube with an emittance texture, an entity triangle) stands where a bounce ray that follows an emitter sample finds
it.  The exhibit is a room seen from inside, open to the sky through a hole in its ceiling, that holds all of them;
tests/test_ext_census_cpu.py counts that the restatement's own rays reach every class of event often enough
(profiles/ext_census.json), tests/test_gpu_ext_exhibit.py compares the kernels with the restatement on it bit for bit."""
import dataclasses

import numpy as np

from chunkyclplugin_amd import scenes

W, H = 64, 48
N_PASSES = 5
DEPTH = 6                                         # (the room fills the 32^3 corner at the origin: a depth-5 octree has no wide tree)
ROOM = 32
EMBED_DEPTHS = {7: 17, 11: 18}                    # embedded depth -> tree argument of the extended kernels there (depth 6: -1)
TEX16 = (16 << 16) | 16
ROOM_TOP = 21                                     # the ceiling's y
BLOCK4 = (12, 8, 20)                              # corner of the 4^3 emitter block (a level-2 leaf)
LEVEL_MASK = (1 << 25) - 1                        # the block pointer of an emitter-list entry's word 3


def word5(spec, metal, rough):
    return spec | (metal << 8) | (rough << 16)


def _material(pal, flags, tint, size, color, ne, spec=0):
    """One raw material record (PackedMaterial.java:89-100), as tests/route_scenes.py writes them."""
    ptr = len(pal.materials)
    pal.materials += [flags, tint, size, color, ne, spec]
    return ptr


def quadrants():
    """The emitter texture of four quadrants: red, green and blue ones and one of alpha 0; no symmetry maps it onto itself."""
    t = np.zeros((16, 16, 4), np.uint8)
    t[:8, :8] = (235, 60, 50, 255)
    t[:8, 8:] = (60, 225, 80, 255)
    t[8:, :8] = (60, 90, 245, 255)
    t[8:, 8:] = (255, 255, 255, 0)
    t[2, 5, :3] = (250, 250, 60)                  # ... and one marked texel off both diagonals
    return t


def _tent(mat, height=0.7):
    """Five one-sided quads: a lid facing up and four walls facing outwards."""
    h = height
    uv = (0.0, 1.0, 0.0, 1.0)
    return [((0.2, h, 0.2), (0, 0, 0.6), (0.6, 0, 0), uv, mat, 1),
            ((0.2, 0, 0.2), (0, h, 0), (0.6, 0, 0), uv, mat, 1),
            ((0.2, 0, 0.8), (0.6, 0, 0), (0, h, 0), uv, mat, 1),
            ((0.2, 0, 0.2), (0, 0, 0.6), (0, h, 0), uv, mat, 1),
            ((0.8, 0, 0.2), (0, h, 0), (0, 0, 0.6), uv, mat, 1)]


def _palette():
    """(atlas, texture records by name, Palettes, material pointers by name, block indices by name): shared by the exhibit and the rooms."""
    rng = np.random.default_rng(20261021)
    ab = scenes.AtlasBuilder(8, 8)
    ramp = np.zeros((16, 16, 4), np.uint8)        # an emittance texture: alpha over 0 ... 255
    ramp[..., :3] = 128
    ramp[..., 3] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    q = quadrants()
    tex = {"floor": ab.add(scenes.noise_texture(rng, (150, 140, 130), 12)),
           "wall": ab.add(scenes.noise_texture(rng, (200, 200, 195), 10)),
           "steel": ab.add(scenes.noise_texture(rng, (170, 180, 200), 8)),
           "plaster": ab.add(scenes.noise_texture(rng, (210, 190, 160), 10)),
           "glow": ab.add(scenes.noise_texture(rng, (255, 235, 190), 4)),
           "ember": ab.add(scenes.noise_texture(rng, (240, 240, 240), 6)),
           "lava": ab.add(scenes.noise_texture(rng, (235, 130, 50), 16)),
           "quadrants": ab.add(q),
           # read at (u, v) this one gives what `quadrants` gives at (v, u) (the atlas read flips v: textureAtlas.h:13)
           "quadrants_t": ab.add(np.ascontiguousarray(q[::-1, ::-1].transpose(1, 0, 2))),
           "ramp": ab.add(ramp),
           "sun": ab.add(scenes.noise_texture(rng, (255, 250, 230), 4, size=32))}
    atlas, recs = ab.build()
    loc = {k: recs[v][1] for k, v in tex.items()}
    assert all(recs[v][0] == TEX16 for k, v in tex.items() if k != "sun")
    pal = scenes.Palettes()
    m = {"plain": _material(pal, 4, 0, TEX16, loc["wall"], 0, 0),
         "floor": _material(pal, 4, 0, TEX16, loc["floor"], 0, word5(70, 0, 0)),           # spec only, rough == 0
         "steel": _material(pal, 4, 0, TEX16, loc["steel"], 0, word5(0, 190, 110)),        # metal, rough > 0
         "plaster": _material(pal, 4, 0, TEX16, loc["plaster"], 0, word5(120, 0, 200)),    # spec, rough > 0
         "chrome": _material(pal, 4, 0, TEX16, loc["steel"], 0, word5(40, 255, 0)),        # metal, rough == 0
         "sheet": _material(pal, 4, 0, TEX16, loc["plaster"], 0, word5(210, 0, 60)),       # two-sided triangles: rn < 0 behind them
         "glow": _material(pal, 4, 0, TEX16, loc["glow"], 255, 0),
         "quadrants": _material(pal, 4, 0, TEX16, loc["quadrants"], 200, 0),
         "quadrants_t": _material(pal, 4, 0, TEX16, loc["quadrants_t"], 200, 0),
         "ember": _material(pal, 4, 0xFF000000 | 0xFF8040, TEX16, loc["ember"], 120, word5(30, 0, 0)),
         "lamp": _material(pal, 4, 0, TEX16, loc["glow"], 230, 0),                          # on model blocks and triangles only
         "lava": _material(pal, 6, 0, TEX16, loc["lava"], loc["ramp"], 0)}                  # flag 2: an emittance texture
    B = {"air": pal.block_invisible()}
    for k in ("plain", "floor", "steel", "plaster", "chrome", "glow", "quadrants", "quadrants_t", "ember", "lava"):
        B[k] = pal.block_cube(m[k])
    B["lamp_box"] = pal.block_aabbs([((0.25, 0.75, 0, 0.8, 0.25, 0.75), 0b0001 << 4 | 0b0110 << 16, (m["lamp"],) * 6)])
    B["lamp_quad"] = pal.block_quads(_tent(m["lamp"]))
    return atlas, recs, tex, pal, m, B


def _scene(t, depth, pal, atlas, sun, sky, camera, width, height, name, sky_intensity=1.0):
    blocks, mats, aabbs, quads = pal.arrays()
    return scenes.PackedScene(octree=scenes.build_octree(t, depth), octree_depth=depth, block_palette=blocks, material_palette=mats,
                              aabb_models=aabbs, quad_models=quads, world_bvh=scenes.empty_bvh(), actor_bvh=scenes.empty_bvh(),
                              bvh_trigs=np.zeros(1, np.int32), atlas=atlas, sky=sky, sky_intensity=sky_intensity, sun=sun,
                              camera=camera, width=width, height=height, name=name)


SUN = (1.0, 0.8, 1.25)                            # altitude, azimuth, intensity: through the hole in the ceiling


def _types(B, broken=False):
    t = np.zeros((1 << DEPTH,) * 3, np.int32)
    S = ROOM
    top = ROOM_TOP
    t[0, :top + 1, :S] = B["steel"]
    t[S - 1, :top + 1, :S] = B["steel"]
    t[:S, :top + 1, 0] = B["plaster"]
    t[:S, :top + 1, S - 1] = B["plaster"]
    t[:S, 0, :S] = B["floor"]
    t[:S, top, :S] = B["plain"]
    t[9:23, top, 9:23] = B["air"]                 # the hole
    t[26:28, 1:9, 6:8] = B["chrome"]              # a pillar
    # listed emitters: one cell, a 2^3 and a 4^3 block on their grids (leaves of level 0, 1, 2), a 2^3 block off the grid (eight level-0 leaves)
    t[5, 1, 12] = B["glow"]
    t[8:10, 2:4, 8:10] = B["glow"]
    x, y, z = BLOCK4
    t[x:x + 4, y:y + 4, z:z + 4] = B["glow"]
    if broken:
        t[x, y, z] = B["air"]                     # ... the 4^3 block less one cell: 7 level-1 and 7 level-0 leaves
    t[17:19, 1:3, 9:11] = B["glow"]
    t[20:22, 2:4, 20:22] = B["quadrants"]         # the textured emitter: a level-1 leaf (the texture tiles) and single cells
    for c in ((24, 1, 12), (10, 1, 22), (0, 6, 14), (14, 5, 31)):
        t[c] = B["quadrants"]
    t[6:8, 6:8, 24:26] = B["ember"]               # a second emitter with another emittance byte and a tint
    for c in ((22, 1, 5), (28, 5, 31), (15, top, 4), (31, 9, 20)):
        t[c] = B["ember"]
    # unlisted emitters
    for c in ((12, 1, 6), (14, 1, 6), (6, 1, 18), (28, 1, 20), (18, 1, 26), (23, 1, 23)):
        t[c] = B["lamp_box"]
    for c in ((20, 1, 8), (9, 1, 14), (25, 1, 25), (4, 1, 26), (16, 1, 14)):
        t[c] = B["lamp_quad"]
    for c in ((22, 1, 16), (12, 1, 28), (28, 1, 10), (31, 4, 12), (16, 1, 18)):
        t[c] = B["lava"]
    return t


def _sheet(rect, y, n, mat):
    """n two-sided triangles: the rectangle at height y cut into strips of two triangles each."""
    (xa, za), (xb, zb) = rect
    strips = (n + 1) // 2
    out = []
    for i in range(n):
        k = i // 2
        x0, x1 = xa + (xb - xa) * k / strips, xa + (xb - xa) * (k + 1) / strips
        if i % 2 == 0:
            out.append(scenes.pack_triangle((x0, y, za), (x1, y, za), (x0, y, zb), (0, 0), (1, 0), (0, 1), mat, True))
        else:
            out.append(scenes.pack_triangle((x1, y, zb), (x0, y, zb), (x1, y, za), (1, 1), (0, 1), (1, 0), mat, True))
    return np.array(out, np.int64).astype(np.int32).reshape(-1, 20)


def with_entities(sc, m, lamp_rect=((5.0, 13.0), (13.0, 21.0)), lamp_y=14.5, sheet_rect=((15.0, 5.0), (27.0, 15.0)), sheet_y=6.5):
    """Emissive two-sided triangles in the world BVH (unlisted emitters), a two-sided specular sheet in the actor BVH (hit from
    behind, the reflected direction points into the surface: rn < 0)."""
    wn, wtr = scenes.build_bvh(_sheet(lamp_rect, lamp_y, 8, m["lamp"]), 2)
    an, atr = scenes.build_bvh(_sheet(sheet_rect, sheet_y, 12, m["sheet"]), 2)
    an = an.copy().reshape(-1, 7)
    an[an[:, 0] <= 0, 0] -= len(wtr)
    return dataclasses.replace(sc, world_bvh=wn, actor_bvh=an.reshape(-1), bvh_trigs=np.concatenate([wtr, atr]), name=sc.name + "_entities")


_CACHE = {}


def palette():
    if "palette" not in _CACHE:
        _CACHE["palette"] = _palette()
    return _CACHE["palette"]


def make(name: str = "exhibit") -> scenes.PackedScene:
    """exhibit[_nosun][_entities][_broken][_d7 | _d11]: the room with the sun flag set (or clear), with the entity BVHs, with the 4^3
    block less one cell, inside a deeper octree."""
    if name in _CACHE:
        return _CACHE[name]
    parts = name.split("_")
    assert parts[0] == "exhibit" and set(parts[1:]) <= {"nosun", "entities", "broken", "d7", "d11"}, name
    atlas, recs, tex, pal, m, B = palette()
    alt, azi, inten = SUN
    sun = scenes.pack_sun(alt, azi, inten, "nosun" not in parts, recs[tex["sun"]])
    sc = _scene(_types(B, "broken" in parts), DEPTH, pal, atlas, sun, scenes.bake_sky(64, scenes.sun_direction(alt, azi)),
                scenes.look_at_camera((3.5, 12.5, 3.5), (19.0, 3.0, 19.0), 85.0), W, H, "exhibit", sky_intensity=inten)
    if "entities" in parts:
        sc = with_entities(sc, m)
    for d in EMBED_DEPTHS:
        if f"d{d}" in parts:
            sc = scenes.embed_deeper(sc, d)
    _CACHE[name] = dataclasses.replace(sc, name=name)
    return _CACHE[name]


def blocks():
    """Block pointers (emitter-list word 3 & LEVEL_MASK, record.material) by name."""
    return {k: 2 * v for k, v in palette()[5].items()}


def expected_levels(broken=False):
    """Emitter-list entries per level of the exhibit, counted by hand from _types."""
    glow0 = 1 + 8 + (7 if broken else 0)
    return {0: glow0 + 4 + 4, 1: 1 + 1 + 1 + (7 if broken else 0), 2: 0 if broken else 1}


def transposed_twin(emitters):
    """A copy of an emitter list whose `quadrants` entries point at the block with the TRANSPOSED texture, which no leaf holds: the
    emitter sample alone then reads the texture with tu and tv swapped."""
    B = blocks()
    out = np.array(emitters, np.int32, copy=True)
    mine = (out[:, 3] & LEVEL_MASK) == B["quadrants"]
    out[mine, 3] = (out[mine, 3] & ~LEVEL_MASK) | B["quadrants_t"]
    return out, int(mine.sum())


# ---- the rooms of the analytic tests: closed, black sky, no sun ----
ROOM_KINDS = ("model", "emit_tex", "entity", "levels")


def room(kind: str, size: int = 14, width: int = 40, height: int = 30) -> scenes.PackedScene:
    """A closed grey room lit by one listed emitter cube and six unlisted emitters of one kind — model blocks, cubes with an
    emittance texture, entity triangles — or ("levels") by merged emitter leaves of level 1 and 2 alone."""
    assert kind in ROOM_KINDS
    atlas, recs, tex, pal, m, B = palette()
    depth = 4
    S = 1 << depth
    a, b = 0, size + 1
    t = np.zeros((S, S, S), np.int32)
    t[a:b + 1, a:b + 1, a:b + 1] = B["plain"]
    t[a + 1:b, a + 1:b, a + 1:b] = B["air"]
    spots = [(3, 1, 4), (11, 1, 3), (4, 1, 11), (12, 1, 12), (7, 1, 8), (9, 1, 5)]
    if kind == "levels":
        t[8:12, 8:12, 8:12] = B["glow"]
        t[4:6, 10:12, 4:6] = B["glow"]
        t[2:4, 2:4, 10:12] = B["ember"]
    else:
        t[7, b, 7] = B["glow"]
        for c in spots:
            if kind != "entity":
                t[c] = B["lamp_box"] if kind == "model" else B["lava"]
    sky = np.zeros((8, 8, 4), np.uint8)
    sky[..., 3] = 255
    sc = _scene(t, depth, pal, atlas, scenes.pack_sun(0.6, 1.2, 1.0, False), sky,
                scenes.look_at_camera((2.5, 8.5, 2.5), (10.0, 3.0, 10.0), 80.0), width, height, "room_" + kind)
    if kind == "entity":
        tris = np.concatenate([_sheet(((x + 0.1, z + 0.1), (x + 0.9, z + 0.9)), 5.5 + (i % 3), 2, m["lamp"]) for i, (x, _y, z) in enumerate(spots)])
        wn, wtr = scenes.build_bvh(tris, 2)
        sc = dataclasses.replace(sc, world_bvh=wn, bvh_trigs=wtr)
    return sc


# ---- what the census counts and the GPU tests compare: option sets on the variant each of them needs ----
OPTION_SETS = {"nee": ("exhibit", dict(nee=1)),
               "nee_bsdf": ("exhibit", dict(nee=1, bsdf=1)),
               "nee_bsdf_sun1": ("exhibit_nosun", dict(nee=1, bsdf=1, sun_sampling=1)),
               "sun0": ("exhibit", dict(sun_sampling=0)),
               "emitters0_nee": ("exhibit", dict(emitters=0, nee=1))}
# classes of events the exhibit has to show (oracle/binding.py EXT_COUNTER_NAMES); the rest is recorded only: dist <= 0.002 and the two
# index clamps are all but unreachable, and the exhibit has no emitter leaf above level 2
CENSUS_CLASSES = (tuple(f"nee_level{i}" for i in range(3)) + tuple(f"nee_face{i}" for i in range(6))
                  + ("nee_rej_cs", "nee_rej_cl", "nee_gate", "nee_occluded", "nee_free", "spec_rough0", "spec_rough", "spec_flip",
                     "sun_rays_auto", "sun_rays_forced", "sun_off_skipped", "an_none", "an_listed", "an_model", "an_emit_tex", "an_entity"))
CENSUS_EXEMPT = ("nee_level3", "nee_clamp_k", "nee_clamp_face", "nee_rej_dist")


def seeds():
    return scenes.java_random_ints(N_PASSES)


def expected(port, name, opts, emitters=None, **port_options):
    """The restatement's image of variant `name` under the extended options `opts` (and, with `emitters`, the test's own copy of
    the emitter list in place of the scene's)."""
    from oracle.binding import PortExt, PortOptions
    sc = make(name)
    ext = PortExt(port, sc, **opts)
    if emitters is not None:
        ext.emitters = np.ascontiguousarray(emitters, np.int32)
        ext.n_emitters = len(ext.emitters)
    with ext, PortOptions(port, **port_options):
        return port.render_passes(sc, seeds())
