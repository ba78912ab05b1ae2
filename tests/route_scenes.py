"""A world of exhibits for the material and model-block routes that no other fixture reaches (tests/golden/routes.npz: outputs of
the reference build; tests/test_routes_cpu.py, tests/test_gpu_routes.py).

Found by coverage of oracle/port.c over the ten golden scenes: the biome-water tint (tint type 3, K/material.h:69-71) and the
emittance texture (material flag 2, K/material.h:76-77) ran zero times, and behind flag 2 sit the model blocks that
scene_records.cpp derive_records leaves on the packed palettes (more than 255 primitives, a material pointer that is no multiple of
6, a quad whose material has flag 2) and the entity BVHs build_bvh_records refuses (a leaf of more than 63 triangles, a triangle
material that is not a whole material).  Every exhibit below is a patch of identical blocks a cell apart on a stone floor, so that
camera, bounce and shadow rays all meet it; ROUTES says how a trace record is recognised as belonging to it.  Every pointer stays
inside its array."""
import dataclasses

import numpy as np

from chunkyclplugin_amd import scenes

W, H = 96, 64
N_PASSES = 4
DEPTH = 6
RECORD_GIDS = np.arange(0, W * H, 7, dtype=np.int32)
EMBED_DEPTHS = {7: 17, 11: 18, 16: 0}            # embedded depth -> tree form the render kernels pick there
ENTITY_SCENES = ["routes_tris", "routes_leaf63", "routes_leaf64", "routes_tri_mod6"]
NAMES = ["routes"] + [f"routes_d{d}" for d in EMBED_DEPTHS] + ENTITY_SCENES
RECORD_SCENES = ["routes"] + ENTITY_SCENES        # the scenes whose trace records routes.npz holds
HELPER_KINDS = [4, 12]
FLOOR_TOP = 2                                     # the exhibits stand on y = 2
SHEET_Y = 6.0                                     # the entity sheets hover here: nothing else of the world reaches above y = 3
PITCH = 7
TEX16 = (16 << 16) | 16


def _material(pal, flags, tint, size, color, ne, spec=0):
    """One raw material record (PackedMaterial.java:89-100): flags (2 = emittance texture, 4 = colour texture), tint, texture
    size, colour (ARGB or atlas location), normal_emittance (byte, or atlas location with flag 2), word 5."""
    ptr = len(pal.materials)
    pal.materials += [flags, tint, size, color, ne, spec]
    return ptr


def _share(pal, kind, block):
    """A second palette block on the model of block `block` (models are shared between blocks: aabb_at / quad_at)."""
    assert pal.blocks[2 * block] == kind
    k = len(pal.blocks) // 2
    pal.blocks += [kind, pal.blocks[2 * block + 1]]
    return k


def _tent(mat, height=0.7, top_mat=None):
    """Five quads: a lid facing up and four walls facing outwards (quads are one-sided: K/primitives.h:298)."""
    h = height
    uv = (0.0, 1.0, 0.0, 1.0)
    return [((0.1, h, 0.1), (0, 0, 0.8), (0.8, 0, 0), uv, mat if top_mat is None else top_mat, 1),
            ((0.1, 0, 0.1), (0, h, 0), (0.8, 0, 0), uv, mat, 1),
            ((0.1, 0, 0.9), (0.8, 0, 0), (0, h, 0), uv, mat, 1),
            ((0.1, 0, 0.1), (0, 0, 0.8), (0, h, 0), uv, mat, 1),
            ((0.9, 0, 0.1), (0, h, 0), (0, 0, 0.8), uv, mat, 1)]


def _layers(n, wall_mat, layer_mat):
    """n quads: four walls and n - 4 lids stacked in a shuffled order; `layer_mat` has texels of alpha 0, so the closest-hit loop
    runs past the first quad it meets."""
    quads = _tent(wall_mat, 0.95)[1:]
    m = n - 4
    for i in range(m):
        y = 0.04 + 0.9 * ((i * 37) % m) / m
        quads.append(((0.1, y, 0.1), (0, 0, 0.8), (0.8, 0, 0), (0.125 * (i % 5), 0.5, 0.125 * (i % 3), 0.5), layer_mat, 1))
    assert len(quads) == n
    return quads


def _pyramid(n, mats, reverse=False):
    """n thin slabs stacked into a stepped pyramid; faces rotated and mirrored by their flag nibbles, some hidden by flag 8."""
    boxes = []
    for i in range(n):
        s = i / (2.5 * n)
        east = 8 if i % 5 == 2 else (i * 5) & 7
        top = 8 if (i % 4 == 1 and i != n - 1) else i & 7
        flags = (east << 4) | (((i * 3) & 7) << 8) | (((i * 7) & 7) << 12) | (top << 16) | ((i & 3) << 20)
        face = tuple(mats[(i + k) % len(mats)] for k in range(6))
        boxes.append(((s, 1 - s, i / n, (i + 1) / n, s, 1 - s), flags, face))
    return boxes[::-1] if reverse else boxes


def _base():
    rng = np.random.default_rng(20261019)
    ab = scenes.AtlasBuilder(8, 8)
    ramp = np.zeros((16, 16, 4), np.uint8)            # the emittance texture: alpha over 0 ... 255, both ends included
    ramp[..., :3] = 128
    ramp[..., 3] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    tex = {"stone": ab.add(scenes.noise_texture(rng, (125, 125, 125), 14)),
           "plank": ab.add(scenes.noise_texture(rng, (162, 130, 78), 10)),
           "water": ab.add(scenes.noise_texture(rng, (200, 200, 200), 12)),
           "lava": ab.add(scenes.noise_texture(rng, (230, 120, 40), 20)),
           "crystal": ab.add(scenes.noise_texture(rng, (120, 200, 220), 20)),
           "holes": ab.add(scenes.noise_texture(rng, (120, 160, 120), 30, holes=0.5)),
           "glow": ab.add(scenes.noise_texture(rng, (250, 220, 150), 5)),
           "ramp": ab.add(ramp),
           "sun": ab.add(scenes.noise_texture(rng, (255, 250, 230), 4, size=32))}
    atlas, recs = ab.build()
    loc = {k: recs[v][1] for k, v in tex.items()}
    assert all(recs[v][0] == TEX16 for k, v in tex.items() if k != "sun")

    pal = scenes.Palettes()
    word5 = lambda spec, metal, rough: spec | (metal << 8) | (rough << 16)
    m = {"stone": _material(pal, 4, 0, TEX16, loc["stone"], 0, word5(0, 0, 0)),
         "plank": _material(pal, 4, 0, TEX16, loc["plank"], 0, word5(60, 0, 90)),
         "holes": _material(pal, 4, 1 << 24, TEX16, loc["holes"], 0, 0),
         "water": _material(pal, 4, 3 << 24, TEX16, loc["water"], 0, word5(200, 0, 10)),
         "water_flat": _material(pal, 0, 3 << 24, 0, 0xFFD0E0F0, 0, 0),
         "emit6a": _material(pal, 6, 0, TEX16, loc["lava"], loc["ramp"], 0),
         "emit6b": _material(pal, 6, 2 << 24, TEX16, loc["crystal"], loc["ramp"], word5(90, 255, 40)),
         "emit2": _material(pal, 2, 0, TEX16, 0xFFE0A060, loc["ramp"], 0),
         "glow": _material(pal, 4, 0, TEX16, loc["glow"], 255, 0)}
    pal.materials += [0, 0, 0]                        # one well-formed material at a pointer = 3 (mod 6) ...
    m["mod6"] = _material(pal, 4, 0xFF000000 | 0xC080F0, TEX16, loc["plank"], 40, word5(30, 0, 128))
    pal.materials += [0, 0, 0]                        # ... and the palette's length a multiple of 6 again
    assert m["mod6"] % 6 == 3 and len(pal.materials) % 6 == 0

    B = {"air": pal.block_invisible()}
    for k in ("stone", "water", "water_flat", "emit6a", "emit2", "glow"):
        B[k] = pal.block_cube(m[k])
    B["water_box"] = pal.block_aabbs([((0.3, 0.7, 0, 1, 0.3, 0.7), 0, (m["water"],) * 6),
                                      ((0, 1, 0.4, 0.6, 0.4, 0.6), 0b0101 << 4 | 0b0010 << 16, (m["water"],) * 6)])
    B["water_quad"] = pal.block_quads(_tent(m["water"]))
    B["emit_box"] = pal.block_aabbs([((0.1, 0.9, 0, 0.8, 0.1, 0.9), 0b0001 << 4 | 0b0110 << 12 | 0b0011 << 16,
                                     (m["emit6a"], m["emit6a"], m["emit6b"], m["emit6a"], m["emit6b"], m["emit6a"]))])
    B["emit_quad"] = pal.block_quads(_tent(m["emit6a"], top_mat=m["emit6b"]))
    B["plain_quad"] = pal.block_quads(_tent(m["plank"], top_mat=m["holes"]))
    faces = (m["plank"], m["stone"], m["holes"], m["plank"], m["water"])
    B["box255"] = pal.block_aabbs(_pyramid(255, faces))
    B["box256"] = pal.block_aabbs(_pyramid(256, faces, reverse=True))
    B["quad255"] = pal.block_quads(_layers(255, m["plank"], m["holes"]))
    B["quad256"] = pal.block_quads(_layers(256, m["stone"], m["holes"]))
    B["mat_mod6_box"] = pal.block_aabbs([((0, 1, 0, 0.5, 0, 1), 0b0110 << 4 | 0b0101 << 12, (m["plank"], m["mod6"], m["plank"], m["mod6"], m["mod6"], m["plank"])),
                                         ((0.25, 0.75, 0.5, 1, 0.25, 0.75), 0, (m["mod6"],) * 6)])
    B["mat_mod6_quad"] = pal.block_quads(_tent(m["plank"], top_mat=m["mod6"])[:1] + _tent(m["mod6"])[1:])
    B["shared_box_a"] = pal.block_aabbs([((0.2, 0.8, 0, 0.6, 0.2, 0.8), 0b0011 << 8, (m["plank"], m["stone"], m["plank"], m["stone"], m["holes"], m["plank"])),
                                         ((0.4, 0.6, 0.6, 1, 0.4, 0.6), 0, (m["stone"],) * 6)])
    B["shared_box_b"] = _share(pal, 2, B["shared_box_a"])
    B["shared_quad_a"] = pal.block_quads(_tent(m["stone"], 0.5, top_mat=m["plank"]))
    B["shared_quad_b"] = _share(pal, 3, B["shared_quad_a"])
    B["zero_box"] = pal.block_aabbs([])               # count 0: never hits
    B["zero_quad"] = pal.block_quads([])

    S = 1 << DEPTH
    t = np.zeros((S, S, S), np.int32)
    t[:, :FLOOR_TOP, :] = B["stone"]
    y = FLOOR_TOP

    def patch(slot, a, b=None, fill=None):
        """3 x 3 blocks `a` a cell apart in slot `slot` of the 5 x 4 grid; `b` alternates with `a`; `fill` goes between them along x."""
        x0, z0 = 3 + PITCH * (slot % 5), 3 + PITCH * (slot // 5)
        for i in range(3):
            for j in range(3):
                t[x0 + 2 * i, y, z0 + 2 * j] = B[a] if b is None or (i + j) % 2 == 0 else B[b]
                if fill is not None and i < 2:
                    t[x0 + 2 * i + 1, y, z0 + 2 * j] = B[fill]

    x0, z0 = 3, 3
    t[x0:x0 + 6, y, z0:z0 + 6] = B["water"]           # water_cube: a raised pond of 6 x 6 full cubes
    for slot, args in enumerate([("water_flat",), ("water_box",), ("water_quad",), ("emit6a",), ("emit2",), ("emit_box",),
                                 ("emit_quad", None, "plain_quad"), ("box255",), ("box256",), ("quad255",), ("quad256",),
                                 ("mat_mod6_box",), ("mat_mod6_quad",), ("shared_box_a", "shared_box_b"),
                                 ("shared_quad_a", "shared_quad_b"), ("zero_box", "zero_quad"), ("glow",)], start=1):
        patch(slot, *args)
    blocks, mats, aabbs, quads = pal.arrays()
    alt, azi, inten = 0.6, 1.2, 1.25
    sc = scenes.PackedScene(octree=scenes.build_octree(t, DEPTH), octree_depth=DEPTH, block_palette=blocks, material_palette=mats,
                            aabb_models=aabbs, quad_models=quads, world_bvh=scenes.empty_bvh(), actor_bvh=scenes.empty_bvh(),
                            bvh_trigs=np.zeros(1, np.int32), atlas=atlas, sky=scenes.bake_sky(64, scenes.sun_direction(alt, azi)),
                            sky_intensity=inten, sun=scenes.pack_sun(alt, azi, inten, True, recs[tex["sun"]]),
                            camera=scenes.look_at_camera((20.0, 30.0, 1.5), (20.0, 2.0, 15.5), 52.0), width=W, height=H, name="routes")
    return sc, {k: 2 * v for k, v in B.items()}, m


_CACHE = {}


def base():
    """(the depth-6 scene `routes`, block pointers by exhibit name, material pointers by name)"""
    if "base" not in _CACHE:
        _CACHE["base"] = _base()
    return _CACHE["base"]


# ---- entity variants: sheets of triangles hovering over the exhibits at y = SHEET_Y ----
SHEETS = {"tris_emit": ((5.0, 8.0), (19.0, 18.0)), "tris_water": ((21.0, 8.0), (35.0, 18.0)),
          "leaf": ((6.0, 8.0), (34.0, 18.0)), "small": ((10.0, 22.0), (14.0, 26.0)), "tri_mod6": ((8.0, 8.0), (32.0, 18.0))}


def _sheet(rect, n, mats):
    """n triangles (int32 [n, 20]): the rectangle cut into strips of two triangles each (an odd n leaves half of the last strip
    open), facing up, every other strip two-sided; triangle i takes mats[i % len(mats)]."""
    (xa, za), (xb, zb) = rect
    strips = (n + 1) // 2
    out = []
    for i in range(n):
        k = i // 2
        x0, x1 = xa + (xb - xa) * k / strips, xa + (xb - xa) * (k + 1) / strips
        ds = k % 2 == 0
        mat = mats[i % len(mats)]
        if i % 2 == 0:
            out.append(scenes.pack_triangle((x0, SHEET_Y, za), (x1, SHEET_Y, za), (x0, SHEET_Y, zb), (0, 0), (1, 0), (0, 1), mat, ds))
        else:
            out.append(scenes.pack_triangle((x1, SHEET_Y, zb), (x0, SHEET_Y, zb), (x1, SHEET_Y, za), (1, 1), (0, 1), (1, 0), mat, ds))
    return np.array(out, np.int64).astype(np.int32).reshape(-1, 20)


def _bounds(tris):
    f = tris[:, 1:13].copy().view(np.float32).reshape(len(tris), 4, 3)
    v = np.concatenate([f[:, 2], f[:, 2] + f[:, 0], f[:, 2] + f[:, 1]])
    lo, hi = v.min(axis=0), v.max(axis=0)
    return [scenes.f2i(lo[0]), scenes.f2i(hi[0]), scenes.f2i(lo[1]), scenes.f2i(hi[1]), scenes.f2i(lo[2]), scenes.f2i(hi[2])]


def _two_leaves(a, b):
    """A BVH of one inner node over two leaves holding all of `a` and all of `b` (PackedBvhNode.java:16-31)."""
    both = np.concatenate([a, b])
    nodes = [14] + _bounds(both) + [0] + _bounds(a) + [-(1 + 20 * len(a))] + _bounds(b)
    trigs = np.concatenate([[len(a)], a.reshape(-1), [len(b)], b.reshape(-1)])
    return np.array(nodes, np.int64).astype(np.int32), trigs.astype(np.int32)


def make(name: str) -> scenes.PackedScene:
    sc, _B, m = base()
    if name == "routes":
        return sc
    if name.startswith("routes_d"):
        return scenes.embed_deeper(sc, int(name[len("routes_d"):]))
    if name == "routes_tris":    # flags-6 triangles in the world BVH, tint-3 triangles in the actor BVH: both on records
        wn, wtr = scenes.build_bvh(_sheet(SHEETS["tris_emit"], 16, [m["emit6a"], m["emit6b"]]), 4)
        an, atr = scenes.build_bvh(_sheet(SHEETS["tris_water"], 16, [m["water"], m["water_flat"]]), 4)
        an = an.copy().reshape(-1, 7)
        an[an[:, 0] <= 0, 0] -= len(wtr)
        return dataclasses.replace(sc, world_bvh=wn, actor_bvh=an.reshape(-1), bvh_trigs=np.concatenate([wtr, atr]), name=name)
    if name in ("routes_leaf63", "routes_leaf64"):   # 63 triangles in one leaf fit a record reference, 64 do not
        n = int(name[-2:])
        wn, wtr = _two_leaves(_sheet(SHEETS["leaf"], n, [m["plank"], m["holes"], m["water"]]), _sheet(SHEETS["small"], 2, [m["stone"]]))
        return dataclasses.replace(sc, world_bvh=wn, bvh_trigs=wtr, name=name)
    if name == "routes_tri_mod6":  # one triangle whose material pointer is no multiple of 6
        tris = _sheet(SHEETS["tri_mod6"], 8, [m["plank"]])
        tris[5, 19] = m["mod6"]
        wn, wtr = scenes.build_bvh(tris, 4)
        return dataclasses.replace(sc, world_bvh=wn, bvh_trigs=wtr, name=name)
    raise KeyError(name)


def _in_sheet(rect, lo=0.0, hi=1.0):
    """The part [lo, hi] (along x) of a sheet as a box round the points of its hits."""
    (xa, za), (xb, zb) = rect
    return ((xa + (xb - xa) * lo, SHEET_Y - 0.01, za), (xa + (xb - xa) * hi, SHEET_Y + 0.01, zb))


def routes():
    """Route name -> how its trace records are recognised: {"scene", "blocks": block pointers (record.material), "materials": the
    material pointers behind it} for block exhibits, {"scene", "box": (lo, hi) round record.point, "materials"} for the entity sheets
    (a triangle hit leaves record.material as the octree left it, K/bvh.h:60-66)."""
    _sc, B, m = base()
    blk = lambda names, mats: {"scene": "routes", "blocks": tuple(B[k] for k in names), "materials": tuple(m[k] for k in mats)}
    r = {"water_cube": blk(["water"], ["water"]), "water_flat": blk(["water_flat"], ["water_flat"]),
         "water_box": blk(["water_box"], ["water"]), "water_quad": blk(["water_quad"], ["water"]),
         "emit_cube6": blk(["emit6a"], ["emit6a"]), "emit_cube2": blk(["emit2"], ["emit2"]),
         "emit_box": blk(["emit_box"], ["emit6a", "emit6b"]), "emit_quad": blk(["emit_quad"], ["emit6a", "emit6b"]),
         "plain_quad": blk(["plain_quad"], ["plank", "holes"]),
         "box255": blk(["box255"], ["plank", "stone", "holes", "water"]), "box256": blk(["box256"], ["plank", "stone", "holes", "water"]),
         "quad255": blk(["quad255"], ["plank", "holes"]), "quad256": blk(["quad256"], ["stone", "holes"]),
         "mat_mod6_box": blk(["mat_mod6_box"], ["mod6", "plank"]), "mat_mod6_quad": blk(["mat_mod6_quad"], ["mod6", "plank"]),
         "shared_box_a": blk(["shared_box_a"], ["plank", "stone", "holes"]), "shared_box_b": blk(["shared_box_b"], ["plank", "stone", "holes"]),
         "shared_quad_a": blk(["shared_quad_a"], ["stone", "plank"]), "shared_quad_b": blk(["shared_quad_b"], ["stone", "plank"])}
    ent = lambda scene, box, mats: {"scene": scene, "box": box, "materials": tuple(m[k] for k in mats)}
    r["tris_emit"] = ent("routes_tris", _in_sheet(SHEETS["tris_emit"]), ["emit6a", "emit6b"])
    r["tris_water"] = ent("routes_tris", _in_sheet(SHEETS["tris_water"]), ["water", "water_flat"])
    r["leaf63"] = ent("routes_leaf63", _in_sheet(SHEETS["leaf"]), ["plank", "holes", "water"])
    r["leaf64"] = ent("routes_leaf64", _in_sheet(SHEETS["leaf"]), ["plank", "holes", "water"])
    r["tri_mod6"] = dict(ent("routes_tri_mod6", _in_sheet(SHEETS["tri_mod6"], 0.5, 0.75), ["mod6"]), upper=True)   # triangle 5: half of the two-sided strip 2 of 4
    return r


# what scene_records.cpp has to decide per exhibit: True = aligned records (block_info word 7 != 0), False = the packed palettes
ON_RECORDS = {"water_box": True, "water_quad": True, "emit_box": True, "emit_quad": False, "plain_quad": True, "box255": True,
              "box256": False, "quad255": True, "quad256": False, "mat_mod6_box": False, "mat_mod6_quad": False,
              "shared_box_a": True, "shared_box_b": True, "shared_quad_a": True, "shared_quad_b": True, "zero_box": False, "zero_quad": False}
BVH_ON_RECORDS = {"routes_tris": True, "routes_leaf63": True, "routes_leaf64": False, "routes_tri_mod6": False}
NEVER_HIT = ["zero_box", "zero_quad"]


def classify(records, route):
    """Boolean mask over `records` (binding.HIT_DTYPE, any shape): the hits that belong to `route` (one entry of routes())."""
    hit = records["hit"] == 1
    if "blocks" in route:
        return hit & np.isin(records["material"], route["blocks"])
    lo, hi = (np.asarray(v, np.float32) for v in route["box"])
    p = records["point"]
    inside = hit & ((p >= lo) & (p <= hi)).all(axis=-1)
    if route.get("upper"):   # the second triangle of the strip only: beyond the strip's diagonal
        inside &= (p[..., 0] - lo[0]) / (hi[0] - lo[0]) + (p[..., 2] - lo[2]) / (hi[2] - lo[2]) > 1.001
    return inside


def all_records(tracer, sc, seeds, gids=None):
    """(records [len(gids), len(seeds), MAX_TRACES], counts [len(gids), len(seeds)]) of `tracer` (port or the reference build)."""
    from oracle import binding
    h = binding.SceneHandle(sc)
    gids = np.arange(sc.width * sc.height) if gids is None else np.asarray(gids)
    rec = np.zeros((len(gids), len(seeds), binding.MAX_TRACES), binding.HIT_DTYPE)
    cnt = np.zeros((len(gids), len(seeds)), np.int32)
    for i, g in enumerate(gids):
        for k, s in enumerate(seeds):
            r, _rad = tracer.trace_records(h, int(s), int(g))
            rec[i, k, :len(r)] = r
            cnt[i, k] = len(r)
    return rec, cnt


def census(tracer, seeds):
    """Route name -> {"records": hits of the route over every pixel x seed, "later": those that are not record 0}."""
    out = {}
    cache = {}
    for name, route in routes().items():
        if route["scene"] not in cache:
            cache[route["scene"]] = all_records(tracer, make(route["scene"]), seeds)[0]
        mask = classify(cache[route["scene"]], route)
        out[name] = {"records": int(mask.sum()), "later": int(mask[..., 1:].sum())}
    return out


def helper_rows(which):
    """golden_scenes.helper_rows on the `routes` palettes (kind 4: BlockPalette_intersectBlock, 12: Material_sample)."""
    import golden_scenes as gs
    return gs.helper_rows(base()[0], which)


# ---- the fixture (tests/golden/routes.npz, written by tests/golden/generate.py write_routes) ----
def fixture():
    import os
    if "fixture" not in _CACHE:
        _CACHE["fixture"] = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "routes.npz"))
    return _CACHE["fixture"]


def fixture_records(name):
    """(records [len(RECORD_GIDS), MAX_TRACES], counts, radiance) of scene `name` as the fixture holds them."""
    from oracle import binding
    g = fixture()
    cnt = g[name + "_counts"]
    flat = g[name + "_records"]
    rec = np.zeros((len(cnt), binding.MAX_TRACES), binding.HIT_DTYPE)
    at = 0
    for i, n in enumerate(cnt):
        rec[i, :n] = flat[at:at + n]
        at += n
    assert at == len(flat)
    return rec, cnt, g[name + "_radiance"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def first_difference(got, want, what=""):
    """None where two arrays are equal bit for bit, else a sentence about the first element that differs."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    if got.shape != want.shape:
        return f"{what}: {got.shape} values against {want.shape}"
    bad = np.flatnonzero(_bits(got) != _bits(want))
    if len(bad) == 0:
        return None
    return f"{what}: {len(bad)} of {got.size} values differ, first at {int(bad[0])}: {got[bad[0]]!r} against {want[bad[0]]!r}"


def records_difference(got, got_counts, want, want_counts, what=""):
    """None where the trace records agree bit for bit (hit, material, distance, normal, colour, emittance of every trace; the point
    of every hit), else the pixel, trace and field of the first difference."""
    if not np.array_equal(got_counts, want_counts):
        i = int(np.flatnonzero(np.asarray(got_counts) != np.asarray(want_counts))[0])
        return f"{what}: gid {int(RECORD_GIDS[i])} has {int(got_counts[i])} traces against {int(want_counts[i])}"
    for i, n in enumerate(want_counts):
        for k in range(int(n)):
            a, b = got[i, k], want[i, k]
            fields = ("hit", "material", "distance", "normal", "color", "emittance") + (("point",) if b["hit"] == 1 else ())
            for f in fields:
                if _bits(a[f]).tolist() != _bits(b[f]).tolist():
                    return f"{what}: gid {int(RECORD_GIDS[i])} trace {k} field {f}: {a[f]!r} against {b[f]!r} (block pointer {int(b['material'])})"
    return None


def __getattr__(name):
    if name == "ROUTES":   # route name -> the block and material pointers (or the box) that identify it in a trace record: routes()
        return routes()
    raise AttributeError(name)
