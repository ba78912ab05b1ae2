"""Scene updates: the table of transitions behind tests/test_scene_updates_cpu.py and tests/test_gpu_scene_updates.py.

Every chunky_scene_set_* call, chunky_scene_load_octree and chunky_scene_write_atlas_tile may be called again on a scene that render
targets already use; capi_scene.hip rebuilds what it derives from the changed array (wide tree, block_info, mat8, aabb_rec, quad_rec,
quad_aux, bvh_rec, the emitter list, model_leaf_permille, addr32) from four dirty flags.  A case here is a chain of scenes, all at the
golden 64 x 48 view: the GPU test walks one scene object and one render target along it and compares every output with a fresh
upload of the same contents and with the oracle.  For a single-field case `stale(k)` is step k's scene with the changed source
array(s) of the step before: what a forgotten invalidation would render.  The CPU test checks, on the oracle alone, that every step
and every stale hybrid differ from what they should differ from in at least 1 % of the pixels, and pins the inputs' digests.

Which entry point is called on an already-rendered scene by which case (SETTERS below says the same, per case):

    chunky_scene_set_octree            octree_swap_ids, octree_resize, every chain_*
    chunky_scene_load_octree           octree_load_mapping
    chunky_scene_set_palette  BLOCK    blocks_kinds, blocks_to_sorted, blocks_to_unsorted
                              MATERIAL materials_words, atlas_to_layers
                              AABB     aabbs_bounds
                              QUAD     quads_vectors
                              TRIG     trigs_words
    chunky_scene_set_bvh      WORLD    world_bvh_empty, both_bvhs_empty
                              ACTOR    actor_bvh_empty, both_bvhs_empty
    chunky_scene_set_atlas             atlas_texels, atlas_more_layers, atlas_to_layers (and with NULL: the tile test)
    chunky_scene_write_atlas_tile      tile_writes() (test_atlas_tile_writes)
    chunky_scene_set_sky               sky_texels, sky_sizes, sky_intensity
    chunky_scene_set_sun               sun_direction, sun_flag, sun_texture
"""
import dataclasses
import functools
from typing import Optional, Tuple

import numpy as np

import golden_scenes as gs
import route_scenes
from chunkyclplugin_amd import scenes

W, H = gs.W, gs.H
N_PASSES = 3
MIN_DIFFERENT = 0.01          # of the pixels, in float bits (image) or ARGB words (preview)

# PackedScene field -> the upload it travels through (load_packed's names); sky_intensity rides with the sky, the depth with the octree
PIECE_OF = {"octree": "octree", "octree_depth": "octree", "block_palette": "blocks", "material_palette": "materials",
            "aabb_models": "aabbs", "quad_models": "quads", "bvh_trigs": "trigs", "world_bvh": "world_bvh", "actor_bvh": "actor_bvh",
            "atlas": "atlas", "sky": "sky", "sky_intensity": "sky", "sun": "sun"}
LOAD_PACKED_ORDER = ("octree", "blocks", "materials", "aabbs", "quads", "trigs", "world_bvh", "actor_bvh", "atlas", "sky", "sun")
# "entities" through the raw setters in another order: the result must be the load_packed scene
UPLOAD_ORDERS = {
    "reversed": LOAD_PACKED_ORDER[::-1],
    "palettes_first": ("blocks", "materials", "aabbs", "quads", "trigs", "octree", "world_bvh", "actor_bvh", "atlas", "sky", "sun"),
    "bvhs_before_triangles": ("octree", "world_bvh", "actor_bvh", "blocks", "materials", "aabbs", "quads", "trigs", "atlas", "sky", "sun"),
    "atlas_sky_sun_first": ("atlas", "sky", "sun", "octree", "blocks", "materials", "aabbs", "quads", "trigs", "world_bvh", "actor_bvh"),
    "interleaved": ("sun", "trigs", "materials", "actor_bvh", "octree", "sky", "quads", "world_bvh", "blocks", "atlas", "aabbs"),
}
# scene_view's order of complaints: (pieces installed at that point, what the message has to name); the last row is complete
INCOMPLETE_STEPS = [((), "octree"), (("octree",), "block/material palette"), (("blocks",), "block/material palette"),
                    (("materials", "aabbs", "quads"), "atlas"), (("atlas",), "sky"), (("sky",), "sun"),
                    (("sun", "world_bvh", "actor_bvh"), "a BVH but no triangles"), (("trigs",), None)]


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    chain: Tuple[scenes.PackedScene, ...]   # chain[0] is uploaded whole and rendered; every later scene is one update of the same object
    fields: Tuple[str, ...] = ()            # the PackedScene fields that change between neighbours; () = everything (load_packed)
    via: str = "setters"                    # "setters" | "load_octree" | "load_packed"
    single: bool = True                     # one source array: stale() exists
    shard: Optional[Tuple[int, int, int]] = None

    @property
    def before(self):
        return self.chain[0]

    @property
    def after(self):
        return self.chain[1]

    def steps(self):
        return list(zip(self.chain[:-1], self.chain[1:]))

    def stale(self, k: int = 1):
        """chain[k] with the changed source array(s) of chain[k - 1]"""
        assert self.single and 1 <= k < len(self.chain)
        return dataclasses.replace(self.chain[k], **{f: getattr(self.chain[k - 1], f) for f in self.fields})

    def pieces(self):
        return tuple(dict.fromkeys(PIECE_OF[f] for f in self.fields))


@functools.lru_cache(maxsize=None)
def golden(name, chunks=2):
    return gs.make(name, chunks)


def _ptr(k):
    return 2 * k


# block-palette indices of scenes.outdoor_world
AIR, BEDROCK, STONE, DIRT, GRASS, SAND, LOG, LEAVES, PLANK, GLOW, SNOW, FLAT, SLAB, POST, PLANT = range(15)
# material indices (6 ints each)
M_BEDROCK, M_STONE, M_DIRT, M_SAND, M_LOG, M_PLANK, M_SNOW, M_GRASS, M_LEAVES, M_PLANT, M_GLOW, M_FLAT = range(12)


def swap_leaves(octree, pairs):
    """The same tree (same ints, same branches) with the leaf values of block a and block b exchanged, for every (a, b)."""
    t = np.asarray(octree, np.int32).copy()
    for a, b in pairs:
        ia, ib = t == -_ptr(a), t == -_ptr(b)
        assert ia.any() and ib.any(), (a, b)
        t[ia], t[ib] = -_ptr(b), -_ptr(a)
    return t


def remapped(octree, n_blocks, seed=3):
    """(treeData, blockMapping) for chunky_scene_load_octree whose remap gives `octree`: leaves hold -j for a shuffled numbering j of
    the blocks, blockMapping[j] the block pointer.  Not the identity, and j = 0 is not air."""
    rng = np.random.default_rng(seed)
    number = rng.permutation(n_blocks)           # block k is number[k] in treeData
    while number[0] == 0 or (number == np.arange(n_blocks)).any():
        number = rng.permutation(n_blocks)
    mapping = np.zeros(n_blocks, np.int32)
    mapping[number] = 2 * np.arange(n_blocks)
    raw = np.asarray(octree, np.int32).copy()
    leaf = (raw <= 0) & (raw != -scenes.ANY_TYPE)
    raw[leaf] = -number[(-raw[leaf]) // 2]
    back = raw.copy()
    back[leaf] = -mapping[-raw[leaf]]
    assert np.array_equal(back, octree)
    return raw, mapping


def model_leaf_permille(sc):
    """scene_records.cpp model_leaf_permille: what scene_view compares with kSortBlocksPermille"""
    t = np.asarray(sc.octree, np.int64)
    b = np.asarray(sc.block_palette, np.int64)
    p = -t[t <= 0]
    p = p[(p != 0) & (p + 1 < len(b))]
    kind = b[p]
    cubes, models = int((kind == 1).sum()), int(((kind == 2) | (kind == 3)).sum())
    return models * 1000 // (cubes + models) if cubes + models else 0


SORT_BLOCKS_PERMILLE = 30     # scene_records.hpp kSortBlocksPermille
# octree depth -> tree form of the wide re-layout (widetree.cpp's default split; golden_scenes.EMBED_FORM): one dense node at depth 6,
# a dense top over two 8^3 levels at 11 - 13, over three at 14 - 15, no wide tree above 15
TREE_FORM = {6: 16, **gs.EMBED_FORM}


def has_bvh(sc):
    return not (np.array_equal(sc.world_bvh, scenes.empty_bvh()) and np.array_equal(sc.actor_bvh, scenes.empty_bvh()))


def expected_kernel(sc):
    """What kernel_info() has to report after a default launch on `sc`, as far as the launch rule (render_pool.hip
    pool_kernel_applies, launch_pool) fixes it for the scenes of this table — all of them small, every index inside its palette,
    so the derived records exist and all three addr32 forms apply.  Stated from the rule, not from a run: a scene object that never
    derives its records, or keeps a stale kernel choice, differs from this even where a fresh scene on the same library agrees
    with it.  Keys: "bvh"; "pool_runs" (render_pool, not a fallback kernel: always, but for entity BVHs without a wide tree);
    without BVHs also "pool" (64 parked paths), and at the depths of TREE_FORM "tree" and "sorted"."""
    form = TREE_FORM.get(int(sc.octree_depth))
    bvh = has_bvh(sc)
    want = {"bvh": bvh, "pool_runs": not (bvh and form == 0)}
    if not bvh:
        want["pool"] = 64
        if form is not None:
            want["tree"] = form
            want["sorted"] = form != 0 and model_leaf_permille(sc) >= SORT_BLOCKS_PERMILLE
    return want


ADDR32_EVERY = 1 | 2 | 4      # native.ADDR32_ATLAS | ADDR32_SKY | ADDR32_RECORDS: every scene here is far below the 32-bit limits


def _blocks(sc, **records):
    b = np.asarray(sc.block_palette, np.int32).copy().reshape(-1, 2)
    for k, rec in records.items():
        b[int(k[1:])] = rec
    return b.reshape(-1)


def _leaves(sc):
    """offsets into bvh_trigs of the first triangle of every leaf of both BVHs, with the leaf's triangle count"""
    out = []
    tr = np.asarray(sc.bvh_trigs)
    for nodes in (sc.world_bvh, sc.actor_bvh):
        n = np.asarray(nodes).reshape(-1, 7)
        if len(n) == 1 and n[0, 0] == 0 and n[0, 1] == scenes.NAN_BITS:
            continue
        for link in n[n[:, 0] <= 0, 0]:
            out.append((int(-link) + 1, int(tr[-link])))
    return out


def sun_view(sc, fov_deg=12.0):
    """The scene seen from its camera's position towards the sun: the disc (0.03 rad) covers a few per cent of the pixels."""
    sun = np.asarray(sc.sun, np.int32).view(np.float32)
    pos = np.asarray(sc.camera[:3], np.float64)
    return dataclasses.replace(sc, camera=scenes.look_at_camera(pos, pos + 50.0 * scenes.sun_direction(float(sun[4]), float(sun[5])), fov_deg))


def _single(name, before, via="setters", **changed):
    return Case(name, (before, dataclasses.replace(before, **changed)), tuple(changed), via)


def _there_and_back(name, before, **changed):
    return Case(name, (before, dataclasses.replace(before, **changed), before), tuple(changed))


@functools.lru_cache(maxsize=None)
def cases():
    E, O = golden("entities"), golden("outdoor")
    out = []

    # ---- octree ----
    out.append(_single("octree_swap_ids", E, octree=swap_leaves(E.octree, [(GRASS, SLAB), (GLOW, DIRT)])))   # same int count: DevBuf::upload copies in place
    O4 = golden("outdoor", 4)
    for f in ("block_palette", "material_palette", "aabb_models", "quad_models", "atlas"):
        assert np.array_equal(getattr(O4, f), getattr(E, f)), f
    assert O4.octree_depth == E.octree_depth and len(O4.octree) != len(E.octree)
    out.append(_single("octree_resize", E, octree=O4.octree))                                                    # another count, same depth: reallocation
    out.append(_single("octree_load_mapping", E, via="load_octree", octree=swap_leaves(E.octree, [(STONE, GRASS), (LOG, LEAVES)])))

    # ---- block palette: leaf ids turn cube -> model, model -> cube, cube -> invisible, invisible -> cube ----
    slab, grass, leaves, glow, bedrock = (E.block_palette.reshape(-1, 2)[k].tolist() for k in (SLAB, GRASS, LEAVES, GLOW, BEDROCK))
    hidden = dataclasses.replace(E, block_palette=_blocks(E, **{f"b{LEAVES}": [0, 0]}))
    out.append(_single("blocks_kinds", hidden, block_palette=_blocks(E, **{f"b{GRASS}": slab, f"b{SLAB}": grass, f"b{LOG}": [0, 0], f"b{LEAVES}": leaves,
                                                                          f"b{GLOW}": bedrock, f"b{BEDROCK}": glow})))   # (and the emitters move: cube <-> cube)
    out.append(_single("blocks_to_sorted", O, block_palette=_blocks(O, **{f"b{GRASS}": slab})))
    R = route_scenes.make("routes").with_view(W, H)
    rb = np.asarray(R.block_palette, np.int32).copy().reshape(-1, 2)
    stone_cube = rb[rb[:, 0] == 1][0].tolist()
    rb[(rb[:, 0] == 2) | (rb[:, 0] == 3)] = stone_cube
    out.append(_single("blocks_to_unsorted", R, block_palette=rb.reshape(-1)))

    # ---- material palette: texture, tint and emittance words ----
    m = np.asarray(E.material_palette, np.int32).copy().reshape(-1, 6)
    m[[M_STONE, M_DIRT, M_GRASS, M_LOG], 3] = m[[M_DIRT, M_GRASS, M_LOG, M_STONE], 3]
    m[M_GRASS, 1] = np.int32(np.uint32(0xFF000000 | 0xC04020).astype(np.int32))
    m[M_LEAVES, 1] = 2 << 24
    m[M_GLOW, 4], m[M_GRASS, 4], m[M_PLANK, 4] = 0, 128, 60
    out.append(_single("materials_words", E, material_palette=m.reshape(-1)))

    # ---- model palettes ----
    a = np.asarray(E.aabb_models, np.int32).copy()
    assert a[0] == 1 and a[14] == 2
    a[4] = scenes.f2i(0.9375)                                      # the slab's top
    a[1], a[2] = scenes.f2i(0.125), scenes.f2i(0.875)
    a[15 + 0], a[15 + 1] = scenes.f2i(0.25), scenes.f2i(0.75)      # the post, thicker in x ...
    a[15 + 3] = scenes.f2i(0.6875)                                 # ... and shorter
    out.append(_single("aabbs_bounds", E, aabb_models=a))
    q = np.asarray(E.quad_models, np.int32).copy()
    assert q[0] == 4 and len(q) == 1 + 4 * 15
    qf = q[1:].reshape(4, 15)[:, :9].copy().view(np.float32)
    qf[:, 1] += 0.25                                               # origins up a quarter, ...
    qf[:, 6:9] *= 0.5                                              # ... half as tall
    qf[:, 3:6] *= np.float32(0.75)
    q[1:].reshape(4, 15)[:, :9] = qf.view(np.int32)
    out.append(_single("quads_vectors", E, quad_models=q))

    # ---- triangles: material words, and vertices moved inside their node's box (edges halved: the BVH's boxes stay valid) ----
    t = np.asarray(E.bvh_trigs, np.int32).copy()
    n_mat = len(E.material_palette) // 6
    for first, n in _leaves(E):
        tri = t[first:first + 20 * n].reshape(n, 20)
        tri[:, 19] = ((tri[:, 19] // 6 + 5) % n_mat) * 6
        e = tri[:, 1:7].copy().view(np.float32)
        tri[:, 1:7] = (e * np.float32(0.5)).view(np.int32)
    out.append(_single("trigs_words", E, bvh_trigs=t))

    # ---- entity BVHs: there, the empty 7-int form, there again ----
    out.append(_there_and_back("world_bvh_empty", E, world_bvh=scenes.empty_bvh()))
    out.append(_there_and_back("actor_bvh_empty", E, actor_bvh=scenes.empty_bvh()))
    out.append(_there_and_back("both_bvhs_empty", E, world_bvh=scenes.empty_bvh(), actor_bvh=scenes.empty_bvh()))

    # ---- atlas ----
    tex = np.asarray(E.atlas, np.uint8).copy()
    tex[..., :3] = 255 - tex[..., :3][..., ::-1]
    out.append(_single("atlas_texels", E, atlas=tex))
    rng = np.random.default_rng(77)
    more = np.concatenate([np.roll(E.atlas, 5, axis=2), rng.integers(0, 256, E.atlas.shape, dtype=np.uint8)])
    more[0, :32, :32] = E.atlas[0, :32, :32]                       # (the sun's texture stays)
    out.append(_single("atlas_more_layers", E, atlas=more))
    AL = golden("atlas_layers")
    assert AL.atlas.shape != E.atlas.shape and np.array_equal(AL.block_palette, E.block_palette)
    EL = dataclasses.replace(E, atlas=AL.atlas, material_palette=AL.material_palette)
    out.append(Case("atlas_to_layers", (E, EL, E), ("atlas", "material_palette"), single=False))

    # ---- sky ----
    sky = np.asarray(E.sky, np.uint8).copy()
    sky[..., :3] = sky[..., :3][..., ::-1] // 2 + 40
    out.append(_single("sky_texels", E, sky=sky))
    wide = np.ascontiguousarray(scenes.bake_sky(64)[::2][:, :, [1, 2, 0, 3]])     # 64 wide, 32 high
    assert wide.shape == (32, 64, 4)
    one = np.array([[[200, 90, 30, 255]]], np.uint8)
    out.append(Case("sky_sizes", (E, dataclasses.replace(E, sky=wide), dataclasses.replace(E, sky=one), E), ("sky",)))
    out.append(_single("sky_intensity", E, sky_intensity=0.4))

    # ---- sun ----
    S = sun_view(E)
    sun = np.asarray(S.sun, np.int32)
    moved = sun.copy()
    moved[4], moved[5] = scenes.f2i(0.62), scenes.f2i(1.22)
    out.append(_single("sun_direction", S, sun=moved))
    flag = sun.copy()
    flag[0] ^= 1
    out.append(_single("sun_flag", S, sun=flag))
    loc = sun.copy()
    loc[2] = (2 << 22) | (2 << 13)                                 # 32 x 32 texels over four of the 16 x 16 textures
    out.append(_single("sun_texture", S, sun=loc))

    # ---- whole scenes on one scene object and one target; each chain returns to its start ----
    I = golden("indoor")
    whole = dict(via="load_packed", single=False)
    out.append(Case("chain_indoor", (O, I, O), **whole))
    out.append(Case("chain_tree_forms", (O, gs.embedded("outdoor", 13), gs.embedded("outdoor", 16), O), **whole))          # forms 16, 18, 0, 16
    fallback = (O, gs.embedded("entities", 16), E, O)                                                                     # pool, fallback, pool with BVH, pool
    out.append(Case("chain_fallback", fallback, **whole))
    out.append(Case("chain_fallback_shard", fallback, shard=(1, 3, 0), **whole))
    # the embeddings above hold the SAME world (scenes.embed_deeper: same image, another tree form), so an image cannot tell their
    # steps apart; these two walk the same forms with a world that changes at every step as well (and add form 19)
    Os = dataclasses.replace(O, octree=swap_leaves(O.octree, [(GRASS, SLAB), (GLOW, DIRT)]))
    Es = dataclasses.replace(E, octree=Os.octree)
    out.append(Case("chain_tree_forms_distinct", (O, scenes.embed_deeper(Os, 13), gs.embedded("outdoor", 16), scenes.embed_deeper(Os, 15), O), **whole))
    out.append(Case("chain_fallback_distinct", (O, scenes.embed_deeper(Es, 16), E, O), **whole))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


SETTERS = {
    "octree_swap_ids": ("set_octree",), "octree_resize": ("set_octree",), "octree_load_mapping": ("load_octree",),
    "blocks_kinds": ("set_palette BLOCK",), "blocks_to_sorted": ("set_palette BLOCK",), "blocks_to_unsorted": ("set_palette BLOCK",),
    "materials_words": ("set_palette MATERIAL",), "aabbs_bounds": ("set_palette AABB",), "quads_vectors": ("set_palette QUAD",),
    "trigs_words": ("set_palette TRIG",), "world_bvh_empty": ("set_bvh WORLD",), "actor_bvh_empty": ("set_bvh ACTOR",),
    "both_bvhs_empty": ("set_bvh WORLD", "set_bvh ACTOR"), "atlas_texels": ("set_atlas",), "atlas_more_layers": ("set_atlas",),
    "atlas_to_layers": ("set_atlas", "set_palette MATERIAL"), "sky_texels": ("set_sky",), "sky_sizes": ("set_sky",),
    "sky_intensity": ("set_sky",), "sun_direction": ("set_sun",), "sun_flag": ("set_sun",), "sun_texture": ("set_sun",),
}
LAUNCH_ORDER_CASES = ("blocks_kinds", "materials_words", "octree_swap_ids")
QUEUED_CASES = ("octree_swap_ids", "octree_resize")     # in-place copy; reallocation


# ---- tile writes ----
def tile_scene():
    """"atlas_layers": thirteen textures over four 32 x 32 layers"""
    return golden("atlas_layers")


def zero_atlas(sc):
    return dataclasses.replace(sc, atlas=np.zeros_like(sc.atlas))


def tile_writes(atlas, seed=11):
    """[(x, y, layer, w, h, rgba)] for chunky_scene_write_atlas_tile that turn a zeroed atlas into `atlas`: 16 x 16 tiles in a shuffled
    order, and among them a tile touching the last row and column of the last layer that is first written with other texels and
    written again later, one full-row strip (w == the atlas's width) over two tiles left out, and a 1 x 1 tile that mends a texel."""
    atlas = np.ascontiguousarray(atlas, np.uint8)
    layers, h, w, _ = atlas.shape
    assert h % 16 == 0 and w % 16 == 0 and w >= 32 and layers >= 2
    rng = np.random.default_rng(seed)
    piece = lambda x, y, l, tw, th: (x, y, l, tw, th, np.ascontiguousarray(atlas[l, y:y + th, x:x + tw]))
    tiles = [(x, y, l) for l in range(layers) for y in range(0, h, 16) for x in range(0, w, 16)]
    strip = (0, 16, 1)                                            # row of tiles y = 16 of layer 1: written as one strip instead
    tiles = [t for t in tiles if not (t[2] == strip[2] and t[1] == strip[1])]
    order = [tiles[i] for i in rng.permutation(len(tiles))]
    last = (w - 16, h - 16, layers - 1)
    writes = [(last[0], last[1], last[2], 16, 16, rng.integers(0, 256, (16, 16, 4), dtype=np.uint8))]   # overwritten below
    px = (5, 7, 0)
    for x, y, l in order:
        wr = piece(x, y, l, 16, 16)
        if (x, y, l) == (0, 0, 0):                               # one texel wrong: the 1 x 1 write mends it
            bad = wr[5].copy()
            bad[px[1], px[0]] ^= 0xFF
            wr = wr[:5] + (bad,)
        writes.append(wr)
    writes.insert(len(writes) // 2, piece(0, strip[1], strip[2], w, 16))
    writes.append(piece(px[0], px[1], px[2], 1, 1))
    return writes


def apply_tiles(shape, writes):
    out = np.zeros(shape, np.uint8)
    for x, y, l, tw, th, rgba in writes:
        out[l, y:y + th, x:x + tw] = rgba
    return out


# ---- a scene in the middle of an update: a shorter triangle palette under the old BVHs ----
def half_updated():
    """("entities", the world BVH's triangles alone, the scene those fit: "entities" without its actor BVH)"""
    E = golden("entities")
    n_world = min(-int(v) for v in np.asarray(E.actor_bvh).reshape(-1, 7)[:, 0] if v <= 0)   # the actor BVH's first leaf starts here
    short = np.ascontiguousarray(E.bvh_trigs[:n_world])
    return E, short, dataclasses.replace(E, bvh_trigs=short, actor_bvh=scenes.empty_bvh())


# ---- digests of every scene of every chain (golden_scenes.input_digest): a generator change must not silently empty a case ----
DIGESTS = {
    "octree_swap_ids": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "0f2bde991d0395b113eb524ce8cb337343158b83989a3d39f3b3bbe083de66cd"),
    "octree_resize": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "8148f88c68489e4fa166dca0f5bd7d47fd03f8aced8868029cd4c2b7bab7652f"),
    "octree_load_mapping": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "8f643cc7f5b1579878a22bd46ec9c2a90730f407eb994836fafe97fdc62ebc05"),
    "blocks_kinds": ("95f93d296ae9363d549fd8e89e6090354bc0f31631ee21e0227a310f642b2f0f",
        "bbdf08dbf29e684ad849be87bc0223bd4abac49048bb081d4f50ad1d29c1c32b"),
    "blocks_to_sorted": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "49f9cf599502ad160a7d996969c53565461b63042d80b4d4bb3858c9feb1d1aa"),
    "blocks_to_unsorted": ("e34d7f472a9fcdbe21c9340b85d316469d8e5904f3897c34fc99e1b0d36db9e2",
        "1b30ead6ee0e6fc5dee143fde538e19e404400dbb6a67c9178d9dbba92336af3"),
    "materials_words": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "0cd0e24ca903fd07ead76811c273f6bbd7b44889137a2131e707e85a17167dce"),
    "aabbs_bounds": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "abc662a5ec81372a339f0e1e3cd966303a9bd71b70740d4574d93594c74832ed"),
    "quads_vectors": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "221df817d0497a581ab4801ea67472d5b47e08347c4dbea762d860878f923ca7"),
    "trigs_words": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "07d56792f8ed49dfcce036bb654dd1507928be534453bb787e67d497c13f28b2"),
    "world_bvh_empty": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "bec7f8658d52c6713da41733b176ccd0a402ecd48c418198ee4485932b557acd",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002"),
    "actor_bvh_empty": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "d511f7cb75441bc1a5fec70aa38921f504b690764b6985c3694515ea4e2913e9",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002"),
    "both_bvhs_empty": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "452cda0b82a99009b1b9847ebc2744d8cae53954d1bb11b2745b7ab922394b1e",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002"),
    "atlas_texels": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "5c763b7f5ec2d832de1b5c738885b1f7d25c2cadaa5d4404fda04b7e5b49888d"),
    "atlas_more_layers": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "2ecd4850a66f15e7c732294c3c11bc21e5417ee0365502490fcf6e2a3e96448c"),
    "atlas_to_layers": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "fec1499e6561e1d1a99b82012a4e79b9d4b679c1a55f8a796fc16bb048ec727f",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002"),
    "sky_texels": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "80beaf3f4cd212177fd4e9d7bb2690bba6b8ca855975201d91b9bc39bd1a6760"),
    "sky_sizes": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "a362d0b78f5541441a15888b880978888b7978849e29f73b667ede4736f6ecc0",
        "fc0a08c27044864295c6045ffef3b8eaa05ed167dbc41e6d13798873c0a5fd28",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002"),
    "sky_intensity": ("ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "04bc4b2dd2621affa020e5956bd0759f2aba85c3619c54db7c84f1229892c580"),
    "sun_direction": ("a2cb8869addd405c99b540f741474806883c5974e1fba9a3851b4c9f48bede45",
        "0411987cb5dac17f60ac8cf70eba276ec8064760784ecfe52a85e5896428877d"),
    "sun_flag": ("a2cb8869addd405c99b540f741474806883c5974e1fba9a3851b4c9f48bede45",
        "b34708bbfaf6710d08823a2c1469eb36abdf0cd68b41ab7b4fc9246b88350111"),
    "sun_texture": ("a2cb8869addd405c99b540f741474806883c5974e1fba9a3851b4c9f48bede45",
        "e39df00d35f339c0ab4a6b714732e3bbe49a1a91fc2e61edad8b671c6e4d36a0"),
    "chain_indoor": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "1ba012cdd86c396fc7aa148b53f73408932b2fbbb39d25ab5faaa04967d27085",
        "a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234"),
    "chain_tree_forms": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "5fcc78e14cc2e7911378054d5366450f5493df6c13852eb2ba2196fd7364497f",
        "71f8527f99018d6602e2a2ad267e37479ed46d3584918f28244f643b02e664d8",
        "a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234"),
    "chain_fallback": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "ed4952fccbdcf5e88e334767f7cccf61be5dd743fb55ef1215f455e9a06846c0",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234"),
    "chain_fallback_shard": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "ed4952fccbdcf5e88e334767f7cccf61be5dd743fb55ef1215f455e9a06846c0",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234"),
    "chain_tree_forms_distinct": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "a2cd3cca7532f798d83e7b85064e6112646d3cf6b6f9d222ada3f74dcc32ef96",
        "71f8527f99018d6602e2a2ad267e37479ed46d3584918f28244f643b02e664d8",
        "cbb9fc0c8bf5b8bd2f6be95469a3e46e4962b8d12537a7fd44ab87c7ae63dccc",
        "a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234"),
    "chain_fallback_distinct": ("a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234",
        "e42783feeebe7dfe0c8ae391e94578ebe6c23110d4b767565eee865a92237081",
        "ebe0dacdb61e7cb94c083fe8f5af5e7a380fe21236e2df6413ccb2cfa68ad002",
        "a1745a1a6866d7cc1bf28c8528822bae92aff12bc495757cd951926214d02234"),
}
