"""Host-side packers/generators (wire formats of SURVEY.md Appendix A)."""
import dataclasses

import numpy as np
import pytest

from chunkyclplugin_amd import scenes


def lookup(tree, depth, x, y, z):
    """Octree_get (K/octree.h:23-39) in Python."""
    level, data = depth, int(tree[0])
    while data > 0:
        level -= 1
        data = int(tree[data + ((((x >> level) & 1) << 2) | (((y >> level) & 1) << 1) | ((z >> level) & 1))])
    return -data, level


def test_octree_roundtrip_and_merge():
    rng = np.random.default_rng(0)
    depth, S = 4, 16
    t = np.zeros((S, S, S), np.int32)
    t[:8, :8, :8] = 3                      # mergeable 8^3 region
    t[8:, 8:, 8:] = rng.integers(0, 5, size=(8, 8, 8))
    t[12, 3, 3] = scenes.ANY_TYPE
    for order in ("bfs", "dfs"):
        tree = scenes.build_octree(t, depth, order)
        assert (tree.size - 1) % 8 == 0
        for _ in range(300):
            x, y, z = rng.integers(0, S, size=3)
            v, level = lookup(tree, depth, int(x), int(y), int(z))
            want = int(t[x, y, z])
            assert v == (scenes.ANY_TYPE if want == scenes.ANY_TYPE else 2 * want)
        v, level = lookup(tree, depth, 1, 2, 3)
        assert (v, level) == (6, 3)        # merged into one level-3 leaf
    a, b = scenes.build_octree(t, depth, "bfs"), scenes.build_octree(t, depth, "dfs")
    assert a.size == b.size


def test_atlas_first_fit_and_location_bits():
    ab = scenes.AtlasBuilder(4, 4)
    rng = np.random.default_rng(1)
    ids = [ab.add(scenes.noise_texture(rng, (10 * i, 20, 30))) for i in range(5)]
    big = ab.add(scenes.noise_texture(rng, (200, 200, 200), size=32))
    atlas, recs = ab.build()
    assert atlas.shape == (1, 64, 64, 4)
    size, loc = recs[big]
    assert size == (32 << 16) | 32 and loc == 0          # largest first, at tile (0,0), layer 0
    # x outer, y inner: after the 2x2 tile, the next free tiles are (0,2), (0,3), (1,2)...
    assert [(recs[i][1] >> 22) & 0x1FF for i in ids[:3]] == [0, 0, 1]
    assert [(recs[i][1] >> 13) & 0x1FF for i in ids[:3]] == [2, 3, 2]
    for i in ids:
        size, loc = recs[i]
        x, y = ((loc >> 22) & 0x1FF) * 16, ((loc >> 13) & 0x1FF) * 16
        assert (atlas[0, y:y + 16, x:x + 16] == ab._tex[i]).all()


def test_bvh_layout():
    sc = scenes.add_entities(scenes.tiny_scene(entities=0), 64, actor_tris=16)
    for nodes in (sc.world_bvh, sc.actor_bvh):
        n = nodes.reshape(-1, 7)
        inner = n[:, 0] > 0
        assert (n[inner, 0] % 7 == 0).all() and (n[inner, 0] < nodes.size).all()
        leaves = -n[~inner, 0]
        assert (leaves >= 0).all() and (leaves < sc.bvh_trigs.size).all()
        cnt = sc.bvh_trigs[leaves]
        assert (cnt >= 1).all() and (cnt <= 4).all()
    e = scenes.empty_bvh()
    assert e[0] == 0 and np.isnan(e[1:].view(np.float32)).all()


def test_sun_and_camera_packing():
    sun = scenes.pack_sun(0.6, 1.2, 1.25, True, (0x200020, 5))
    assert sun[0] == 1 and sun[1] == 0x200020 and sun[2] == 5
    assert np.allclose(sun[3:].view(np.float32), [1.25, 0.6, 1.2])
    cam = scenes.look_at_camera((1, 2, 3), (4, 2, 7))
    assert cam.shape == (15,)
    M = cam[3:12].reshape(3, 3)
    assert np.allclose(M @ M.T, np.eye(3), atol=1e-6)
    assert np.allclose(M[:, 2], np.array([3, 0, 4]) / 5, atol=1e-6)   # third column = forward


def test_wide_tree_relayout_preserves_every_lookup():
    """The upload-time re-layout (widetree.hpp) must return the reference's (leaf value, leaf level)
    for every cell — K/octree.h:81-89 is a pure function of the cell."""
    import pytest
    from chunkyclplugin_amd import native
    rng = np.random.default_rng(5)
    sc = scenes.outdoor_world(chunks=2, height=48, seed=101)          # depth 6, with ANY_TYPE interior
    S = 1 << sc.octree_depth
    xyz = rng.integers(0, S, size=(4000, 3)).astype(np.int32)
    want = np.array([lookup(sc.octree, sc.octree_depth, *map(int, c)) for c in xyz])
    for bits in (None, [3, 3], [2, 2, 2], [1, 1, 1, 1, 1, 1], [6], [4, 2], [1, 2, 3]):
        data, level, n = native.widetree_lookup(sc.octree, sc.octree_depth, xyz, bits)
        np.testing.assert_array_equal(data, want[:, 0], err_msg=str(bits))
        np.testing.assert_array_equal(level, want[:, 1], err_msg=str(bits))
        assert n >= 8
    assert (want[:, 0] == scenes.ANY_TYPE).any() and (want[:, 1] > 1).any()
    # single-leaf world, and rejects what it cannot express
    d, l, n = native.widetree_lookup(np.array([-6], np.int32), 4, [[1, 2, 3]])
    assert (d[0], l[0]) == (6, 4)
    with pytest.raises(native.ChunkyHipError):
        native.widetree_lookup(sc.octree, sc.octree_depth, xyz, [3, 2])     # bits do not sum to depth
    with pytest.raises(native.ChunkyHipError):
        native.widetree_lookup(np.array([-(1 << 28)], np.int32), 3, [[0, 0, 0]])  # pointer too large


def test_octree2_reader_on_the_reference_benchmark_scene():
    """`.octree2` reader: 3091 palette entries, depth 10, 345 557 branches,
    2 764 457 packed ints; every leaf is a valid block pointer or ANY_TYPE."""
    import os
    import pytest
    from chunkyclplugin_amd import octree2
    src = "/root/reference/benchmark/OpenCL_test/OpenCL_test.octree2"
    if not os.path.exists(src):
        pytest.skip("reference benchmark fixture not present on this machine")
    palette, depth, stream = octree2.read_octree2(src)
    assert (len(palette), depth) == (3091, 10)
    assert int((stream == -1).sum()) == 345557 and stream.size == 345557 + 2418900
    assert palette[0]["Name"] == "minecraft:air" and palette[1]["Name"] == "minecraft:stone"
    tree = octree2.pack_preorder(stream, len(palette))
    assert tree.size == 2764457
    leaves = -tree[tree <= 0].astype(np.int64)
    ok = (leaves == scenes.ANY_TYPE) | ((leaves % 2 == 0) & (leaves < 2 * 3091))
    assert ok.all() and int((leaves == scenes.ANY_TYPE).sum()) == 312369
    # first leaf cell of the stream round-trips through the packed layout
    sc = octree2.cached_benchmark_scene(64, 36)
    assert sc.octree.size == tree.size and sc.octree_depth == 10


def test_asset_pack_gives_palette_entries_their_model_class():
    """octree2.asset_pack (row f1): a palette entry's NAME and PROPERTIES decide its model — the geometry Minecraft gives the
    class — and every block name gets one texture; entries of one class and material share a model."""
    from chunkyclplugin_amd import octree2
    cls, boxes = octree2._model_class, octree2._model_boxes
    assert boxes(cls("stone_brick_slab", {"type": "top"})) == [(0, 1, 0.5, 1, 0, 1)]
    assert boxes(cls("stone_brick_slab", {"type": "double"})) is None                       # a full cube
    assert boxes(cls("spruce_stairs", {"half": "bottom", "facing": "east"})) == [(0, 1, 0, 0.5, 0, 1), (0.5, 1, 0.5, 1, 0, 1)]
    assert boxes(cls("spruce_stairs", {"half": "top", "facing": "north"})) == [(0, 1, 0.5, 1, 0, 1), (0, 1, 0, 0.5, 0, 0.5)]
    fence = boxes(cls("oak_fence", {"north": "true", "east": "false", "south": "false", "west": "true"}))
    assert fence[0] == (0.375, 0.625, 0, 1, 0.375, 0.625) and len(fence) == 3               # post + two arms
    assert boxes(cls("iron_bars", {}))[0] == (0.4375, 0.5625, 0, 1, 0.4375, 0.5625)
    assert boxes(cls("rail", {})) == [(0, 1, 0, 0.0625, 0, 1)] and boxes(cls("oak_trapdoor", {"half": "top"})) == [(0, 1, 0.8125, 1, 0, 1)]
    assert cls("poppy", {}) == ("plant",) and cls("stone", {}) == ("cube",) and boxes(cls("stone", {})) is None
    palette = [{"Name": "minecraft:air"}, {"Name": "minecraft:stone"}, {"Name": "minecraft:oak_slab", "Properties": {"type": "bottom"}},
               {"Name": "minecraft:oak_slab", "Properties": {"type": "bottom", "waterlogged": "true"}}, {"Name": "minecraft:poppy"},
               {"Name": "minecraft:oak_slab", "Properties": {"type": "double"}}]
    pal, atlas, recs, tsun = octree2.asset_pack(palette)
    blocks, mats, aabbs, quads = pal.arrays()
    b = blocks.reshape(-1, 2)
    assert b[:, 0].tolist() == [0, 1, 2, 2, 3, 1]                                            # invisible, cube, AABB, AABB, quads, cube
    assert b[2, 1] == b[3, 1] and aabbs[0] == 1 and quads[0] == 4                            # the two bottom slabs share one model
    assert mats.size == 6 * 3 and (mats.reshape(-1, 6)[:, 0] == 4).all()                     # three names, all textured
    assert atlas.shape[1] % 16 == 0 and recs[tsun][0] == (32 << 16) | 32


def test_benchmark_fixture_is_what_the_loader_makes_of_the_reference_files():
    """Where the reference's data files exist: the committed fixture equals load_scene's output array for array."""
    import os
    import pytest
    from chunkyclplugin_amd import octree2
    if not os.path.exists(octree2.REFERENCE_SCENE + ".octree2"):
        pytest.skip("reference benchmark files not present on this machine")
    made = octree2.load_scene(octree2.REFERENCE_SCENE + ".octree2", octree2.REFERENCE_SCENE + ".json")
    kept = octree2.cached_benchmark_scene(made.width, made.height)
    for f in ("octree", "block_palette", "material_palette", "aabb_models", "quad_models", "atlas", "sky", "sun", "camera"):
        np.testing.assert_array_equal(np.asarray(getattr(made, f)), np.asarray(getattr(kept, f)), err_msg=f)
    kinds = kept.block_palette.reshape(-1, 2)[:, 0]
    assert (kinds == 2).sum() > 1000 and (kinds == 3).sum() >= 20 and (kinds == 1).sum() > 1500   # model blocks are part of the city now


def test_slab_octree_builder_equals_the_dense_builder():
    """build_octree_slab (the beyond-cache world of bench.py --config 5 is 2048 x 256 x 2048: its dense cube would be 34 GB) packs
    a slab exactly as build_octree packs the same world padded with air: same merging, same breadth-first numbering."""
    rng = np.random.default_rng(3)
    n, h, depth = 64, 16, 6
    t = np.zeros((n, h, n), np.int16)
    hm = (rng.random((n, n)) * 12).astype(int)
    for x in range(n):
        for z in range(n):
            t[x, :hm[x, z] + 1, z] = 1 + (x * 7 + z) % 3
    t[5:9, 2:4, 5:9] = 255
    t[16:32, 0:16, 32:48] = 2          # a whole 16^3 cell: merges one level above the slab's thickness
    dense = np.zeros((n, n, n), np.int32)
    dense[:, :h, :] = t
    dense[dense == 255] = scenes.ANY_TYPE
    np.testing.assert_array_equal(scenes.build_octree_slab(t, depth, 255), scenes.build_octree(dense, depth, "bfs"))
    # a slab as thick as the world is wide, and an all-air world
    cube = (rng.random((8, 8, 8)) < 0.3).astype(np.int16)
    np.testing.assert_array_equal(scenes.build_octree_slab(cube, 3, 255), scenes.build_octree(cube.astype(np.int32), 3, "bfs"))
    assert list(scenes.build_octree_slab(np.zeros((8, 2, 8), np.int16), 3, 255)) == [0]


def test_big_world_generator_small():
    """big_outdoor_world at 16 x 16 chunks: the outdoor world's palettes, a depth-8 octree whose wide re-layout answers every sampled
    cell as the reference walk does."""
    from chunkyclplugin_amd import native
    sc = scenes.big_outdoor_world(chunks=16, width=64, img_height=48)
    small = scenes.outdoor_world(chunks=1, height=16, width=64, img_height=48)
    assert sc.octree_depth == 8 and np.array_equal(sc.block_palette, small.block_palette) and np.array_equal(sc.atlas, small.atlas)
    rng = np.random.default_rng(5)
    xyz = rng.integers(0, 256, size=(4000, 3)).astype(np.int32)
    data, level, _n = native.widetree_lookup(sc.octree, sc.octree_depth, xyz)
    for (x, y, z), d, l in zip(xyz[:600], data[:600], level[:600]):
        lv, v = sc.octree_depth, int(sc.octree[0])
        while v > 0:
            lv -= 1
            v = int(sc.octree[v + ((((x >> lv) & 1) << 2) | (((y >> lv) & 1) << 1) | ((z >> lv) & 1))])
        assert (-v, lv) == (int(d), int(l))


# ---- scenes.embed_deeper and the default split of the wide tree above depth 10 ----
EMBED_SLOTS = {"origin": lambda k: [0] * k, "offset": lambda k: [(3 * i + 5) % 8 for i in range(k)]}
# default_wide_levels (csrc/widetree.cpp): bits of the dense top node and 8^3 levels below it, by octree depth
DEFAULT_SPLIT = {6: (6, 0), 7: (4, 1), 8: (5, 1), 9: (6, 1), 10: (7, 1), 11: (5, 2), 12: (6, 2), 13: (7, 2), 14: (5, 3), 15: (6, 3)}


def _embedded(depth, which):
    """A depth-6 golden world in a depth-`depth` octree, siblings of every new level alternately stone, ANY_TYPE and air."""
    sc = scenes.outdoor_world(chunks=2, height=48, seed=101)
    k = depth - sc.octree_depth
    slots = EMBED_SLOTS[which](k)
    sib = {}
    for i in range(k):
        free = [s for s in range(8) if s != slots[i]]
        sib[(i, free[i % 7])] = 2
        sib[(i, free[(i + 3) % 7])] = scenes.ANY_TYPE
    return sc, scenes.embed_deeper(sc, depth, slots=slots, siblings=sib), slots, sib


def _sibling_cells(rng, depth, slots, n_per):
    """Cells inside every sibling cube of every new level, with the (level, slot) they belong to."""
    cells, want = [], []
    for i in range(len(slots)):
        level = depth - 1 - i
        base = scenes.embed_offset(depth, slots[:i])
        for s in range(8):
            if s == slots[i]:
                continue
            corner = base + (np.array([(s >> 2) & 1, (s >> 1) & 1, s & 1], np.int64) << level)
            pts = corner + rng.integers(0, 1 << level, size=(n_per, 3))
            pts[0], pts[1] = corner, corner + (1 << level) - 1        # the cube's first and last cell
            cells.append(pts)
            want += [(i, s)] * n_per
    return np.concatenate(cells), want


@pytest.mark.parametrize("which", list(EMBED_SLOTS))
@pytest.mark.parametrize("depth", range(7, 21))
def test_embed_deeper_keeps_every_lookup(depth, which):
    """The reference walk (K/octree.h:23-39) of the embedded tree at cell + offset is the walk of the original at cell; elsewhere it
    finds the sibling's value at the sibling's level.  Up to depth 15 the wide re-layout with the default split answers the same
    (data, level) — big sibling leaves included — and its entry count names the split: 2^(3 top bits) + 512 per 8^3 node."""
    from chunkyclplugin_amd import native
    rng = np.random.default_rng(depth)
    sc, deep, slots, sib = _embedded(depth, which)
    off = scenes.embed_offset(depth, slots)
    assert deep.octree_depth == depth and deep.octree.size == sc.octree.size + 8 * (depth - 6)
    assert (off == 0).all() == (which == "origin")
    np.testing.assert_array_equal(deep.camera[:3], (sc.camera[:3] + off.astype(np.float32)).astype(np.float32))
    inner = rng.integers(0, 64, size=(3000, 3))
    inner[:8] = [[(c >> 2 & 1) * 63, (c >> 1 & 1) * 63, (c & 1) * 63] for c in range(8)]     # the world's corners
    want_in = [lookup(sc.octree, 6, *map(int, c)) for c in inner]
    got_in = [lookup(deep.octree, depth, *map(int, c + off)) for c in inner]
    assert got_in == want_in
    outer, owner = _sibling_cells(rng, depth, slots, 6)
    want_out = []
    for (i, s) in owner:
        t = sib.get((i, s), 0)
        want_out.append((scenes.ANY_TYPE if t == scenes.ANY_TYPE else 2 * t, depth - 1 - i))
    assert [lookup(deep.octree, depth, *map(int, c)) for c in outer] == want_out
    assert {v for v, _l in want_out} == {0, 4, scenes.ANY_TYPE}
    xyz = np.concatenate([inner + off, outer]).astype(np.int32)
    if depth > 15:
        with pytest.raises(native.ChunkyHipError):
            native.widetree_lookup(deep.octree, depth, xyz)
        return
    data, level, n = native.widetree_lookup(deep.octree, depth, xyz)
    np.testing.assert_array_equal(data, [v for v, _l in want_in + want_out])
    np.testing.assert_array_equal(level, [l for _v, l in want_in + want_out])
    top, n3 = DEFAULT_SPLIT[depth]
    # the top node and some 8^3 nodes: far fewer entries than the next larger top alone would have
    assert n >= (1 << (3 * top)) and (n - (1 << (3 * top))) % 512 == 0, (n, top)
    assert n < (1 << (3 * (top + 1))), "the entry count of a sparse world names the top node"
    assert top + 3 * n3 == depth


@pytest.mark.parametrize("depth", sorted(DEFAULT_SPLIT))
def test_default_split_by_entry_count(depth):
    """The default split itself, through the entry count of a world that is ONE branch chain down to a single stone cell at the
    origin: the top node plus exactly one 8^3 node per lower level — 2^(3 top) + 512 n3 identifies (top, n3) uniquely."""
    from chunkyclplugin_amd import native
    tree = [1]
    for i in range(depth):
        tree += [1 + 8 * (i + 1) if i + 1 < depth else -4] + [0] * 7
    tree = np.array(tree, np.int32)
    cells = [[0, 0, 0], [1, 0, 0], [(1 << depth) - 1] * 3]
    data, level, n = native.widetree_lookup(tree, depth, cells)
    assert data.tolist() == [4, 0, 0] and level.tolist() == [0, 0, depth - 1]
    top, n3 = DEFAULT_SPLIT[depth]
    assert n == (1 << (3 * top)) + 512 * n3, (depth, n)
    sizes = {(1 << (3 * t)) + 512 * k: (t, k) for t in range(1, 8) for k in range(0, 6) if t + 3 * k == depth}
    assert sizes[n] == (top, n3)


def test_embed_deeper_moves_pregenerated_rays_and_refuses_what_it_cannot_do():
    sc = scenes.outdoor_world(chunks=2, height=48, seed=101, width=8, img_height=4)
    rays = np.arange(8 * 4 * 6, dtype=np.float32)
    pre = sc.with_view(8, 4, camera=rays, projector_type=-1)
    deep = scenes.embed_deeper(pre, 9, slots=[4, 0, 3])
    off = scenes.embed_offset(9, [4, 0, 3])
    assert off.tolist() == [256, 64, 64]
    np.testing.assert_array_equal(deep.camera.reshape(-1, 6)[:, :3], rays.reshape(-1, 6)[:, :3] + off.astype(np.float32))
    np.testing.assert_array_equal(deep.camera.reshape(-1, 6)[:, 3:], rays.reshape(-1, 6)[:, 3:])
    assert pre.camera[0] == 0.0                                        # the input is left alone
    single = scenes.embed_deeper(dataclasses.replace(sc, octree=np.array([-4], np.int32), octree_depth=2), 4, slots=[7, 7])
    assert lookup(single.octree, 4, 15, 15, 15) == (4, 2) and lookup(single.octree, 4, 0, 0, 0) == (0, 3)
    ents = scenes.add_entities(sc, 8)
    assert scenes.embed_deeper(ents, 8).world_bvh is ents.world_bvh     # at the origin entities stay where they are
    for bad in (lambda: scenes.embed_deeper(sc, 6), lambda: scenes.embed_deeper(sc, 8, slots=[0]),
                lambda: scenes.embed_deeper(sc, 8, slots=[0, 8]), lambda: scenes.embed_deeper(sc, 8, siblings={(0, 0): 2}),
                lambda: scenes.embed_deeper(sc, 8, siblings={(2, 1): 2}), lambda: scenes.embed_deeper(ents, 8, slots=[1, 0])):
        with pytest.raises(ValueError):
            bad()
