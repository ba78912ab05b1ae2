"""hit_top — 1 + the highest cell y of any leaf that can be hit (widetree.cpp annotate_wide_tree), the height above which render_pool
ends the march of a ray that runs upwards — against a brute-force scan of every cell of the world through chunky_widetree_lookup:
worlds of depth 4 to 6 whose top leaf sits at y = 0, in the middle, in the last row, is a leaf of level 2, a full column, or does
not exist; on the default split (one dense node), on two-level splits and on a split with a padded top; and after palette changes
that turn an invisible block above everything into a cube (hit_top rises) or hide the top block (it falls).  No GPU."""
import numpy as np
import pytest

import march_cap_scenes as mc

from chunkyclplugin_amd import native, scenes


def brute_force(octree, depth, blocks):
    """max over the cells that can be hit of the end of the cell's leaf (K/block.h:32-47: air, ANY_TYPE, a pointer outside the
    palette and model type 0 / unknown cannot)"""
    S = 1 << depth
    g = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    data, level, _n = native.widetree_lookup(octree, depth, g)
    data = data.astype(np.int64)
    inside = (data != 0) & (data != scenes.ANY_TYPE) & (data + 1 < len(blocks))
    kinds = np.zeros(len(data), np.int64)
    kinds[inside] = np.asarray(blocks, np.int64)[data[inside]]
    can = inside & (kinds >= 1) & (kinds <= 3)
    if not can.any():
        return 0
    y = g[can, 1].astype(np.int64)
    lv = level[can].astype(np.int64)
    return int((((y >> lv) << lv) + (1 << lv)).max())


def splits(depth):
    out = [None]
    if depth > 3:
        out.append([depth - 3, 3])
    if depth > 4:
        out.append([depth - 4, 2, 2])
    out.append([depth - 2, 3])  # one padding bit in the top node
    return out


@pytest.mark.parametrize("depth", [4, 5, 6])
@pytest.mark.parametrize("kind", mc.KINDS)
def test_hit_top_is_the_brute_force_scan(kind, depth):
    sc, top = mc.world(kind, depth)
    want = brute_force(sc.octree, depth, sc.block_palette)
    assert want == top, "the world is not what its name says"
    for bits in splits(depth):
        assert native.widetree_hit_top(sc.octree, depth, sc.block_palette, bits) == want, (kind, depth, bits)
    if kind == "big_leaf":  # the top leaf is larger than a cell
        S = 1 << depth
        _d, level, _n = native.widetree_lookup(sc.octree, depth, [[5, S // 2 + 1, 9]])
        assert level[0] == 2


def test_a_world_of_one_leaf():
    sc, cube, _model, ghost = mc.base()
    for depth in (0, 4, 7):
        for block, want in ((cube, 1 << depth), (ghost, 0), (0, 0)):
            assert native.widetree_hit_top(np.array([-2 * block], np.int32), depth, sc.block_palette) == want
        assert native.widetree_hit_top(np.array([-scenes.ANY_TYPE], np.int32), depth, sc.block_palette) == 0


@pytest.mark.parametrize("depth", [4, 6])
def test_palette_changes_move_hit_top(depth):
    sc, top = mc.world("middle", depth)
    _sc, cube, model, ghost = mc.base()
    S = 1 << depth
    blocks = np.asarray(sc.block_palette, np.int32)
    assert native.widetree_hit_top(sc.octree, depth, blocks) == top
    # the invisible block above everything becomes a cube: its highest cells are the world's last rows
    raised = blocks.copy()
    raised[2 * ghost:2 * ghost + 2] = blocks[2 * cube:2 * cube + 2]
    assert native.widetree_hit_top(sc.octree, depth, raised) == S == brute_force(sc.octree, depth, raised)
    # the model block on top of the pillar is hidden: the pillar's last cube is the top
    lowered = blocks.copy()
    lowered[2 * model] = 0
    assert native.widetree_hit_top(sc.octree, depth, lowered) == top - 1 == brute_force(sc.octree, depth, lowered)
    # every cube hidden: the model block alone; everything hidden: nothing
    no_cubes = blocks.copy()
    no_cubes[0::2][blocks[0::2] == 1] = 0
    assert native.widetree_hit_top(sc.octree, depth, no_cubes) == top == brute_force(sc.octree, depth, no_cubes)
    assert native.widetree_hit_top(sc.octree, depth, np.zeros_like(blocks)) == 0
    # a palette shorter than the pointers of the tree: those leaves cannot be hit
    assert native.widetree_hit_top(sc.octree, depth, blocks[:2]) == 0 == brute_force(sc.octree, depth, blocks[:2])


def test_bad_arguments():
    sc, _top = mc.world("floor", 4)
    with pytest.raises(native.ChunkyHipError):
        native.widetree_hit_top(sc.octree, 4, sc.block_palette, [2, 1])  # fewer bits than the depth
    with pytest.raises(native.ChunkyHipError):
        native.widetree_hit_top(np.array([-(1 << 28)], np.int32), 3, sc.block_palette)  # pointer too large for the re-layout
