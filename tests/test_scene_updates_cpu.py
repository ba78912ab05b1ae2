"""The table of scene updates (tests/scene_update_cases.py) can detect a failure: on the oracle alone, every step of every case
changes at least 1 % of the pixels of the image (3 passes) or of the preview, and so does every stale hybrid — the step's scene
with the changed source array of the step before, what a forgotten invalidation would render.  A case that does not separate them
could not notice the bug it is there for.  The inputs are pinned by digest."""
import numpy as np
import pytest

import golden_scenes as gs
import scene_update_cases as suc
from chunkyclplugin_amd import scenes

SEEDS = scenes.java_random_ints(suc.N_PASSES)
CASES = [c.name for c in suc.cases()]
_images = {}


def oracle(port, sc):
    """(image, preview) of the oracle, once per distinct scene"""
    key = gs.input_digest(sc)
    if key not in _images:
        _images[key] = (port.render_passes(sc, SEEDS), port.preview(sc))
    return _images[key]


def different(a, b):
    """share of the pixels that differ: (image, in float bits; preview)"""
    img = (a[0].view(np.uint32).reshape(-1, 3) != b[0].view(np.uint32).reshape(-1, 3)).any(axis=1).mean()
    return float(img), float((a[1] != b[1]).mean())


def same_world(a, b):
    """both hold one world, at another octree depth (scenes.embed_deeper): every array but the octree is equal, and so are the leaves"""
    rest = [f for f in suc.PIECE_OF if f not in ("octree", "octree_depth")]
    return a.octree_depth != b.octree_depth and all(np.array_equal(getattr(a, f), getattr(b, f)) for f in rest) \
        and np.array_equal(np.sort(a.octree[a.octree < 0]), np.sort(b.octree[b.octree < 0]))


def test_every_scene_has_the_golden_view():
    for c in suc.cases():
        for sc in c.chain:
            assert (sc.width, sc.height) == (suc.W, suc.H) == (64, 48), c.name


def test_the_table_names_its_setters():
    singles = [c.name for c in suc.cases() if c.via != "load_packed"]
    assert sorted(suc.SETTERS) == sorted(singles)
    called = {s for v in suc.SETTERS.values() for s in v}
    assert called == {"set_octree", "load_octree", "set_palette BLOCK", "set_palette MATERIAL", "set_palette AABB", "set_palette QUAD",
                      "set_palette TRIG", "set_bvh WORLD", "set_bvh ACTOR", "set_atlas", "set_sky", "set_sun"}
    for c in suc.cases():
        if c.via == "setters":   # the fields that differ between neighbours are the ones the case names, and all of them
            for a, b in c.steps():
                changed = {f for f in suc.PIECE_OF if not np.array_equal(getattr(a, f), getattr(b, f))}
                assert changed == set(c.fields), (c.name, changed)
            assert set(c.pieces()) == {{"set_octree": "octree", "set_palette BLOCK": "blocks", "set_palette MATERIAL": "materials",
                                        "set_palette AABB": "aabbs", "set_palette QUAD": "quads", "set_palette TRIG": "trigs",
                                        "set_bvh WORLD": "world_bvh", "set_bvh ACTOR": "actor_bvh", "set_atlas": "atlas", "set_sky": "sky",
                                        "set_sun": "sun"}[s] for s in suc.SETTERS[c.name]}, c.name


@pytest.mark.parametrize("name", CASES)
def test_every_step_changes_the_image(port, name):
    c = suc.case(name)
    for k, (a, b) in enumerate(c.steps(), start=1):
        img, pre = different(oracle(port, a), oracle(port, b))
        print(f"{name} step {k}: image {img:.4f} preview {pre:.4f}")
        if same_world(a, b):
            # scenes.embed_deeper: the same world under more octree levels is the same image by construction; what such a step
            # changes is the tree form (kernel_info on the GPU).  chain_*_distinct walk the same forms with a world that changes too
            assert (img, pre) == (0.0, 0.0) and a.octree_depth != b.octree_depth and not np.array_equal(a.octree, b.octree), (name, k)
            continue
        assert max(img, pre) >= suc.MIN_DIFFERENT, f"{name} step {k}: {img:.4f} of the image, {pre:.4f} of the preview"
        if c.single:
            stale = c.stale(k)
            img, pre = different(oracle(port, stale), oracle(port, b))
            print(f"{name} step {k} stale: image {img:.4f} preview {pre:.4f}")
            assert max(img, pre) >= suc.MIN_DIFFERENT, f"{name} step {k}, stale hybrid: {img:.4f} of the image, {pre:.4f} of the preview"
    if len(c.chain) > 2:   # a chain returns to its start
        assert gs.input_digest(c.chain[-1]) == gs.input_digest(c.chain[0])


@pytest.mark.parametrize("name", CASES)
def test_inputs_are_pinned(name):
    c = suc.case(name)
    assert [gs.input_digest(sc) for sc in c.chain] == list(suc.DIGESTS[name]), name


def test_the_sort_threshold_is_crossed_in_both_directions():
    up, down = suc.case("blocks_to_sorted"), suc.case("blocks_to_unsorted")
    T = suc.SORT_BLOCKS_PERMILLE
    assert suc.model_leaf_permille(up.before) < T <= suc.model_leaf_permille(up.after)
    assert suc.model_leaf_permille(down.after) < T <= suc.model_leaf_permille(down.before)


def test_block_kinds_turn_every_way():
    """cube -> model, model -> cube, cube -> invisible, invisible -> cube, each on a block the octree holds"""
    c = suc.case("blocks_kinds")
    a, b = (np.asarray(s.block_palette).reshape(-1, 2)[:, 0] for s in (c.before, c.after))
    turns = {(int(a[k]), int(b[k])) for k in range(len(a)) if (np.asarray(c.before.octree) == -2 * k).any()}
    assert {(1, 2), (2, 1), (1, 0), (0, 1)} <= turns, turns


def test_octree_cases_cover_both_upload_paths_and_the_remap():
    same, other, remap = (suc.case(n) for n in ("octree_swap_ids", "octree_resize", "octree_load_mapping"))
    assert len(same.after.octree) == len(same.before.octree) and same.after.octree_depth == same.before.octree_depth
    assert len(other.after.octree) != len(other.before.octree) and other.after.octree_depth == other.before.octree_depth
    raw, mapping = suc.remapped(remap.after.octree, len(remap.after.block_palette) // 2)
    assert not np.array_equal(mapping, 2 * np.arange(len(mapping))) and not np.array_equal(raw, remap.after.octree)


def test_triangle_edits_stay_inside_the_bvh_boxes():
    """the edited triangles' vertices lie inside the old ones' hull, so the node boxes of the unchanged BVHs still hold them"""
    c = suc.case("trigs_words")
    for first, n in suc._leaves(c.before):
        old = c.before.bvh_trigs[first:first + 20 * n].reshape(n, 20)[:, 1:10].copy().view(np.float32)
        new = c.after.bvh_trigs[first:first + 20 * n].reshape(n, 20)[:, 1:10].copy().view(np.float32)
        np.testing.assert_array_equal(new[:, 6:9], old[:, 6:9])
        np.testing.assert_array_equal(new[:, :6], old[:, :6] * np.float32(0.5))
    mats = c.after.bvh_trigs[[f + 19 for f, n in suc._leaves(c.after)]]
    assert (mats % 6 == 0).all() and (mats >= 0).all() and (mats < len(c.after.material_palette)).all()


def test_sky_sizes_and_sun_words():
    shapes = [s.sky.shape[:2] for s in suc.case("sky_sizes").chain]
    assert (32, 64) in shapes and (1, 1) in shapes
    for name, word in (("sun_direction", (4, 5)), ("sun_flag", (0,)), ("sun_texture", (2,))):
        c = suc.case(name)
        assert tuple(np.flatnonzero(np.asarray(c.before.sun) != np.asarray(c.after.sun))) == word, name
    c = suc.case("sky_intensity")
    assert c.before.sky_intensity != c.after.sky_intensity and np.array_equal(c.before.sky, c.after.sky)


def test_tile_writes_rebuild_the_atlas():
    atlas = suc.tile_scene().atlas
    writes = suc.tile_writes(atlas)
    layers, h, w, _ = atlas.shape
    np.testing.assert_array_equal(suc.apply_tiles(atlas.shape, writes), atlas)
    shapes = {(tw, th) for _x, _y, _l, tw, th, _t in writes}
    assert (1, 1) in shapes and (w, 16) in shapes and (16, 16) in shapes
    last = [i for i, (x, y, l, tw, th, _t) in enumerate(writes) if (x + tw, y + th, l) == (w, h, layers - 1)]
    assert len(last) == 2 and not np.array_equal(writes[last[0]][5], writes[last[1]][5])
    first = [(x, y, l) for x, y, l, tw, th, _t in writes if (tw, th) == (16, 16)]
    assert first[1:] != sorted(first[1:])   # shuffled
    for x, y, l, tw, th, t in writes:
        assert t.shape == (th, tw, 4) and 0 <= x and x + tw <= w and 0 <= y and y + th <= h and 0 <= l < layers


def test_the_zeroed_atlas_changes_the_image(port):
    sc = suc.tile_scene()
    img, pre = different(oracle(port, sc), oracle(port, suc.zero_atlas(sc)))
    assert max(img, pre) >= suc.MIN_DIFFERENT


def test_upload_orders_are_permutations_other_than_load_packed():
    assert len(suc.UPLOAD_ORDERS) >= 4
    for name, order in suc.UPLOAD_ORDERS.items():
        assert sorted(order) == sorted(suc.LOAD_PACKED_ORDER) and tuple(order) != suc.LOAD_PACKED_ORDER, name
    assert len({tuple(o) for o in suc.UPLOAD_ORDERS.values()}) == len(suc.UPLOAD_ORDERS)
    assert [p for step, _ in suc.INCOMPLETE_STEPS for p in step] == list(suc.LOAD_PACKED_ORDER[:1] + ("blocks", "materials", "aabbs", "quads", "atlas", "sky", "sun", "world_bvh", "actor_bvh", "trigs"))


def test_the_half_updated_scene_separates(port):
    E, short, done = suc.half_updated()
    assert 0 < len(short) < len(E.bvh_trigs)
    world_leaves = [-int(v) for v in np.asarray(E.world_bvh).reshape(-1, 7)[:, 0] if v <= 0]
    assert max(world_leaves) < len(short)
    img, pre = different(oracle(port, E), oracle(port, done))
    assert max(img, pre) >= suc.MIN_DIFFERENT


def test_expected_kernels_cover_every_family():
    """the table reaches render_pool without and with BVH phases, sorted and unsorted, the four tree forms, and the fallback kernels"""
    seen = [suc.expected_kernel(sc) for c in suc.cases() for sc in c.chain]
    assert {k.get("tree") for k in seen} >= {16, 18, 19, 0}
    assert {k.get("sorted") for k in seen} >= {True, False}
    assert {(k["bvh"], k["pool_runs"]) for k in seen} == {(False, True), (True, True), (True, False)}
