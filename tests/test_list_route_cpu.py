"""What tests/test_gpu_list_route.py and tests/test_gpu_adaptive_edges.py take for granted, checked without a device: the pixel lists
(every list a pre-generated camera renders is a derangement: no slot holds its own index, so slot and pixel cannot be confused), the
tree form and the entity-BVH heights that select the render_pool instantiation each cell names, and the non-degeneracy of every
adaptive setting that is meant to run the list route — chosen here, on the CPU oracle, and imported by the GPU files."""
import dataclasses
import functools

import numpy as np
import pytest

import adaptive_spec as sp
import golden_scenes as gs
from chunkyclplugin_amd import native, scenes
from test_adaptive_cpu import FLOOR, MAX_SPP, params, samples_of

W, H, NP = gs.W, gs.H, gs.W * gs.H

# ---- pixel lists ------------------------------------------------------------------------------------------------------------------
LIST_LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, NP - 1]  # partial and whole sub-blocks of 4 slots, the tile edge, every pixel but one
LIST_ORDERS = ["natural", "reversed", "permuted"]
PASS_COUNTS = [1, 3, 64, 65]  # a wave claims 64 passes of one sub-block: below, at and above


def is_derangement(listed):
    listed = np.asarray(listed)
    return len(np.unique(listed)) == listed.size and not (listed == np.arange(listed.size)).any()


OMITTED = {"natural": 0, "reversed": 1000, "permuted": NP - 1}  # the pixel the list of every pixel but one leaves out


@functools.lru_cache(maxsize=None)
def _subset(n, order, seed=0):
    """n distinct pixels in the given order, redrawn until no slot k holds pixel k.  In natural (ascending) order that rules pixel 0
    out; the reversed and permuted lists hold pixel 0, and from two entries on the last pixel as well."""
    while True:
        rng = np.random.default_rng(1000 * n + 10 * seed + LIST_ORDERS.index(order))
        if n == NP - 1:
            a = np.delete(np.arange(NP), OMITTED[order])
        elif order == "natural":
            a = np.sort(rng.permutation(np.arange(1, NP))[:n])
        else:
            ends = [0, NP - 1][:min(n, 2)]
            a = np.sort(np.concatenate([ends, rng.permutation(np.arange(1, NP - 1))[:n - len(ends)]]))
        a = {"natural": a, "reversed": a[::-1], "permuted": rng.permutation(a)}[order].astype(np.int32)
        if is_derangement(a):
            return a
        seed += 1


def pixel_list(n, order):
    return _subset(n, order).copy()


def whole_image(name):
    """All 64 x 48 pixels in row-major order; for the pre-generated camera that order starts at pixel 1 and ends with pixel 0 (the
    identity would let a ray table indexed by the slot pass)."""
    a = np.arange(NP, dtype=np.int32)
    return np.roll(a, -1) if name == "pregen" else a


def last_row_and_column():
    """The last row right to left, then the rest of the last column bottom to top: 64 + 47 pixels, the image's far edges only."""
    row = (H - 1) * W + np.arange(W - 1, -1, -1)
    col = np.arange(H - 2, -1, -1) * W + (W - 1)
    return np.concatenate([row, col]).astype(np.int32)


def cell_list(seed, n=1337):
    """The permuted subset a matrix cell renders (not a multiple of 256 or of 4: the last tile and the last sub-block are partial)."""
    k = 0
    while True:
        listed = np.random.default_rng(7919 * seed + k).permutation(NP)[:n].astype(np.int32)
        if is_derangement(listed):
            return listed
        k += 1


def shape_lists():
    """(id, list) of every list-shape case, the same for "outdoor" and for "pregen" but for the whole image."""
    out = []
    for n in LIST_LENGTHS:
        for order in LIST_ORDERS if n > 1 else LIST_ORDERS[:1]:
            out.append((f"{order}-{n}", pixel_list(n, order)))
    out.append(("edges-111", last_row_and_column()))
    return out


def test_every_list_a_pregenerated_camera_renders_is_a_derangement():
    for what, listed in shape_lists():
        assert is_derangement(listed), what
        assert listed.min() >= 0 and listed.max() < NP
    assert is_derangement(whole_image("pregen")) and sorted(whole_image("pregen").tolist()) == list(range(NP))
    assert np.array_equal(whole_image("outdoor"), np.arange(NP))
    for seed in range(64):  # every seed the matrix uses
        assert is_derangement(cell_list(seed)) and cell_list(seed).size % 4 == 1
    assert is_derangement(cell_list(3, SPLIT_LIST))
    edge = last_row_and_column()
    assert edge.size == W + H - 1 and ((edge // W == H - 1) | (edge % W == W - 1)).all()
    assert [len(l) for _w, l in shape_lists()] == [1] + [n for n in LIST_LENGTHS[1:] for _ in range(3)] + [111]
    for n in LIST_LENGTHS[1:]:  # ascending, descending, neither; pixel 0 and the last pixel are listed where the order allows
        nat, rev, per = (pixel_list(n, o) for o in LIST_ORDERS)
        assert (np.diff(nat) > 0).all() and (np.diff(rev) < 0).all() and nat[0] > 0
        assert rev[-1] == 0 and 0 in per and (n < 2 or (rev[0] == NP - 1 and (NP - 1 in per or n == NP - 1)))
        assert n < 5 or not ((np.diff(per) > 0).all() or (np.diff(per) < 0).all())
    for order, gone in OMITTED.items():
        assert sorted(set(range(NP)) - set(pixel_list(NP - 1, order).tolist())) == [gone]


# ---- launch splitting -------------------------------------------------------------------------------------------------------------
# for_each_launch (csrc/pass_schedule.hpp) cuts an adaptive round into launches of at most launch_pass_cap(T, ..., kStagingBytes, kMaxPassesPerLaunch)
# passes: min(256, 8 GiB / 12 bytes / padded slots, 2^31 / padded slots - 1).  A list of 5 pixels pads to one tile of 256 slots, so
# the cap is kMaxPassesPerLaunch = 256 (the seeds of a launch travel in the kernel arguments) and 257 passes make two launches, of
# 256 and of 1 pass; the staging budget never binds at a size a test could afford (8 GiB / 12 / 256 passes = 2.8 million slots).
SPLIT_PASSES = 257
SPLIT_LIST = 5


# ---- scenes of the matrix and the instantiation each selects ----------------------------------------------------------------------
ENTITY_ARGS = dict(n_tris=600, seed=5, actor_tris=120, region=((2, 20, 2), (30, 44, 30)))  # golden_scenes.make("entities")


@functools.lru_cache(maxsize=None)
def scene(name, form=16, leaf=4):
    """Golden scene `name` in the octree that selects tree form `form`; "entities" with BVH leaves of `leaf` triangles."""
    chunks = gs.DEEP_CHUNKS if form == 17 else 2
    if name == "entities":
        sc = scenes.add_entities(gs.make("outdoor", chunks), leaf_size=leaf, **ENTITY_ARGS)
    else:
        sc = gs.make(name, chunks)
    depth = {16: 0, 17: 0, 18: 11, 19: 15, 0: 16}[form]
    return scenes.embed_deeper(sc, depth) if depth else sc


def bvh_height(nodes):
    """Levels of inner nodes above the deepest leaf (csrc/scene_records.cpp bvh_links_height)."""
    n = np.asarray(nodes)
    todo, height = [(0, 0)], 0
    while todo:
        at, d = todo.pop()
        height = max(height, d)
        if n[at] > 0:
            todo += [(at + 7, d + 1), (int(n[at]), d + 1)]
    return height


def bvh_pool(sc):
    """Parked paths per wave launch_pool gives a scene with entity BVHs: every path of the pool owns a to-visit stack of (height of
    the taller BVH + 1) entries in LDS, and 32 parked paths are taken while five workgroups of four waves fit 160 KB."""
    entries = max(bvh_height(sc.world_bvh), bvh_height(sc.actor_bvh)) + 1
    return 32 if 5 * 4 * (32 * 136 + (64 + 32) * entries * 4) <= 160 * 1024 else 16


BVH_LEAF = {32: 4, 16: 1}  # leaf size of scenes.build_bvh -> the pool: leaves of one triangle make the tree two levels taller


def test_entity_bvh_heights_select_both_pools():
    for form in (16, 17, 18):
        for pool, leaf in BVH_LEAF.items():
            assert bvh_pool(scene("entities", form, leaf)) == pool, (form, leaf)
    assert np.array_equal(scene("entities").world_bvh, gs.make("entities").world_bvh)  # leaf size 4 is the golden scene itself
    assert bvh_height(scene("entities").world_bvh) == 8 and bvh_height(scene("entities", 16, 1).world_bvh) == 10


def host_tree_form(sc):
    """The tree form of sc from the host side of the wide re-layout: 16 + the number of 8^3 levels under the dense top node — the
    default split's entry count is that of exactly one explicit split of this kind; 0 where the re-layout refuses the octree.
    (The count is 2^(3 top bits) entries of the top node plus 512 per 8^3 node the world needs below it, and a world needs a
    different number of nodes at every split, so a match names the split: tests/test_scenes.py test_default_split_by_entry_count
    does the same on a one-branch world, where the count can be written down.  The assertion below fails if two splits tie.)"""
    from test_scenes import DEFAULT_SPLIT
    cells = np.array([[0, 0, 0], [5, 40, 5]], np.int32)
    depth = int(sc.octree_depth)
    try:
        _data, _level, n = native.widetree_lookup(sc.octree, depth, cells)
    except native.ChunkyHipError:
        return 0
    same = [k for k in range(0, 4) if 1 <= depth - 3 * k <= 7
            and native.widetree_lookup(sc.octree, depth, cells, [depth - 3 * k] + [3] * k)[2] == n]
    assert same == [DEFAULT_SPLIT[depth][1]], (depth, n, same)
    return 16 + same[0]


def test_scenes_report_the_tree_form_the_cells_expect():
    for name in ("outdoor", "pregen", "entities", "dof", "inside"):
        for form in (16, 17, 18, 19, 0):
            if name in ("dof", "inside") and form not in (16, 17):
                continue
            assert host_tree_form(scene(name, form)) == form, (name, form)
            assert (scene(name, form).width, scene(name, form).height) == (W, H)
    assert host_tree_form(gs.embedded_offset()) == 18 and host_tree_form(gs.embedded_any()) == 19
    assert gs.EMBED_FORM[11] == 18 and gs.EMBED_FORM[15] == 19 and gs.EMBED_FORM[16] == 0


# ---- adaptive runs at the edges of the convergence kernels ------------------------------------------------------------------------
def fit_view(sc, w, h):
    """sc seen through w x h pixels with the field of view scaled so that the longer side spans what the 64 x 48 view spans across
    (a 16 384 x 1 view is a scan line over the landscape, not a fan of 16 384 rays along the horizon)."""
    cam = np.asarray(sc.camera, np.float32).copy()
    cam[14] = np.float32(cam[14] * (W / H) / max(w / h, W / H))
    return sc.with_view(w, h, camera=cam)


SMALL_SIZES = [(1, 1), (1, 7), (7, 1), (15, 15), (16, 16), (17, 17), (33, 1), (31, 47), (65, 5)]
TOO_SMALL = [(1, 1), (1, 7)]  # equality only: too few pixels for three counts
SMALL_SETTING = {"outdoor": (4, 2, 0.2), "entities": (4, 3, 0.4)}  # (min_spp, check_interval, threshold), max_spp = MAX_SPP
PREGEN_VIEW = (17, 17, 41, (4, 2, 0.2))  # width, height, seed of gs.pregen_rays, setting
# one tile row of exactly 1023, 1024, 1025 and 2049 tiles (adaptive_scan_kernel takes 1024 tile counts at a time): the ABI takes them
SCAN_WIDTHS = [16368, 16384, 16400, 32784]
SCAN_SETTING = (4, 2, 0.2)
SCAN_SPP = 12
# parameters at their edges, on "outdoor" at 64 x 48: id -> (max_spp, setting).  chunky_adaptive_params refuses min_spp below 2 (the
# statistic of one sample says nothing: tests/test_adaptive_cpu.py test_parameter_errors), so the smallest min_spp there is stands for 1
PARAM_EDGES = {"interval-1": (MAX_SPP, (8, 1, 0.2)), "min-spp-2": (MAX_SPP, (2, 4, 0.2)), "max-spp-39": (39, (8, 4, 0.2))}
ALL_LEAVE = ("outdoor", (8, 4, 1.0e6))  # every pixel leaves at the first check
NONE_LEAVES = ("inside", (8, 4, 0.0))   # no pixel ever leaves
TWO_RUNS = ((8, 4, 0.1), (6, 5, 0.3))   # on one target of "outdoor": the second run's lists are shorter than the first's


def small_scene(name, w, h):
    return fit_view(gs.make(name), w, h)


def pregen_scene():
    w, h, seed, _setting = PREGEN_VIEW
    sc = gs.make("outdoor")
    return sc.with_view(w, h, camera=gs.pregen_rays(sc, w, h, seed=seed), projector_type=-1)


def scan_scene(width):
    return fit_view(gs.make("outdoor"), width, 1)


_edge_samples = {}


def edge_samples(key, sc, n, tracer=None):
    if key not in _edge_samples:
        from oracle import binding
        _edge_samples[key] = sp.oracle_samples(tracer or binding.port(), sc, native.java_random_ints(n))
    return _edge_samples[key]


def check_points(setting, max_spp):
    mn, ci, _thr = setting
    return list(range(mn, max_spp, ci))


def host_active(counts, setting, max_spp):
    """The active pixels after every check of the run that gave `counts` (a run ends at the check that leaves none)."""
    out = []
    for d in check_points(setting, max_spp):
        out.append(int((counts > d).sum()))
        if out[-1] == 0:
            break
    return out


def non_degenerate(counts, max_spp, last_active):
    """The condition of every adaptive case that is meant to run the list route — on the host's counts here, on the device's there."""
    early = float((counts < max_spp).mean())
    return len(np.unique(counts)) >= 3 and 0.1 <= early <= 0.9 and last_active > 0


def assert_condition(s, setting, what):
    counts, _img, _st = native.adaptive_host(s, params(*setting))
    trace = []
    wc, _i, _s = sp.adaptive(s, setting[2], FLOOR, setting[0], setting[1], trace)
    assert np.array_equal(counts, wc), what
    assert host_active(counts, setting, s.shape[0]) == trace, what
    assert non_degenerate(counts, s.shape[0], trace[-1]), (what, np.unique(counts).tolist(), trace)
    return counts


@pytest.mark.parametrize("name", sorted(SMALL_SETTING))
def test_small_views_are_not_degenerate(port, name):
    for (w, h) in SMALL_SIZES:
        s = edge_samples((name, w, h), small_scene(name, w, h), MAX_SPP, port)
        assert s.shape == (MAX_SPP, h, w, 3)
        if (w, h) in TOO_SMALL:
            continue
        assert_condition(s, SMALL_SETTING[name], f"{name} {w} x {h}")


def test_pregen_view_is_not_degenerate(port):
    sc = pregen_scene()
    assert sc.camera.size == 6 * 17 * 17
    assert_condition(edge_samples("pregen17", sc, MAX_SPP, port), PREGEN_VIEW[3], "pregen 17 x 17")


@pytest.mark.parametrize("width", SCAN_WIDTHS)
def test_scan_views_are_not_degenerate(port, width):
    assert (width + 15) // 16 == {16368: 1023, 16384: 1024, 16400: 1025, 32784: 2049}[width]
    s = edge_samples(("scan", width), scan_scene(width), SCAN_SPP, port)
    counts = assert_condition(s, SCAN_SETTING, f"{width} x 1")
    act = counts.reshape(-1) == SCAN_SPP  # pixels active to the end lie in tiles on both sides of the scan's 1024-tile chunk edge
    if width > 16384:
        assert act[:16384].any() and act[16384:].any()


def test_parameter_edges_are_not_degenerate(port):
    s = samples_of("outdoor", port)
    for what, (max_spp, setting) in PARAM_EDGES.items():
        assert_condition(s[:max_spp], setting, what)
    mx, (mn, ci, _t) = PARAM_EDGES["max-spp-39"]
    assert (mx - mn) % ci != 0
    assert native.lib().chunky_adaptive_host(W, H, native.ptr(s), MAX_SPP, native.C.byref(params(1, 4, 0.2)), None, None, None) == native.E_INVALID
    for setting in TWO_RUNS:
        assert_condition(s, setting, f"two runs {setting}")
    a = host_active(native.adaptive_host(s, params(*TWO_RUNS[0]))[0], TWO_RUNS[0], MAX_SPP)
    b = host_active(native.adaptive_host(s, params(*TWO_RUNS[1]))[0], TWO_RUNS[1], MAX_SPP)
    assert max(b) < min(a), "every list of the second run is shorter than every list of the first"


def test_all_leave_and_none_leaves(port):
    name, setting = ALL_LEAVE
    counts = native.adaptive_host(samples_of(name, port), params(*setting))[0]
    assert (counts == setting[0]).all()
    name, setting = NONE_LEAVES
    counts = native.adaptive_host(samples_of(name, port), params(*setting))[0]
    assert (counts == MAX_SPP).all()
