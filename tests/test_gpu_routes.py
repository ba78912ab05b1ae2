"""The exhibits of tests/route_scenes.py on a real MI355X, bit for bit against tests/golden/routes.npz (outputs of the reference
build): the biome-water tint, the emittance texture, and the model blocks and entity BVHs that scene_records.cpp leaves on the packed
palettes — the second copy of the block and triangle arithmetic that no other fixture renders.  tests/test_routes_cpu.py proves
that the reference's own rays reach every route (the census) and which route the derivation picks for every exhibit; here every
case also asserts the kernel instantiation that ran.  The extensions have no reference: oracle/port.c is their specification."""
import numpy as np
import pytest

import golden_scenes as gs
import route_scenes as rs
from aov_spec import expected_aov
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader
from oracle import binding
from oracle.binding import PortExt
from test_shard_map_cpu import owner_table

pytestmark = pytest.mark.gpu
SEEDS = scenes.java_random_ints(rs.N_PASSES)


def make_renderer(gpu_instance, sc, variant=0):
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    return loader, r


def scene_and_fixture(name):
    g = rs.fixture()
    sc = rs.make(name)
    assert gs.input_digest(sc) == str(g[name + "_digest"]), "the regenerated scene is not the one the fixture was made from"
    assert np.array_equal(g["seeds"], SEEDS)
    return sc, g


def assert_image(r, g, name, what):
    diff = rs.first_difference(r.read(), g[name + "_res"], f"{name} radiance, {what}")
    if diff is not None:   # name the trace and the field: the first recorded pixel whose records differ
        if name in rs.RECORD_SCENES:
            want, cnt, _rad = rs.fixture_records(name)
            rec, got_cnt, _ = r.trace_records(int(SEEDS[0]), rs.RECORD_GIDS)
            diff += "; " + str(rs.records_difference(rec, got_cnt, want, cnt, "records"))
        pytest.fail(diff)


# ---- the exhibits at depth 6: every kernel that can render them ----
# variant -> (pool, tree, sorted) the launch has to report; pool < 0: a fallback kernel (render_waves / render_lanes)
ROUTES_KERNELS = {0: (64, 16, True), 512: (64, 16, False), 256: (64, 16, True), 8: (-1, None, False), 1: (64, 0, False), 2: (-1, None, False)}


@pytest.mark.parametrize("variant", list(ROUTES_KERNELS))
def test_exhibits_on_every_kernel(gpu_instance, variant):
    sc, g = scene_and_fixture("routes")
    loader, r = make_renderer(gpu_instance, sc, variant)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    pool, tree, sorted_ = ROUTES_KERNELS[variant]
    assert (info["pool"] == pool if pool > 0 else info["pool"] < 0) and info["sorted"] == sorted_ and not info["bvh"] and not info["ext"], info
    assert tree is None or info["tree"] == tree, info
    assert_image(r, g, "routes", f"variant {variant}")
    r.close()
    loader.close()


@pytest.mark.parametrize("depth", list(rs.EMBED_DEPTHS))
def test_exhibits_in_deeper_octrees(gpu_instance, depth):
    """Depth 7 is the form the timed views run (render_pool<17, 64, ...>), 11 a dense top over two 8^3 levels, 16 no wide tree."""
    name = f"routes_d{depth}"
    sc, g = scene_and_fixture(name)
    loader, r = make_renderer(gpu_instance, sc)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    form = rs.EMBED_DEPTHS[depth]
    assert (info["tree"], info["pool"], info["bvh"], info["ext"], info["sorted"]) == (form, 64, False, False, form != 0), info
    assert_image(r, g, name, f"tree form {form}")
    np.testing.assert_array_equal(r.preview(), g[name + "_preview"])
    r.close()
    loader.close()


# ---- the entity variants ----
@pytest.mark.parametrize("name", rs.ENTITY_SCENES)
def test_entity_variants(gpu_instance, name):
    """Triangles with an emittance texture and the water tint and a leaf of 63 triangles run render_pool's BVH instantiation on the
    aligned records; a leaf of 64 and a material pointer that is no multiple of 6 make the library itself choose the fallback
    kernels, which walk the packed arrays (no variant bit is set)."""
    sc, g = scene_and_fixture(name)
    loader, r = make_renderer(gpu_instance, sc)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["bvh"] and not info["ext"], info
    if rs.BVH_ON_RECORDS[name]:
        assert info["pool"] in (16, 32) and info["tree"] == -1, info
    else:
        assert info["pool"] < 0, info
    assert_image(r, g, name, "default kernel")
    np.testing.assert_array_equal(r.preview(), g[name + "_preview"])
    r.close()
    loader.close()


# ---- the other entry points ----
def test_preview(gpu_instance):
    sc, g = scene_and_fixture("routes")
    loader, r = make_renderer(gpu_instance, sc)
    np.testing.assert_array_equal(r.preview(), g["routes_preview"])
    r.close()
    loader.close()


@pytest.mark.parametrize("name", rs.RECORD_SCENES)
def test_trace_records(gpu_instance, name):
    sc, g = scene_and_fixture(name)
    want, cnt, rad = rs.fixture_records(name)
    loader, r = make_renderer(gpu_instance, sc)
    rec, got_cnt, got_rad = r.trace_records(int(SEEDS[0]), rs.RECORD_GIDS)
    diff = rs.records_difference(rec, got_cnt, want, cnt, name)
    assert diff is None, diff
    diff = rs.first_difference(got_rad, rad, f"{name} radiance of the recorded samples")
    assert diff is None, diff
    r.close()
    loader.close()


@pytest.mark.parametrize("tree", [0, 1])
@pytest.mark.parametrize("which", rs.HELPER_KINDS)
def test_device_helpers(gpu_instance, which, tree):
    """BlockPalette_intersectBlock (4) and Material_sample (12) as the device evaluates them, on rows drawn from the exhibits'
    palettes, against the reference's own helpers."""
    sc, g = scene_and_fixture("routes")
    rows = rs.helper_rows(which)
    assert gs.rows_digest(rows) == str(g[f"in{which}_sha256"])
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    got, _used = loader.selftest_helpers(which, rows, tree=tree)
    want = g[f"out{which}"]
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i, c = np.argwhere(~same)[0]
        pytest.fail(f"helper {which}: {int((~same).any(axis=1).sum())} of {len(want)} rows differ; first: row {i} column {c} got {got[i, c]!r} "
                    f"want {want[i, c]!r} (row starts with int {int(rows[i, :1].view(np.int32)[0])})")
    loader.close()


def test_aov_shows_the_water_tint(gpu_instance, port):
    """The albedo image is record.color of record 0 (tests/aov_spec.py), so tint 3 shows in it."""
    sc, _g = scene_and_fixture("routes")
    loader, r = make_renderer(gpu_instance, sc)
    r.render_aov(SEEDS)
    gids = np.arange(sc.width * sc.height)
    want = expected_aov(port, binding.SceneHandle(sc), SEEDS, gids)
    got = (r.read_aov(native.AOV_ALBEDO).reshape(-1, 3), r.read_aov(native.AOV_NORMAL).reshape(-1, 3))
    for k, kind in enumerate(("albedo", "normal")):
        diff = rs.first_difference(got[k], want[k], kind)
        assert diff is None, diff
    assert r.aov_info()["launches"] == 1
    r.close()
    loader.close()


def test_two_shards_of_blocks_sum_to_the_image(gpu_instance):
    sc, g = scene_and_fixture("routes")
    loader, r = make_renderer(gpu_instance, sc)
    full = g["routes_res"].reshape(-1, 3)
    own = owner_table(sc.width, sc.height, 2, 0)
    total = np.zeros_like(full)
    for rank in range(2):
        r.set_shard(rank, 2, 0)   # tile 0: 16 x 16-pixel blocks dealt round-robin
        r.reset()
        r.render_passes(SEEDS)
        assert r.kernel_info()["pool"] == 64, r.kernel_info()
        part = r.read().reshape(-1, 3)
        want = np.where((own == rank)[:, None], full, np.float32(0))
        diff = rs.first_difference(part, want, f"rank {rank} of 2")
        assert diff is None, diff
        total += part
    assert rs.first_difference(total, full, "sum of the shards") is None
    r.close()
    loader.close()


# ---- the extensions: oracle/port.c is their specification ----
def test_emitter_list(gpu_instance, port):
    """Cubes with an emittance texture (flag 2) are no emitters of the next-event estimation (scene_records.cpp list_emitters)."""
    sc, _g = scene_and_fixture("routes")
    _sc, B, _m = rs.base()
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    with PortExt(port, sc) as e:
        want = e.emitters[:e.n_emitters]
    got = loader.emitters()
    np.testing.assert_array_equal(got, want)
    blocks = got[:, 3] & ((1 << 25) - 1)
    assert len(got) == 9 and set(blocks.tolist()) == {B["glow"]}, got
    loader.close()


def test_extended_render(gpu_instance, port):
    sc, _g = scene_and_fixture("routes")
    loader, r = make_renderer(gpu_instance, sc)
    r.set_option(native.OPT_BSDF, 1)
    r.set_option(native.OPT_EMITTER_NEE, 1)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert info["ext"] and info["pool"] == 32 and not info["sorted"], info
    with PortExt(port, sc, bsdf=1, nee=1):
        want = port.render_passes(sc, SEEDS)
    diff = rs.first_difference(r.read(), want, "bsdf + nee")
    assert diff is None, diff
    assert not np.array_equal(want.view(np.uint32), rs.fixture()["routes_res"].view(np.uint32)), "the options changed nothing"
    r.close()
    loader.close()
