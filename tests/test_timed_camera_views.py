"""The camera kinds, tints and atlas layers on the kernels that are timed.  Every golden world has octree depth 6 (render_pool<16, ...>)
and the timed rows hold pinhole views only, so depth of field, pre-generated rays, a camera outside the world, a flooded world,
textures over several atlas layers, sun draws indoors and the extended integrator never ran on render_pool<17, ...> in a test.
(The flooded world does not stand for the biome-water tint: 4 of the 400 726 traces of its rows land on water, and none of the small
`water` goldens' — profiles/route_census.json.  tests/test_gpu_routes.py compares tint 3, on render_pool<17, ...> too.)
tests/golden/timed_camera_rows.npz holds rows of such views at the timed sizes (golden_scenes.camera_view), rendered by the REFERENCE
build (tests/golden/generate.py cameras).  The C restatement must reproduce them (CPU), and so must the HIP kernels (GPU), in the
instantiation golden_scenes.CAMERA_KERNEL names, in the other block-test order, in block shards and in launches longer than the
kernel-argument segment.  Small depth-7 copies of the golden scenes run every kernel variant on the same tree form, and the extended
integrator is checked against its specification there and on the timed worlds."""
import os

import numpy as np
import pytest

import golden_scenes as gs
from chunkyclplugin_amd import scenes
from oracle import binding

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "timed_camera_rows.npz"))
THREADS = binding.usable_threads()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_VIEWS = {}


@pytest.fixture(scope="module")
def views():
    def get(name):
        if name not in _VIEWS:
            _VIEWS.clear()   # one 1080p scene (and its 50 MB ray buffer) at a time
            sc = gs.camera_view(name)
            assert gs.input_digest(sc) == str(GOLD[name + "_digest"]), "regenerated scene differs from the one the golden rows were made from"
            _VIEWS[name] = sc
        return _VIEWS[name]
    return get


def row_gids(sc, rows):
    return np.concatenate([np.arange(y * sc.width, (y + 1) * sc.width) for y in rows]).astype(np.int32)


def test_fixture_holds_every_view():
    assert sorted(k[:-len("_digest")] for k in GOLD.files if k.endswith("_digest")) == sorted(gs.CAMERA_VIEWS)
    np.testing.assert_array_equal(GOLD["seeds"], scenes.java_random_ints(gs.TIMED_PASSES))


@pytest.mark.parametrize("name", gs.CAMERA_VIEWS)
def test_restatement_matches_the_reference_on_camera_views(port, views, name):
    sc = views(name)
    rows = GOLD[name + "_rows"]
    assert rows.tolist() == gs.camera_rows(sc)
    gids = row_gids(sc, rows)
    got = port.render_gids(binding.SceneHandle(sc), GOLD["seeds"], gids, threads=THREADS).reshape(-1, 3)[gids]
    np.testing.assert_array_equal(bits(got), bits(GOLD[name + "_res"].reshape(-1, 3)))


def test_reference_still_gives_a_committed_row_of_the_entity_rays(ref, views):
    """Where the reference build exists: one row of pre-generated rays into the entity world is what it returns today."""
    sc = views("entities_pregen")
    y = int(GOLD["entities_pregen_rows"][2])
    full = ref.render_passes(binding.SceneHandle(sc), GOLD["seeds"], gid_range=(y * sc.width, (y + 1) * sc.width), threads=THREADS)
    np.testing.assert_array_equal(bits(full.reshape(-1, 3)[y * sc.width:(y + 1) * sc.width]), bits(GOLD["entities_pregen_res"][2]))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
def make(gpu_instance, sc, variant=0, **opts):
    from chunkyclplugin_amd import native
    from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader
    loader = HipSceneLoader(gpu_instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    r.set_option(native.OPT_KERNEL, variant)
    for k, v in opts.items():
        r.set_option({"sun_sampling": native.OPT_SUN_SAMPLING, "emitters": native.OPT_EMITTERS, "bsdf": native.OPT_BSDF,
                      "nee": native.OPT_EMITTER_NEE}[k], v)
    return loader, r


def assert_kernel(info, tree, bvh, sorted_, ext=False):
    assert (info["tree"], info["bvh"], info["sorted"], info["ext"]) == (tree, bvh, sorted_, ext), info
    assert (info["pool"] in (16, 32)) if bvh else (info["pool"] == 64), info


def assert_rows(got, want, gids, what):
    same = (bits(got) == bits(want)).all(axis=1)
    assert same.all(), f"{what}: {int((~same).sum())} of {len(gids)} pixels differ (first gid {int(gids[np.argmin(same)])})"


@pytest.mark.gpu
@pytest.mark.parametrize("name", gs.CAMERA_VIEWS)
def test_hip_matches_the_reference_on_camera_views(gpu_instance, views, name):
    sc = views(name)
    loader, r = make(gpu_instance, sc)
    r.render_passes(GOLD["seeds"])
    assert_kernel(r.kernel_info(), *gs.CAMERA_KERNEL[name])
    gids = row_gids(sc, GOLD[name + "_rows"])
    assert_rows(r.read().reshape(-1, 3)[gids], GOLD[name + "_res"].reshape(-1, 3), gids, name)
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant,sorted_", [("outdoor_dof", 256, True), ("outdoor_pregen", 256, True), ("city_dof", 512, False)])
def test_the_other_block_test_order_on_camera_views(gpu_instance, views, name, variant, sorted_):
    """CHUNKY_OPT_KERNEL bit 8 / bit 9: the block-test order these views do NOT run by default gives the reference build's rows too."""
    sc = views(name)
    loader, r = make(gpu_instance, sc, variant)
    r.render_passes(GOLD["seeds"])
    assert_kernel(r.kernel_info(), 17, False, sorted_)
    gids = row_gids(sc, GOLD[name + "_rows"])
    assert_rows(r.read().reshape(-1, 3)[gids], GOLD[name + "_res"].reshape(-1, 3), gids, f"{name}, variant {variant}")
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", gs.CAMERA_VIEWS)
def test_hip_matches_the_live_reference_build_on_camera_views(gpu_instance, ref, views, name):
    """Where the reference build travelled to the GPU box (skipped elsewhere): the WHOLE image, 2 passes of a java.util.Random
    stream the fixture does not hold, rendered by the reference kernel on the host's CPUs and by the HIP kernels, bit for bit."""
    from chunkyclplugin_amd import native
    sc = views(name)
    seeds = native.java_random_ints(2, seed=24681357)
    want = ref.render_passes(binding.SceneHandle(sc), seeds, threads=THREADS)
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    assert_kernel(r.kernel_info(), *gs.CAMERA_KERNEL[name])
    same = (bits(r.read()) == bits(want)).reshape(-1, 3).all(axis=1)
    assert same.all(), f"{name}: {int((~same).sum())} of {same.size} pixels differ from the live reference build (first gid {int(np.argmin(same))})"
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["outdoor_dof", "outdoor_pregen"])
def test_block_shards_of_camera_views(gpu_instance, port, views, name):
    """The 16 x 16 block split of bench.py --gpus 3, every rank (the ragged view's padded edge blocks included): each rank's pixels of
    the fixture's rows against the C restatement, nobody else's pixels touched, and the ranks' pixel sets partition the image."""
    from chunkyclplugin_amd import native, parallel
    sc = views(name)
    n = sc.width * sc.height
    seeds = native.java_random_ints(16)
    gids = row_gids(sc, GOLD[name + "_rows"])
    want = port.render_gids(binding.SceneHandle(sc), seeds, gids, threads=THREADS).reshape(-1, 3)
    loader, r = make(gpu_instance, sc)
    covered = np.zeros(n, np.int32)
    for rank in range(3):
        r.reset()
        r.set_shard(rank, 3, 0)
        r.render_passes(seeds)
        assert_kernel(r.kernel_info(), 17, False, False)
        own = parallel.owned_gids(n, rank, 3, 0, sc.width)
        covered[own] += 1
        mine = np.intersect1d(gids, own)
        img = r.read().reshape(-1, 3)
        assert_rows(img[mine], want[mine], mine, f"{name} block share {rank}/3")
        mask = np.ones(n, bool)
        mask[own] = False
        assert not img[mask].any(), f"{name} share {rank}/3 wrote pixels of another rank"
    assert (covered == 1).all()
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["outdoor_dof", "outdoor_pregen"])
def test_one_launch_longer_than_the_argument_segment_on_camera_views(gpu_instance, port, views, name):
    """300 passes in ONE launch of render_pool<17, 64> (the seeds beyond 256 come from device memory) on a few rows."""
    from chunkyclplugin_amd import native
    sc = views(name)
    seeds = native.java_random_ints(300)
    loader, r = make(gpu_instance, sc)
    r.kernel_time()
    r.render_passes(seeds)
    info = r.kernel_info()
    assert_kernel(info, 17, False, False)
    assert info["passes_per_launch"] > 256 and r.kernel_time()[1] == 1, info
    rows = GOLD[name + "_rows"]
    gids = row_gids(sc, (rows[3], rows[-1]))[::3]
    want = port.render_gids(binding.SceneHandle(sc), seeds, gids, threads=THREADS).reshape(-1, 3)[gids]
    assert_rows(r.read().reshape(-1, 3)[gids], want, gids, f"{name} 300 passes")
    r.close()
    loader.close()


# ---- the variant matrix on tree 17: depth-7 copies of the golden scenes --------------------------------------------------------
_DEEP = {}


def deep(name):
    if name not in _DEEP:
        _DEEP[name] = gs.make(name, gs.DEEP_CHUNKS)
    return _DEEP[name]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 64, 128, 8, 9, 8 | 16, 256, 512])
@pytest.mark.parametrize("name", gs.DEEP_NAMES)
def test_depth7_golden_copies_match_the_restatement(gpu_instance, port, name, variant):
    """Every CHUNKY_OPT_KERNEL variant of test_gpu_parity.VARIANTS on the 8-chunk copies (octree depth 7): image and preview."""
    sc = deep(name)
    assert sc.octree_depth == 7
    seeds = scenes.java_random_ints(gs.N_PASSES)
    loader, r = make(gpu_instance, sc, variant)
    r.render_passes(seeds)
    if variant == 0:
        assert r.kernel_info()["tree"] == 17, r.kernel_info()
    np.testing.assert_array_equal(bits(r.read()), bits(port.render_passes(sc, seeds, threads=THREADS)))
    np.testing.assert_array_equal(r.preview(), port.preview(sc))
    r.close()
    loader.close()


# ---- the extended integrator on render_pool<17, ...> ----------------------------------------------------------------------------
DEEP_EXT_CASES = [("outdoor_nosun", dict(sun_sampling=1, bsdf=1)), ("dof", dict(bsdf=1, nee=1)), ("pregen", dict(bsdf=1, sun_sampling=0)),
                  ("inside", dict(bsdf=1, nee=1)), ("water", dict(bsdf=1, sun_sampling=1, nee=1)), ("atlas_layers", dict(emitters=0, bsdf=1))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts", DEEP_EXT_CASES)
def test_extended_kernel_on_depth7_worlds(gpu_instance, port, name, opts):
    from oracle.binding import PortExt
    from test_gpu_extensions import with_spec_words
    sc = with_spec_words(deep(name))
    seeds = scenes.java_random_ints(6)
    loader, r = make(gpu_instance, sc, **opts)
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["ext"] and info["tree"] == 17 and info["pool"] > 0, info
    with PortExt(port, sc, **opts):
        want = port.render_passes(sc, seeds, threads=THREADS)
    np.testing.assert_array_equal(bits(r.read()), bits(want))
    assert not np.array_equal(bits(port.render_passes(sc, seeds, threads=THREADS)), bits(want)), "the options changed nothing"
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,opts", [("outdoor", dict(bsdf=1, nee=1)), ("indoor", dict(nee=1)), ("entities", dict(bsdf=1))])
def test_extended_kernel_on_timed_worlds(gpu_instance, port, name, opts):
    """The extended integrator on the timed outdoor world and the emitter-lit room (render_pool<17, 64, ext>: the outdoor world has
    no emitters, the room's NEE draws them) and on the 100 000-triangle entity world (render_pool<17, ., bvh, ext>), whole rows
    against its specification."""
    from chunkyclplugin_amd import native
    from oracle.binding import PortExt
    from test_gpu_extensions import with_spec_words
    _VIEWS.clear()
    sc = with_spec_words(gs.timed_view(name))
    seeds = native.java_random_ints(4)
    loader, r = make(gpu_instance, sc, **opts)
    r.render_passes(seeds)
    info = r.kernel_info()
    assert info["ext"] and info["tree"] == 17 and info["bvh"] == (name == "entities") and info["pool"] > 0, info
    gids = row_gids(sc, (202, 540, 877))
    with PortExt(port, sc, **opts):
        want = port.render_gids(binding.SceneHandle(sc), seeds, gids, threads=THREADS).reshape(-1, 3)[gids]
    assert_rows(r.read().reshape(-1, 3)[gids], want, gids, f"{name} {opts}")
    base = port.render_gids(binding.SceneHandle(sc), seeds, gids, threads=THREADS).reshape(-1, 3)[gids]
    assert not np.array_equal(bits(base), bits(want)), "the options changed nothing on these rows"
    r.close()
    loader.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [dict(emitters=0), dict(nee=1)])
def test_extended_options_refuse_max_depth_255(gpu_instance, port, opts):
    """render_pool marks a fresh path with depth 255, so max depth 255 runs the fallback kernels, which have none of the extended
    options: render_passes refuses (E_STATE) instead of rendering the reference's transport, and writes nothing.  At 254 the
    extended kernel runs and gives its specification's image at that depth."""
    from chunkyclplugin_amd import native
    from oracle.binding import PortExt, PortOptions
    sc = gs.make("indoor_sun").with_view(40, 24)
    seeds = scenes.java_random_ints(2)
    loader, r = make(gpu_instance, sc, **opts)
    r.set_option(native.OPT_MAX_DEPTH, 255)
    with pytest.raises(native.ChunkyHipError) as e:
        r.render_passes(seeds)
    assert e.value.code == native.E_STATE
    assert not r.read().any()
    r.set_option(native.OPT_MAX_DEPTH, 254)
    r.render_passes(seeds)
    assert r.kernel_info()["ext"] and r.kernel_info()["pool"] >= 0, r.kernel_info()
    with PortExt(port, sc, **opts), PortOptions(port, max_depth=254):
        want = port.render_passes(sc, seeds)
    np.testing.assert_array_equal(bits(r.read()), bits(want))
    r.close()
    loader.close()
