"""Biome tints by block position on the device (chunky_scene_set_biome_tints): every float and every ARGB bit
against the oracle's image of the expanded world (tests/biome_spec.py expand: the tinted blocks replaced, cell by cell, by copies with
constant tints) — on the C restatement, and on the reference build where it exists.  Two fixtures: the golden `water` world with a
patch map (tree form 16, served by the generic walk; eleven tinted leaves larger than one cell) and the 32^3 exhibit (entity BVHs; a
tinted AABB model and a tinted quad model; all three tint types inside and outside the map, tests/test_biome_cpu.py test_census).
Every comparison is over every pixel and every channel, without tolerance."""
import dataclasses

import numpy as np
import pytest

import biome_spec as bs
import golden_scenes as gs
from aov_ex_spec import expected_aov_ex
from aov_spec import expected_aov
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.native import ChunkyHipError
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance
from oracle.binding import PortOptions

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(3)
FIXTURES = {"exhibit": bs.exhibit, "water": bs.water_world}
LANES, REFERENCE_TREE = 2, 1  # CHUNKY_OPT_KERNEL bits


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(instance, sc, **options):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    for k, v in options.items():
        r.set_option(getattr(native, "OPT_" + k.upper()), v)
    return loader, r


def close(*xs):
    for x in xs:
        x.close()


def assert_image(got, want, what):
    g, w = bits(got).reshape(-1, 3), bits(want).reshape(-1, 3)
    same = (g == w).all(axis=1)
    if not same.all():
        i = int(np.argmin(same))
        pytest.fail(f"{what}: {int((~same).sum())} of {len(same)} pixels differ (first: pixel {i}, {g[i].view(np.float32).tolist()!r} against "
                    f"{w[i].view(np.float32).tolist()!r})")


@pytest.fixture(scope="module")
def oracle(port):
    """The oracle's image of the expanded world of a scene with a map, computed once per (scene, seeds, options) and never changed."""
    cache = {}

    def get(sc, seeds=SEEDS, first_spp=0, key=None, **options):
        k = (key or sc.name, sc.width, sc.height, tuple(int(s) for s in seeds), first_spp, tuple(sorted(options.items())))
        if k not in cache:
            with PortOptions(port, **options):
                img = port.render_passes(bs.expand(sc), seeds, first_spp=first_spp)
            img.setflags(write=False)
            cache[k] = img
        return cache[k]
    return get


def kernel(r):
    i = r.kernel_info()
    return i["tree"], i["bvh"], i["pool"], i["biome"]


# the instantiation each fixture runs by default: the exhibit has entity triangles (five workgroups of 32 parked paths fit beside its stacks)
DEFAULT_KERNEL = {"exhibit": (-1, True, 32, True), "water": (-1, False, native.BIOME_POOL_PARK, True)}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_whole_images(gpu_instance, oracle, port, name):
    sc = FIXTURES[name]()
    loader, r = make(gpu_instance, sc)
    assert kernel(r) == DEFAULT_KERNEL[name]  # named before the first launch ...
    r.render_passes(SEEDS)
    got = r.read()
    assert kernel(r) == DEFAULT_KERNEL[name] and r.kernel_info()["blocks"] > 0  # ... and after it
    assert_image(got, oracle(sc), name)
    plain = port.render_passes(dataclasses.replace(sc, biome=None), SEEDS)
    assert bits(got).tobytes() != bits(plain).tobytes()  # the map is seen
    close(r, loader)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_whole_images_on_the_reference_build(gpu_instance, ref, name):
    sc = FIXTURES[name]()
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    assert_image(r.read(), ref.render_passes(bs.expand(sc), SEEDS), name + " (reference build)")
    close(r, loader)


def test_two_calls_equal_one(gpu_instance, oracle):
    sc = bs.exhibit()
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS[:2])
    r.render_passes(SEEDS[2:], first_buffer_spp=2)
    assert_image(r.read(), oracle(sc), "2 + 1 passes")
    close(r, loader)


def test_first_buffer_spp(gpu_instance, oracle):
    sc = bs.water_world()
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS, first_buffer_spp=7)
    assert_image(r.read(), oracle(sc, first_spp=7), "first_buffer_spp 7")
    close(r, loader)


@pytest.mark.parametrize("depth", [1, 8])
def test_max_depth(gpu_instance, oracle, depth):
    sc = bs.exhibit()
    loader, r = make(gpu_instance, sc, max_depth=depth)
    r.render_passes(SEEDS)
    assert_image(r.read(), oracle(sc, max_depth=depth), f"max depth {depth}")
    close(r, loader)


def sun_off(sc):
    sun = np.array(sc.sun, np.int32)
    sun[0] &= ~1
    return dataclasses.replace(sc, sun=sun, name=sc.name + "-nosun")


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_sun_flag_off(gpu_instance, oracle, name):
    sc = sun_off(FIXTURES[name]())
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    assert_image(r.read(), oracle(sc), name + ", sun flag off")
    close(r, loader)


def test_emitter_scale_zero(gpu_instance, oracle):
    sc = bs.water_world()
    loader, r = make(gpu_instance, sc, emitter_scale=0.0)
    r.render_passes(SEEDS)
    assert_image(r.read(), oracle(sc, emitter_scale=0.0), "emitter scale 0")
    close(r, loader)


@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("variant", [0, LANES])
def test_constants_map_and_option_off(gpu_instance, name, variant):
    """A map of the reference's constants renders the image the same target renders with the option off, and the option off with a map
    is a scene without one — and then exactly the kernels of a scene without one run."""
    sc = FIXTURES[name]()
    x0, z0, rgb = sc.biome
    plain = dataclasses.replace(sc, biome=None)
    lp, rp = make(gpu_instance, plain, kernel=variant)
    rp.render_passes(SEEDS)
    want, info = rp.read(), rp.kernel_info()
    assert not info["biome"]
    loader, r = make(gpu_instance, dataclasses.replace(sc, biome=(x0, z0, bs.constants_map(rgb.shape[1], rgb.shape[0]))), kernel=variant)
    r.render_passes(SEEDS)
    assert r.kernel_info()["biome"]
    assert_image(r.read(), want, "a map of constants")
    r.set_option(native.OPT_BIOME_TINT, 0)
    r.reset()
    r.render_passes(SEEDS)
    assert {k: v for k, v in r.kernel_info().items() if k != "blocks"} == {k: v for k, v in info.items() if k != "blocks"}
    assert_image(r.read(), want, "option off, constants")
    close(r, loader)
    loader, r = make(gpu_instance, sc, kernel=variant, biome_tint=0)
    r.render_passes(SEEDS)
    assert not r.kernel_info()["biome"]
    assert_image(r.read(), want, "option off with a patch map")
    assert np.array_equal(r.preview(), rp.preview())
    close(r, loader, rp, lp)


def with_water_map(sc, chunks=2):
    x0, z0, sx, sz, patch = bs.WATER_MAP
    if chunks != 2:
        sx, sz = 16 * chunks - 24, 16 * chunks - 32
    return dataclasses.replace(sc, biome=(x0, z0, scenes.biome_patches(sx, sz, patch, seed=77)), name=sc.name + "+biome")


# (key, scene, kernel option, the instantiation that must run: tree, entity BVHs, pool): the rigs of tests/test_gpu_lights.py test_tree_forms
def form_cases():
    for key, build, (form, bvh) in gs.form_cases():
        chunks = gs.DEEP_CHUNKS if key.startswith("deep-") else 2
        served = form if form in ((17,) if bvh else (0, 17, 18)) else -1   # 19 runs the generic walk; with entities 18 does too
        yield key, (lambda b=build, c=chunks: with_water_map(b(), c)), 0, (served, bvh, None if bvh else native.BIOME_POOL_PARK)
    yield "water-reference-tree", bs.water_world, REFERENCE_TREE, (0, False, native.BIOME_POOL_PARK)       # the pool kernel's form 0
    yield "water-lanes", bs.water_world, LANES, (-1, False, -1)                                           # the fallback route: variant bit 1
    yield "water-lanes-reference-tree", bs.water_world, LANES | REFERENCE_TREE, (0, False, -1)
    yield "exhibit-lanes", bs.exhibit, LANES, (-1, True, -1)                                              # ... with the entity walk
    yield "exhibit-waves-forced", bs.exhibit, 8, (-1, True, -1)                                           # render_waves' plans run render_lanes
    yield "water-pool-rig-32", bs.water_world, 2 << 6, (-1, False, native.BIOME_POOL_PARK)                # rig pool sizes go to the biome kernel's
    yield "water-sorted-forced", bs.water_world, 256, (-1, False, native.BIOME_POOL_PARK)                 # sorted goes to unsorted


FORM_CASES = list(form_cases())


@pytest.mark.parametrize("key,build,variant,want", FORM_CASES, ids=[c[0] for c in FORM_CASES])
def test_tree_forms_and_routes(gpu_instance, oracle, key, build, variant, want):
    sc = build()
    loader, r = make(gpu_instance, sc, kernel=variant)
    r.render_passes(SEEDS)
    info = r.kernel_info()
    assert (info["tree"], info["bvh"]) == want[:2] and info["biome"] and not info["sorted"] and not info["ext"], info
    assert info["pool"] == want[2] if want[2] is not None else info["pool"] in native.BIOME_POOL_BVH_PARKS, info   # (with entities: what fits beside the stacks)
    assert_image(r.read(), oracle(sc, key=key), key)
    close(r, loader)


def test_pregenerated_camera(gpu_instance, oracle):
    base = bs.water_world()
    sc = dataclasses.replace(base, camera=gs.make("pregen").camera, projector_type=-1, name="water+biome-pregen")
    loader, r = make(gpu_instance, sc)
    r.render_passes(SEEDS)
    assert kernel(r) == DEFAULT_KERNEL["water"]
    assert_image(r.read(), oracle(sc), "pre-generated rays")
    close(r, loader)


def owner(sc, world, tile):
    gid = np.arange(sc.width * sc.height)
    if tile > 0:
        return (gid // tile) % world
    bw = (sc.width + 15) // 16
    return ((gid // sc.width // 16) * bw + (gid % sc.width) // 16) % world


@pytest.mark.parametrize("tile,variant", [(0, 0), (7, 0), (0, LANES)])
def test_shards(gpu_instance, oracle, tile, variant):
    """A block shard and a run shard, every rank (and a block shard under render_lanes, which takes the rank's pixels as a list)."""
    sc = bs.exhibit()
    want = oracle(sc).reshape(-1, 3)
    for rank in range(3):
        loader, r = make(gpu_instance, sc, kernel=variant)
        r.set_shard(rank, 3, tile)
        r.render_passes(SEEDS)
        got = r.read().reshape(-1, 3)
        mine = owner(sc, 3, tile) == rank
        assert mine.any() and not mine.all() and r.kernel_info()["biome"]
        assert_image(got[mine], want[mine], f"rank {rank} of 3, tile {tile}")
        assert not bits(got[~mine]).any()
        close(r, loader)


def test_group_equals_one_context(gpu_instance, oracle):
    g = RendererInstance.group([0, 0])
    sc = bs.exhibit()
    lg, rg = make(g, sc)
    rg.render_passes(SEEDS[:2])
    rg.render_passes(SEEDS[2:], first_buffer_spp=2)
    assert_image(rg.read(), oracle(sc), "a two-member group")
    assert rg.kernel_info()["biome"]
    assert np.array_equal(rg.preview(), HipPreview.of(gpu_instance, sc))
    close(rg, lg, g)


class HipPreview:
    @staticmethod
    def of(instance, sc):
        loader, r = make(instance, sc)
        out = r.preview()
        close(r, loader)
        return out


def test_set_twice_and_removal_against_fresh_uploads(gpu_instance, oracle, port):
    """The setter again, with another rectangle, and the removal — each against a fresh upload, with passes queued in between and
    never waited for: launches already queued finish on the old map."""
    sc = bs.exhibit()
    second = dataclasses.replace(sc, biome=(0, 3, scenes.biome_patches(29, 17, 4, seed=5)), name="biome-exhibit-second-map")
    plain = dataclasses.replace(sc, biome=None)
    loader, r = make(gpu_instance, sc)
    r2 = HipPathTracingRenderer(loader, sc.width, sc.height)   # a second target on the same scene keeps the first map's image
    r2.set_camera(sc.projector_type, sc.camera)
    r2.render_passes(SEEDS, sync=False)
    loader.set_biome_tints(*second.biome)
    r.render_passes(SEEDS, sync=False)
    loader.set_biome_tints(0, 0, None)
    r3 = HipPathTracingRenderer(loader, sc.width, sc.height)
    r3.set_camera(sc.projector_type, sc.camera)
    r3.render_passes(SEEDS, sync=False)
    assert not r3.kernel_info()["biome"]
    assert_image(r2.read(), oracle(sc), "queued before the second map")
    assert_image(r.read(), oracle(second), "the second map")
    assert_image(r3.read(), port.render_passes(plain, SEEDS), "after removal")
    lf, rf = make(gpu_instance, second)
    rf.render_passes(SEEDS)
    assert bits(rf.read()).tobytes() == bits(r.read()).tobytes()   # ... and a fresh upload of the second map
    close(r, r2, r3, rf, loader, lf)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_preview(gpu_instance, port, name):
    sc = FIXTURES[name]()
    loader, r = make(gpu_instance, sc)
    got = r.preview()
    assert np.array_equal(got, port.preview(bs.expand(sc)))
    assert not np.array_equal(got, port.preview(dataclasses.replace(sc, biome=None)))
    r.set_option(native.OPT_KERNEL, REFERENCE_TREE)
    assert np.array_equal(r.preview(), got)
    close(r, loader)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_albedo_and_normal(gpu_instance, port, name):
    """The AOV's albedo is the expanded world's; the normal image is the image without a map."""
    sc = FIXTURES[name]()
    gids = np.arange(sc.width * sc.height)
    loader, r = make(gpu_instance, sc)
    r.render_aov(SEEDS)
    info = r.aov_info()
    assert info["biome"] and info["bvh"] == (name == "exhibit") and info["tree"] == (-1 if name == "exhibit" else 16), info
    albedo, normal = r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL)
    want_a, want_n = expected_aov(port, bs.expand(sc), SEEDS, gids)
    assert_image(albedo, want_a, "albedo")
    assert_image(normal, want_n, "normal")
    lp, rp = make(gpu_instance, dataclasses.replace(sc, biome=None))
    rp.render_aov(SEEDS)
    assert not rp.aov_info()["biome"]
    assert bits(rp.read_aov(native.AOV_NORMAL)).tobytes() == bits(normal).tobytes()
    assert bits(rp.read_aov(native.AOV_ALBEDO)).tobytes() != bits(albedo).tobytes()
    close(r, loader, rp, lp)


def test_aov_tree_form_17(gpu_instance, port):
    sc = with_water_map(gs.make(gs.DEEP_NAMES[0], gs.DEEP_CHUNKS), gs.DEEP_CHUNKS)
    gids = np.arange(sc.width * sc.height)
    loader, r = make(gpu_instance, sc)
    r.render_aov(SEEDS)
    info = r.aov_info()
    assert info["biome"] and info["tree"] == 17, info
    want_a, want_n = expected_aov(port, bs.expand(sc), SEEDS, gids)
    assert_image(r.read_aov(native.AOV_ALBEDO), want_a, "albedo, form 17")
    assert_image(r.read_aov(native.AOV_NORMAL), want_n, "normal, form 17")
    close(r, loader)


EX_IMAGES = {"albedo": native.AOV_ALBEDO, "normal": native.AOV_NORMAL, "alpha": native.AOV_ALPHA, "depth": native.AOV_DEPTH,
             "position": native.AOV_POSITION, "emittance": native.AOV_EMITTANCE, "block": native.AOV_BLOCK}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_ex_images_mattes_and_occlusion_do_not_see_the_map(gpu_instance, port, name):
    """The _ex images other than albedo (the block id reports the octree's own block pointers), the mattes and the occlusion images:
    bit-identical with and without the map; the _ex albedo is the expanded world's."""
    sc = FIXTURES[name]()
    lp, rp = make(gpu_instance, dataclasses.replace(sc, biome=None))
    loader, r = make(gpu_instance, sc)
    for x in (rp, r):
        x.render_aov_ex(SEEDS)
        x.render_matte(SEEDS)
        x.render_occlusion(SEEDS, 3.0)
    assert r.aov_info()["biome"] and not rp.aov_info()["biome"]
    for k, which in EX_IMAGES.items():
        a, b = r.read_aov_ex(which), rp.read_aov_ex(which)
        assert (bits(a).tobytes() == bits(b).tobytes()) == (k != "albedo"), k
    want = expected_aov_ex(port, bs.expand(sc), SEEDS, np.arange(sc.width * sc.height))
    assert_image(r.read_aov_ex(native.AOV_ALBEDO), want["albedo"], "_ex albedo")
    for a, b in zip(r.read_matte(), rp.read_matte()):
        assert np.array_equal(a, b)
    for which in (native.AOV_AO, native.AOV_SUN):
        assert bits(r.read_occlusion(which)).tobytes() == bits(rp.read_occlusion(which)).tobytes()
    close(r, loader, rp, lp)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_trace_records(gpu_instance, port, name):
    """Every field of every record of pass 0 is the expanded world's, with `material` mapped back to the octree's own block pointer."""
    sc = FIXTURES[name]()
    ex, origin = bs.expand(sc, with_origin=True)
    gids = np.arange(0, sc.width * sc.height, 5, dtype=np.int32)
    loader, r = make(gpu_instance, sc)
    rec, cnt, rad = r.trace_records(int(SEEDS[0]), gids)
    copies = 0
    for i, gid in enumerate(gids):
        want, want_rad = port.trace_records(ex, int(SEEDS[0]), int(gid))
        assert cnt[i] == len(want)
        copies += sum(int(m) in origin for m in want["material"])
        want = want.copy()
        want["material"] = [origin.get(int(m), int(m)) for m in want["material"]]
        assert rec[i, :cnt[i]].tobytes() == want.tobytes(), int(gid)
        assert bits(rad[i]).tobytes() == bits(want_rad).tobytes()
    assert copies > 50
    close(r, loader)


REFUSED_OPTIONS = [("sun_sampling", 1), ("emitters", 0), ("bsdf", 1), ("emitter_nee", 1), ("kernel", 4)]


@pytest.mark.parametrize("option,value", REFUSED_OPTIONS, ids=[o for o, _v in REFUSED_OPTIONS])
def test_options_without_a_biome_kernel_are_refused(gpu_instance, option, value):
    """The extended light-transport options and the phase statistics: CHUNKY_E_STATE with the reason, nothing rendered; with the
    option at 0 the same call is served."""
    sc = bs.water_world()
    loader, r = make(gpu_instance, sc, **{option: value})
    with pytest.raises(ChunkyHipError) as e:
        r.render_passes(SEEDS)
    assert e.value.code == native.E_STATE and "biome" in str(e.value)
    assert not bits(r.read()).any() and r.kernel_info()["blocks"] == 0
    r.set_option(native.OPT_BIOME_TINT, 0)
    r.render_passes(SEEDS)
    assert r.read().any()
    close(r, loader)


def test_projected_camera_is_refused_on_the_pool_kernel_and_served_by_render_lanes(gpu_instance, port):
    from chunkyclplugin_amd.renderer import camera_rays
    from test_camera_lens_ods_cpu import projected
    kind = native.PROJ_FISHEYE
    sc = projected(bs.water_world(), kind)
    loader, r = make(gpu_instance, sc)
    with pytest.raises(ChunkyHipError) as e:
        r.render_passes(SEEDS)
    assert e.value.code == native.E_STATE and "projected" in str(e.value)
    assert not bits(r.read()).any()
    r.set_option(native.OPT_KERNEL, LANES)
    r.render_passes(SEEDS)
    want = None
    for i, seed in enumerate(SEEDS):
        table = dataclasses.replace(bs.expand(sc), camera=camera_rays(kind, sc.camera, sc.width, sc.height, int(seed)), projector_type=-1)
        want = port.render_passes(table, [seed], first_spp=i, res=want)
    assert_image(r.read(), want, "fisheye under render_lanes")
    close(r, loader)


def test_light_groups_and_adaptive_are_refused(gpu_instance):
    sc = bs.water_world()
    loader, r = make(gpu_instance, sc)
    for call in (lambda: r.render_lights(SEEDS), lambda: r.render_adaptive(native.java_random_ints(32)),
                 lambda: r.render_list(np.arange(4, dtype=np.int32), SEEDS)):
        with pytest.raises(ChunkyHipError) as e:
            call()
        assert e.value.code == native.E_STATE and "biome" in str(e.value)
    # nothing was allocated: the images these calls make do not exist
    with pytest.raises(ChunkyHipError) as e:
        r.read_light(native.LIGHT_ALL)
    assert e.value.code == native.E_STATE
    with pytest.raises(ChunkyHipError) as e:
        r.adaptive_counts()
    assert e.value.code == native.E_STATE
    assert not bits(r.read()).any()
    r.set_option(native.OPT_BIOME_TINT, 0)   # the way out the message names
    r.render_lights(SEEDS)
    r.render_passes(SEEDS)
    assert bits(r.read_light(native.LIGHT_ALL).reshape(-1)).tobytes() == bits(r.read()).tobytes()
    close(r, loader)


def test_abi_errors_on_a_device(gpu_instance):
    L = native.lib()
    loader = HipSceneLoader(gpu_instance)
    rgb = np.zeros(2 * 3 * 3, np.int32)
    p = native.ptr(rgb)
    for args in ((p, 0, 0, -1, 2), (p, 0, 0, 2, -3), (p, 0, 0, 0, 3), (p, 0, 0, 2, 0), (None, 0, 0, 2, 3), (p, 0, 0, 0, 0),
                 (p, 0, 0, 1 << 14, (1 << 12) + 1), (p, 0, 0, 1 << 30, 1 << 30)):
        assert L.chunky_scene_set_biome_tints(loader._h, *args) == native.E_INVALID, args
        assert b"set_biome_tints" in L.chunky_last_error()
    assert L.chunky_scene_set_biome_tints(loader._h, p, -5, 1 << 30, 2, 3) == 0     # any origin
    assert L.chunky_scene_set_biome_tints(loader._h, None, 0, 0, 0, 0) == 0          # removal, also of nothing
    assert L.chunky_scene_set_biome_tints(loader._h, None, 7, 9, 0, 0) == 0
    r_sc = bs.water_world()
    loader.load_packed(r_sc)
    r = HipPathTracingRenderer(loader, r_sc.width, r_sc.height)
    for bad in (2, -1):
        assert L.chunky_render_set_option(r._h, native.OPT_BIOME_TINT, bad) == native.E_INVALID
    close(r, loader)


def test_isolation(gpu_instance, port, oracle):
    """Beauty with the option off is unchanged by biome launches on the same scene, before and after them; and the map's cells far
    from the origin (a negative origin, the world inside the rectangle) index as the near ones do."""
    sc = bs.water_world()
    plain = port.render_passes(dataclasses.replace(sc, biome=None), SEEDS)
    loader, r = make(gpu_instance, sc, biome_tint=0)
    r.render_passes(SEEDS)
    assert_image(r.read(), plain, "option off, before")
    r_on = HipPathTracingRenderer(loader, sc.width, sc.height)
    r_on.set_camera(sc.projector_type, sc.camera)
    r_on.render_passes(SEEDS)
    r_on.preview()
    r_on.render_aov(SEEDS)
    assert_image(r_on.read(), oracle(sc), "option on")
    r.reset()
    r.render_passes(SEEDS)
    assert_image(r.read(), plain, "option off, after")
    # a rectangle that starts left of and in front of the world
    x0, z0, rgb = sc.biome
    wide = np.zeros((rgb.shape[0] + z0 + 9, rgb.shape[1] + x0 + 5, 3), np.int32)
    wide[:, :] = bs.CONSTANTS
    wide[z0 + 9:, x0 + 5:] = rgb
    shifted = dataclasses.replace(sc, biome=(-5, -9, wide), name="water+biome-negative-origin")
    loader.set_biome_tints(*shifted.biome)
    r_on.reset()
    r_on.render_passes(SEEDS)
    assert_image(r_on.read(), oracle(sc), "a map with a negative origin")   # constants around the same patches: the same image
    close(r, r_on, loader)


def test_the_instantiation_a_1080p_world_gets(gpu_instance, port):
    """An 8-chunk deep golden world (depth 7: render_pool<17, 64> with position tinting) at 1920 x 1080: eight seeded rows of one pass."""
    sc = with_water_map(gs.make("water", gs.DEEP_CHUNKS), gs.DEEP_CHUNKS).with_view(1920, 1080)
    seeds = native.java_random_ints(1, seed=11)
    loader, r = make(gpu_instance, sc)
    r.render_passes(seeds)
    assert kernel(r) == (17, False, native.BIOME_POOL_PARK, True)
    got = r.read().reshape(sc.height, sc.width, 3)
    ex = bs.expand(sc)
    rows = np.random.default_rng(3).choice(sc.height, 8, replace=False)
    differ = 0
    for row in sorted(int(y) for y in rows):
        want = port.render_passes(ex, seeds, gid_range=(row * sc.width, (row + 1) * sc.width)).reshape(sc.height, sc.width, 3)[row]
        assert_image(got[row], want, f"row {row}")
        plain = port.render_passes(dataclasses.replace(sc, biome=None), seeds, gid_range=(row * sc.width, (row + 1) * sc.width)).reshape(sc.height, sc.width, 3)[row]
        differ += int((bits(plain) != bits(want)).sum())
    assert differ > 1000   # the rows see the map
    close(r, loader)
