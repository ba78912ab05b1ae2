"""The emitter light groups (chunky_render_light_set_emitter_groups / _read_group / _mix_groups; csrc/lights_groups.hip) on the device,
bit for bit against the specification on the C restatement of the reference (emitter_groups_spec.expected_groups: group g's image is
the oracle's EMITTERS image of the scene in which every other emitter was darkened): `routes` split three ways plus the rest, the
entity groups of `routes_tris` and of its variant whose actor sheet emits, eight groups, every tree form, a fisheye camera, a shard,
split calls and the launch cut, a two-member group, the four images beside the groups, dropping the groups, palettes that change
after the set call, the device mix, and the ABI's errors.  Every comparison is over every float, NaNs by their bits, without
tolerance."""
import dataclasses

import numpy as np
import pytest

import emitter_groups_spec as es
import route_scenes as rs
from lights_spec import IMAGES, WHICH, expected_lights
from chunkyclplugin_amd import native, scenes
from chunkyclplugin_amd.native import ChunkyHipError, check, ptr
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance, camera_rays
from test_camera_lens_ods_cpu import projected

pytestmark = pytest.mark.gpu
SEEDS = native.java_random_ints(rs.N_PASSES)
WORLD, ACTOR = es.WORLD, es.ACTOR
ENTITY_GROUPS = ({WORLD: 1, ACTOR: 2}, 3)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(instance, sc):
    loader = HipSceneLoader(instance)
    loader.load_packed(sc)
    r = HipPathTracingRenderer(loader, sc.width, sc.height)
    r.set_camera(sc.projector_type, sc.camera)
    return loader, r


def close(*xs):
    for x in xs:
        x.close()


def group_images(r, n):
    out = [r.read_light_group(g).reshape(-1) for g in range(n)]
    assert all(v.dtype == np.float32 for v in out)
    return out


def four_images(r):
    return {k: r.read_light(WHICH[k]).reshape(-1) for k in IMAGES}


def assert_same(got, want, what, keep=None):
    """every float of every group image; `keep`: a mask over pixels"""
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        g, w = bits(a).reshape(-1, 3), bits(b).reshape(-1, 3)
        if keep is not None:
            g, w = g[keep], w[keep]
        same = (g == w).all(axis=1)
        if not same.all():
            i = int(np.argmin(same))
            pytest.fail(f"{what}: group {k} differs at {int((~same).sum())} of {len(same)} pixels (first at row {i}: "
                        f"{g[i].view(np.float32).tolist()!r} against {w[i].view(np.float32).tolist()!r})")


def assert_four_same(got, want, what):
    for k in IMAGES:
        assert bits(got[k]).tobytes() == bits(want[k]).tobytes(), f"{what}: {k}"


@pytest.fixture(scope="module")
def oracle(port):
    """Group images on the oracle, computed once per key and never changed."""
    cache = {}

    def get(key, sc, mapping, n, seeds=SEEDS, **options):
        if key not in cache:
            imgs = es.expected_groups(port, sc, mapping, n, seeds, **options)
            for v in imgs:
                v.setflags(write=False)
            cache[key] = imgs
        return cache[key]
    return get


def render_groups(instance, sc, mapping, n, seeds=SEEDS):
    loader, r = make(instance, sc)
    assert r.set_emitter_groups(mapping, n) == n
    r.render_lights(seeds)
    return loader, r


def test_routes_in_three_groups_and_the_rest(gpu_instance, oracle):
    sc = rs.make("routes")
    mapping, n = es.routes_split()
    want = oracle("routes", sc, mapping, n)
    shares = [es.lit_share(g) for g in want]
    print("lit shares on the oracle", shares)
    assert min(shares[1:]) >= 0.01, shares      # the reference gives 9.7 / 5.8 / 4.0 %
    loader, r = render_groups(gpu_instance, sc, mapping, n)
    assert_same(group_images(r, n), want, "routes")
    info = r.lights_info()
    assert info["groups"] and not info["bvh"] and info["launches"] == 1, info
    assert r.lights_time()[1] == 1
    close(r, loader)


def test_routes_tris_entity_groups(gpu_instance, oracle):
    """The world sheet emits, the actor sheet does not; the emissive blocks under them are the rest."""
    sc = rs.make("routes_tris")
    mapping, n = ENTITY_GROUPS
    want = oracle("routes_tris", sc, mapping, n)
    assert es.lit_share(want[1]) >= 0.01 and want[0].any()     # the reference gives 18.3 %
    assert not bits(want[2]).any()
    loader, r = render_groups(gpu_instance, sc, mapping, n)
    assert r.lights_info()["bvh"] and r.lights_info()["groups"]
    got = group_images(r, n)
    assert_same(got, want, "routes_tris")
    assert not bits(got[2]).any()
    close(r, loader)


def test_actor_sheet_emits(gpu_instance, oracle):
    sc = es.routes_tris_actor_emits()
    mapping, n = ENTITY_GROUPS
    want = oracle("actor_emits", sc, mapping, n)
    assert es.lit_share(want[2]) >= 0.01 and not bits(want[1]).any()
    loader, r = render_groups(gpu_instance, sc, mapping, n)
    assert_same(group_images(r, n), want, "routes_tris with an emissive actor sheet")
    close(r, loader)


def test_eight_groups(gpu_instance, oracle):
    """Seven block pointers and the world entity, each a group of its own: the maximum."""
    sc = rs.make("routes_tris")
    ids = es.all_emitters(sc)
    assert len(ids) == native.LIGHT_MAX_EMITTER_GROUPS and WORLD in ids
    mapping = {i: k for k, i in enumerate(ids)}
    want = oracle("eight", sc, mapping, 8)
    assert all(g.any() for g in want)
    loader, r = render_groups(gpu_instance, sc, mapping, 8)
    assert_same(group_images(r, 8), want, "eight groups")
    close(r, loader)


@pytest.mark.parametrize("depth", sorted(rs.EMBED_DEPTHS))
def test_tree_forms(gpu_instance, oracle, depth):
    """routes_d7, _d11, _d16: the lookup forms 17, 18 and 0."""
    sc = rs.make(f"routes_d{depth}")
    mapping, n = es.routes_split()
    assert sorted(mapping) == scenes.emitter_ids(sc)[0].tolist()
    want = oracle(f"d{depth}", sc, mapping, n)
    assert min(es.lit_share(g) for g in want[1:]) >= 0.01
    loader, r = render_groups(gpu_instance, sc, mapping, n)
    assert r.lights_info()["tree"] == rs.EMBED_DEPTHS[depth]
    assert_same(group_images(r, n), want, f"routes_d{depth}")
    close(r, loader)


def test_fisheye_camera(gpu_instance, port):
    """A pass of a projected camera is the pass on the table of its rays."""
    kind = native.PROJ_FISHEYE
    sc = projected(rs.make("routes"), kind)
    mapping, n = es.routes_split()
    want = None
    for i, seed in enumerate(SEEDS):
        table = dataclasses.replace(sc, camera=camera_rays(kind, sc.camera, sc.width, sc.height, int(seed)), projector_type=-1)
        want = es.expected_groups(port, table, mapping, n, [seed], first_spp=i, init=want)
    assert all(g.any() for g in want[1:])
    loader, r = render_groups(gpu_instance, sc, mapping, n)
    assert_same(group_images(r, n), want, "fisheye")
    close(r, loader)


def test_shard(gpu_instance, port):
    """33 x 17 under set_shard(rank 1 of 3, runs of 5 pixels): the rank's pixels are the whole image's, every other word stays 0."""
    sc = rs.make("routes").with_view(33, 17)
    mapping, n = es.routes_split()
    want = es.expected_groups(port, sc, mapping, n, SEEDS)
    assert any(g.any() for g in want)
    loader, r = make(gpu_instance, sc)
    r.set_shard(1, 3, 5)
    r.set_emitter_groups(mapping, n)
    r.render_lights(SEEDS)
    got = group_images(r, n)
    mine = (np.arange(33 * 17) // 5) % 3 == 1
    assert_same(got, want, "rank 1 of 3, tile 5", keep=mine)
    for g in got:
        assert not bits(g).reshape(-1, 3)[~mine].any()
    assert any(bits(g).reshape(-1, 3)[mine].any() for g in got)
    close(r, loader)


def test_split_calls_equal_one(gpu_instance, oracle):
    """Four passes in one call equal 1 + 3 continued with first_buffer_spp."""
    sc = rs.make("routes")
    mapping, n = es.routes_split()
    loader, r = make(gpu_instance, sc)
    r.set_emitter_groups(mapping, n)
    r.render_lights(SEEDS[:1])
    r.render_lights(SEEDS[1:], first_buffer_spp=1)
    assert_same(group_images(r, n), oracle("routes", sc, mapping, n), "1 + 3 passes")
    close(r, loader)


def test_launch_cut_is_invisible(gpu_instance, port):
    """257 passes on a 7 x 5 view: 256 in the first launch, one in the second."""
    sc = rs.make("routes").with_view(7, 5)
    seeds = native.java_random_ints(257)
    mapping, n = es.routes_split()
    want = es.expected_groups(port, sc, mapping, n, seeds)
    assert any(g.any() for g in want)
    loader, r = render_groups(gpu_instance, sc, mapping, n, seeds)
    assert r.lights_info()["launches"] == 2 and r.lights_time()[1] == 2
    assert_same(group_images(r, n), want, "257 passes")
    close(r, loader)


def test_two_member_group(gpu_instance, oracle):
    g = RendererInstance.group([0, 0])
    sc = rs.make("routes_tris")
    mapping, n = ENTITY_GROUPS
    lg, rg = make(g, sc)
    rg.set_emitter_groups(mapping, n)
    rg.render_lights(SEEDS[:2])
    rg.render_lights(SEEDS[2:], first_buffer_spp=2)
    assert_same(group_images(rg, n), oracle("routes_tris", sc, mapping, n), "a two-member group")
    assert rg.lights_info()["groups"]
    assert rg.mix_light_groups(1, 1, [1, 1, 1]).any()
    rg.reset_lights()
    assert not any(bits(v).any() for v in group_images(rg, n))
    close(rg, lg, g)


def test_the_four_images_are_untouched_and_groups_can_be_dropped(gpu_instance, oracle):
    """With groups set the four images are the ungrouped call's, bit for bit; n_groups = 0 restores today's kernel."""
    sc = rs.make("routes_tris")
    mapping, n = ENTITY_GROUPS
    loader, r = make(gpu_instance, sc)
    r.render_lights(SEEDS)
    assert not r.lights_info()["groups"]
    plain = four_images(r)
    assert plain["emitters"].any() and plain["sky"].any()
    r.set_emitter_groups(mapping, n)
    assert_four_same(four_images(r), plain, "setting groups leaves the four images alone")
    r.reset_lights()
    r.render_lights(SEEDS)
    assert r.lights_info()["groups"]
    assert_four_same(four_images(r), plain, "grouped passes")
    assert_same(group_images(r, n), oracle("routes_tris", sc, mapping, n), "after a reset")
    # reset zeroes the group images too
    r.reset_lights()
    assert not any(bits(v).any() for v in group_images(r, n))
    # setting groups again zeroes the group images only: they lag behind the four
    r.render_lights(SEEDS)
    r.set_emitter_groups(mapping, n)
    assert_four_same(four_images(r), plain, "a second set call")
    with pytest.raises(ChunkyHipError) as e:
        r.read_light_group(0)
    assert e.value.code == native.E_STATE
    r.render_lights([], first_buffer_spp=0)
    assert not any(bits(v).any() for v in group_images(r, n))
    # dropped
    assert r.set_emitter_groups({}) == 0
    with pytest.raises(ChunkyHipError) as e:
        r.read_light_group(0)
    assert e.value.code == native.E_STATE
    r.reset_lights()
    r.render_lights(SEEDS)
    assert not r.lights_info()["groups"]
    assert_four_same(four_images(r), plain, "after the groups were dropped")
    close(r, loader)


def with_glow_copy(sc):
    """(`routes` with a copy of its `glow` cube appended to the block palette and every glow leaf pointing at the copy, the copy's pointer)"""
    B = rs.base()[1]
    blocks = np.asarray(sc.block_palette, np.int32)
    p = len(blocks)
    tree = np.array(sc.octree, np.int32)
    assert (tree == -B["glow"]).any()
    tree[tree == -B["glow"]] = -p
    return dataclasses.replace(sc, octree=tree, block_palette=np.concatenate([blocks, blocks[B["glow"]:B["glow"] + 2]]), name="routes+glow_copy"), p


def upload(loader, sc, grow):
    """the octree and block palette of `sc` into the loaded scene, in the order that keeps every pointer of the tree inside the palette"""
    L = native.lib()
    tree, blocks = np.ascontiguousarray(sc.octree, np.int32), np.ascontiguousarray(sc.block_palette, np.int32)
    steps = [lambda: check(L.chunky_scene_set_palette(loader._h, native.PALETTE_BLOCK, ptr(blocks), blocks.size)),
             lambda: check(L.chunky_scene_set_octree(loader._h, ptr(tree), tree.size, int(sc.octree_depth)))]
    for step in (steps if grow else steps[::-1]):
        step()


def test_palette_shortened_after_the_set_call(gpu_instance, port):
    """Groups set against a longer palette, the palette then cut back: the table outlives the blocks it names."""
    short = rs.make("routes")
    long_, p = with_glow_copy(short)
    B = rs.base()[1]
    loader, r = make(gpu_instance, long_)
    r.set_emitter_groups({p: 2, B["emit6a"]: 1}, 3)
    upload(loader, short, grow=False)
    r.render_lights(SEEDS)
    want = es.expected_groups(port, short, {B["emit6a"]: 1}, 3, SEEDS)
    assert want[0].any() and want[1].any() and not bits(want[2]).any()
    assert_same(group_images(r, 3), want, "palette shortened")
    close(r, loader)


def test_palette_grown_after_the_set_call(gpu_instance, port):
    """A pointer beyond the stored table is group 0: the glow cubes move to a block the table has never seen."""
    short = rs.make("routes")
    long_, p = with_glow_copy(short)
    B = rs.base()[1]
    mapping = {B["glow"]: 2, B["emit6a"]: 1}
    loader, r = make(gpu_instance, short)
    with pytest.raises(ChunkyHipError) as e:
        r.set_emitter_groups({p: 1}, 2)                    # beyond the palette as it is now
    assert e.value.code == native.E_INVALID
    r.set_emitter_groups(mapping, 3)
    upload(loader, long_, grow=True)
    r.render_lights(SEEDS)
    want = es.expected_groups(port, long_, mapping, 3, SEEDS)     # nothing is left at B["glow"]; p is not in the mapping: the rest
    assert want[0].any() and want[1].any() and not bits(want[2]).any()
    moved = es.expected_groups(port, short, mapping, 3, SEEDS)
    assert moved[2].any() and bits(moved[2]).tobytes() != bits(want[2]).tobytes()
    assert_same(group_images(r, 3), want, "palette grown")
    close(r, loader)


@pytest.mark.parametrize("weights", [(1, 1, (1, 1, 1, 1)), (0.5, 2, (0, 3, 0.25, 1.5)), (0, 0, (0, 0, 0, 7))], ids=["sum", "regrade", "one-group"])
def test_mix_groups(gpu_instance, weights):
    """((w_sky * SKY + w_sun * SUN) + w[0] * G0) + w[1] * G1 ... per float in float32, each operation rounded once."""
    sc = rs.make("routes")
    mapping, n = es.routes_split()
    loader, r = render_groups(gpu_instance, sc, mapping, n)
    four, groups = four_images(r), group_images(r, n)
    want = es.mix(four["sky"], four["sun"], groups, *weights)
    assert want.any()
    got = r.mix_light_groups(*weights)
    assert got.shape == (rs.H, rs.W, 3) and got.dtype == np.float32
    assert bits(got.reshape(-1)).tobytes() == bits(want).tobytes()
    assert_same(group_images(r, n), groups, "the mix changes no group image")
    assert_four_same(four_images(r), four, "the mix changes no image")
    close(r, loader)


def test_errors_on_a_device(gpu_instance):
    L = native.lib()
    sc = rs.make("routes")
    loader, r = make(gpu_instance, sc)
    n = 3 * sc.width * sc.height
    out = np.zeros(n, np.float32)
    w = np.ones(8, np.float32)
    n_blocks = len(np.asarray(sc.block_palette))

    def set_groups(n_groups, ids, groups):
        i, g = np.array(ids, np.int32), np.array(groups, np.uint8)
        return L.chunky_render_light_set_emitter_groups(r._h, n_groups, i.ctypes.data if len(i) else None, g.ctypes.data if len(g) else None, len(i))

    read = lambda g, count=n, buf=out: L.chunky_render_light_read_group(r._h, g, None if buf is None else buf.ctypes.data, count)
    mix = lambda n_groups, ws=w, wk=1.0, wu=1.0, count=n, buf=out: L.chunky_render_light_mix_groups(
        r._h, wk, wu, None if ws is None else ws.ctypes.data, n_groups, None if buf is None else buf.ctypes.data, count)
    # nothing set
    assert read(0) == native.E_STATE and mix(1) == native.E_STATE
    assert set_groups(0, [], []) == 0                                     # dropping nothing
    # the validator's refusals reach the caller, and change nothing
    assert set_groups(2, [8], [1]) == 0
    for bad in ((-1, [], []), (9, [], []), (0, [8], [0]), (2, [9], [1]), (2, [n_blocks], [1]), (2, [-1], [1]), (2, [-4], [1]),
                (3, [8, 10, 8], [1, 2, 1]), (3, [WORLD, WORLD], [1, 2]), (2, [8], [2])):
        assert set_groups(*bad) == native.E_INVALID, bad
    assert L.chunky_render_light_set_emitter_groups(r._h, 2, None, None, 1) == native.E_INVALID
    assert L.chunky_render_light_set_emitter_groups(r._h, 2, None, None, -1) == native.E_INVALID
    # set, not rendered yet
    assert read(0) == native.E_STATE and mix(2) == native.E_STATE
    # a non-finite emitter scale is refused while groups are set, and only then
    for scale in (np.inf, -np.inf, np.nan):
        r.set_option(native.OPT_EMITTER_SCALE, scale)
        assert L.chunky_render_light_passes(r._h, SEEDS.ctypes.data, 1, 0) == native.E_STATE
        assert b"EMITTER_SCALE" in L.chunky_last_error()
    assert read(0) == native.E_STATE
    r.set_option(native.OPT_EMITTER_SCALE, 13.0)
    # the refusals of the ungrouped pass stay
    r.set_option(native.OPT_BSDF, 1)
    assert L.chunky_render_light_passes(r._h, SEEDS.ctypes.data, 1, 0) == native.E_STATE
    r.set_option(native.OPT_BSDF, 0)
    r.render_lights(SEEDS[:1])
    assert read(0) == 0 and read(1) == 0 and out.any()
    for g in (-1, 2, 8):
        assert read(g) == native.E_INVALID
    assert read(0, n - 1) == native.E_INVALID and read(0, n // 3) == native.E_INVALID and read(0, buf=None) == native.E_INVALID
    assert mix(2) == 0
    for bad_n in (-1, 0, 1, 3, 9):
        assert mix(bad_n) == native.E_INVALID, bad_n
    assert mix(2, ws=None) == native.E_INVALID and mix(2, buf=None) == native.E_INVALID and mix(2, count=n - 3) == native.E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        assert mix(2, wk=bad) == native.E_INVALID and mix(2, wu=bad) == native.E_INVALID
        for i in range(2):
            wb = np.ones(8, np.float32)
            wb[i] = bad
            assert mix(2, ws=wb) == native.E_INVALID
        wb = np.ones(8, np.float32)
        wb[2] = bad
        assert mix(2, ws=wb) == 0                                         # (only the target's two weights are read)
    # a refused set call left the groups as they were
    held = group_images(r, 2)
    assert set_groups(2, [9], [1]) == native.E_INVALID
    assert_same(group_images(r, 2), held, "after a refused set call")
    # an infinite scale without groups is the ungrouped pass's own business
    assert set_groups(0, [], []) == 0
    r.set_option(native.OPT_EMITTER_SCALE, np.inf)
    assert L.chunky_render_light_passes(r._h, SEEDS.ctypes.data, 1, 1) == 0
    r.sync()
    close(r, loader)
