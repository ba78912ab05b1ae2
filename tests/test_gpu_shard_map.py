"""The shard-to-pixel map on the device: the functions every image-writing kernel takes its pixels from (shard_gid, pool_slot_gid,
pool_slot_pixel, fast_quotient: chunky_selftest_shard_map) against the numpy restatement of tests/test_shard_map_cpu.py, and the kernels
that go through them — render_pool and fold_kernel, render_waves, render_lanes, the AOV kernel, gather_kernel<true / false>,
clear_foreign_kernel — at tiles,
worlds and image sizes no other file reaches: tiles that are no multiple of the 4-slot sub-block, tiles at and above the pixel count,
more ranks than tiles, images smaller than one 16 x 16 block.  Everything is compared bit for bit; a rank's image must be the
oracle's on the brute-force owned set and exactly zero elsewhere, which holds for black pixels too.

Thinning (tests/SHARD_MAP.md has the branch table).  Map layer: MAP_VIEWS x worlds 1, 2, 3, 5, 9 x the 19 tiles of the sanitizer
grid, every rank.  Kernel layer: every (view, tile) of KERNEL_VIEWS x kernel_tiles once; its world rotates through 2, 3, 5 and
"units + 1" (one more rank than there are runs or blocks; taken only where that is at most 9, so that summing over ranks stays
cheap) by (view index + tile index) % 4, its rank through first, last and middle by (view index + 2 x tile index) % 3.  Each cell
renders every rank on render_pool (each rank's image exact, and their sum the one-rank image) and the cell's own rank on
render_waves, render_lanes and the AOV kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the library loads: torch brings a HIP runtime of its own, and the second runtime of a process finds no device

import golden_scenes as gs
from aov_spec import expected_aov
from chunkyclplugin_amd import native
from chunkyclplugin_amd.renderer import HipPathTracingRenderer, HipSceneLoader, RendererInstance
from oracle import binding
from test_shard_map_cpu import clamped, grid_tiles, n_local, owner_table, slot_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INT_MAX = 2 ** 31 - 1
SEEDS = native.java_random_ints(257)
MARKER = 7.25
KERNEL_VIEWS = [(1, 1), (7, 1), (1, 7), (15, 17), (16, 16), (17, 33), (33, 17), (100, 60)]
MAP_VIEWS = KERNEL_VIEWS[:7] + [(2, 2), (16, 1), (17, 1), (1, 17), (31, 33), (32, 32), (40, 36)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- map layer
def check_rows(gpu_instance, w, h, rank, world, tile, n_slots):
    rows, view = gpu_instance.selftest_shard_map(w, h, rank, world, tile, n_slots)
    assert view == (rank, world, clamped(w * h, tile), n_local(w, h, rank, world, tile)), (w, h, rank, world, tile, view)
    want = slot_table(w, h, rank, world, tile, n_slots)
    if not np.array_equal(rows, want):
        bad = np.flatnonzero((rows != want).any(axis=1))
        pytest.fail(f"{w}x{h} rank {rank}/{world} tile {tile}: {bad.size} of {n_slots} slots differ (first: slot {int(bad[0])}: "
                    f"{rows[bad[0]].tolist()} against {want[bad[0]].tolist()})")
    return rows


@pytest.mark.parametrize("w,h", MAP_VIEWS, ids=[f"{w}x{h}" for w, h in MAP_VIEWS])
def test_map_grid(gpu_instance, w, h):
    """Slots 0 .. n_local + 299 (the padding of the last tile and a whole tile beyond it are part of the domain) of every rank."""
    n = w * h
    for world in (1, 2, 3, 5, 9):
        for tile in grid_tiles(n):
            seen, own_of = np.zeros(n, np.int64), owner_table(w, h, world, tile)
            for rank in range(world):
                nl = n_local(w, h, rank, world, tile)
                slots = (nl if world != 1 else ((w + 15) // 16) * ((h + 15) // 16) * 256) + 300
                rows = check_rows(gpu_instance, w, h, rank, world, tile, slots)
                gid, pgid, x, y = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
                valid = gid < n
                assert (gid >= 0).all() and np.array_equal(gid, pgid)
                assert np.array_equal(y[valid] * w + x[valid], gid[valid])  # column and row agree with the index wherever it is one
                assert (gid[nl:] == n).all() if world != 1 else True        # padding slots give exactly width * height
                np.add.at(seen, gid[valid], 1)
                assert (own_of[gid[valid]] == rank).all()
            assert (seen == 1).all(), (w, h, world, tile)                  # every pixel in exactly one slot of exactly one rank


@pytest.mark.parametrize("w,h", [(7, 1), (17, 33), (100, 60)])
def test_map_clamped_extremes(gpu_instance, w, h):
    n = w * h
    for tile in (1 << 20, 1 << 30, INT_MAX - 1, INT_MAX, n, n + 1):
        for world in (2, 1 << 20, 1 << 30, INT_MAX):
            for rank in (0, 1, world - 1):
                rows = check_rows(gpu_instance, w, h, rank, world, tile, n + 300)
                assert np.array_equal(rows[:, 0], np.arange(n + 300).clip(max=n) if rank == 0 else np.full(n + 300, n))
    for world in (1 << 20, 1 << 30, INT_MAX):  # 16 x 16 blocks over more ranks than an int product of slots allows beyond the first tile
        for rank in (0, 1, world - 1):
            check_rows(gpu_instance, w, h, rank, world, 0, 256)
    L = native.lib()
    out = np.zeros(5 * 600, np.int32)
    assert L.chunky_selftest_shard_map(gpu_instance._h, 0, w, h, 1, INT_MAX, 0, 600, None, out.ctypes.data, None) == native.E_INVALID  # 2 x INT_MAX + 1
    assert L.chunky_selftest_shard_map(gpu_instance._h, 0, w, h, 2, 2, 3, 10, None, out.ctypes.data, None) == native.E_INVALID        # rank = world
    assert L.chunky_selftest_shard_map(gpu_instance._h, 0, w, h, 0, 2, -1, 10, None, out.ctypes.data, None) == native.E_INVALID
    assert L.chunky_selftest_shard_map(gpu_instance._h, 2, w, h, 0, 2, 3, 10, None, out.ctypes.data, None) == native.E_INVALID


def test_fast_quotient(gpu_instance):
    """Every divisor 1 .. 4100 and 2^k, 2^k +- 1 for k <= 26; numerators 0, 1, d - 1, d, d + 1, 2^31 - 1 and 64 seeded ones."""
    ds = np.array(sorted(set(range(1, 4101)) | {(1 << k) + e for k in range(27) for e in (-1, 0, 1) if (1 << k) + e >= 1}), np.int64)
    rng = np.random.default_rng(11)
    nums = np.concatenate([np.stack([np.zeros_like(ds), np.ones_like(ds), ds - 1, ds, ds + 1, np.full_like(ds, INT_MAX)], axis=1),
                           rng.integers(0, 1 << 31, (len(ds), 64))], axis=1)
    d = np.repeat(ds, nums.shape[1])
    n = nums.reshape(-1)
    got = gpu_instance.selftest_fast_quotient(n, d)
    assert len(got) > 4100 * 70 and np.array_equal(got.astype(np.int64), n // d)


# ---------------------------------------------------------------------------------------------------------------- kernel layer
def kernel_tiles(n):
    return list(dict.fromkeys([0, 1, 3, 5, 64, 255, 257, n - 1, n, n + 1, 1 << 30]))  # (1 x 1: n - 1 is tile 0 again)


def units(w, h, tile):
    return ((w + 15) // 16) * ((h + 15) // 16) if tile == 0 else -(-(w * h) // clamped(w * h, tile))


def kernel_cells():
    cells = []
    for vi, (w, h) in enumerate(KERNEL_VIEWS):
        for ti, tile in enumerate(kernel_tiles(w * h)):
            world = (2, 3, 5, units(w, h, tile) + 1)[(vi + ti) % 4]
            if world > 9:
                world = (2, 3, 5)[(vi + ti) % 3]
            rank = (0, world - 1, world // 2)[(vi + 2 * ti) % 3]
            cells.append((w, h, tile, world, rank))
    return cells


CELLS = kernel_cells()
assert any(world > units(w, h, tile) for w, h, tile, world, _ in CELLS) and {c[3] for c in CELLS} >= {2, 3, 5}


class Views:
    """One scene upload, one render target per view, and the oracle's whole image per view: all made once."""

    def __init__(self, instance, port, name):
        self.instance, self.port, self.base = instance, port, gs.make(name)
        self.loader = HipSceneLoader(instance)
        self.loader.load_packed(self.base)
        self.targets, self.refs, self.aovs = {}, {}, {}

    def scene(self, w, h):
        return self.base.with_view(w, h)

    def target(self, w, h):
        if (w, h) not in self.targets:
            sc = self.scene(w, h)
            r = HipPathTracingRenderer(self.loader, w, h)
            r.set_camera(sc.projector_type, sc.camera)
            self.targets[w, h] = r
        return self.targets[w, h]

    def ref(self, w, h, passes=2):
        """port.render_gids over every pixel: a rank's expected image is this on its owned set (pixels are independent) and 0 elsewhere."""
        if (w, h, passes) not in self.refs:
            img = self.port.render_gids(self.scene(w, h), SEEDS[:passes], np.arange(w * h, dtype=np.int32), threads=binding.usable_threads())
            img.setflags(write=False)
            self.refs[w, h, passes] = img.reshape(-1, 3)
        return self.refs[w, h, passes]

    def aov(self, w, h):
        if (w, h) not in self.aovs:
            self.aovs[w, h] = expected_aov(self.port, binding.SceneHandle(self.scene(w, h)), SEEDS[:2], np.arange(w * h))
        return self.aovs[w, h]

    def close(self):
        for r in self.targets.values():
            r.close()
        self.loader.close()


@pytest.fixture(scope="module")
def outdoor(gpu_instance, port):
    v = Views(gpu_instance, port, "outdoor")
    yield v
    v.close()


def masked(ref, own):
    want = np.zeros_like(ref)
    want[own] = ref[own]
    return want


def assert_image(got, ref, own, what):
    """Equal to the oracle inside the owned set, exactly zero (the bits of +0.0) outside."""
    got, want = bits(got).reshape(-1, 3), bits(masked(ref, own))
    same = (got == want).all(axis=1)
    if not same.all():
        k = int(np.argmin(same))
        inside = np.zeros(len(same), bool)
        inside[own] = True
        pytest.fail(f"{what}: {int((~same).sum())} pixels differ ({int((~same & inside).sum())} owned, {int((~same & ~inside).sum())} foreign; first: pixel {k}, "
                    f"{'owned' if inside[k] else 'foreign'}: {got[k].view(np.float32).tolist()} against {want[k].view(np.float32).tolist()})")


def render(r, variant, shard, seeds):
    r.set_option(native.OPT_KERNEL, variant)
    r.set_shard(*shard)
    r.reset()
    r.render_passes(seeds)
    return r.read()


@pytest.mark.parametrize("w,h,tile,world,rank", CELLS, ids=[f"{w}x{h}-tile{t}-world{wd}-rank{rk}" for w, h, t, wd, rk in CELLS])
def test_kernels(outdoor, w, h, tile, world, rank):
    r, ref, own_of = outdoor.target(w, h), outdoor.ref(w, h), owner_table(w, h, world, tile)
    try:
        total = np.zeros(3 * w * h, np.float32)
        for k in range(world):  # render_pool and fold_kernel: every rank, and what the read-back reduce would make of them
            own = np.flatnonzero(own_of == k)
            part = render(r, 0, (k, world, tile), SEEDS[:2])
            if own.size:
                assert r.kernel_info()["pool"] >= 0, r.kernel_info()
            assert_image(part, ref, own, f"render_pool rank {k}")
            total += part
        assert np.array_equal(bits(total), bits(render(r, 0, (0, 1, 256), SEEDS[:2]))) and np.array_equal(bits(total).reshape(-1, 3), bits(ref))
        own = np.flatnonzero(own_of == rank)
        for variant, name in ((8, "render_waves"), (2, "render_lanes")):
            part = render(r, variant, (rank, world, tile), SEEDS[:2])
            if own.size:
                info = r.kernel_info()
                assert info["pool"] < 0 and (info["group"] == 0) == (variant == 2), info
            assert_image(part, ref, own, name)
        r.set_option(native.OPT_KERNEL, 0)
        r.reset_aov()
        r.render_aov(SEEDS[:2])
        for got, want, kind in zip((r.read_aov(native.AOV_ALBEDO), r.read_aov(native.AOV_NORMAL)), outdoor.aov(w, h), ("albedo", "normal")):
            assert_image(got, want, own, f"AOV {kind}")
    finally:
        r.set_option(native.OPT_KERNEL, 0)
        r.set_shard(0, 1, 256)


def test_entity_cell(gpu_instance, port):
    """Entity BVHs under a share of 16 x 16 blocks: render_pool's BVH instantiation maps the blocks itself, the fallback kernels take the
    same pixels as a list (block_pixel_list); and under an odd run length."""
    v = Views(gpu_instance, port, "entities")
    w, h = 17, 33
    r, ref = v.target(w, h), v.ref(w, h)
    try:
        for world, tile, rank in ((3, 0, 1), (2, 5, 1)):
            own = np.flatnonzero(owner_table(w, h, world, tile) == rank)
            assert own.size
            assert_image(render(r, 0, (rank, world, tile), SEEDS[:2]), ref, own, "render_pool with entities")
            info = r.kernel_info()
            assert info["pool"] >= 0 and info["bvh"], info
            for variant in (8, 2):
                assert_image(render(r, variant, (rank, world, tile), SEEDS[:2]), ref, own, f"variant {variant} with entities")
                assert r.kernel_info()["pool"] < 0 and r.kernel_info()["bvh"]
    finally:
        v.close()


def test_long_launch_under_a_shard(outdoor):
    """257 passes over a share of 5 pixels (7 x 1, runs of 5, rank 0) are one launch whose seeds travel in device memory."""
    w, h, passes = 7, 1, 257
    r = outdoor.target(w, h)
    own = np.flatnonzero(owner_table(w, h, 2, 5) == 0)
    assert own.tolist() == [0, 1, 2, 3, 4]
    try:
        r.kernel_time()
        got = render(r, 0, (0, 2, 5), SEEDS[:passes])
        info = r.kernel_info()
        assert info["pool"] >= 0 and info["passes_per_launch"] == 1024 and r.kernel_time()[1] == 1, info
        assert_image(got, outdoor.ref(w, h, passes), own, "257 passes")
    finally:
        r.set_shard(0, 1, 256)


# ---------------------------------------------------------------------------------------------------------------- exchange kernels
RAGGED = [(7, 1), (1, 7), (15, 17), (17, 33), (33, 17)]


def outer_shards(n):
    return [(0, 1, 0), (0, 1, 3), (1, 2, 0), (0, 2, 3), (2, 3, 257), (1, 2, n + 1)]


@pytest.fixture(scope="module", params=[3, 2], ids=["three-members", "two-members"])
def group(request, port):
    g = RendererInstance.group([0] * request.param)
    v = Views(g, port, "outdoor")
    yield v
    v.close()
    g.close()


@pytest.mark.parametrize("w,h", RAGGED, ids=[f"{w}x{h}" for w, h in RAGGED])
def test_group_gather(group, w, h):
    """Members on one device, alone and inside an outer share: gather_kernel<true> packs every member's slots, gather_kernel<false>
    scatters them into member 0's image — here a caller's buffer full of a marker.  The group's pixels are the oracle's; under
    the gather every pixel outside the group's share is untouched."""
    n = w * h
    r, ref = group.target(w, h), group.ref(w, h)
    members = group.instance.group_size()
    for rank, world, tile in outer_shards(n):
        fb = torch.full((3 * n,), MARKER, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        r.set_device_buffer(fb.data_ptr())
        try:
            r.set_shard(rank, world, tile)
            r.render_passes(SEEDS[:2])
            got = r.read().reshape(-1, 3)
        finally:
            r.set_device_buffer(None)
        own_of = owner_table(w, h, world, tile)
        own = own_of == rank
        what = f"{members} members as rank {rank}/{world} tile {tile}"
        assert np.array_equal(bits(got[own]), bits(ref[own])), what
        assert (bits(got[~own]) == bits(np.float32(MARKER))).all(), what + ": a pixel of another rank was written"
        # ... and the members' shares are the outer share dealt again: member i is rank + world * i of world * members
        inner = owner_table(w, h, world * members, tile)
        assert np.array_equal(np.isin(inner, [rank + world * i for i in range(members)]), own)
    r.set_shard(0, 1, 0)


def reduce_child(tmp_path, devices, cells, **env):
    """tests/shard_reduce_child.py in a process of its own, on the build that reads the rig variables: (what it says of its transport, its images)."""
    e = dict(os.environ)
    for k in ("CHUNKY_RCCL_LIB", "CHUNKY_GROUP_TRANSPORT", "CHUNKY_GROUP_SELF_EXCHANGE", "CHUNKY_RCCL_TRY_SHARED", "RCCL_STUB_MODE",
              "CHUNKY_GROUP_NO_PROBE", "CHUNKY_GROUP_TIMEOUT_MS"):
        e.pop(k, None)
    e["CHUNKY_HIP_LIB"] = native.build_tuning()
    e.update({k: str(v) for k, v in env.items()}, CHUNKY_GROUP_TRANSPORT="rccl-reduce")
    out = str(tmp_path / "images.npz")
    cmd = [sys.executable, os.path.join(HERE, "shard_reduce_child.py"), devices, json.dumps(cells), repr(MARKER), out]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e)
    assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-3000:])
    images = np.load(out)
    return json.loads(str(images["info"])), images


REDUCE_CELLS = [(w, h) + shard for w, h in RAGGED for shard in outer_shards(w * h)]


@pytest.mark.parametrize("members", [3, 1], ids=["stand-in-rccl-three-members", "real-rccl-one-member"])
def test_group_reduce_clears_foreign_pixels(outdoor, tmp_path, members):
    """The reduce transport: every member runs clear_foreign_kernel on its own share, then one ncclReduce sums the images onto member 0.
    Three members on one device get a communicator only from the stand-in RCCL (tests/rccl_stub/), which reports success and moves
    nothing: member 0's image is then exactly what its clear left, its own share of the outer share (rank of world x 3) and zero
    everywhere else.  Only member 0's result is asserted there: members 1 and 2 run the kernel too, but nothing reads their images
    back (their ranks are member 0's of other cells).  One member on the real RCCL is the whole exchange: a true ncclReduce, after which the image is the outer share's
    pixels and zero elsewhere.  Either way every pixel outside started as the marker, so a zero there is the kernel's store, and a
    marker left, or an owned pixel cleared, is a wrong owner (gid / tile, the block index, unit % world) at odd tiles, a tile above
    the pixel count and images one pixel wide."""
    if members == 3:
        stub = str(tmp_path / "librccl_stub.so")
        subprocess.run(["gcc", "-shared", "-fPIC", "-O1", os.path.join(HERE, "rccl_stub", "rccl_stub.c"), "-o", stub], check=True)
        info, images = reduce_child(tmp_path, "0,0,0", REDUCE_CELLS, CHUNKY_RCCL_LIB=stub, CHUNKY_RCCL_TRY_SHARED=1, CHUNKY_GROUP_NO_PROBE=1, RCCL_STUB_MODE="ok")
    else:
        info, images = reduce_child(tmp_path, "0", REDUCE_CELLS)
    assert info["members"] == members and info["before"]["name"] == "rccl-reduce" and f"{members} rank(s)" in info["before"]["detail"], info
    assert info["during"] == ["rccl-reduce"] * len(REDUCE_CELLS) and info["after"]["name"] == "rccl-reduce", info  # no read-back fell back to peer copies
    cleared = 0
    for w, h, rank, world, tile in REDUCE_CELLS:
        own = np.flatnonzero(owner_table(w, h, world * members, tile) == rank)  # member 0 of the group: rank of world x members
        assert_image(images[f"{w}x{h}:{rank},{world},{tile}"], outdoor.ref(w, h), own, f"{members} member(s) as rank {rank}/{world} tile {tile} on {w}x{h}")
        cleared += w * h - own.size
    assert cleared > 1000  # (pixels that held the marker and must read as zero)


def test_group_refuses_a_world_beyond_int(group):
    """world x members beyond INT_MAX: E_INVALID, and the group still renders its old share."""
    w, h = 7, 1
    r = group.target(w, h)
    members = group.instance.group_size()
    r.set_shard(0, 1, 3)
    with pytest.raises(native.ChunkyHipError) as e:
        r.set_shard(1, INT_MAX // members + 1, 3)
    assert e.value.code == native.E_INVALID and "does not fit an int" in str(e.value)
    r.set_shard(INT_MAX // members - 1, INT_MAX // members, 3)  # the largest world a group of this size takes: its members own nothing here
    r.reset()
    r.render_passes(SEEDS[:2])
    assert not r.read().any()
    r.set_shard(0, 1, 3)
    r.reset()
    r.render_passes(SEEDS[:2])
    assert np.array_equal(bits(r.read()).reshape(-1, 3), bits(group.ref(w, h)))
    r.set_shard(0, 1, 0)


# ---------------------------------------------------------------------------------------------------------------- refusals and no-ops
def test_adaptive_still_refuses_a_shard_at_an_odd_tile(outdoor):
    r = outdoor.target(15, 17)
    try:
        r.set_shard(0, 2, 3)
        with pytest.raises(native.ChunkyHipError) as e:
            r.render_adaptive(SEEDS[:32])
        assert e.value.code == native.E_STATE
    finally:
        r.set_shard(0, 1, 256)


@pytest.mark.parametrize("shard", [(5, 8, 3), (1, 2, 1 << 30), (INT_MAX - 1, INT_MAX, INT_MAX), (2, 3, 0), (INT_MAX - 1, INT_MAX, 0)],
                         ids=["more-ranks-than-runs", "tile-above-the-image", "int-max", "more-ranks-than-blocks", "int-max-blocks"])
def test_a_rank_that_owns_nothing(outdoor, shard):
    """Render, AOV, read and gather return OK having done nothing, on every kernel; the images stay zero; the denoiser's state check
    still names the share."""
    w, h = 7, 1
    r = outdoor.target(w, h)
    assert not (owner_table(w, h, shard[1], shard[2]) == shard[0]).any() if shard[1] < 100 else True
    try:
        for variant in (0, 8, 2):
            assert not render(r, variant, shard, SEEDS[:2]).any()
        r.gather()
        r.reset_aov()
        r.render_aov(SEEDS[:2])
        assert not r.read_aov(native.AOV_ALBEDO).any() and not r.read_aov(native.AOV_NORMAL).any()
        with pytest.raises(native.ChunkyHipError) as e:
            r.denoise()
        assert e.value.code == native.E_STATE and f"rank {shard[0]} of {shard[1]}" in str(e.value)
    finally:
        r.set_option(native.OPT_KERNEL, 0)
        r.set_shard(0, 1, 256)


def test_the_whole_image_at_the_largest_tile(outdoor):
    """Rank 0 at tiles far above the pixel count, among 2 ranks and among INT_MAX: it owns every pixel.  (Slot counts taken in int
    overflow here, and a rank whose count comes out as 0 renders nothing and returns OK: tests/SHARD_MAP.md.)"""
    for w, h in ((7, 1), (100, 60)):
        r = outdoor.target(w, h)
        try:
            for shard in ((0, 2, INT_MAX), (0, INT_MAX, INT_MAX), (0, 2, 1 << 30)):
                got = render(r, 0, shard, SEEDS[:2])
                assert np.array_equal(bits(got).reshape(-1, 3), bits(outdoor.ref(w, h))), shard
        finally:
            r.set_shard(0, 1, 256)
