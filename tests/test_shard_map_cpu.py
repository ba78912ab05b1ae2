"""The shard-to-pixel map, restated in numpy from the prose rule, and the host side of it held to that restatement: `parallel.local_slots`
and `parallel.owned_gids` (no device).  tests/test_gpu_shard_map.py compares the device functions and the kernels with the same
restatement; tests/sanitize/shard_map_fuzz.cpp holds csrc/shard_map.hpp to a brute-force table of its own.

The rule.  A rank owns units of the image dealt round-robin: unit u belongs to rank u % world.  With tile > 0 a unit is a run of `tile`
consecutive pixel indices (a tile at or above the pixel count is the pixel count); with tile 0 it is a 16 x 16 block of pixels,
blocks numbered row-major.  A rank's pixel slots are its units in order: `tile` slots per run (the image's last run is padded), 256
per block.  One rank owns everything, in blocks.  Inside a block the 256 slots are 64 sub-blocks of 2 x 2 pixels, row-major over the
block's 8 x 8 sub-blocks, and row-major inside a sub-block; a slot whose pixel lies outside the image is padding."""
import numpy as np
import pytest

from chunkyclplugin_amd import parallel


def clamped(n_pixels, tile):
    return min(tile, n_pixels)


def n_local(width, height, rank, world, tile):
    n = width * height
    if world == 1:
        return n
    if tile == 0:
        units, per = ((width + 15) // 16) * ((height + 15) // 16), 256
    else:
        per = clamped(n, tile)
        units = -(-n // per)
    return len(range(rank, units, world)) * per


def owner_table(width, height, world, tile):
    """The rank that owns each pixel: brute force, one pixel at a time."""
    n = width * height
    own = np.zeros(n, np.int64)
    for gid in range(n):
        if tile == 0:
            x, y = gid % width, gid // width
            unit = (y // 16) * ((width + 15) // 16) + x // 16
        else:
            unit = gid // clamped(n, tile)
        own[gid] = unit % world
    return own


def owned(width, height, rank, world, tile):
    return np.flatnonzero(owner_table(width, height, world, tile) == rank)


def slot_table(width, height, rank, world, tile, n_slots):
    """What the device gives for slots 0 .. n_slots - 1 of the view set_shard stores: columns pool_slot_gid, then gid / x / y of
    pool_slot_pixel, then shard_gid (-1 where the kernels do not evaluate it).  Padding slots: gid = width * height; a run shard's
    slots below n_local in the padded last run give the run formula's index, at or beyond the pixel count."""
    n = width * height
    nl = n_local(width, height, rank, world, tile)
    s = np.arange(n_slots, dtype=np.int64)
    out = np.zeros((n_slots, 5), np.int64)
    if world != 1 and tile != 0:
        t = clamped(n, tile)
        gid = np.where(s < nl, ((s // t) * world + rank) * t + s % t, n)
        out[:, 0] = out[:, 1] = gid
        out[:, 2], out[:, 3] = gid % width, gid // width
        out[:, 4] = np.where(s < nl, gid, -1)
        return out
    bw, bh = (width + 15) // 16, (height + 15) // 16
    b, i = s // 256, s % 256
    if world != 1:
        b = b * world + rank
    sb, px = i // 4, i % 4
    x = (b % bw) * 16 + (sb % 8) * 2 + px % 2
    y = (b // bw) * 16 + (sb // 8) * 2 + px // 2
    gid = np.where((x < width) & (y < height), y * width + x, n)
    if world != 1:  # a block beyond the image: padding, and the pool kernel's column and row are 0
        beyond = b >= bw * bh
        gid, x, y = np.where(beyond, n, gid), np.where(beyond, 0, x), np.where(beyond, 0, y)
    out[:, 0] = out[:, 1] = gid
    out[:, 2], out[:, 3] = x, y
    out[:, 4] = np.where(s < nl, s, -1) if world == 1 else -1
    return out


def slot_pixels(width, height, rank, world, tile):
    """The rank's pixels in slot order, padding left out (one rank: the slots of all the image's blocks, more than it has pixels)."""
    n_slots = n_local(width, height, rank, world, tile) if world != 1 else ((width + 15) // 16) * ((height + 15) // 16) * 256
    g = slot_table(width, height, rank, world, tile, n_slots)[:, 0]
    return g[g < width * height]


def grid_tiles(n):
    return sorted({0, 1, 2, 3, 4, 5, 7, 15, 16, 17, 63, 64, 100, 255, 256, 257, n - 1, n, n + 1})


VIEWS = [(1, 1), (7, 1), (1, 7), (15, 17), (16, 16), (17, 33), (33, 17), (40, 36), (100, 60)]


@pytest.mark.parametrize("width,height", VIEWS)
def test_the_restatement_partitions_the_image(width, height):
    """The slot table against the brute-force owner table: the two halves of the restatement check each other."""
    n = width * height
    for world in (1, 2, 3, 5, 9):
        for tile in grid_tiles(n) + [1 << 30]:
            own = owner_table(width, height, world, tile)
            for rank in range(world):
                got = slot_pixels(width, height, rank, world, tile)
                assert np.array_equal(np.sort(got), np.flatnonzero(own == rank)), (world, tile, rank)
            if tile >= n and world > 1:
                assert [n_local(width, height, r, world, tile) for r in range(world)] == [n] + [0] * (world - 1)


@pytest.mark.parametrize("width,height", VIEWS)
def test_parallel_follows_the_rule(width, height):
    """parallel.local_slots is n_local; parallel.owned_gids is the rank's pixels in slot order (one rank: every pixel, in index order —
    the order there is each kernel's own: blocks under render_pool, indices under the others)."""
    n = width * height
    for world in (1, 2, 3, 5, 9):
        for tile in grid_tiles(n) + [1 << 30, 2 ** 31 - 1]:
            for rank in range(world):
                assert parallel.local_slots(n, rank, world, tile, width) == n_local(width, height, rank, world, tile), (world, tile, rank)
                got = parallel.owned_gids(n, rank, world, tile, width)
                want = slot_pixels(width, height, rank, world, tile)
                assert got.dtype == np.int32 and np.array_equal(got, np.sort(want) if world == 1 else want), (world, tile, rank)


def test_a_rank_beyond_the_units_owns_nothing():
    assert parallel.local_slots(7, 5, 8, 3) == 0 and parallel.owned_gids(7, 5, 8, 3).size == 0          # 3 runs, 8 ranks
    assert parallel.local_slots(30 * 12, 2, 3, 0, 30) == 0 and parallel.owned_gids(30 * 12, 2, 3, 0, 30).size == 0  # 2 blocks, 3 ranks
    assert n_local(7, 1, 5, 8, 3) == 0 and n_local(30, 12, 2, 3, 0) == 0
