// shard_map.hpp — the host arithmetic of the shard-to-pixel map: which pixel slots a rank owns (n_local_slots), the view
// chunky_render_set_shard stores (make_shard_view), a group member's share of an outer share (member_shard), the pixel list of a
// block shard for the kernels without the block mapping (block_pixel_list), and the host half of the division by a launch constant
// (fast_div).  Plain C++17 over ints, no device call: everything here is reached by caller-supplied ints (any tile >= 0, any
// 0 <= rank < world <= INT_MAX, any image of at most 2^30 pixels), so tests/sanitize/shard_map_fuzz.cpp runs it under
// AddressSanitizer + UBSan against a brute-force owner table.  The device half (path_state.hpp shard_gid / pool_slot_gid /
// pool_slot_pixel / fast_quotient) reads the views made here.
#pragma once
#include <climits>
#include <cstdint>
#include <vector>

namespace chunky {

// Image-tile ownership of this process: tiles of `tile` consecutive pixel
// indices dealt round-robin over `world` ranks; n_local = pixel slots owned by `rank`.
struct ShardView {
    int rank, world, tile, n_local;
    // block shards (tile 0) under a kernel that cannot map 16 x 16 blocks itself (launch_fallback): the rank's pixels, in
    // block order, as an explicit list on the device (block_pixel_list); null otherwise
    const int* list = nullptr;
    int n_list = 0;
};

// A run length at or above the pixel count means one run, the whole image: clamped to the pixel count, so that no product of a run
// index and the run length below — here or on the device — leaves the range of an int.
inline int clamp_tile(int width, int height, int tile) {
    const int64_t n_pixels = (int64_t)width * height;
    return (int64_t)tile > n_pixels ? (int)n_pixels : tile;
}

// Pixel slots (whole tiles, padding included) of rank t.rank: every intermediate in 64 bits.  The result fits an int for every run
// length (mine * tile < n_pixels + tile <= 2^31 after the clamp); a share of 16 x 16 blocks of a very thin, very long image can need
// more slots than an int holds (256 per block, 16 pixels of it used): the caller refuses those (make_shard_view).
inline int64_t n_local_slots(int width, int height, const ShardView& t) {
    const int64_t n_pixels = (int64_t)width * height;
    if (t.world == 1) return n_pixels;
    int64_t units, per_unit;
    if (t.tile == 0) {  // 16 x 16 blocks rank, rank + world, ... of the image, edge blocks padded
        units = (int64_t)((width + 15) / 16) * ((height + 15) / 16);
        per_unit = 256;
    } else {  // runs rank, rank + world, ... of the pixel indices, the last one padded
        per_unit = clamp_tile(width, height, t.tile);
        units = (n_pixels + per_unit - 1) / per_unit;
    }
    if ((int64_t)t.rank >= units) return 0;  // more ranks than tiles: this one owns nothing
    const int64_t mine = (units - t.rank + t.world - 1) / t.world;
    return mine * per_unit;
}

// The view chunky_render_set_shard stores for (rank, world, tile) on a width x height image — the run length clamped, n_local
// counted; false when the share needs more slots than an int holds.  Expects 0 <= rank < world, tile >= 0, width * height <= 2^30.
inline bool make_shard_view(int width, int height, int rank, int world, int tile, ShardView* out) {
    ShardView t{rank, world, clamp_tile(width, height, tile), 0};
    const int64_t n = n_local_slots(width, height, t);
    if (n > INT_MAX) return false;
    t.n_local = (int)n;
    *out = t;
    return true;
}

// Member i of n renders rank + world * i of world * n of the image (rank / world: the caller's own share, chunky_render_set_shard:
// its tiles are t = rank (mod world); dealing them round-robin to n members gives member i the tiles t = rank + world * i
// (mod world * n)).  False when world * n does not fit an int: such a group is refused, not mis-sharded.  n_local is left 0.
inline bool member_shard(const ShardView& outer, int i, int n, ShardView* out) {
    if (n < 1 || i < 0 || i >= n || outer.world < 1 || outer.rank < 0 || outer.rank >= outer.world) return false;
    const int64_t world = (int64_t)outer.world * n;
    if (world > INT_MAX) return false;
    *out = ShardView{(int)(outer.rank + (int64_t)outer.world * i), (int)world, outer.tile, 0};  // (rank < world: it fits as well)
    return true;
}

// The pixels of a block shard (tile 0) in block order, padding left out: what launch_fallback's kernels render when
// render_pool does not apply to a sharded target (same ownership rule as pool_slot_gid, so the gather finds every pixel).
inline std::vector<int32_t> block_pixel_list(int width, int height, const ShardView& t) {
    std::vector<int32_t> out;
    const int bw = (width + 15) / 16, bh = (height + 15) / 16;
    for (int64_t b = t.rank; b < (int64_t)bw * bh; b += t.world) {
        const int bx = (int)(b % bw) * 16, by = (int)(b / bw) * 16;
        for (int y = by; y < by + 16 && y < height; y++)
            for (int x = bx; x < bx + 16 && x < width; x++) out.push_back(y * width + x);
    }
    return out;
}

// Exact n / d for n < 2^31 by one multiply-high and one shift (d fixed for a launch, the pair made on the host): with 2^s < d <= 2^(s+1)
// and m = ceil(2^(32+s) / d) — a 32-bit number — the error term m * d - 2^(32+s) is below d, and n * d < 2^(32+s) keeps the quotient exact.
// The quotient is (n * m) >> (32 + s) in 64 bits (path_state.hpp fast_quotient: __umulhi, then the shift); m == 0 stands for d == 1.
struct FastDiv {
    unsigned m;  // 0: d == 1
    int s;
};
inline FastDiv fast_div(unsigned d) {
    if (d <= 1) return FastDiv{0u, 0};
    int s = 0;
    while (s < 31 && (2u << s) < d) s++;  // 2^s < d <= 2^(s+1) (s stops at 31: 2u << 31 is no longer 2^32)
    const unsigned long long m = (((unsigned long long)1 << (32 + s)) + d - 1) / d;
    return FastDiv{(unsigned)m, s};
}

}  // namespace chunky
