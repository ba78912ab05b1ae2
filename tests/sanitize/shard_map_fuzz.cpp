// tests/sanitize/shard_map_fuzz.cpp — TEST-ONLY: the host arithmetic of the shard-to-pixel map (csrc/shard_map.hpp: n_local_slots,
// make_shard_view, member_shard, block_pixel_list, fast_div) under AddressSanitizer + UBSan on the CPU.  Plain C++: nothing here
// touches a device.
//
// The reference is a brute-force owner table written from the rule, not from the code: owner[gid] = unit(gid) % world, where the
// unit of a pixel is gid / tile, or (tile 0) the index of its 16 x 16 block, row-major over blocks; a tile at or above the pixel
// count is the pixel count.  Required, for every rank of every geometry of the grid: n_local = (units the rank owns) x (slots per
// unit), the pixels enumerated from the view — block_pixel_list, or the run formula slot -> ((slot / tile) * world + rank) * tile
// + slot % tile over slots 0 .. n_local - 1 — are exactly the pixels the table gives the rank, and over all ranks every pixel
// appears once.  At the extremes of what the ABI takes (tile and world up to INT_MAX, images of 2^30 pixels) the counts are
// compared with the rule evaluated in 64 bits, and no arithmetic may be undefined.   (tests/test_sanitize.py)
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../chunkyclplugin_amd/csrc/shard_map.hpp"

using namespace chunky;

static long long n_geometries = 0, n_ranks = 0, n_enumerated = 0, n_extreme = 0, n_refused_views = 0, n_member_ok = 0, n_member_refused = 0,
                 n_member_sets = 0, n_div_pairs = 0;

#define REQUIRE(cond, ...)                                   \
    do {                                                     \
        if (!(cond)) {                                       \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);  \
            fprintf(stderr, __VA_ARGS__);                    \
            fprintf(stderr, "\n");                           \
            exit(1);                                         \
        }                                                    \
    } while (0)

// the rule: the unit of every pixel, and how many units there are
static int64_t units_of(int w, int h, int tile, std::vector<int64_t>* unit) {
    const int64_t n = (int64_t)w * h;
    if (unit) unit->assign((size_t)n, 0);
    if (tile == 0) {
        const int bw = (w + 15) / 16, bh = (h + 15) / 16;
        if (unit)
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) (*unit)[(size_t)y * w + x] = (int64_t)(y / 16) * bw + x / 16;
        return (int64_t)bw * bh;
    }
    const int64_t t = (int64_t)tile > n ? n : tile;
    if (unit)
        for (int64_t g = 0; g < n; g++) (*unit)[(size_t)g] = g / t;
    return (n + t - 1) / t;
}

// the pixels a view enumerates, in slot order (padding left out)
static std::vector<int64_t> enumerate(int w, int h, const ShardView& v) {
    const int64_t n = (int64_t)w * h;
    std::vector<int64_t> out;
    if (v.world != 1 && v.tile == 0) {
        for (int32_t g : block_pixel_list(w, h, v)) out.push_back(g);
        REQUIRE((int64_t)out.size() <= v.n_local, "block list longer than n_local");
        return out;
    }
    for (int64_t s = 0; s < v.n_local; s++) {
        int64_t g = s;
        if (v.world != 1) g = ((s / v.tile) * v.world + v.rank) * v.tile + s % v.tile;
        REQUIRE(g >= 0 && g <= INT_MAX, "slot %lld of %dx%d rank %d/%d tile %d maps to %lld: not an int", (long long)s, w, h, v.rank, v.world, v.tile, (long long)g);
        if (g < n) out.push_back(g);
    }
    return out;
}

static void check_geometry(int w, int h, int world, int tile) {
    const int64_t n = (int64_t)w * h;
    std::vector<int64_t> unit;
    const int64_t units = units_of(w, h, tile, &unit);
    const int64_t per_unit = tile == 0 ? 256 : ((int64_t)tile > n ? n : tile);
    std::vector<int> seen((size_t)n, 0);
    for (int rank = 0; rank < world; rank++) {
        ShardView v;
        REQUIRE(make_shard_view(w, h, rank, world, tile, &v), "%dx%d rank %d/%d tile %d refused", w, h, rank, world, tile);
        REQUIRE(v.rank == rank && v.world == world && v.tile == (tile == 0 ? 0 : (int)per_unit), "view fields");
        int64_t mine = 0;
        for (int64_t u = 0; u < units; u++) mine += (u % world == rank);
        const int64_t want = world == 1 ? n : mine * per_unit;
        REQUIRE(v.n_local == want, "%dx%d rank %d/%d tile %d: n_local %d, the rule says %lld", w, h, rank, world, tile, v.n_local, (long long)want);
        if ((int64_t)tile >= n && tile != 0 && world > 1) REQUIRE(v.n_local == (rank == 0 ? n : 0) && v.n_local <= n, "a tile >= n_pixels: rank 0 owns all");
        for (int64_t g : enumerate(w, h, v)) {
            REQUIRE(unit[(size_t)g] % world == rank, "%dx%d rank %d/%d tile %d enumerates pixel %lld of rank %lld", w, h, rank, world, tile, (long long)g,
                    (long long)(unit[(size_t)g] % world));
            seen[(size_t)g]++;
            n_enumerated++;
        }
        n_ranks++;
    }
    for (int64_t g = 0; g < n; g++) REQUIRE(seen[(size_t)g] == 1, "%dx%d world %d tile %d: pixel %lld enumerated %d times", w, h, world, tile, (long long)g, seen[(size_t)g]);
    n_geometries++;
}

// the rule in closed form, in 64 bits: units rank, rank + world, ... below `units`
static int64_t owned_units(int64_t units, int rank, int world) { return rank < units ? (units - 1 - rank) / world + 1 : 0; }

static void check_extreme(int w, int h, int rank, int world, int tile) {
    const int64_t n = (int64_t)w * h;
    const int64_t units = units_of(w, h, tile, nullptr);
    const int64_t per_unit = tile == 0 ? 256 : ((int64_t)tile > n ? n : tile);
    const int64_t want = world == 1 ? n : owned_units(units, rank, world) * per_unit;
    ShardView v{-1, -1, -1, -1};
    const bool ok = make_shard_view(w, h, rank, world, tile, &v);
    if (want > INT_MAX) {
        REQUIRE(!ok, "%dx%d rank %d/%d tile %d: %lld slots accepted", w, h, rank, world, tile, (long long)want);
        n_refused_views++;
        return;
    }
    REQUIRE(ok && v.n_local == want, "%dx%d rank %d/%d tile %d: n_local %d, the rule says %lld", w, h, rank, world, tile, v.n_local, (long long)want);
    REQUIRE(v.tile <= n && (tile == 0) == (v.tile == 0), "tile not clamped");
    if (tile != 0 && (int64_t)tile >= n && world > 1) REQUIRE(v.n_local == (rank == 0 ? n : 0), "a tile >= n_pixels: rank 0 owns all, the others nothing");
    if (tile != 0 && world > 1 && v.n_local > 0) {  // the last slot's pixel index, as the device computes it, stays an int
        const int64_t s = v.n_local - 1, g = ((s / v.tile) * v.world + v.rank) * v.tile + s % v.tile;
        REQUIRE(g <= INT_MAX && g < n + v.tile, "last slot maps to %lld", (long long)g);
    }
    n_extreme++;
}

static void check_members(int w, int h, int rank, int world, int tile, int members, bool sets) {
    const ShardView outer{rank, world, tile, 0};
    std::vector<ShardView> share((size_t)members);
    bool ok = true;
    for (int i = 0; i < members; i++) ok = member_shard(outer, i, members, &share[(size_t)i]) && ok;
    if ((int64_t)world * members > INT_MAX) {
        for (int i = 0; i < members; i++) REQUIRE(!member_shard(outer, i, members, &share[(size_t)i]), "world %d x %d members accepted", world, members);
        n_member_refused++;
        return;
    }
    REQUIRE(ok, "world %d x %d members refused", world, members);
    for (int i = 0; i < members; i++) {
        const ShardView& m = share[(size_t)i];
        REQUIRE((int64_t)m.world == (int64_t)world * members && (int64_t)m.rank == rank + (int64_t)world * i && m.rank < m.world && m.tile == tile,
                "member %d of %d of rank %d/%d: %d/%d", i, members, rank, world, m.rank, m.world);
    }
    n_member_ok++;
    if (!sets) return;
    // the members' pixels are the outer share's, each once
    const int64_t n = (int64_t)w * h;
    std::vector<int> seen((size_t)n, 0);
    for (int i = 0; i < members; i++) {
        ShardView v;
        REQUIRE(make_shard_view(w, h, share[(size_t)i].rank, share[(size_t)i].world, share[(size_t)i].tile, &v), "member view refused");
        for (int64_t g : enumerate(w, h, v)) seen[(size_t)g]++;
    }
    std::vector<int64_t> unit;
    units_of(w, h, tile, &unit);
    for (int64_t g = 0; g < n; g++)
        REQUIRE(seen[(size_t)g] == (unit[(size_t)g] % world == rank ? 1 : 0), "%dx%d outer %d/%d tile %d, %d members: pixel %lld seen %d times", w, h, rank, world,
                tile, members, (long long)g, seen[(size_t)g]);
    n_member_sets++;
}

// fast_quotient (csrc/path_state.hpp) restated: the high half of the 64-bit product, then the shift
static uint32_t quotient(uint32_t a, FastDiv f) { return f.m ? (uint32_t)((((uint64_t)a * f.m) >> 32) >> f.s) : a; }

static void check_divisor(uint32_t d, std::mt19937& rng) {
    const FastDiv f = fast_div(d);
    REQUIRE(f.s >= 0 && f.s < 32, "shift %d", f.s);
    uint32_t a[6 + 64] = {0u, 1u, d - 1u, d, d + 1u, 0x7FFFFFFFu};
    for (int i = 6; i < 70; i++) a[i] = (uint32_t)rng() & 0x7FFFFFFFu;
    for (uint32_t x : a) {
        if (x > 0x7FFFFFFFu) continue;  // (numerators are pixel indices: below 2^31; d - 1, d, d + 1 of the largest divisors are not)
        REQUIRE(quotient(x, f) == x / d, "%u / %u: %u, not %u", x, d, quotient(x, f), x / d);
        n_div_pairs++;
    }
}

int main() {
    // ---- the exhaustive grid
    for (int w = 1; w <= 40; w++)
        for (int h = 1; h <= 36; h++) {
            const int n = w * h;
            const int tiles[] = {0, 1, 2, 3, 4, 5, 7, 15, 16, 17, 63, 64, 100, 255, 256, 257, n - 1, n, n + 1};
            for (int world = 1; world <= 9; world++)
                for (int tile : tiles)
                    check_geometry(w, h, world, tile);  // (n - 1 = 0 on a 1 x 1 image is the block form again)
        }
    // ---- the extremes: counts only
    const int images[][2] = {{1, 1}, {1, 1 << 30}, {1 << 30, 1}, {32768, 32768}, {7, 1}, {17, 33}, {100, 60}};
    const int big_tiles[] = {0, 1, 255, 1 << 20, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, INT_MAX - 1, INT_MAX};
    const int worlds[] = {1, 2, 3, 1 << 20, 1 << 30, INT_MAX};
    for (const auto& im : images)
        for (int tile : big_tiles)
            for (int world : worlds) {
                const int ranks[] = {0, 1, world / 2, world - 1};
                for (int rank : ranks)
                    if (rank >= 0 && rank < world) check_extreme(im[0], im[1], rank, world, tile);
            }
    // ---- a group's members inside an outer share
    const int outer_worlds[] = {1, 2, 3, 5, 1 << 20, 1 << 28, INT_MAX / 8, INT_MAX / 8 + 1, INT_MAX / 3, INT_MAX / 3 + 1, INT_MAX / 2, INT_MAX / 2 + 1, 1 << 30, INT_MAX};
    const int member_counts[] = {1, 2, 3, 8};
    const int small[][2] = {{17, 33}, {7, 1}, {1, 7}, {33, 17}};
    for (int world : outer_worlds)
        for (int members : member_counts) {
            const int ranks[] = {0, 1, world - 1};
            for (int rank : ranks) {
                if (rank < 0 || rank >= world) continue;
                if (world <= 5) {
                    for (const auto& im : small)
                        for (int tile : {0, 1, 3, 64, 257, im[0] * im[1] + 1}) check_members(im[0], im[1], rank, world, tile, members, true);
                } else {
                    for (int tile : {0, 3, INT_MAX}) check_members(17, 33, rank, world, tile, members, false);
                }
            }
        }
    // ---- fast_div
    std::mt19937 rng(11u);
    for (uint32_t d = 1; d <= 4100; d++) check_divisor(d, rng);
    for (int k = 0; k <= 26; k++)
        for (int e = -1; e <= 1; e++) {
            const int64_t d = ((int64_t)1 << k) + e;
            if (d >= 1) check_divisor((uint32_t)d, rng);
        }
    // divisors no image produces, which fast_div still has to take without shifting by the width of its type: 2^31 and beyond
    for (uint32_t d : {0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xC0000000u, 0xFFFFFFFEu, 0xFFFFFFFFu}) check_divisor(d, rng);
    printf("{\"geometries\": %lld, \"ranks\": %lld, \"pixels_enumerated\": %lld, \"extreme_views\": %lld, \"refused_views\": %lld, \"member_shares\": %lld, "
           "\"member_refusals\": %lld, \"member_sets\": %lld, \"quotients\": %lld}\n",
           n_geometries, n_ranks, n_enumerated, n_extreme, n_refused_views, n_member_ok, n_member_refused, n_member_sets, n_div_pairs);
    return 0;
}
