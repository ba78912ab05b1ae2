// pass_schedule_fuzz — how passes become launches (csrc/pass_schedule.hpp: launch_pass_cap, for_each_launch, stage_passes) over the
// grids of tests/test_pass_schedule_cpu.py.  Header-only code: nothing is linked; built with AddressSanitizer + UBSan like the
// programs beside it.  What can be checked without a table is checked here (a failure is a message and exit status 1); what the test
// compares with its own arithmetic or with tests/golden/pass_caps.npz is printed.
//   pass_schedule_fuzz caps    launch_pass_cap over images x shards x budgets x most: rows of 9 int64, binary, on stdout —
//                              width height rank world tile n_local budget most cap
//   pass_schedule_fuzz cut     for_each_launch over n x cap: "n cap : the launches' pass counts" per line
//   pass_schedule_fuzz stage   stage_passes with an allocator that refuses above a limit: "name held_before limit : bytes passes : the
//                              sizes asked for" per line
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../chunkyclplugin_amd/csrc/pass_schedule.hpp"

using namespace chunky;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

static int caps() {
    static const int kImages[7][2] = {{1, 1}, {15, 17}, {16, 16}, {17, 16}, {1920, 1080}, {8192, 8192}, {32768, 32768}};
    static const int kShards[5][2] = {{1, 256}, {2, 256}, {8, 256}, {2, 0}, {8, 0}};  // world, tile: whole; runs of 256; 16 x 16 blocks
    static const size_t kBudgets[5] = {0, 11, 12, (size_t)1 << 20, (size_t)8 << 30};
    static const int kMost[2] = {kMaxPassesPerLaunch, kMaxPoolPasses};
    for (const auto& im : kImages)
        for (const auto& sh : kShards)
            for (int last = 0; last < (sh[0] > 1 ? 2 : 1); last++)  // rank 0 and the last rank (which owns no tile of a small image)
                for (size_t budget : kBudgets)
                    for (int most : kMost) {
                        const int width = im[0], height = im[1], rank = last ? sh[0] - 1 : 0;
                        ShardView T;
                        CHECK(make_shard_view(width, height, rank, sh[0], sh[1], &T), "no view for %d x %d rank %d of %d tile %d", width, height, rank, sh[0], sh[1]);
                        const int cap = launch_pass_cap(T, width, height, budget, most);
                        const int64_t slots = (int64_t)(staging_floats(T, width, height, 1) / 3);
                        CHECK(cap <= most, "cap %d above most %d", cap, most);
                        if (cap >= 1 && slots > 0) {
                            CHECK((__int128)cap * slots * 12 <= (__int128)budget, "cap %d x %lld slots x 12 exceeds the budget %zu", cap, (long long)slots, budget);
                            CHECK((int64_t)cap * slots < ((int64_t)1 << 31), "cap %d x %lld slots reaches 2^31", cap, (long long)slots);
                        }
                        const int64_t row[9] = {width, height, T.rank, T.world, T.tile, T.n_local, (int64_t)budget, most, cap};
                        fwrite(row, sizeof(row), 1, stdout);
                    }
    return 0;
}

static int cut() {
    static const int kN[8] = {0, 1, 255, 256, 257, 300, 1024, 1025};
    static const int kCap[5] = {1, 2, 255, 256, 1024};
    for (int n : kN)
        for (int cap : kCap) {
            std::vector<int32_t> seeds((size_t)n);  // exactly n: a read past the caller's seeds is a sanitizer report
            for (int i = 0; i < n; i++) seeds[(size_t)i] = 1000003 * i - 77;
            const int first_spp = 40 + n;
            int done = 0;
            printf("%d %d :", n, cap);
            const int rc = for_each_launch(n ? seeds.data() : nullptr, n, first_spp, cap, [&](const PassSeeds& P, const int32_t* launch_seeds) {
                CHECK(P.n >= 1 && P.n <= cap && P.n <= n - done, "n %d cap %d: a launch of %d passes at offset %d", n, cap, P.n, done);
                CHECK(P.n == (n - done < cap ? n - done : cap), "n %d cap %d: a launch of %d passes at offset %d is not the longest", n, cap, P.n, done);
                CHECK(P.first_spp == first_spp + done, "n %d cap %d: first_spp %d at offset %d", n, cap, P.first_spp, done);
                CHECK(launch_seeds == seeds.data() + done, "n %d cap %d: the seeds handed through are not at offset %d", n, cap, done);
                if (P.n <= kMaxPassesPerLaunch)
                    CHECK(memcmp(P.seed, seeds.data() + done, (size_t)P.n * 4) == 0, "n %d cap %d: P.seed at offset %d", n, cap, done);
                printf(" %d", P.n);
                done += P.n;
                return 0;
            });
            printf("\n");
            CHECK(rc == 0 && done == n, "n %d cap %d: %d passes cut, code %d", n, cap, done, rc);
            if (n > 2) {  // a code from the callback ends the cut and comes back
                int calls = 0;
                CHECK(for_each_launch(seeds.data(), n, 0, 1, [&](const PassSeeds&, const int32_t*) { return ++calls == 2 ? 7 : 0; }) == 7 && calls == 2, "n %d: the cut went on past a code", n);
            }
        }
    return 0;
}

// one call of the staging rule with an allocator that refuses above `limit` bytes
static void stage_case(const char* name, size_t held, int launch, int cap, int reserve, size_t free_bytes, size_t limit) {
    const int width = 16, height = 16;
    const ShardView whole{0, 1, 256, width * height};
    std::vector<size_t> asked;
    const StagedLaunch got = stage_passes(held, whole, width, height, launch, cap, reserve, free_bytes, [&](size_t bytes) {
        asked.push_back(bytes);
        return bytes <= limit;
    });
    CHECK(got.passes <= launch && got.passes >= 0, "%s: %d passes per launch of %d", name, got.passes, launch);
    CHECK(got.bytes >= held || got.passes == 0, "%s: the array shrank from %zu to %zu bytes", name, held, got.bytes);
    if (got.passes > 0) CHECK(got.bytes >= staging_floats(whole, width, height, got.passes) * sizeof(float), "%s: %zu bytes do not hold %d passes", name, got.bytes, got.passes);
    if (!asked.empty() && got.passes > 0) CHECK(got.bytes == asked.back() && asked.back() <= limit, "%s: %zu bytes held, the last request was %zu", name, got.bytes, asked.back());
    printf("%s %zu %zu : %zu %d :", name, held, limit, got.bytes, got.passes);
    for (size_t b : asked) printf(" %zu", b);
    printf("\n");
}

static int stage() {
    const size_t pass = 16 * 16 * 3 * sizeof(float);  // one pass of a 16 x 16 image: one tile
    const size_t any = SIZE_MAX;
    // the halving: 256 passes, no reserve
    stage_case("halve_1", 0, 256, 256, 0, any, 1 * pass);
    stage_case("halve_2", 0, 256, 256, 0, any, 2 * pass);
    stage_case("halve_3", 0, 256, 256, 0, any, 3 * pass);
    stage_case("halve_255", 0, 256, 256, 0, any, 255 * pass);
    stage_case("halve_none", 0, 256, 256, 0, any, pass - 1);
    stage_case("fits", 0, 256, 256, 0, any, 256 * pass);
    stage_case("odd_300_of_1024", 0, 300, 1024, 0, any, 74 * pass);  // 300, 150, 75, 38
    // it grows only
    stage_case("held_enough", 256 * pass, 256, 256, 0, any, 0);
    stage_case("held_more", 300 * pass, 8, 256, 64, any, 0);
    stage_case("held_short", 7 * pass, 8, 256, 0, any, any);
    stage_case("nothing_to_stage", 0, 0, 256, 64, any, 0);
    // the reserve: taken when it exceeds the launch and is at most half the free bytes; clamped to the cap and to 256
    stage_case("reserve", 0, 8, 256, 64, any, any);
    stage_case("reserve_half_free", 0, 8, 256, 64, 128 * pass, any);
    stage_case("reserve_over_half_free", 0, 8, 256, 64, 128 * pass - 1, any);
    stage_case("reserve_below_launch", 0, 64, 256, 8, any, any);
    stage_case("reserve_equals_launch", 0, 64, 256, 64, any, any);
    stage_case("reserve_clamped_to_cap", 0, 8, 100, 300, any, any);
    stage_case("reserve_clamped_to_256", 0, 8, 1024, 1024, any, any);
    stage_case("reserve_refused", 0, 8, 256, 64, any, 10 * pass);
    stage_case("reserve_refused_then_halved", 0, 8, 256, 64, any, 5 * pass);
    stage_case("reserve_held_short", 4 * pass, 8, 256, 64, any, any);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "caps")) return caps();
    if (argc == 2 && !strcmp(argv[1], "cut")) return cut();
    if (argc == 2 && !strcmp(argv[1], "stage")) return stage();
    fprintf(stderr, "usage: pass_schedule_fuzz caps | cut | stage\n");
    return 2;
}
