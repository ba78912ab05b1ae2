// launch_plan_sweep — plan_render (csrc/launch_plan.cpp) over an enumeration of its inputs (tests/test_launch_plan_cpu.py).  Links
// csrc/launch_plan.cpp alone, built with AddressSanitizer + UBSan like the fuzzers beside it.
//
// A row is one combination of the values below, numbered in mixed radix with the first dimension the fastest; the enumeration has
// 23 357 030 400 rows.  Every row printed is also checked here: a pool plan names a listed instantiation, its words are
// pool_words(ext, bvh), its LDS bytes 4 * pool_wave_lds_bytes(park, words, depth); a waves or lanes plan names a listed one too.
//   launch_plan_sweep dims                 the dimensions, "name radix" per line
//   launch_plan_sweep list                 the render_pool instantiations, "tree park stats bvh ext sorted" per line
//   launch_plan_sweep stride FIRST STRIDE  rows FIRST, FIRST + STRIDE, ...: kFields int32 each, binary, on stdout
//   launch_plan_sweep rows I J ...         the same for the rows named
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../chunkyclplugin_amd/csrc/launch_plan.hpp"

using namespace chunky;

struct Dim {
    const char* name;
    int radix;
};
static const Dim kDims[] = {{"variant", 1024}, {"tree", 8},  {"entities", 3}, {"stack", 5}, {"addr32", 3}, {"blocks", 3},  {"opts", 5},
                            {"proj", 2},       {"queue", 2}, {"passes", 11},  {"seeds", 2}, {"fold", 2},   {"n_local", 6}, {"shard", 4}};
constexpr int kNDims = (int)(sizeof(kDims) / sizeof(kDims[0]));
static const int kStack[5] = {0, 10, 11, 64, 65};  // the entity pool holds 32 parked paths up to 10 entries, 16 above
static const unsigned kAddr[3] = {0u, 3u, 7u};
static const int kPasses[11] = {1, 15, 16, 31, 32, 63, 64, 256, 257, 1024, 1025};
static const int kLocal[6] = {0, 1, (3 << 17) - 1, 3 << 17, (3 << 18) - 1, 3 << 18};
static const int kSomeList[1] = {0};

struct Row {
    int variant;
    SceneFacts F;
    RenderOpts O;
    int projector_type;
    ShardView T;
    int n_passes;
    bool queue, seeds, fold;
};

static uint64_t row_count() {
    uint64_t n = 1;
    for (const Dim& d : kDims) n *= (uint64_t)d.radix;
    return n;
}

static Row decode(uint64_t index) {
    int v[kNDims];
    for (int i = 0; i < kNDims; i++) {
        v[i] = (int)(index % (uint64_t)kDims[i].radix);
        index /= (uint64_t)kDims[i].radix;
    }
    Row r{};
    r.variant = v[0];
    // tree: 0 no wide tree; 1-5 that many levels, 3 bits each below the top; 6 three levels, one of them not 3 bits; 7 six levels
    r.F.wide = v[1] != 0;
    r.F.wide_nlev = v[1] == 0 ? 0 : (v[1] <= 5 ? v[1] : (v[1] == 6 ? 3 : 6));
    for (int i = 0; i < 6; i++) r.F.wide_bits[i] = i == 0 ? 6 : 3;
    if (v[1] == 6) r.F.wide_bits[2] = 2;
    // entities: 0 none, 1 both BVHs with their records, 2 both without
    r.F.world_bvh_empty = r.F.actor_bvh_empty = v[2] == 0;
    r.F.bvh_records = v[2] == 1;
    r.F.bvh_stack_entries = kStack[v[3]];
    r.F.addr32 = kAddr[v[4]];
    // blocks: 0 sorted with block_info, 1 unsorted with block_info, 2 sorted without
    r.F.sort_blocks = v[5] != 1;
    r.F.block_info = v[5] != 2;
    // opts: 0 default, 1 nee, 2 draw depth 65536, 3 max depth 255, 4 nee with max depth 255
    r.O = RenderOpts{256, 5, 13.0f, -1, 1, 0, 0, 0};
    if (v[6] == 1 || v[6] == 4) r.O.nee = 1;
    if (v[6] == 2) r.O.draw_depth = 65536;
    if (v[6] == 3 || v[6] == 4) r.O.max_depth = 255;
    r.projector_type = v[7] ? 2 : 0;
    r.queue = v[8] != 0;
    r.n_passes = kPasses[v[9]];
    r.seeds = v[10] != 0;
    r.fold = v[11] != 0;
    const int n_local = kLocal[v[12]];
    // shard: 0 the whole image, 1 two ranks in runs, 2 two ranks in blocks with the pixel list, 3 in blocks without
    switch (v[13]) {
        case 0: r.T = ShardView{0, 1, 256, n_local}; break;
        case 1: r.T = ShardView{1, 2, 256, n_local}; break;
        case 2: r.T = ShardView{1, 2, 0, n_local, kSomeList, n_local / 2 + 1}; break;
        default: r.T = ShardView{1, 2, 0, n_local}; break;
    }
    return r;
}

constexpr int kFields = 17;
static void fields(const RenderPlan& p, int32_t* out) {
    const int32_t f[kFields] = {(int)p.family, p.tree, p.park, p.words, p.group, p.depth, p.bvh, p.ext, p.stats, p.sorted, p.proj, (int32_t)p.lds,
                                p.most, p.needs_list, (int)p.status, (int)p.ext_refusal, (int)p.why};
    memcpy(out, f, sizeof f);
}

struct PoolInstance {
    int tree, park;
    bool stats, bvh, ext, sorted;
};
#define AS_POOL_INSTANCE(TREE, K, STATS, BVH, EXT, SORT) {TREE, K, STATS, BVH, EXT, SORT},
static const PoolInstance kPoolList[] = {CHUNKY_POOL_INSTANCES(AS_POOL_INSTANCE) CHUNKY_POOL_BVH_INSTANCES(AS_POOL_INSTANCE)};
struct WavesInstance {
    int tree, group;
    bool bvh;
};
#define AS_WAVES_INSTANCE(TREE, G, BVH) {TREE, G, BVH},
static const WavesInstance kWavesList[] = {CHUNKY_WAVES_INSTANCES(AS_WAVES_INSTANCE)};
#define AS_LANES_INSTANCE(TREE) TREE,
static const int kLanesList[] = {CHUNKY_LANES_INSTANCES(AS_LANES_INSTANCE)};

static bool listed(const RenderPlan& p) {
    if (p.family == KernelFamily::pool) {
        for (const PoolInstance& k : kPoolList)
            if (k.tree == p.tree && k.park == p.park && k.stats == p.stats && k.bvh == p.bvh && k.ext == p.ext && k.sorted == p.sorted) return true;
    } else if (p.family == KernelFamily::waves) {
        for (const WavesInstance& k : kWavesList)
            if (k.tree == p.tree && k.group == p.group && k.bvh == p.bvh) return true;
    } else {
        for (int tree : kLanesList)
            if (tree == p.tree) return true;
    }
    return false;
}

static bool emit(uint64_t index) {
    const Row r = decode(index);
    const RenderPlan p = plan_render(r.variant, r.F, r.O, r.projector_type, r.T, r.n_passes, r.queue, r.seeds, r.fold);
    if (p.status == PlanStatus::ok) {
        const char* wrong = nullptr;
        if (!listed(p)) wrong = "names no listed instantiation";
        if (p.family == KernelFamily::pool && p.words != pool_words(p.ext, p.bvh)) wrong = "words is not pool_words(ext, bvh)";
        if (p.family == KernelFamily::pool && p.lds != 4u * (size_t)pool_wave_lds_bytes(p.park, p.words, (unsigned)p.depth)) wrong = "LDS is not four waves of pool_wave_lds_bytes";
        if (p.lds > kCuLdsBytes) wrong = "more LDS than a compute unit has";
        if (wrong) {
            fprintf(stderr, "row %llu: the plan %s (family %d tree %d park %d words %d group %d depth %d lds %zu)\n", (unsigned long long)index, wrong,
                    (int)p.family, p.tree, p.park, p.words, p.group, p.depth, p.lds);
            return false;
        }
    }
    int32_t out[kFields];
    fields(p, out);
    return fwrite(out, sizeof out, 1, stdout) == 1;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "dims")) {
        for (const Dim& d : kDims) printf("%s %d\n", d.name, d.radix);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "list")) {
        for (const PoolInstance& k : kPoolList) printf("%d %d %d %d %d %d\n", k.tree, k.park, (int)k.stats, (int)k.bvh, (int)k.ext, (int)k.sorted);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "stride")) {
        const uint64_t first = strtoull(argv[2], nullptr, 10), stride = strtoull(argv[3], nullptr, 10), n = row_count();
        if (stride == 0) return 2;
        for (uint64_t i = first; i < n; i += stride)
            if (!emit(i)) return 1;
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "rows")) {
        for (int a = 2; a < argc; a++) {
            const uint64_t i = strtoull(argv[a], nullptr, 10);
            if (i >= row_count() || !emit(i)) return 1;
        }
        return 0;
    }
    return 2;
}
