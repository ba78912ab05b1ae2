// adaptive_state_fuzz — the parser of a caller-supplied (possibly file-restored) adaptive state, adaptive_state_valid of
// csrc/adaptive_host.cpp, through the entry points that reach it (chunky_adaptive_state_check, chunky_adaptive_host_begin, _resume),
// under AddressSanitizer + UBSan.  Links adaptive_host.cpp and capi_error.cpp and nothing else.
//   1. every state _begin leaves, and _resume leaves after each cut of a short run on random samples, is accepted;
//   2. from each accepted state every rule of the check is broken in turn: CHUNKY_E_INVALID with that rule's message, nothing written;
//   3. the caller's header lives in a heap block of exactly the size it declares (the first version, sizeof, sizeof + 24) and the arrays
//      in blocks of exactly their length, so a read or write past either is ASan's to find; `size` and the bytes beyond sizeof survive;
//   4. one JSON line of counts.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../../chunkyclplugin_amd/csrc/adaptive_spec.h"
#include "../../include/chunky_hip.h"

static long long failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, chunky_last_error()); \
        }                                                                  \
    } while (0)

constexpr size_t kFirst = offsetof(chunky_adaptive_state, summary) + sizeof(chunky_adaptive_summary);  // the first version of the struct
constexpr size_t kTail = 24;
constexpr unsigned char kTailByte = 0xA5;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;  // fixed seed
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
static float rnd01() { return (float)(rnd() & 0xFFFFFF) / 16777216.0f; }

// a heap block of exactly n bytes (n == 0: one byte nobody may touch is not needed; malloc(0) may be NULL, so keep 1 and never use it)
template <class T>
struct Block {
    T* p;
    size_t n;
    explicit Block(size_t count) : p((T*)malloc(count ? count * sizeof(T) : 1)), n(count) {}
    Block(const Block& o) : p((T*)malloc(o.n ? o.n * sizeof(T) : 1)), n(o.n) { if (n) memcpy(p, o.p, n * sizeof(T)); }
    Block& operator=(const Block&) = delete;
    ~Block() { free(p); }
    bool same(const Block& o) const { return n == o.n && (n == 0 || memcmp(p, o.p, n * sizeof(T)) == 0); }
};

// the caller's header: `size` bytes on the heap, holding the first `size` bytes of a chunky_adaptive_state (or, beyond sizeof, kTailByte)
struct Header {
    Block<unsigned char> b;
    explicit Header(size_t size) : b(size) {
        memset(b.p, kTailByte, size);
        if (size >= sizeof(size_t)) memcpy(b.p, &size, sizeof size);
    }
    chunky_adaptive_state* st() { return (chunky_adaptive_state*)b.p; }
    chunky_adaptive_state get() const {  // the members the block holds, the rest zero
        chunky_adaptive_state s;
        memset(&s, 0, sizeof s);
        memcpy(&s, b.p, b.n < sizeof s ? b.n : sizeof s);
        return s;
    }
    void put(const chunky_adaptive_state& s) { memcpy(b.p, &s, b.n < sizeof s ? b.n : sizeof s); }
    bool tail_intact() const {
        for (size_t i = sizeof(chunky_adaptive_state); i < b.n; i++)
            if (b.p[i] != kTailByte) return false;
        return true;
    }
};

struct Run {  // a state: header and arrays, each in its own exact block
    Header h;
    Block<int32_t> count;
    Block<float> mean, stat;
    Block<uint8_t> active;
    Run(size_t size, size_t np) : h(size), count(np), mean(3 * np), stat(2 * np), active(np) {}
};

static std::map<std::string, long long> refused;
static long long accepted = 0, cuts = 0;

// the state is refused with the rule's message, by the check and by _resume, and neither writes anything
static void expect_refused(const char* rule, const char* text, Run& m, const float* one_pass) {
    const Run before(m);
    int rc = chunky_adaptive_state_check(m.h.st(), m.count.p, m.active.p);
    bool ok = rc == CHUNKY_E_INVALID && strstr(chunky_last_error(), text) != nullptr;
    if (ok) {
        rc = chunky_adaptive_host_resume(m.h.st(), one_pass, 1, m.count.p, m.mean.p, m.stat.p, m.active.p);
        ok = rc == CHUNKY_E_INVALID && strstr(chunky_last_error(), text) != nullptr;
    }
    ok = ok && m.h.b.same(before.h.b) && m.count.same(before.count) && m.mean.same(before.mean) && m.stat.same(before.stat) && m.active.same(before.active);
    if (ok) {
        refused[rule] += 1;
    } else if (failures++ < 20) {
        fprintf(stderr, "rule %s: rc %d, \"%s\" (expected CHUNKY_E_INVALID with \"%s\" and nothing written)\n", rule, rc, chunky_last_error(), text);
    }
}

// every rule of adaptive_state_valid broken in turn, each on a copy of the accepted state `r`
static void break_rules(const Run& r, const float* one_pass) {
    const chunky_adaptive_state s0 = r.h.get();
    const size_t np = (size_t)s0.width * s0.height;
    const chunky_adaptive_params& p = s0.params;
    auto with_header = [&](const char* rule, const char* text, auto edit) {
        Run m(r);
        chunky_adaptive_state s = s0;
        edit(s);
        m.h.put(s);
        expect_refused(rule, text, m, one_pass);
    };
    auto with_arrays = [&](const char* rule, const char* text, auto edit) {
        Run m(r);
        edit(m);
        expect_refused(rule, text, m, one_pass);
    };
    // size below the first version: the block is as short as it says
    for (size_t size : {kFirst - 1, kFirst - sizeof(chunky_adaptive_summary), sizeof(size_t)}) {
        Run m(r);
        Header small(size);
        memcpy(small.b.p, m.h.b.p, size);
        memcpy(small.b.p, &size, sizeof size);
        const Block<unsigned char> before(small.b);
        int rc = chunky_adaptive_state_check(small.st(), m.count.p, m.active.p);
        bool ok = rc == CHUNKY_E_INVALID && strstr(chunky_last_error(), "is smaller than the struct");
        rc = chunky_adaptive_host_resume(small.st(), one_pass, 1, m.count.p, m.mean.p, m.stat.p, m.active.p);
        ok = ok && rc == CHUNKY_E_INVALID && strstr(chunky_last_error(), "is smaller than the struct");
        chunky_adaptive_params dp;
        EXPECT(chunky_adaptive_default_params(&dp) == CHUNKY_OK);
        rc = chunky_adaptive_host_begin(s0.width, s0.height, &dp, small.st(), m.count.p, m.mean.p, m.stat.p, m.active.p);
        ok = ok && rc == CHUNKY_E_INVALID && strstr(chunky_last_error(), "is smaller than the struct");
        ok = ok && small.b.same(before) && m.count.same(r.count) && m.active.same(r.active);
        if (ok) refused["size_below_first"] += 1; else EXPECT(!"size below the first version is refused");
    }
    with_header("negative_passes", " passes", [](chunky_adaptive_state& s) { s.passes = -1 - (int)(rnd() % 5); s.summary.passes = s.passes; });
    // last_check: g (the largest grid point <= passes, 0 if none) or, when g == passes, the grid point before it; g + 1 and -1 are neither
    with_header("last_check", "last_check", [&](chunky_adaptive_state& s) { s.last_check = ad_grid_floor(s.passes, p.min_spp, p.check_interval) + 1; });
    with_header("last_check", "last_check", [](chunky_adaptive_state& s) { s.last_check = -1; });
    if (ad_grid_floor(s0.passes, p.min_spp, p.check_interval) > 0 && ad_grid_floor(s0.passes, p.min_spp, p.check_interval) != s0.passes)
        with_header("last_check", "last_check", [&](chunky_adaptive_state& s) {  // off the grid point, the one before it is not allowed
            s.last_check = ad_grid_before(ad_grid_floor(s.passes, p.min_spp, p.check_interval), p.min_spp, p.check_interval);
        });
    with_arrays("active_is_2", "not 0 or 1", [&](Run& m) { m.active.p[rnd() % np] = 2; });
    with_arrays("active_is_2", "not 0 or 1", [&](Run& m) { m.active.p[np - 1] = 255; });
    std::vector<size_t> on, off;
    for (size_t i = 0; i < np; i++) (r.active.p[i] ? on : off).push_back(i);
    if (!on.empty()) {
        with_arrays("active_wrong_count", "is active with count", [&](Run& m) { m.count.p[on[rnd() % on.size()]] = s0.passes + 1; });
        with_arrays("active_wrong_count", "is active with count", [&](Run& m) { m.count.p[on[rnd() % on.size()]] = s0.passes - 1; });
    }
    if (!off.empty()) {
        // 0 and min_spp - 1 are below the grid; min_spp + 1 is off it unless every pass is a grid point
        with_arrays("inactive_off_grid", "is inactive with count", [&](Run& m) { m.count.p[off[rnd() % off.size()]] = 0; });
        with_arrays("inactive_off_grid", "is inactive with count", [&](Run& m) { m.count.p[off[rnd() % off.size()]] = p.min_spp - 1; });
        if (p.check_interval > 1) with_arrays("inactive_off_grid", "is inactive with count", [&](Run& m) { m.count.p[off[rnd() % off.size()]] = p.min_spp + 1; });
        with_arrays("inactive_past_last_check", "is inactive with count", [&](Run& m) { m.count.p[off[rnd() % off.size()]] = s0.last_check + p.check_interval; });
    }
    with_header("state_active", "state.active is", [](chunky_adaptive_state& s) { s.active += 1; });
    with_header("state_active", "state.active is", [](chunky_adaptive_state& s) { s.active -= 1; });
    with_header("summary_passes", "summary.passes", [](chunky_adaptive_state& s) { s.summary.passes += 1; });
    with_header("summary_passes", "summary.passes", [](chunky_adaptive_state& s) { s.summary.passes -= 1; });
    with_header("summary_samples", "summary.samples", [](chunky_adaptive_state& s) { s.summary.samples += 1; });
    with_header("summary_samples", "summary.samples", [](chunky_adaptive_state& s) { s.summary.samples -= 1; });
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    for (float v : {nan, inf, -inf, -1.0f, -0.0f - 1e-30f})
        with_header("params", "threshold must be", [&](chunky_adaptive_state& s) { s.params.threshold = v; });
    for (float v : {nan, inf, -inf, -1.0f, 0.0f})
        with_header("params", "floor must be", [&](chunky_adaptive_state& s) { s.params.floor = v; });
    with_header("params", "min_spp", [](chunky_adaptive_state& s) { s.params.min_spp = 1; });
    with_header("params", "check_interval", [](chunky_adaptive_state& s) { s.params.check_interval = 0; });
    with_header("params", "unknown flags", [](chunky_adaptive_state& s) { s.params.flags = 1u << (rnd() % 32); });
    with_header("params", "params.size", [](chunky_adaptive_state& s) { s.params.size = offsetof(chunky_adaptive_params, flags); });
    with_header("dims", "bad size", [](chunky_adaptive_state& s) { s.width = 0; });
    with_header("dims", "bad size", [](chunky_adaptive_state& s) { s.height = -s.height; });
    with_header("dims", "bad size", [](chunky_adaptive_state& s) { s.width = INT_MAX; s.height = INT_MAX; });
    // a summary no run can have left: the continuation indexes summary.active with summary.checks and counts both members up
    with_header("summary_counts", "summary.rounds", [](chunky_adaptive_state& s) { s.summary.checks = -1 - (int)(rnd() % 70); });
    with_header("summary_counts", "summary.rounds", [](chunky_adaptive_state& s) { s.summary.checks = INT_MAX; });
    with_header("summary_counts", "summary.rounds", [](chunky_adaptive_state& s) { s.summary.rounds = INT_MAX; });
    with_header("summary_counts", "summary.rounds", [](chunky_adaptive_state& s) { s.summary.rounds = -1; });
}

static void expect_accepted(Run& r, size_t size, const float* one_pass) {
    EXPECT(chunky_adaptive_state_check(r.h.st(), r.count.p, r.active.p) == CHUNKY_OK);
    size_t kept = 0;
    memcpy(&kept, r.h.b.p, sizeof kept);
    EXPECT(kept == size && r.h.tail_intact());  // the caller's size survives every call, and so do the bytes this library does not know
    accepted += 1;
    break_rules(r, one_pass);
}

int main() {
    const int images[4][2] = {{1, 1}, {3, 2}, {17, 5}, {16, 16}};  // no neighbour, edges only, an interior, a full tile
    std::vector<size_t> sizes = {kFirst, sizeof(chunky_adaptive_state), sizeof(chunky_adaptive_state) + kTail};
    const int mins[] = {2, 3, 5}, intervals[] = {1, 3, 4}, targets[] = {4, 9, 13};
    long long finished = 0, still_active = 0;
    for (const auto& wh : images) {
        const int width = wh[0], height = wh[1];
        const size_t np = (size_t)width * height;
        for (int mn : mins)
            for (int ci : intervals)
                for (int B : targets) {
                    // samples: a base colour per pixel plus noise of a per-pixel amplitude; a third of the pixels have none and leave at the first check
                    Block<float> samples(3 * np * (size_t)B);
                    std::vector<float> base(3 * np), amp(np);
                    for (size_t i = 0; i < np; i++) {
                        amp[i] = rnd() % 3 == 0 ? 0.0f : rnd01();
                        for (int c = 0; c < 3; c++) base[3 * i + c] = 0.1f + rnd01();
                    }
                    for (int k = 0; k < B; k++)
                        for (size_t i = 0; i < 3 * np; i++) samples.p[3 * np * (size_t)k + i] = base[i] + amp[i / 3] * (rnd01() - 0.5f);
                    chunky_adaptive_params p;
                    EXPECT(chunky_adaptive_default_params(&p) == CHUNKY_OK);
                    p.min_spp = mn;
                    p.check_interval = ci;
                    for (size_t size : sizes)
                        for (int d = 0; d < B; d++) {  // d = 0: the start state straight to B
                            Run r(size, np);
                            EXPECT(chunky_adaptive_host_begin(width, height, &p, r.h.st(), r.count.p, r.mean.p, r.stat.p, r.active.p) == CHUNKY_OK);
                            if (d == 0) expect_accepted(r, size, samples.p);
                            if (d > 0) {
                                Block<float> head(3 * np * (size_t)d);  // exactly the passes of the call
                                memcpy(head.p, samples.p, head.n * sizeof(float));
                                EXPECT(chunky_adaptive_host_resume(r.h.st(), head.p, d, r.count.p, r.mean.p, r.stat.p, r.active.p) == CHUNKY_OK);
                                expect_accepted(r, size, samples.p);
                                cuts += 1;
                            }
                            Block<float> rest(3 * np * (size_t)(B - d));
                            memcpy(rest.p, samples.p + 3 * np * (size_t)d, rest.n * sizeof(float));
                            EXPECT(chunky_adaptive_host_resume(r.h.st(), rest.p, B - d, r.count.p, r.mean.p, r.stat.p, r.active.p) == CHUNKY_OK);
                            expect_accepted(r, size, samples.p);
                            const chunky_adaptive_state s = r.h.get();
                            EXPECT(s.passes == B || s.active == 0);
                            finished += 1;
                            still_active += s.active;
                            // n == 0 and NULL samples: nothing changes
                            const Run before(r);
                            EXPECT(chunky_adaptive_host_resume(r.h.st(), nullptr, 0, r.count.p, r.mean.p, r.stat.p, r.active.p) == CHUNKY_OK);
                            EXPECT(r.h.b.same(before.h.b) && r.count.same(before.count) && r.mean.same(before.mean) && r.stat.same(before.stat) && r.active.same(before.active));
                        }
                }
    }
    printf("{\"images\": %d, \"sizes\": [", (int)(sizeof images / sizeof images[0]));
    for (size_t i = 0; i < sizes.size(); i++) printf("%s%zu", i ? ", " : "", sizes[i]);
    printf("], \"first_version\": %zu, \"sizeof\": %zu, \"states_accepted\": %lld, \"cuts\": %lld, \"runs\": %lld, \"active_at_end\": %lld, \"refused\": {", kFirst,
           sizeof(chunky_adaptive_state), accepted, cuts, finished, still_active);
    bool first = true;
    for (const auto& kv : refused) {
        printf("%s\"%s\": %lld", first ? "" : ", ", kv.first.c_str(), kv.second);
        first = false;
    }
    printf("}, \"failures\": %lld}\n", failures);
    return failures != 0;
}
