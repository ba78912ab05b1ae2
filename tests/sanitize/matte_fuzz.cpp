// matte_fuzz — the host half of the ID mattes (csrc/matte_host.cpp: chunky_matte_host_fold, _ranks, _extract, chunky_matte_state_check)
// in a stand-alone program under AddressSanitizer + UBSan.  Links matte_host.cpp and capi_error.cpp and nothing else.  Every array
// lives in a heap block of exactly its size, so a read or write past a plane is caught.  Driven with: states a fold leaves (against
// a fold written out here with arrays), hostile states (random words, INT32_MIN / INT32_MAX counts and ids, holes, duplicates),
// hostile sets (unsorted, duplicates, INT32_MIN, 65 536 ids), null pointers and sizes of 0 and below.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/chunky_hip.h"

static long long failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

struct State {
    int64_t n;
    std::vector<int32_t> ids, counts, other;
    explicit State(int64_t n_) : n(n_), ids(6 * (size_t)n_, 0), counts(6 * (size_t)n_, 0), other((size_t)n_, 0) {}
};

// the three rules with arrays and loops
static void fold_plain(State* s, const std::vector<int32_t>& samples, int n_passes) {
    for (int k = 0; k < n_passes; k++)
        for (int64_t i = 0; i < s->n; i++) {
            const int32_t v = samples[(size_t)k * s->n + i];
            int slot = -1;
            for (int t = 0; t < 6 && slot < 0; t++)
                if (s->counts[(size_t)t * s->n + i] > 0 && s->ids[(size_t)t * s->n + i] == v) slot = t;
            for (int t = 0; t < 6 && slot < 0; t++)
                if (s->counts[(size_t)t * s->n + i] == 0) slot = t;
            if (slot < 0) {
                s->other[(size_t)i] += 1;
            } else {
                s->ids[(size_t)slot * s->n + i] = v;
                s->counts[(size_t)slot * s->n + i] += 1;
            }
        }
}

static long long folds = 0, accepted = 0, refused = 0, extracts = 0;

static void valid_runs() {
    const int64_t sizes[] = {1, 2, 7, 64, 257};
    const int alphabets[] = {1, 3, 6, 7, 40};
    for (int64_t n : sizes)
        for (int alphabet : alphabets)
            for (int n_passes : {0, 1, 5, 97}) {
                std::vector<int32_t> samples((size_t)n * n_passes);
                for (auto& v : samples) v = (int32_t)(rnd() % alphabet) - 3;  // the entity ids and the sky among them
                State a(n), b(n), c(n);
                EXPECT(chunky_matte_host_fold(samples.data(), n_passes, n, a.ids.data(), a.counts.data(), a.other.data()) == CHUNKY_OK);
                fold_plain(&b, samples, n_passes);
                EXPECT(a.ids == b.ids && a.counts == b.counts && a.other == b.other);
                folds++;
                // cut in two
                const int cut = n_passes / 3;
                EXPECT(chunky_matte_host_fold(samples.data(), cut, n, c.ids.data(), c.counts.data(), c.other.data()) == CHUNKY_OK);
                EXPECT(chunky_matte_host_fold(samples.data() + (size_t)cut * n, n_passes - cut, n, c.ids.data(), c.counts.data(), c.other.data()) == CHUNKY_OK);
                EXPECT(a.ids == c.ids && a.counts == c.counts && a.other == c.other);
                EXPECT(chunky_matte_state_check(a.ids.data(), a.counts.data(), a.other.data(), n, n_passes) == CHUNKY_OK);
                accepted++;
                if (n_passes == 0) continue;
                std::vector<int32_t> r_ids(6 * (size_t)n, 77);
                std::vector<float> r_cov(6 * (size_t)n, -1.0f), mask((size_t)n, -1.0f);
                EXPECT(chunky_matte_host_ranks(a.ids.data(), a.counts.data(), n, n_passes, r_ids.data(), r_cov.data()) == CHUNKY_OK);
                for (int64_t i = 0; i < n; i++) {
                    long long sum = 0;
                    for (int t = 0; t < 6; t++) {
                        const float cov = r_cov[(size_t)t * n + i];
                        EXPECT(cov >= 0.0f && cov <= 1.0f);
                        if (t > 0) EXPECT(cov <= r_cov[(size_t)(t - 1) * n + i]);
                        EXPECT((cov == 0.0f) == (r_ids[(size_t)t * n + i] == CHUNKY_MATTE_EMPTY));
                        sum += a.counts[(size_t)t * n + i];
                    }
                    EXPECT(sum + a.other[(size_t)i] == n_passes);
                }
                // the set of every id there is: what the slots hold
                std::vector<int32_t> set;
                for (int v = -3; v < alphabet - 3; v++) set.push_back(v), set.push_back(v);
                EXPECT(chunky_matte_host_extract(a.ids.data(), a.counts.data(), n, n_passes, set.data(), (int)set.size(), mask.data()) == CHUNKY_OK);
                for (int64_t i = 0; i < n; i++) EXPECT(mask[(size_t)i] == (float)(n_passes - a.other[(size_t)i]) / (float)n_passes);
                EXPECT(chunky_matte_host_extract(a.ids.data(), a.counts.data(), n, n_passes, nullptr, 0, mask.data()) == CHUNKY_OK);
                for (int64_t i = 0; i < n; i++) EXPECT(mask[(size_t)i] == 0.0f);
                extracts += 2;
            }
}

static int32_t hostile_word() {
    switch (rnd() % 8) {
        case 0: return INT32_MIN;
        case 1: return INT32_MAX;
        case 2: return -1;
        case 3: return 0;
        case 4: return (int32_t)rnd();
        default: return (int32_t)(rnd() % 5);
    }
}

// states nobody folded: every call either refuses them or works on them inside the arrays and inside int32
static void hostile_states() {
    for (int round = 0; round < 4000; round++) {
        const int64_t n = 1 + rnd() % 9;
        State s(n);
        for (auto& v : s.ids) v = hostile_word();
        for (auto& v : s.counts) v = hostile_word();
        for (auto& v : s.other) v = hostile_word();
        const int32_t passes = (rnd() & 1) ? hostile_word() : (int32_t)(rnd() % 12);
        const int rc = chunky_matte_state_check(s.ids.data(), s.counts.data(), s.other.data(), n, passes);
        EXPECT(rc == CHUNKY_OK || rc == CHUNKY_E_INVALID);
        if (rc == CHUNKY_OK) {
            accepted++;
            for (int64_t i = 0; i < n; i++) {  // what the check promises
                long long sum = s.other[(size_t)i];
                bool empty_seen = false;
                for (int t = 0; t < 6; t++) {
                    const int32_t c = s.counts[(size_t)t * n + i];
                    EXPECT(c >= 0);
                    if (c == 0) empty_seen = true;
                    else EXPECT(!empty_seen && s.ids[(size_t)t * n + i] != CHUNKY_MATTE_EMPTY);
                    sum += c;
                }
                EXPECT(sum == 0 || sum == passes);
            }
        } else {
            refused++;
        }
        std::vector<int32_t> r_ids(6 * (size_t)n), set(1 + rnd() % 5);
        std::vector<float> r_cov(6 * (size_t)n), mask((size_t)n);
        for (auto& v : set) v = hostile_word();
        int rc2 = chunky_matte_host_ranks(s.ids.data(), s.counts.data(), n, passes, r_ids.data(), r_cov.data());
        EXPECT(rc2 == CHUNKY_OK || rc2 == CHUNKY_E_INVALID);
        if (rc == CHUNKY_OK && passes > 0) EXPECT(rc2 == CHUNKY_OK);
        rc2 = chunky_matte_host_extract(s.ids.data(), s.counts.data(), n, passes, set.data(), (int)set.size(), mask.data());
        EXPECT(rc2 == CHUNKY_OK || rc2 == CHUNKY_E_INVALID);
        bool empty_in_set = false;
        for (int32_t v : set) empty_in_set |= v == CHUNKY_MATTE_EMPTY;
        if (empty_in_set) EXPECT(rc2 == CHUNKY_E_INVALID);
        const int n_passes = (int)(rnd() % 4);
        std::vector<int32_t> samples((size_t)n * n_passes);
        for (auto& v : samples) v = hostile_word();
        State before = s;
        rc2 = chunky_matte_host_fold(samples.data(), n_passes, n, s.ids.data(), s.counts.data(), s.other.data());
        EXPECT(rc2 == CHUNKY_OK || rc2 == CHUNKY_E_INVALID);
        if (rc2 != CHUNKY_OK) EXPECT(before.ids == s.ids && before.counts == s.counts && before.other == s.other);  // refused: nothing written
        else folds++;
    }
    // at the edge of int32: INT32_MAX - 1 samples take one more pass and then no more
    State e(1);
    e.ids[0] = 4;
    e.counts[0] = INT32_MAX - 1;
    const int32_t four = 4;
    EXPECT(chunky_matte_host_fold(&four, 1, 1, e.ids.data(), e.counts.data(), e.other.data()) == CHUNKY_OK && e.counts[0] == INT32_MAX);
    EXPECT(chunky_matte_host_fold(&four, 1, 1, e.ids.data(), e.counts.data(), e.other.data()) == CHUNKY_E_INVALID && e.counts[0] == INT32_MAX);
    EXPECT(chunky_matte_state_check(e.ids.data(), e.counts.data(), e.other.data(), 1, INT32_MAX) == CHUNKY_OK);
    int32_t rid[6];
    float rcov[6], m = -1;
    EXPECT(chunky_matte_host_ranks(e.ids.data(), e.counts.data(), 1, INT32_MAX, rid, rcov) == CHUNKY_OK && rid[0] == 4 && rcov[0] == 1.0f && rid[1] == CHUNKY_MATTE_EMPTY);
    EXPECT(chunky_matte_host_extract(e.ids.data(), e.counts.data(), 1, INT32_MAX, &four, 1, &m) == CHUNKY_OK && m == 1.0f);
}

static void hostile_arguments() {
    State s(3);
    int32_t sample[3] = {1, 2, 3};
    float f[18];
    int32_t o[18];
    EXPECT(chunky_matte_host_fold(nullptr, 1, 3, s.ids.data(), s.counts.data(), s.other.data()) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(nullptr, 0, 3, s.ids.data(), s.counts.data(), s.other.data()) == CHUNKY_OK);
    EXPECT(chunky_matte_host_fold(sample, -1, 3, s.ids.data(), s.counts.data(), s.other.data()) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(sample, 1, 0, s.ids.data(), s.counts.data(), s.other.data()) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(sample, 1, -5, s.ids.data(), s.counts.data(), s.other.data()) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(sample, 1, 3, nullptr, s.counts.data(), s.other.data()) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(sample, 1, 3, s.ids.data(), nullptr, s.other.data()) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(sample, 1, 3, s.ids.data(), s.counts.data(), nullptr) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_fold(sample, 1, 3, s.ids.data(), s.counts.data(), s.other.data()) == CHUNKY_OK);
    EXPECT(chunky_matte_host_ranks(nullptr, s.counts.data(), 3, 1, o, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_ranks(s.ids.data(), s.counts.data(), 3, 1, nullptr, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_ranks(s.ids.data(), s.counts.data(), 3, 1, o, nullptr) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_ranks(s.ids.data(), s.counts.data(), -3, 1, o, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_ranks(s.ids.data(), s.counts.data(), 3, 0, o, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_ranks(s.ids.data(), s.counts.data(), 3, INT32_MIN, o, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 1, sample, -1, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 1, sample, INT32_MIN, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 1, nullptr, 2, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 1, sample, 3, nullptr) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 0, sample, 3, f) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_state_check(nullptr, s.counts.data(), s.other.data(), 3, 1) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_state_check(s.ids.data(), nullptr, s.other.data(), 3, 1) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_state_check(s.ids.data(), s.counts.data(), nullptr, 3, 1) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_state_check(s.ids.data(), s.counts.data(), s.other.data(), 0, 1) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_state_check(s.ids.data(), s.counts.data(), s.other.data(), 3, -1) == CHUNKY_E_INVALID);
    EXPECT(chunky_matte_state_check(s.ids.data(), s.counts.data(), s.other.data(), 3, 1) == CHUNKY_OK);
    // a set of 65 536 ids, descending, every one twice over: the pixel's three ids are in it
    std::vector<int32_t> big;
    for (int v = 65535; v >= 0; v--) big.push_back(v - 100);
    for (int v = 0; v < 65536; v++) big.push_back(v - 100);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 1, big.data(), (int)big.size(), f) == CHUNKY_OK && f[0] == 1.0f && f[1] == 1.0f && f[2] == 1.0f);
    big.push_back(CHUNKY_MATTE_EMPTY);
    EXPECT(chunky_matte_host_extract(s.ids.data(), s.counts.data(), 3, 1, big.data(), (int)big.size(), f) == CHUNKY_E_INVALID);
    extracts += 2;
}

int main() {
    valid_runs();
    hostile_states();
    hostile_arguments();
    printf("{\"failures\": %lld, \"folds\": %lld, \"accepted\": %lld, \"refused\": %lld, \"extracts\": %lld}\n", failures, folds, accepted, refused, extracts);
    return failures ? 1 : 0;
}
