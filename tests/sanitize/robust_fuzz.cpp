// robust_fuzz.cpp — the host half of firefly-robust accumulation (csrc/robust_host.cpp over csrc/robust_spec.h) under AddressSanitizer +
// UBSan, through its entry points (chunky_robust_default_params, chunky_robust_host, chunky_robust_host_resolve).  Links
// robust_host.cpp and capi_error.cpp and nothing else.  Every array lives in a heap block of exactly the size the call may touch, so a
// read or write one element past it is reported; the values include NaN, the infinities, -0, 1e30, 3e38 and denormals, so the
// float-to-int conversion of the trim sees everything it must survive.  Checked beside the sanitizers' own findings: the trim is in
// 0 .. h and MEAN / MEDIAN force it; a fold in two parts equals the fold in one; refused calls write nothing.
// Prints one JSON line; exit status 0 iff no check failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/chunky_hip.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            failures++;                                                    \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);             \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static float odd_value(uint32_t r) {
    static const float special[] = {0.0f, -0.0f, 1e30f, 3e38f, -3e38f, 1e-45f, 1e-41f, -1e-40f, 1e4f, 0.5f, 0.5f, 0.25f};
    switch (r % 16) {
        case 0: return NAN;
        case 1: return INFINITY;
        case 2: return -INFINITY;
        default: break;
    }
    if (r % 16 < 8) return special[(r >> 4) % (sizeof special / sizeof *special)];
    return (float)((r >> 8) % 4096) / 1024.0f;
}

int main() {
    long folds = 0, resolves = 0, refused = 0;
    chunky_robust_params def;
    def.size = 0;
    CHECK(chunky_robust_default_params(&def) == CHUNKY_OK && def.size == (int32_t)sizeof def && def.mode == CHUNKY_ROBUST_GINI && def.gain == 1.0f);
    CHECK(chunky_robust_default_params(nullptr) == CHUNKY_E_INVALID);
    const int sizes[][2] = {{1, 1}, {3, 2}, {17, 5}, {16, 16}};
    const int modes[] = {CHUNKY_ROBUST_MEAN, CHUNKY_ROBUST_MEDIAN, CHUNKY_ROBUST_GINI};
    const float gains[] = {0.0f, 0.5f, 1.0f, 3.7f, 1e30f, 3e38f, 1e-45f};
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        const size_t np = (size_t)w * h, plane = 3 * np;
        for (int M = 3; M <= 15; M += 2) {
            for (int n : {0, 1, M - 1, M, 2 * M + 3, 47}) {
                for (int first : {0, 7, INT32_MAX - 47}) {
                    for (int wild = 0; wild < 2; wild++) {  // ordinary values, then the odd ones
                        std::unique_ptr<float[]> s(new float[plane * (size_t)n + (n == 0)]);
                        for (size_t i = 0; i < plane * (size_t)n; i++) s[i] = wild ? odd_value(rnd()) : (float)(rnd() % 4096) / 1024.0f;
                        std::unique_ptr<float[]> b(new float[plane * M]()), b2(new float[plane * M]());
                        CHECK(chunky_robust_host(w, h, s.get(), n, M, first, b.get()) == CHUNKY_OK);
                        folds++;
                        const int cut = n / 3;  // in two parts
                        CHECK(chunky_robust_host(w, h, s.get(), cut, M, first, b2.get()) == CHUNKY_OK);
                        CHECK(chunky_robust_host(w, h, s.get() + plane * (size_t)cut, n - cut, M, first + cut, b2.get()) == CHUNKY_OK);
                        CHECK(memcmp(b.get(), b2.get(), plane * M * sizeof(float)) == 0);
                        std::unique_ptr<float[]> out(new float[plane]);
                        std::unique_ptr<uint8_t[]> trim(new uint8_t[np]);
                        for (int mode : modes)
                            for (float gain : gains) {
                                chunky_robust_params p = def;
                                p.mode = mode;
                                p.gain = gain;
                                CHECK(chunky_robust_host_resolve(M, (int64_t)np, b.get(), &p, out.get(), trim.get()) == CHUNKY_OK);
                                resolves++;
                                const int hh = (M - 1) / 2;
                                for (size_t i = 0; i < np; i++) {
                                    CHECK(trim[i] <= hh);
                                    if (mode == CHUNKY_ROBUST_MEAN || (mode == CHUNKY_ROBUST_GINI && gain == 0.0f)) CHECK(trim[i] == 0);
                                    if (mode == CHUNKY_ROBUST_MEDIAN) CHECK(trim[i] == hh);
                                }
                                if (mode == CHUNKY_ROBUST_GINI && gain == 1.0f)  // without the trim map: nothing else changes
                                {
                                    std::unique_ptr<float[]> out2(new float[plane]);
                                    CHECK(chunky_robust_host_resolve(M, (int64_t)np, b.get(), &p, out2.get(), nullptr) == CHUNKY_OK);
                                    CHECK(memcmp(out.get(), out2.get(), plane * sizeof(float)) == 0);
                                }
                            }
                    }
                }
            }
        }
        // refused calls write nothing
        std::unique_ptr<float[]> b(new float[plane * 3]()), s(new float[plane]()), out(new float[plane]());
        std::vector<float> zero(plane * 3, 0.0f);
        for (int M : {0, 1, 2, 4, 16, 17, -3}) {
            CHECK(chunky_robust_host(w, h, s.get(), 1, M, 0, b.get()) == CHUNKY_E_INVALID);
            CHECK(chunky_robust_host_resolve(M, (int64_t)np, b.get(), &def, out.get(), nullptr) == CHUNKY_E_INVALID);
            refused += 2;
        }
        CHECK(chunky_robust_host(w, h, s.get(), 1, 3, INT32_MAX, b.get()) == CHUNKY_E_INVALID);
        CHECK(chunky_robust_host(w, h, nullptr, 1, 3, 0, b.get()) == CHUNKY_E_INVALID);
        CHECK(chunky_robust_host(w, h, s.get(), 1, 3, 0, nullptr) == CHUNKY_E_INVALID);
        chunky_robust_params p = def;
        p.gain = NAN;
        CHECK(chunky_robust_host_resolve(3, (int64_t)np, b.get(), &p, out.get(), nullptr) == CHUNKY_E_INVALID);
        p = def;
        p.mode = 7;
        CHECK(chunky_robust_host_resolve(3, (int64_t)np, b.get(), &p, out.get(), nullptr) == CHUNKY_E_INVALID);
        p = def;
        p.size = 8;
        CHECK(chunky_robust_host_resolve(3, (int64_t)np, b.get(), &p, out.get(), nullptr) == CHUNKY_E_INVALID);
        p.size = -12;
        CHECK(chunky_robust_host_resolve(3, (int64_t)np, b.get(), &p, out.get(), nullptr) == CHUNKY_E_INVALID);
        refused += 7;
        CHECK(memcmp(b.get(), zero.data(), plane * 3 * sizeof(float)) == 0 && memcmp(out.get(), zero.data(), plane * sizeof(float)) == 0);
    }
    printf("{\"failures\": %d, \"folds\": %ld, \"resolves\": %ld, \"refused\": %ld}\n", failures, folds, resolves, refused);
    return failures ? 1 : 0;
}
