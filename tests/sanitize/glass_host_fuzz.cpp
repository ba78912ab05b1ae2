// glass_host_fuzz.cpp — the device-free half of translucent blocks (csrc/glass_host.cpp: chunky_translucency_check,
// chunky_selftest_plan_glass over csrc/launch_plan.cpp) in a stand-alone program, built with AddressSanitizer + UBSan by
// tests/test_glass_cpu.py: every struct lives in a heap block of exactly the size it declares (a read past what the caller promised is a
// heap overflow), members run over ordinary, huge, denormal and non-finite values, and the planner runs over every combination of its
// inputs' interesting values.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/chunky_hip.h"

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float alphas[] = {0.0f, -0.0f, 1e-45f, 0.04f, 0.5f, 0.99f, 1.0f, 1.0000001f, 1.5f, -1.0f, 3e38f, -3e38f, inf, -inf, nan};
    const int32_t caps[] = {INT32_MIN, -1, 0, 1, 2, 8, 31, 32, 255, INT32_MAX};
    const size_t S = sizeof(chunky_translucency);
    const size_t sizes[] = {0, 1, 8, S - 4, S - 1, S, S + 1, S + 16, 4096, 4097};
    long accepted = 0, refused = 0, failures = 0;
    for (size_t size : sizes) {
        // the block holds what the struct declares, and at least the size member itself
        const size_t bytes = size < sizeof(size_t) ? sizeof(size_t) : size;
        for (float a : alphas)
            for (int32_t cap : caps) {
                unsigned char* block = (unsigned char*)calloc(1, bytes);
                chunky_translucency t;
                memset(&t, 0, sizeof t);
                t.size = size;
                t.opaque_alpha = a, t.max_crossings = cap;
                memcpy(block, &t, bytes < sizeof t ? bytes : sizeof t);
                const int rc = chunky_translucency_check((const chunky_translucency*)block);
                const bool fits = size >= S && size <= 4096;
                const bool fine = a > 0.0f && a <= 1.0f && cap >= 1 && cap <= 31;
                if (rc == CHUNKY_OK) accepted++;
                else refused++;
                if ((rc == CHUNKY_OK) != (fits && fine) || (rc != CHUNKY_OK && rc != CHUNKY_E_INVALID)) failures++;
                free(block);
            }
    }
    if (chunky_translucency_check(nullptr) != CHUNKY_OK) failures++;
    // a newer caller's struct with a member this library does not know set
    {
        const size_t size = S + 8;
        unsigned char* block = (unsigned char*)calloc(1, size);
        chunky_translucency t;
        memset(&t, 0, sizeof t);
        t.size = size, t.opaque_alpha = 0.99f, t.max_crossings = 8;
        memcpy(block, &t, sizeof t);
        if (chunky_translucency_check((const chunky_translucency*)block) != CHUNKY_OK) failures++;
        block[size - 1] = 1;
        if (chunky_translucency_check((const chunky_translucency*)block) != CHUNKY_E_INVALID) failures++;
        free(block);
    }
    // the planner: every combination; a plan is named exactly when nothing is refused, and then it is one of the six instantiations
    std::vector<int32_t> rows;
    for (int word : {0, 1, 2, 4, 8, 16, 64, 128, 256, 512, 0x3FF})
        for (int proj : {-1, 0, 1, 5, 8})
            for (int max_depth : {1, 5, 254, 255, 100000})
                for (int wide : {0, 1})
                    for (int bvh : {0, 1})
                        for (int records : {0, 1})
                            for (int biome : {0, 1})
                                for (int levels : {0, 1, 2, 3, 4, 5, 6})
                                    for (int fog : {0, 1}) rows.insert(rows.end(), {word, proj, max_depth, wide, bvh, records, biome, levels, fog});
    const int64_t n = (int64_t)rows.size() / 9;
    std::vector<int32_t> out((size_t)n * 8);
    std::vector<char> text((size_t)n * 256);
    long planned = 0;
    if (chunky_selftest_plan_glass(rows.data(), n, out.data(), text.data()) != CHUNKY_OK) failures++;
    for (int64_t i = 0; i < n; i++) {
        const int32_t* o = &out[8 * i];
        const bool refusal = o[1] != 0;
        if (refusal != (text[256 * i] != 0)) failures++;
        if (rows[9 * i + 8] && o[1] != 1) failures++;  // a fog layer is refused first, whatever else
        if (!refusal && o[0] == 0) {
            planned++;
            const bool bvh = o[4] != 0;
            if (!(o[2] == 17 || o[2] == 18 || o[2] == -1) || o[3] != (bvh ? 16 : 32) || o[5] != 1 || o[6] != 0 || o[7] != 12) failures++;
        }
    }
    if (chunky_selftest_plan_glass(nullptr, 1, out.data(), nullptr) != CHUNKY_E_INVALID) failures++;
    printf("{\"accepted\": %ld, \"refused\": %ld, \"planned\": %ld, \"plans\": %lld, \"failures\": %ld}\n", accepted, refused, planned, (long long)n, failures);
    return failures ? 1 : 0;
}
