// fog_host_fuzz.cpp — the device-free half of the ground-fog layer (csrc/fog_host.cpp: chunky_fog_check, chunky_selftest_plan_fog over
// csrc/launch_plan.cpp) in a stand-alone program, built with AddressSanitizer + UBSan by tests/test_fog_cpu.py: every struct lives in a
// heap block of exactly the size it declares (a read past what the caller promised is a heap overflow), members run over ordinary,
// huge, denormal and non-finite values, and the planner runs over every combination of its inputs' interesting values.
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
    const float vals[] = {0.0f, -0.0f, 1e-45f, 0.04f, 0.5f, 1.0f, 1.5f, 64.0f, -1.0f, 3e38f, -3e38f, inf, -inf, nan};
    const size_t sizes[] = {0, 1, 8, sizeof(chunky_fog) - 4, sizeof(chunky_fog) - 1, sizeof(chunky_fog), sizeof(chunky_fog) + 1, sizeof(chunky_fog) + 16, 4096, 4097};
    long accepted = 0, refused = 0, failures = 0;
    for (size_t size : sizes) {
        // the block holds what the struct declares, and at least the size member itself
        const size_t bytes = size < sizeof(size_t) ? sizeof(size_t) : size;
        for (float density : vals)
            for (float y_min : {0.0f, 10.0f, -inf, nan})
                for (float y_max : {10.0f, 64.0f, inf})
                    for (float c : vals) {
                        unsigned char* block = (unsigned char*)calloc(1, bytes);
                        chunky_fog f;
                        f.size = size;
                        f.density = density, f.y_min = y_min, f.y_max = y_max;
                        f.color[0] = 0.5f, f.color[1] = c, f.color[2] = 1.0f;
                        memcpy(block, &f, bytes < sizeof f ? bytes : sizeof f);
                        const int rc = chunky_fog_check((const chunky_fog*)block);
                        const bool fits = size >= sizeof(chunky_fog) && size <= 4096;
                        const bool fine = std::isfinite(density) && density >= 0 && std::isfinite(y_min) && std::isfinite(y_max) && y_min < y_max && c >= 0 && c <= 1;
                        if (rc == CHUNKY_OK) accepted++;
                        else refused++;
                        if ((rc == CHUNKY_OK) != (fits && fine) || (rc != CHUNKY_OK && rc != CHUNKY_E_INVALID)) failures++;
                        free(block);
                    }
    }
    if (chunky_fog_check(nullptr) != CHUNKY_OK) failures++;
    // a newer caller's struct with a member this library does not know set
    {
        const size_t size = sizeof(chunky_fog) + 8;
        unsigned char* block = (unsigned char*)calloc(1, size);
        chunky_fog f{size, 0.1f, 0.0f, 64.0f, {1.0f, 1.0f, 1.0f}};
        memcpy(block, &f, sizeof f);
        if (chunky_fog_check((const chunky_fog*)block) != CHUNKY_OK) failures++;
        block[size - 1] = 1;
        if (chunky_fog_check((const chunky_fog*)block) != CHUNKY_E_INVALID) failures++;
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
                                for (int levels : {0, 1, 2, 3, 4, 5, 6}) rows.insert(rows.end(), {word, proj, max_depth, wide, bvh, records, biome, levels});
    const int64_t n = (int64_t)rows.size() / 8;
    std::vector<int32_t> out(rows.size());
    std::vector<char> text((size_t)n * 256);
    long planned = 0;
    if (chunky_selftest_plan_fog(rows.data(), n, out.data(), text.data()) != CHUNKY_OK) failures++;
    for (int64_t i = 0; i < n; i++) {
        const int32_t* o = &out[8 * i];
        const bool refusal = o[1] != 0;
        if (refusal != (text[256 * i] != 0)) failures++;
        if (!refusal && o[0] == 0) {
            planned++;
            const bool bvh = o[4] != 0;
            if (!(o[2] == 17 || o[2] == 18 || o[2] == -1) || o[3] != (bvh ? 16 : 32) || o[5] != 1 || o[6] != 0) failures++;
        }
    }
    if (chunky_selftest_plan_fog(nullptr, 1, out.data(), nullptr) != CHUNKY_E_INVALID) failures++;
    printf("{\"accepted\": %ld, \"refused\": %ld, \"planned\": %ld, \"plans\": %lld, \"failures\": %ld}\n", accepted, refused, planned, (long long)n, failures);
    return failures ? 1 : 0;
}
