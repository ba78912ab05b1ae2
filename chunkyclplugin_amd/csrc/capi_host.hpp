// capi_host.hpp — what capi_host.cpp shares with the files that talk to the device.  Plain C++: no HIP type.
#pragma once
#include <cstdint>

namespace {
struct JavaRandom {  // java.util.Random: 48-bit LCG, nextInt() = top 32 bits
    uint64_t s;
    explicit JavaRandom(int64_t seed) : s(((uint64_t)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1)) {}
    int32_t next_int() {
        s = (s * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int32_t)(int64_t)(s >> 16);
    }
};
}  // namespace

#pragma GCC visibility push(hidden)
int check_ints(const int32_t* p, int64_t n, const char* what);
bool is_projected_type(int type);
int check_projected(const char* who, int type, const float* s, int64_t n, int height);
int check_lens(const char* who, float aperture, float focus);
const float* gamma_thresholds();
#pragma GCC visibility pop
