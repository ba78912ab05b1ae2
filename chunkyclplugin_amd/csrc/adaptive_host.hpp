// adaptive_host.hpp — the checks of adaptive_host.cpp that the device half (capi_adaptive.hip) shares.  Plain C++: no HIP type.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/chunky_hip.h"

constexpr size_t kAdaptiveStateFirst = offsetof(chunky_adaptive_state, summary) + sizeof(chunky_adaptive_summary);  // the first version of the struct

#pragma GCC visibility push(hidden)
// the caller's struct, as far as this library knows it, checked against the pass count
int adaptive_params(const char* who, const chunky_adaptive_params* params, int max_spp, chunky_adaptive_params* p);
void adaptive_empty_state(int width, int height, const chunky_adaptive_params& p, chunky_adaptive_state* s);
int adaptive_dims(const char* who, int width, int height);
// chunky_adaptive_state_check; *s receives the state as far as this library knows the caller's struct, its params checked
int adaptive_state_valid(const char* who, const chunky_adaptive_state* st, const int32_t* count, const uint8_t* active, chunky_adaptive_state* s);
// the caller's hooks, as far as its struct holds them (as chunky_render_run_ex reads chunky_run_callbacks)
int adaptive_callbacks(const char* who, const chunky_adaptive_callbacks* callbacks, chunky_adaptive_callbacks* cb);
bool same_adaptive_params(const chunky_adaptive_params& a, const chunky_adaptive_params& b);
#pragma GCC visibility pop
