// robust_host.hpp — the checks of robust_host.cpp that the device half (capi_robust.hip) shares.  Plain C++: no HIP type.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/chunky_hip.h"

#pragma GCC visibility push(hidden)
// the caller's struct, as far as this library knows it, checked
int robust_params(const char* who, const chunky_robust_params* params, chunky_robust_params* p);
// CHUNKY_E_INVALID for a bucket count the specification does not take
int robust_buckets(const char* who, int n_buckets);
#pragma GCC visibility pop
