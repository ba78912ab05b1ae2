// matte_host.hpp — the checks of matte_host.cpp that the device half (capi_matte.hip) shares.  Plain C++: no HIP type.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/chunky_hip.h"

#pragma GCC visibility push(hidden)  // internal to the library

// the caller's id set, ascending with every value once (what matte_spec.h matte_in_set searches); CHUNKY_E_INVALID for n_set < 0, a
// null set with n_set > 0, or CHUNKY_MATTE_EMPTY in the set
int matte_sorted_set(const char* who, const int32_t* set, int n_set, std::vector<int32_t>* sorted);
// chunky_matte_state_check under the caller's name
int matte_state_valid(const char* who, const int32_t* ids, const int32_t* counts, const int32_t* other, int64_t n_pixels, int32_t passes);

#pragma GCC visibility pop
