// denoise_host.hpp — the checks of denoise_host.cpp that the device half (capi_denoise.hip) shares.  Plain C++: no HIP type.
#pragma once
#include "../../include/chunky_hip.h"
#include "denoise_spec.h"

// chunky_denoise_params.flags bits 8-9 (include/chunky_hip.h): capi_denoise.hip holds them to kernels.hpp's kDenoiseGather / kDenoisePacked
constexpr int kDenoiseFormGather = 0, kDenoiseFormPacked = 1;

#pragma GCC visibility push(hidden)
// the caller's struct, as far as this library knows it, turned into the per-iteration coefficients and the kernel form
int denoise_params(const char* who, const chunky_denoise_params* params, DnCoeffs* K, int* form);
int denoise_images(const char* who, int width, int height, const void* color, const void* albedo, const void* normal, const void* out);
#pragma GCC visibility pop
