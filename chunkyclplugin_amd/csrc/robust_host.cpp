// robust_host.cpp — firefly-robust accumulation on the host: the specification (robust_spec.h) as loops over an image, and the checks
// of a caller's params.  Plain C++: no device code, no HIP type.
#include "robust_host.hpp"

#include <cmath>
#include <cstring>

#include "capi_error.hpp"
#include "robust_spec.h"

static_assert(CHUNKY_ROBUST_MEAN == RB_MODE_MEAN && CHUNKY_ROBUST_MEDIAN == RB_MODE_MEDIAN && CHUNKY_ROBUST_GINI == RB_MODE_GINI, "robust_spec.h");
static_assert(CHUNKY_ROBUST_MIN_BUCKETS == RB_MIN_BUCKETS && CHUNKY_ROBUST_MAX_BUCKETS == RB_MAX_BUCKETS, "robust_spec.h");

extern "C" int chunky_robust_default_params(chunky_robust_params* p) {
    if (!p) return fail(CHUNKY_E_INVALID, "robust_default_params: NULL params");
    p->size = (int32_t)sizeof(chunky_robust_params);
    p->mode = CHUNKY_ROBUST_GINI;
    p->gain = 1.0f;
    return CHUNKY_OK;
}

int robust_params(const char* who, const chunky_robust_params* params, chunky_robust_params* p) {
    if (!params) return fail(CHUNKY_E_INVALID, "%s: NULL params", who);
    constexpr size_t kFirst = offsetof(chunky_robust_params, gain) + sizeof(float);  // the first version of the struct
    if (params->size < 0 || !take_versioned(params, (size_t)params->size, kFirst, p))
        return fail(CHUNKY_E_INVALID, "%s: params.size %d is smaller than the struct (%zu)", who, params->size, kFirst);
    if (p->mode != CHUNKY_ROBUST_MEAN && p->mode != CHUNKY_ROBUST_MEDIAN && p->mode != CHUNKY_ROBUST_GINI)
        return fail(CHUNKY_E_INVALID, "%s: unknown mode %d", who, p->mode);
    if (!std::isfinite(p->gain) || p->gain < 0.0f) return fail(CHUNKY_E_INVALID, "%s: gain must be finite and >= 0, got %g", who, (double)p->gain);
    return CHUNKY_OK;
}

int robust_buckets(const char* who, int n_buckets) {
    if (!rb_buckets_ok(n_buckets))
        return fail(CHUNKY_E_INVALID, "%s: %d buckets: the count must be odd and in %d .. %d", who, n_buckets, RB_MIN_BUCKETS, RB_MAX_BUCKETS);
    return CHUNKY_OK;
}

// CALL(M) for the run-time bucket count m (checked by robust_buckets before): a switch over the instantiations
#define ROBUST_DISPATCH(m, CALL) \
    switch (m) {                 \
        case 3: CALL(3); break;  \
        case 5: CALL(5); break;  \
        case 7: CALL(7); break;  \
        case 9: CALL(9); break;  \
        case 11: CALL(11); break; \
        case 13: CALL(13); break; \
        default: CALL(15); break; \
    }

extern "C" int chunky_robust_host(int width, int height, const float* samples, int n, int n_buckets, int first_index, float* buckets) {
    if (int rc = robust_buckets("robust_host", n_buckets)) return rc;
    if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 16) return fail(CHUNKY_E_INVALID, "robust_host: bad size %dx%d", width, height);
    if (n < 0 || first_index < 0 || (int64_t)first_index + n > INT32_MAX) return fail(CHUNKY_E_INVALID, "robust_host: samples %d .. %d + %d", first_index, first_index, n);
    if (!buckets || (n > 0 && !samples)) return fail(CHUNKY_E_INVALID, "robust_host: NULL argument");
    const size_t plane = 3 * (size_t)width * height;
    for (int k = 0; k < n; k++) {
        const int j = first_index + k;
        float* b = buckets + (size_t)(j % n_buckets) * plane;
        const float* s = samples + (size_t)k * plane;
        for (size_t i = 0; i < plane; i++) b[i] = ad_mean(b[i], s[i], j / n_buckets);
    }
    return CHUNKY_OK;
}

template <int M>
static void resolve_all(int64_t n_pixels, const float* buckets, int mode, float gain, float* out, uint8_t* trim) {
    const size_t plane = 3 * (size_t)n_pixels;
    for (int64_t p = 0; p < n_pixels; p++) {
        int most = 0;
        for (int c = 0; c < 3; c++) {
            float x[M];
            for (int k = 0; k < M; k++) x[k] = buckets[(size_t)k * plane + 3 * (size_t)p + c];
            int t;
            out[3 * (size_t)p + c] = rb_resolve<M>(x, mode, gain, &t);
            most = t > most ? t : most;
        }
        if (trim) trim[p] = (uint8_t)most;
    }
}

extern "C" int chunky_robust_host_resolve(int n_buckets, int64_t n_pixels, const float* buckets, const chunky_robust_params* params, float* out,
                                          uint8_t* trim) {
    chunky_robust_params p;
    if (int rc = robust_params("robust_host_resolve", params, &p)) return rc;
    if (int rc = robust_buckets("robust_host_resolve", n_buckets)) return rc;
    if (n_pixels <= 0 || n_pixels > INT32_MAX / 16) return fail(CHUNKY_E_INVALID, "robust_host_resolve: %lld pixels", (long long)n_pixels);
    if (!buckets || !out) return fail(CHUNKY_E_INVALID, "robust_host_resolve: NULL argument");
#define ROBUST_RESOLVE(M) resolve_all<M>(n_pixels, buckets, p.mode, p.gain, out, trim)
    ROBUST_DISPATCH(n_buckets, ROBUST_RESOLVE)
#undef ROBUST_RESOLVE
    return CHUNKY_OK;
}
