// denoise_host.cpp — the denoiser on the host: the specification loop (denoise_spec.h) and the checks of a caller's params and images.
// Plain C++: no device code, no HIP type.
#include "denoise_host.hpp"

#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "capi_error.hpp"

static_assert(CHUNKY_DENOISE_KERNEL_MASK >> CHUNKY_DENOISE_KERNEL_SHIFT == 3, "two bits of kernel form");
constexpr float kDenoiseSigmaColor = 4.0f, kDenoiseSigmaNormal = 0.5f, kDenoiseSigmaAlbedo = 0.1f;
constexpr int kDenoiseIterations = 5;

extern "C" int chunky_denoise_default_params(chunky_denoise_params* p) {
    if (!p) return fail(CHUNKY_E_INVALID, "denoise_default_params: NULL params");
    p->size = sizeof(chunky_denoise_params);
    p->iterations = kDenoiseIterations;
    p->sigma_color = kDenoiseSigmaColor;
    p->sigma_normal = kDenoiseSigmaNormal;
    p->sigma_albedo = kDenoiseSigmaAlbedo;
    p->flags = CHUNKY_DENOISE_DEMODULATE;
    return CHUNKY_OK;
}

int denoise_params(const char* who, const chunky_denoise_params* params, DnCoeffs* K, int* form) {
    if (!params) return fail(CHUNKY_E_INVALID, "%s: NULL params", who);
    constexpr size_t kFirst = offsetof(chunky_denoise_params, flags) + sizeof(uint32_t);  // the first version of the struct
    chunky_denoise_params p;
    if (!take_versioned(params, params->size, kFirst, &p)) return fail(CHUNKY_E_INVALID, "%s: params.size %zu is smaller than the struct (%zu)", who, params->size, kFirst);
    if (p.iterations < 1 || p.iterations > DN_MAX_ITERATIONS) return fail(CHUNKY_E_INVALID, "%s: iterations %d outside 1 .. %d", who, p.iterations, DN_MAX_ITERATIONS);
    const float sig[3] = {p.sigma_color, p.sigma_normal, p.sigma_albedo};
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(sig[i]) || !(sig[i] > 0.0f)) return fail(CHUNKY_E_INVALID, "%s: sigma %d must be finite and > 0, got %g", who, i, (double)sig[i]);
    if (p.flags & ~(CHUNKY_DENOISE_DEMODULATE | CHUNKY_DENOISE_KERNEL_MASK)) return fail(CHUNKY_E_INVALID, "%s: unknown flags 0x%x", who, p.flags);
    const int f = (int)((p.flags & CHUNKY_DENOISE_KERNEL_MASK) >> CHUNKY_DENOISE_KERNEL_SHIFT);
    if (f != kDenoiseFormPacked && f != kDenoiseFormGather) return fail(CHUNKY_E_INVALID, "%s: unknown kernel form %d", who, f);
    if (!dn_coeffs(p.iterations, p.sigma_color, p.sigma_normal, p.sigma_albedo, (int)(p.flags & CHUNKY_DENOISE_DEMODULATE), K))
        return fail(CHUNKY_E_INVALID, "%s: a sigma is too small or too large for a float coefficient", who);
    if (form) *form = f;
    return CHUNKY_OK;
}

int denoise_images(const char* who, int width, int height, const void* color, const void* albedo, const void* normal, const void* out) {
    if (width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX / 16 || height > 65535 * 4)
        return fail(CHUNKY_E_INVALID, "%s: bad size %dx%d", who, width, height);
    if (!color || !albedo || !normal || !out) return fail(CHUNKY_E_INVALID, "%s: NULL image", who);
    return CHUNKY_OK;
}

namespace {
struct HostFetch {  // 3 floats per pixel in each image
    const float *d, *n, *a;
    int width;
    void load(int x, int y, float* dq, float* nq, float* aq) const {
        const size_t o = 3 * ((size_t)y * width + x);
        for (int k = 0; k < 3; k++) {
            dq[k] = d[o + k];
            nq[k] = n[o + k];
            aq[k] = a[o + k];
        }
    }
};
// rows [y0, y1) of every band at once: pixels are independent, so the split changes no bit
template <class F>
void over_rows(int height, F body) {
    unsigned n = std::thread::hardware_concurrency();
    n = n < 1 ? 1 : (n > 16 ? 16 : n);
    if ((int)n > height) n = (unsigned)height;
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < n; t++) pool.emplace_back(body, (int)((int64_t)height * t / n), (int)((int64_t)height * (t + 1) / n));
    body(0, (int)((int64_t)height / n));
    for (auto& t : pool) t.join();
}
}  // namespace

extern "C" int chunky_denoise_host(int width, int height, const float* color, const float* albedo, const float* normal,
                                   const chunky_denoise_params* params, float* out) {
    DnCoeffs K;
    if (int rc = denoise_params("denoise_host", params, &K, nullptr)) return rc;
    if (int rc = denoise_images("denoise_host", width, height, color, albedo, normal, out)) return rc;
    const size_t n = (size_t)width * height;
    std::vector<float> buf[2];
    buf[0].resize(3 * n);
    buf[1].resize(3 * n);
    over_rows(height, [&](int y0, int y1) {
        for (size_t i = (size_t)y0 * width; i < (size_t)y1 * width; i++) dn_demodulate(color + 3 * i, albedo + 3 * i, K.demodulate, &buf[0][3 * i]);
    });
    for (int it = 0; it < K.iterations; it++) {
        const float* src = buf[it & 1].data();
        float* dst = buf[(it + 1) & 1].data();
        over_rows(height, [&, src, dst](int y0, int y1) {
            const HostFetch F{src, normal, albedo, width};
            for (int y = y0; y < y1; y++)
                for (int x = 0; x < width; x++) dn_filter_pixel(F, x, y, width, height, 1 << it, K.c_i[it], K.c_n, K.c_a, dst + 3 * ((size_t)y * width + x));
        });
    }
    const float* last = buf[K.iterations & 1].data();
    over_rows(height, [&](int y0, int y1) {
        for (size_t i = (size_t)y0 * width; i < (size_t)y1 * width; i++) dn_finish(last + 3 * i, albedo + 3 * i, color + 3 * i, K.demodulate, out + 3 * i);
    });
    return CHUNKY_OK;
}

extern "C" int chunky_denoise_exp(const float* x, int n, float* out) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(CHUNKY_E_INVALID, "denoise_exp: bad arguments");
    for (int i = 0; i < n; i++) out[i] = dn_exp(x[i]);
    return CHUNKY_OK;
}
