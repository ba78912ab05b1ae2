// capi_filter.hip — the tone map on the device (filter.hip).
#include "capi_internal.hpp"

int device_gamma_table(chunky_ctx* ctx, const float** out) {
    if (!ctx->gamma_table) {
        HIP_TRY(hipMalloc(&ctx->gamma_table, 256 * sizeof(float)));
        HIP_TRY(hipMemcpy(ctx->gamma_table, gamma_thresholds(), 256 * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = (const float*)ctx->gamma_table;
    return CHUNKY_OK;
}

extern "C" int chunky_filter_frame(chunky_ctx* ctx, int width, int height, double exposure, const double* input,
                                   int32_t* argb_out, int type) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "filter_frame: NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];  // a group: the tone map of one frame runs on its first member
    if (width < 0 || height < 0) return fail(CHUNKY_E_INVALID, "filter_frame: %dx%d", width, height);
    const long long n = (long long)width * height;
    if (n == 0) return CHUNKY_OK;
    if (!input || !argb_out) return fail(CHUNKY_E_INVALID, "filter_frame: NULL buffer");
    std::lock_guard<std::recursive_mutex> guard(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf in, out;
    HIP_TRY(in.upload(input, (size_t)n * 24, ctx->stream));
    HIP_TRY(out.alloc((size_t)n * 4));
    const float* table = nullptr;
    if (int rc = device_gamma_table(ctx, &table)) return rc;
    HIP_TRY(launch_filter(n, (float)exposure, (const double*)in.p, (unsigned*)out.p, type, ctx->stream, table));
    HIP_TRY(hipMemcpyAsync(argb_out, out.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_filter_frame_alpha(chunky_ctx* ctx, int width, int height, double exposure, const double* input, const float* alpha,
                                         int32_t* argb_out, int type) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "filter_frame_alpha: NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];
    if (width < 0 || height < 0) return fail(CHUNKY_E_INVALID, "filter_frame_alpha: %dx%d", width, height);
    const long long n = (long long)width * height;
    if (n == 0) return CHUNKY_OK;
    if (!input || !alpha || !argb_out) return fail(CHUNKY_E_INVALID, "filter_frame_alpha: NULL buffer");
    std::lock_guard<std::recursive_mutex> guard(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf in, cover, out;
    HIP_TRY(in.upload(input, (size_t)n * 24, ctx->stream));
    HIP_TRY(cover.upload(alpha, (size_t)n * 4, ctx->stream));
    HIP_TRY(out.alloc((size_t)n * 4));
    const float* table = nullptr;
    if (int rc = device_gamma_table(ctx, &table)) return rc;
    HIP_TRY(launch_filter_alpha(n, (float)exposure, (const double*)in.p, (const float*)cover.p, (unsigned*)out.p, type, ctx->stream, table));
    HIP_TRY(hipMemcpyAsync(argb_out, out.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_filter_frame_device(chunky_ctx* ctx, int64_t n_pixels, float exposure, const void* d_input,
                                          void* d_argb, int type, int repeat, float* kernel_ms) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "filter_frame_device: NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];
    if (n_pixels < 0 || repeat < 1) return fail(CHUNKY_E_INVALID, "filter_frame_device: n_pixels=%lld repeat=%d", (long long)n_pixels, repeat);
    if (n_pixels > 0 && (!d_input || !d_argb)) return fail(CHUNKY_E_INVALID, "filter_frame_device: NULL buffer");
    if ((reinterpret_cast<uintptr_t>(d_input) & 7u) || (reinterpret_cast<uintptr_t>(d_argb) & 3u))
        return fail(CHUNKY_E_INVALID, "filter_frame_device: misaligned buffer");
    std::lock_guard<std::recursive_mutex> guard(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const float* table = nullptr;
    if (int rc = device_gamma_table(ctx, &table)) return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipError_t err = hipEventRecord(e0, ctx->stream);
    for (int k = 0; k < repeat && err == hipSuccess; k++)
        err = launch_filter(n_pixels, exposure, (const double*)d_input, (unsigned*)d_argb, type, ctx->stream, table);
    if (err == hipSuccess) err = hipEventRecord(e1, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    float ms = 0;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(CHUNKY_E_HIP, "filter_frame_device: %s", hipGetErrorString(err));
    if (kernel_ms) *kernel_ms = ms / (float)repeat;
    return CHUNKY_OK;
}
