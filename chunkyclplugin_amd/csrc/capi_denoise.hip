// capi_denoise.hip — the denoiser on the device (denoise_spec.h, denoise.hip); its host twin is denoise_host.cpp.
#include "capi_internal.hpp"
#include "denoise_host.hpp"

static_assert(kDenoiseFormGather == kDenoiseGather && kDenoiseFormPacked == kDenoisePacked, "denoise_host.hpp");

extern "C" int chunky_denoise_frame(chunky_ctx* ctx, int width, int height, const float* color, const float* albedo, const float* normal,
                                    const chunky_denoise_params* params, float* out) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "denoise_frame: NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];  // a group: one frame is filtered on its first member
    DnCoeffs K;
    int form = 0;
    if (int rc = denoise_params("denoise_frame", params, &K, &form)) return rc;
    if (int rc = denoise_images("denoise_frame", width, height, color, albedo, normal, out)) return rc;
    std::lock_guard<std::recursive_mutex> guard(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)width * height * 12;
    DevBuf c, a, n, o, work;
    HIP_TRY(c.upload(color, bytes, ctx->stream));
    HIP_TRY(a.upload(albedo, bytes, ctx->stream));
    HIP_TRY(n.upload(normal, bytes, ctx->stream));
    HIP_TRY(o.alloc(bytes));
    work.bytes = denoise_work_bytes(width, height);
    HIP_TRY(hipMalloc(&work.p, work.bytes));
    HIP_TRY(launch_denoise(form, width, height, (const float*)c.p, (const float*)a.p, (const float*)n.p, K, (float*)o.p, work.p, work.bytes, ctx->stream, nullptr));
    HIP_TRY(hipMemcpyAsync(out, o.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return CHUNKY_OK;
}

// on one device: `color` holds the whole image — r's framebuffer (a single-device target, or member 0 of a group after the exchange),
// or the resolved image of chunky_render_robust_denoise
int render_denoise(chunky_render* r, const DnCoeffs& K, int form, const float* color, float* out) {
    LOCK_RENDER(r);
    if (!r->aov_pass.images.p) return fail(CHUNKY_E_STATE, "render_denoise before any AOV pass");
    const size_t bytes = aov_image_bytes(r), need = denoise_work_bytes(r->width, r->height);
    if (!r->dn_work.p) {
        HIP_TRY(r->dn_work.alloc(need));
        HIP_TRY(r->dn_out.alloc(bytes));
    }
    if (r->dn_clock.full())
        if (int rc = r->dn_clock.collect()) return rc;
    const float* albedo = (const float*)r->aov_pass.images.p;
    const float* normal = (const float*)((const char*)r->aov_pass.images.p + bytes);
    int launches = 0;
    if (int rc = r->dn_clock.open(r->ctx->stream)) return rc;
    HIP_TRY(launch_denoise(form, r->width, r->height, color, albedo, normal, K, (float*)r->dn_out.p, r->dn_work.p, r->dn_work.bytes, r->ctx->stream, &launches));
    if (int rc = r->dn_clock.close(r->ctx->stream, launches)) return rc;
    const int64_t n = (int64_t)(bytes / 4);  // (checked against the caller's count by chunky_render_denoise)
    return read_floats("render_denoise", r, r->dn_out.p, out, n, n);
}

extern "C" int chunky_render_denoise(chunky_render* r, const chunky_denoise_params* params, float* out, int64_t n_floats) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    DnCoeffs K;
    int form = 0;
    if (int rc = denoise_params("render_denoise", params, &K, &form)) return rc;
    const int64_t need = (int64_t)r->width * r->height * 3;
    if (!out || n_floats != need) return fail(CHUNKY_E_INVALID, "render_denoise: need %lld floats, got %lld", (long long)need, (long long)n_floats);
    if (int rc = denoise_images("render_denoise", r->width, r->height, out, out, out, out)) return rc;
    std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
    const ShardView& share = r->parts.empty() ? r->shard : r->outer;
    if (share.world > 1) return fail(CHUNKY_E_STATE, "render_denoise: this target holds rank %d of %d of the image, not all of it", share.rank, share.world);
    if (r->parts.empty()) return render_denoise(r, K, form, r->fb, out);
    if (!r->parts[0]->aov_pass.images.p) return fail(CHUNKY_E_STATE, "render_denoise before any AOV pass");
    if (int rc = group_gather(r)) return rc;  // member 0's buffer then holds the whole image (chunky_render_read's exchange)
    return render_denoise(r->parts[0], K, form, r->parts[0]->fb, out);
}

extern "C" int chunky_render_denoise_kernel_time(chunky_render* r, float* total_ms, int* launches) {
    if (r && !r->parts.empty()) return chunky_render_denoise_kernel_time(r->parts[0], total_ms, launches);
    LOCK_RENDER(r);
    return r->dn_clock.take(total_ms, launches);
}
