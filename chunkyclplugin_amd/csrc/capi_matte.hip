// capi_matte.hip — the antialiased ID mattes on the device (matte_spec.h, matte.hip); the host twins are matte_host.cpp.
#include "capi_internal.hpp"
#include "matte_host.hpp"

constexpr int kMattePlanes = 2 * CHUNKY_MATTE_SLOTS + 1;  // six of ids, six of counts, `other`
static size_t matte_plane_bytes(const chunky_render* r) { return (size_t)r->width * r->height * 4; }
static size_t matte_bytes(const chunky_render* r) { return matte_plane_bytes(r) * kMattePlanes; }

// n passes over the pixel slots of shard T (a single-device target: its own share; member 0 of a group: the caller's share)
static int matte_passes(chunky_render* r, ShardView T, const int32_t* seeds, int n) {
    LOCK_RENDER(r);
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "matte_passes before set_camera");
    const bool first = !r->matte_pass.images.p;
    if (int rc = r->matte_pass.ensure(matte_bytes(r), r->ctx->stream)) return rc;
    if (first) r->matte_passes = 0;
    if (n > INT32_MAX - r->matte_passes) return fail(CHUNKY_E_INVALID, "matte_passes: %d more passes after %d exceed 2^31 - 1", n, r->matte_passes);
    r->matte_pass.last_launches = 0;
    if (n == 0) return CHUNKY_OK;
    r->matte_passes += n;  // (a rank that owns nothing keeps its planes empty, and they read as such after any number of passes)
    if (T.n_local <= 0) return CHUNKY_OK;
    SceneView S;
    if (int rc = target_scene_view(r, &S)) return rc;
    int* planes = (int*)r->matte_pass.images.p;
    int* counter = r->matte_pass.counter();
    return first_hit_launches(r, r->matte_pass, seeds, n, 0, [&](const PassSeeds& ps) {  // (each continues the counts)
        HIP_TRY(launch_matte(r->kernel_variant, S, r->cam, r->opts, T, ps, planes, counter, r->ctx->stream, &r->matte_pass.choice));
        return (int)CHUNKY_OK;
    });
}

extern "C" int chunky_render_matte_passes(chunky_render* r, const int32_t* seeds, int n) {
    if (n < 0 || (n > 0 && !seeds)) return fail(CHUNKY_E_INVALID, "matte_passes: bad arguments");
    return on_first_member("matte_passes", r, [&](chunky_render* m, const ShardView& t) { return matte_passes(m, t, seeds, n); });
}

extern "C" int chunky_render_matte_reset(chunky_render* r) {
    if (r && !r->parts.empty()) return chunky_render_matte_reset(r->parts[0]);
    LOCK_RENDER(r);
    if (r->matte_pass.images.p) HIP_TRY(hipMemsetAsync(r->matte_pass.images.p, 0, matte_bytes(r), r->ctx->stream));
    r->matte_passes = 0;
    return CHUNKY_OK;
}

static int matte_size(const char* who, const chunky_render* r, int64_t n_pixels) {
    const int64_t need = (int64_t)r->width * r->height;
    if (n_pixels != need) return fail(CHUNKY_E_INVALID, "%s: need %lld pixels, got %lld", who, (long long)need, (long long)n_pixels);
    return CHUNKY_OK;
}

extern "C" int chunky_render_matte_read(chunky_render* r, int32_t* ids, int32_t* counts, int32_t* other, int64_t n_pixels, int32_t* passes) {
    if (r && !r->parts.empty()) return chunky_render_matte_read(r->parts[0], ids, counts, other, n_pixels, passes);
    LOCK_RENDER(r);
    if (!ids || !counts || !other || !passes) return fail(CHUNKY_E_INVALID, "matte_read: NULL output");
    if (int rc = matte_size("matte_read", r, n_pixels)) return rc;
    if (int rc = r->matte_pass.ensure(matte_bytes(r), r->ctx->stream)) return rc;  // (before any pass: empty planes, and matte_passes is 0)
    const char* src = (const char*)r->matte_pass.images.p;
    const size_t plane = matte_plane_bytes(r);
    HIP_TRY(hipMemcpyAsync(ids, src, CHUNKY_MATTE_SLOTS * plane, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(counts, src + CHUNKY_MATTE_SLOTS * plane, CHUNKY_MATTE_SLOTS * plane, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(other, src + 2 * CHUNKY_MATTE_SLOTS * plane, plane, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    *passes = r->matte_passes;
    return CHUNKY_OK;
}

extern "C" int chunky_render_matte_restore(chunky_render* r, const int32_t* ids, const int32_t* counts, const int32_t* other, int64_t n_pixels,
                                           int32_t passes) {
    if (r && !r->parts.empty()) return chunky_render_matte_restore(r->parts[0], ids, counts, other, n_pixels, passes);
    LOCK_RENDER(r);
    if (!ids || !counts || !other) return fail(CHUNKY_E_INVALID, "matte_restore: NULL input");
    if (int rc = matte_size("matte_restore", r, n_pixels)) return rc;
    if (int rc = matte_state_valid("matte_restore", ids, counts, other, n_pixels, passes)) return rc;
    if (int rc = r->matte_pass.ensure(matte_bytes(r), r->ctx->stream)) return rc;
    char* dst = (char*)r->matte_pass.images.p;
    const size_t plane = matte_plane_bytes(r);
    HIP_TRY(hipMemcpyAsync(dst, ids, CHUNKY_MATTE_SLOTS * plane, hipMemcpyHostToDevice, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(dst + CHUNKY_MATTE_SLOTS * plane, counts, CHUNKY_MATTE_SLOTS * plane, hipMemcpyHostToDevice, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(dst + 2 * CHUNKY_MATTE_SLOTS * plane, other, plane, hipMemcpyHostToDevice, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // the caller may reuse its arrays on return
    r->matte_passes = passes;
    return CHUNKY_OK;
}

// the read-outs' device buffer (kept between calls)
static int matte_work(chunky_render* r, size_t bytes) {
    if (r->matte_work.p && r->matte_work.bytes >= bytes) return CHUNKY_OK;
    HIP_TRY(r->matte_work.alloc(bytes));
    return CHUNKY_OK;
}

extern "C" int chunky_render_matte_ranks(chunky_render* r, int32_t* ids, float* coverage, int64_t n_pixels) {
    if (r && !r->parts.empty()) return chunky_render_matte_ranks(r->parts[0], ids, coverage, n_pixels);
    LOCK_RENDER(r);
    if (!ids || !coverage) return fail(CHUNKY_E_INVALID, "matte_ranks: NULL output");
    if (int rc = matte_size("matte_ranks", r, n_pixels)) return rc;
    if (!r->matte_pass.images.p || r->matte_passes == 0) return fail(CHUNKY_E_STATE, "matte_ranks before any matte pass");
    const size_t half = CHUNKY_MATTE_SLOTS * matte_plane_bytes(r);
    if (int rc = matte_work(r, 2 * half)) return rc;
    int* d_ids = (int*)r->matte_work.p;
    float* d_cov = (float*)((char*)r->matte_work.p + half);
    HIP_TRY(launch_matte_ranks((const int*)r->matte_pass.images.p, n_pixels, r->matte_passes, d_ids, d_cov, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(ids, d_ids, half, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(coverage, d_cov, half, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_render_matte_extract(chunky_render* r, const int32_t* set, int n_set, float* out, int64_t n_pixels) {
    if (r && !r->parts.empty()) return chunky_render_matte_extract(r->parts[0], set, n_set, out, n_pixels);
    LOCK_RENDER(r);
    if (!out) return fail(CHUNKY_E_INVALID, "matte_extract: NULL output");
    std::vector<int32_t> sorted;
    if (int rc = matte_sorted_set("matte_extract", set, n_set, &sorted)) return rc;
    if (int rc = matte_size("matte_extract", r, n_pixels)) return rc;
    if (!r->matte_pass.images.p || r->matte_passes == 0) return fail(CHUNKY_E_STATE, "matte_extract before any matte pass");
    if (int rc = matte_work(r, matte_plane_bytes(r))) return rc;
    HIP_TRY(r->matte_set.upload(sorted.data(), sorted.size() * 4, r->ctx->stream));  // (an empty set: a word nobody reads)
    HIP_TRY(launch_matte_extract((const int*)r->matte_pass.images.p, n_pixels, r->matte_passes, (const int*)r->matte_set.p, (int)sorted.size(),
                                 (float*)r->matte_work.p, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, r->matte_work.p, matte_plane_bytes(r), hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_render_matte_kernel_time(chunky_render* r, float* total_ms, int* launches) {
    return first_hit_kernel_time(r, &chunky_render::matte_pass, total_ms, launches);
}

extern "C" int chunky_render_matte_kernel_info(chunky_render* r, int32_t out4[4]) {
    return first_hit_kernel_info("matte_kernel_info", r, &chunky_render::matte_pass, out4);
}
