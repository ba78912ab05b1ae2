// capi_robust.hip — firefly-robust accumulation on the device (robust_spec.h, robust.hip); its host twin is robust_host.cpp.
#include "capi_internal.hpp"
#include "denoise_host.hpp"
#include "robust_host.hpp"

static size_t robust_plane_bytes(const chunky_render* r) { return (size_t)r->width * r->height * 3 * sizeof(float); }

extern "C" int chunky_render_robust_begin(chunky_render* r, int n_buckets) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    if (n_buckets != 0)
        if (int rc = robust_buckets("render_robust_begin", n_buckets)) return rc;
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_robust_begin: a group's target (the buckets live on one device)");
    LOCK_RENDER(r);
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // queued folds may still write the buckets
    r->rb_count = 0;
    if (n_buckets != r->rb_m) {
        r->rb_m = 0;
        r->rb_buckets.release();
        if (n_buckets == 0) {
            r->rb_out.release();
            r->rb_trim.release();
            return CHUNKY_OK;
        }
        HIP_TRY(r->rb_buckets.alloc((size_t)n_buckets * robust_plane_bytes(r)));
        r->rb_m = n_buckets;
    }
    if (r->rb_m) HIP_TRY(hipMemsetAsync(r->rb_buckets.p, 0, r->rb_buckets.bytes, r->ctx->stream));
    return CHUNKY_OK;
}

// what a robust pass needs of the target: the state, a camera, and render_pool for the scene and options as they are
static int robust_state(const char* who, chunky_render* r, SceneView* S) {
    if (!r->rb_m) return fail(CHUNKY_E_STATE, "%s before render_robust_begin", who);
    return needs_render_pool(who, r, S);
}

extern "C" int chunky_render_robust_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    if (n < 0 || (n > 0 && !seeds) || first_buffer_spp < 0) return fail(CHUNKY_E_INVALID, "render_robust_passes: bad arguments");
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_robust_passes: a group's target (the buckets live on one device)");
    LOCK_RENDER(r);
    SceneView S;
    if (int rc = robust_state("render_robust_passes", r, &S)) return rc;
    if ((int64_t)r->rb_count + n > INT32_MAX || (int64_t)first_buffer_spp + n > INT32_MAX)
        return fail(CHUNKY_E_INVALID, "render_robust_passes: %d more passes leave the range of the sample count", n);
    if (n == 0) return CHUNKY_OK;
    r->ad_resumable = false;  // the call is accepted: it writes the framebuffer
    if (r->rb_clock.full())
        if (int rc = r->rb_clock.collect()) return rc;
    const ShardView& T = r->shard;
    if (T.n_local <= 0) {  // this rank owns no tile of so small an image: nothing to render, the samples still count
        r->rb_count += n;
        return CHUNKY_OK;
    }
    hipStream_t st = r->ctx->stream;
    int cap = 0;
    if (int rc = stage_fold_launches("render_robust_passes", r, T, n, &cap)) return rc;
    return for_each_launch(seeds, n, first_buffer_spp, cap, [&](const PassSeeds& ps, const int32_t*) {
        StagedFold fold;
        fold.kind = StagedFold::buckets;
        fold.bucket_images = (float*)r->rb_buckets.p;
        fold.n_buckets = r->rb_m;
        fold.first_index = r->rb_count;
        if (int rc = r->rb_clock.open(st)) return rc;
        HIP_TRY(launch_render_fold(r->kernel_variant, S, r->cam, r->opts, T, ps, r->fb, (int*)r->work_counter.p, st, &r->last_choice,
                                   (float*)r->staging.p, nullptr, fold));
        if (int rc = r->rb_clock.close(st)) return rc;
        r->rb_count += ps.n;  // (per launch: a launch that failed leaves the count of those that ran)
        return (int)CHUNKY_OK;
    });
}

extern "C" int chunky_render_robust_read_bucket(chunky_render* r, int b, float* out, int64_t n_floats, int32_t* count) {
    if (r && !r->parts.empty()) return fail(CHUNKY_E_STATE, "render_robust_read_bucket: a group's target has no robust state");
    LOCK_RENDER(r);
    if (!r->rb_m) return fail(CHUNKY_E_STATE, "render_robust_read_bucket before render_robust_begin");
    if (b < 0 || b >= r->rb_m) return fail(CHUNKY_E_INVALID, "render_robust_read_bucket: bucket %d of %d", b, r->rb_m);
    if (int rc = read_floats("render_robust_read_bucket", r, (const char*)r->rb_buckets.p + (size_t)b * robust_plane_bytes(r), out, n_floats,
                             (int64_t)r->width * r->height * 3))
        return rc;
    if (count) *count = r->rb_count;
    return CHUNKY_OK;
}

// the resolve into r->rb_out (and r->rb_trim where asked), queued on the stream and timed; the caller holds the lock
static int robust_resolve(const char* who, chunky_render* r, const chunky_robust_params& p, bool want_trim) {
    if (!r->rb_m) return fail(CHUNKY_E_STATE, "%s before render_robust_begin", who);
    if (r->rb_count < r->rb_m)
        return fail(CHUNKY_E_STATE, "%s: %d samples folded, %d buckets: a bucket would be empty", who, r->rb_count, r->rb_m);
    const size_t np = (size_t)r->width * r->height;
    if (!r->rb_out.p) HIP_TRY(r->rb_out.alloc(robust_plane_bytes(r)));
    if (want_trim && !r->rb_trim.p) HIP_TRY(r->rb_trim.alloc(np));
    if (r->rb_resolve_clock.full())
        if (int rc = r->rb_resolve_clock.collect()) return rc;
    if (int rc = r->rb_resolve_clock.open(r->ctx->stream)) return rc;
    HIP_TRY(launch_robust_resolve((const float*)r->rb_buckets.p, r->rb_m, (long long)np, p.mode, p.gain, (float*)r->rb_out.p,
                                  want_trim ? (unsigned char*)r->rb_trim.p : nullptr, r->ctx->stream));
    return r->rb_resolve_clock.close(r->ctx->stream);
}

extern "C" int chunky_render_robust_resolve(chunky_render* r, const chunky_robust_params* params, float* out, int64_t n_floats, uint8_t* trim,
                                            int64_t n_pixels) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    chunky_robust_params p;
    if (int rc = robust_params("render_robust_resolve", params, &p)) return rc;
    const int64_t np = (int64_t)r->width * r->height;
    if (!out || n_floats != 3 * np) return fail(CHUNKY_E_INVALID, "render_robust_resolve: need %lld floats, got %lld", (long long)(3 * np), (long long)n_floats);
    if (trim && n_pixels != np) return fail(CHUNKY_E_INVALID, "render_robust_resolve: the trim map has %lld bytes, got %lld", (long long)np, (long long)n_pixels);
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_robust_resolve: a group's target has no robust state");
    LOCK_RENDER(r);
    if (int rc = robust_resolve("render_robust_resolve", r, p, trim != nullptr)) return rc;
    if (trim) HIP_TRY(hipMemcpyAsync(trim, r->rb_trim.p, (size_t)np, hipMemcpyDeviceToHost, r->ctx->stream));
    return read_floats("render_robust_resolve", r, r->rb_out.p, out, n_floats, 3 * np);
}

extern "C" int chunky_render_robust_denoise(chunky_render* r, const chunky_robust_params* robust_params_, const chunky_denoise_params* denoise_params_,
                                            float* out, int64_t n_floats) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    chunky_robust_params p;
    if (int rc = robust_params("render_robust_denoise", robust_params_, &p)) return rc;
    DnCoeffs K;
    int form = 0;
    if (int rc = denoise_params("render_robust_denoise", denoise_params_, &K, &form)) return rc;
    const int64_t need = (int64_t)r->width * r->height * 3;
    if (!out || n_floats != need) return fail(CHUNKY_E_INVALID, "render_robust_denoise: need %lld floats, got %lld", (long long)need, (long long)n_floats);
    if (int rc = denoise_images("render_robust_denoise", r->width, r->height, out, out, out, out)) return rc;
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_robust_denoise: a group's target has no robust state");
    LOCK_RENDER(r);
    if (r->shard.world > 1)
        return fail(CHUNKY_E_STATE, "render_robust_denoise: this target holds rank %d of %d of the image, not all of it", r->shard.rank, r->shard.world);
    if (!r->aov_pass.images.p) return fail(CHUNKY_E_STATE, "render_robust_denoise before any AOV pass");
    if (int rc = robust_resolve("render_robust_denoise", r, p, false)) return rc;
    return render_denoise(r, K, form, (const float*)r->rb_out.p, out);
}

extern "C" int chunky_render_robust_kernel_time(chunky_render* r, float* total_ms, int* launches, float* resolve_ms) {
    if (r && !r->parts.empty()) return fail(CHUNKY_E_STATE, "render_robust_kernel_time: a group's target has no robust state");
    LOCK_RENDER(r);
    if (int rc = r->rb_clock.take(total_ms, launches)) return rc;
    return r->rb_resolve_clock.take(resolve_ms, nullptr);
}

extern "C" int chunky_selftest_robust(chunky_ctx* ctx, int width, int height, const float* samples, int n, int n_buckets, int first_index,
                                      const chunky_robust_params* params, float* buckets_out, float* image_out, uint8_t* trim_out) {
    if (!ctx) return fail(CHUNKY_E_INVALID, "NULL context");
    if (!ctx->members.empty()) ctx = ctx->members[0];
    chunky_robust_params p;
    if (int rc = robust_params("selftest_robust", params, &p)) return rc;
    if (int rc = robust_buckets("selftest_robust", n_buckets)) return rc;
    if (width <= 0 || height <= 0 || (int64_t)width * height > (1 << 20)) return fail(CHUNKY_E_INVALID, "selftest_robust: bad size %dx%d", width, height);
    if (!samples || n < 1 || n > kMaxPassesPerLaunch || first_index < 0 || (int64_t)first_index + n > INT32_MAX)
        return fail(CHUNKY_E_INVALID, "selftest_robust: bad arguments");
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const ShardView whole{0, 1, 256, width * height};
    const long long n_tiles = pool_tiles(whole, width, height);
    const size_t np = (size_t)width * height, plane = np * 3 * sizeof(float);
    DevBuf s, staging, res, buckets, image, trim;
    HIP_TRY(s.upload(samples, plane * (size_t)n, st));
    HIP_TRY(staging.alloc(staging_floats(whole, width, height, n) * sizeof(float)));
    HIP_TRY(res.alloc(plane));
    HIP_TRY(buckets.alloc(plane * (size_t)n_buckets));
    HIP_TRY(image.alloc(plane));
    HIP_TRY(trim.alloc(np));
    HIP_TRY(hipMemsetAsync(staging.p, 0, staging.bytes, st));
    HIP_TRY(hipMemsetAsync(res.p, 0, plane, st));
    HIP_TRY(hipMemsetAsync(buckets.p, 0, buckets.bytes, st));
    HIP_TRY(launch_robust_stage((const float*)s.p, (float*)staging.p, width, height, n_tiles, n, st));
    HIP_TRY(launch_fold_buckets((const float*)staging.p, (float*)res.p, (float*)buckets.p, n_buckets, first_index, whole, width, height, n_tiles, n, 0, st));
    HIP_TRY(launch_robust_resolve((const float*)buckets.p, n_buckets, (long long)np, p.mode, p.gain, (float*)image.p, (unsigned char*)trim.p, st));
    if (buckets_out) HIP_TRY(hipMemcpyAsync(buckets_out, buckets.p, buckets.bytes, hipMemcpyDeviceToHost, st));
    if (image_out) HIP_TRY(hipMemcpyAsync(image_out, image.p, plane, hipMemcpyDeviceToHost, st));
    if (trim_out) HIP_TRY(hipMemcpyAsync(trim_out, trim.p, np, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CHUNKY_OK;
}
