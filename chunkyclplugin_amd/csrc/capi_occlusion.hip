// capi_occlusion.hip — the sun-shadow and ambient-occlusion images of the beauty sample's rays (occlusion.hip).
#include "capi_internal.hpp"

static size_t occlusion_plane_bytes(const chunky_render* r) { return (size_t)r->width * r->height * sizeof(float); }

// n passes over the pixel slots of shard T (a single-device target: its own share; member 0 of a group: the caller's share)
static int occlusion_passes(chunky_render* r, ShardView T, const int32_t* seeds, int n, int first_buffer_spp, float ao_distance) {
    LOCK_RENDER(r);
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "occlusion_passes before set_camera");
    if (int rc = r->occlusion_pass.ensure(2 * occlusion_plane_bytes(r), r->ctx->stream)) return rc;  // AO then SUN
    r->occlusion_pass.last_launches = 0;
    if (n == 0 || T.n_local <= 0) return CHUNKY_OK;
    SceneView S;
    if (int rc = target_scene_view(r, &S)) return rc;
    float* ao = (float*)r->occlusion_pass.images.p;
    float* sun = (float*)((char*)r->occlusion_pass.images.p + occlusion_plane_bytes(r));
    int* counter = r->occlusion_pass.counter();
    return first_hit_launches(r, r->occlusion_pass, seeds, n, first_buffer_spp, [&](const PassSeeds& ps) {  // (each continues the running means)
        HIP_TRY(launch_occlusion(r->kernel_variant, S, r->cam, r->opts, T, ps, ao, sun, ao_distance, counter, r->ctx->stream, &r->occlusion_pass.choice));
        return (int)CHUNKY_OK;
    });
}

extern "C" int chunky_render_occlusion_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp, float ao_distance) {
    if (n < 0 || (n > 0 && !seeds) || first_buffer_spp < 0) return fail(CHUNKY_E_INVALID, "occlusion_passes: bad arguments");
    if (!(ao_distance > 0)) return fail(CHUNKY_E_INVALID, "occlusion_passes: ao_distance must be > 0 (+inf allowed), got %g", (double)ao_distance);  // (a NaN too)
    return on_first_member("occlusion_passes", r, [&](chunky_render* m, const ShardView& t) { return occlusion_passes(m, t, seeds, n, first_buffer_spp, ao_distance); });
}

extern "C" int chunky_render_occlusion_read(chunky_render* r, int which, float* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_occlusion_read(r->parts[0], which, out, n);
    LOCK_RENDER(r);
    if (which != CHUNKY_AOV_AO && which != CHUNKY_AOV_SUN) return fail(CHUNKY_E_INVALID, "occlusion_read: unknown image %d", which);
    const char* images = (const char*)r->occlusion_pass.images.p;
    const char* src = images ? images + (which == CHUNKY_AOV_SUN ? occlusion_plane_bytes(r) : 0) : nullptr;  // null before any pass
    return read_floats("occlusion_read", r, src, out, n, (int64_t)r->width * r->height);
}

extern "C" int chunky_render_occlusion_reset(chunky_render* r) {
    if (r && !r->parts.empty()) return chunky_render_occlusion_reset(r->parts[0]);
    LOCK_RENDER(r);
    if (r->occlusion_pass.images.p) HIP_TRY(hipMemsetAsync(r->occlusion_pass.images.p, 0, 2 * occlusion_plane_bytes(r), r->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_render_occlusion_kernel_time(chunky_render* r, float* total_ms, int* launches) {
    return first_hit_kernel_time(r, &chunky_render::occlusion_pass, total_ms, launches);
}

extern "C" int chunky_render_occlusion_kernel_info(chunky_render* r, int32_t out4[4]) {
    return first_hit_kernel_info("occlusion_kernel_info", r, &chunky_render::occlusion_pass, out4);
}
