// capi_aov.hip — albedo and normal images for denoisers, and the first-hit images of chunky_render_aov_passes_ex (aov.hip).
#include "capi_internal.hpp"

// words per pixel of the images of chunky_render_aov_read_ex, and the offset (in words per pixel) of each inside r->aov_ex
static const int kAovWords[7] = {3, 3, 1, 1, 3, 1, 1};
static const int kAovExOffset[7] = {0, 0, 0, 1, 2, 5, 6};  // alpha, depth, position, emittance, block
constexpr int kAovExWords = 7;
static size_t aov_ex_bytes(const chunky_render* r) { return (size_t)r->width * r->height * kAovExWords * 4; }

// the five first-hit images: allocated, zeroed, by the first chunky_render_aov_passes_ex
static int aov_ex_ensure(chunky_render* r) {
    if (r->aov_ex.p) return CHUNKY_OK;
    HIP_TRY(r->aov_ex.alloc(aov_ex_bytes(r)));
    HIP_TRY(hipMemsetAsync(r->aov_ex.p, 0, aov_ex_bytes(r), r->ctx->stream));
    return CHUNKY_OK;
}

// n passes over the pixel slots of shard T (a single-device target: its own share; member 0 of a group: the caller's share)
// `ex`: chunky_render_aov_passes_ex, which folds the five first-hit images from the same trace
static int aov_passes(chunky_render* r, ShardView T, const int32_t* seeds, int n, int first_buffer_spp, bool ex) {
    LOCK_RENDER(r);
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "aov_passes before set_camera");
    if (int rc = r->aov_pass.ensure(2 * aov_image_bytes(r), r->ctx->stream)) return rc;  // albedo, normal
    if (ex)
        if (int rc = aov_ex_ensure(r)) return rc;
    r->aov_pass.last_launches = 0;
    if (n == 0 || T.n_local <= 0) return CHUNKY_OK;
    SceneView S;
    if (int rc = target_scene_view(r, &S)) return rc;
    int* counter = r->aov_pass.counter();
    char* aov = (char*)r->aov_pass.images.p;
    const size_t plane = (size_t)r->width * r->height;  // words of a one-word image
    AovExImages images{(float*)aov, (float*)(aov + aov_image_bytes(r)), nullptr, nullptr, nullptr, nullptr, nullptr};  // albedo, normal
    if (ex) {
        float* exf = (float*)r->aov_ex.p;
        images.alpha = exf + kAovExOffset[CHUNKY_AOV_ALPHA] * plane;
        images.depth = exf + kAovExOffset[CHUNKY_AOV_DEPTH] * plane;
        images.position = exf + kAovExOffset[CHUNKY_AOV_POSITION] * plane;
        images.emittance = exf + kAovExOffset[CHUNKY_AOV_EMITTANCE] * plane;
        images.block = (int*)exf + kAovExOffset[CHUNKY_AOV_BLOCK] * plane;
    }
    BiomeMap biome;
    const bool tinted = biome_map(r, &biome);  // the albedo is the beauty pass's: tinted by position where that is (aov_biome.hip)
    return first_hit_launches(r, r->aov_pass, seeds, n, first_buffer_spp, [&](const PassSeeds& ps) {  // (each continues the running mean)
        if (tinted && ex) HIP_TRY(launch_aov_ex_biome(r->kernel_variant, S, biome, r->cam, r->opts, T, ps, images, counter, r->ctx->stream, &r->aov_pass.choice));
        else if (tinted) HIP_TRY(launch_aov_biome(r->kernel_variant, S, biome, r->cam, r->opts, T, ps, images.albedo, images.normal, counter, r->ctx->stream, &r->aov_pass.choice));
        else if (ex) HIP_TRY(launch_aov_ex(r->kernel_variant, S, r->cam, r->opts, T, ps, images, counter, r->ctx->stream, &r->aov_pass.choice));
        else HIP_TRY(launch_aov(r->kernel_variant, S, r->cam, r->opts, T, ps, images.albedo, images.normal, counter, r->ctx->stream, &r->aov_pass.choice));
        return (int)CHUNKY_OK;
    });
}

static int aov_passes_entry(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp, bool ex) {
    if (n < 0 || (n > 0 && !seeds) || first_buffer_spp < 0) return fail(CHUNKY_E_INVALID, "aov_passes: bad arguments");
    return on_first_member("aov_passes", r, [&](chunky_render* m, const ShardView& t) { return aov_passes(m, t, seeds, n, first_buffer_spp, ex); });
}

extern "C" int chunky_render_aov_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp) {
    return aov_passes_entry(r, seeds, n, first_buffer_spp, false);
}

extern "C" int chunky_render_aov_passes_ex(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp) {
    return aov_passes_entry(r, seeds, n, first_buffer_spp, true);
}

extern "C" int chunky_render_aov_read(chunky_render* r, int which, float* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_aov_read(r->parts[0], which, out, n);
    LOCK_RENDER(r);
    if (which != CHUNKY_AOV_ALBEDO && which != CHUNKY_AOV_NORMAL) return fail(CHUNKY_E_INVALID, "aov_read: unknown image %d", which);
    const char* aov = (const char*)r->aov_pass.images.p;
    const char* src = aov ? aov + (which == CHUNKY_AOV_NORMAL ? aov_image_bytes(r) : 0) : nullptr;  // null before any AOV pass
    return read_floats("aov_read", r, src, out, n, (int64_t)r->width * r->height * 3);
}

extern "C" int chunky_render_aov_read_ex(chunky_render* r, int which, void* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_aov_read_ex(r->parts[0], which, out, n);
    LOCK_RENDER(r);
    if (which < CHUNKY_AOV_ALBEDO || which > CHUNKY_AOV_BLOCK) return fail(CHUNKY_E_INVALID, "aov_read_ex: unknown image %d", which);
    const int64_t need = (int64_t)r->width * r->height * kAovWords[which];
    const char* aov = (const char*)r->aov_pass.images.p;
    const char* src;  // null before any pass that writes the image
    if (which <= CHUNKY_AOV_NORMAL) src = aov ? aov + (which == CHUNKY_AOV_NORMAL ? aov_image_bytes(r) : 0) : nullptr;
    else src = r->aov_ex.p ? (const char*)r->aov_ex.p + (size_t)kAovExOffset[which] * r->width * r->height * 4 : nullptr;
    return read_floats("aov_read_ex", r, src, out, n, need);
}

extern "C" int chunky_render_aov_reset(chunky_render* r) {
    if (r && !r->parts.empty()) return chunky_render_aov_reset(r->parts[0]);
    LOCK_RENDER(r);
    if (r->aov_pass.images.p) HIP_TRY(hipMemsetAsync(r->aov_pass.images.p, 0, 2 * aov_image_bytes(r), r->ctx->stream));
    if (r->aov_ex.p) HIP_TRY(hipMemsetAsync(r->aov_ex.p, 0, aov_ex_bytes(r), r->ctx->stream));
    return CHUNKY_OK;
}

// ... and of every first-hit pass (capi_matte.hip's too): the record of member 0 on a group
int first_hit_kernel_time(chunky_render* r, FirstHitPass chunky_render::*pass, float* total_ms, int* launches) {
    if (r && !r->parts.empty()) r = r->parts[0];
    LOCK_RENDER(r);
    return (r->*pass).clock.take(total_ms, launches);
}

int first_hit_kernel_info(const char* who, chunky_render* r, FirstHitPass chunky_render::*pass, int32_t out4[4]) {
    if (r && !r->parts.empty()) r = r->parts[0];
    LOCK_RENDER(r);
    if (!out4) return fail(CHUNKY_E_INVALID, "%s: NULL output", who);
    const FirstHitPass& fp = r->*pass;
    out4[0] = fp.choice.tree, out4[1] = fp.choice.bvh;
    out4[2] = fp.choice.blocks, out4[3] = fp.last_launches;
    return CHUNKY_OK;
}

extern "C" int chunky_render_aov_kernel_time(chunky_render* r, float* total_ms, int* launches) {
    return first_hit_kernel_time(r, &chunky_render::aov_pass, total_ms, launches);
}

extern "C" int chunky_render_aov_kernel_info(chunky_render* r, int32_t out4[4]) {
    return first_hit_kernel_info("aov_kernel_info", r, &chunky_render::aov_pass, out4);
}
