// capi_lights.hip — light groups: the sky's, the sun's and the emitters' share of the beauty image (lights.hip).
#include "capi_internal.hpp"

constexpr int kLightImages = 4;  // CHUNKY_LIGHT_SKY, _SUN, _EMITTERS, _ALL
static_assert(CHUNKY_LIGHT_SKY == 0 && CHUNKY_LIGHT_SUN == 1 && CHUNKY_LIGHT_EMITTERS == 2 && CHUNKY_LIGHT_ALL == 3, "the images lie in this order");

static float* light_image(const chunky_render* r, int which) { return (float*)((char*)r->light_pass.images.p + (size_t)which * aov_image_bytes(r)); }

// ---- emitter groups (chunky_render_light_set_emitter_groups): r->light_groups holds, in this order, the group images, the per-sample
// sums (3 * groups floats per pixel), the touched words (one per pixel) and the table's bytes
static_assert(CHUNKY_LIGHT_MAX_EMITTER_GROUPS == kLightMaxGroups, "the header's limit is the kernel's");
static size_t light_group_pixels(const chunky_render* r) { return (size_t)r->width * r->height; }
static size_t light_group_state_bytes(const chunky_render* r, int n_groups) {  // images, sums, touched words
    return (size_t)n_groups * aov_image_bytes(r) * 2 + light_group_pixels(r) * sizeof(int);
}
static LightGroupImages light_group_images(const chunky_render* r) {
    const int n = r->light_table.n_groups;
    char* base = (char*)r->light_groups.p;
    LightGroupImages G;
    G.n_groups = n;
    G.images = (float*)base;
    G.acc = (float*)(base + (size_t)n * aov_image_bytes(r));
    G.touched = (int*)(base + (size_t)n * aov_image_bytes(r) * 2);
    G.of_block = (const unsigned char*)(base + light_group_state_bytes(r, n));
    G.n_blocks = (int)r->light_table.of_block.size();
    G.world_group = r->light_table.world, G.actor_group = r->light_table.actor;
    return G;
}

// n passes over the pixel slots of shard T (a single-device target: its own share; member 0 of a group: the caller's share)
static int light_passes(chunky_render* r, ShardView T, const int32_t* seeds, int n, int first_buffer_spp) {
    LOCK_RENDER(r);
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "light_passes before set_camera");
    if (opts_extended(r->opts))  // they change what the beauty image is, and this pass walks the reference's path only
        return fail(CHUNKY_E_STATE, "light_passes: not with CHUNKY_OPT_SUN_SAMPLING, _EMITTERS, _BSDF or _EMITTER_NEE away from their defaults");
    if (int rc = refuse_biome("light_passes", r)) return rc;  // (before anything is allocated)
    if (int rc = refuse_fog("light_passes", r)) return rc;
    if (int rc = refuse_glass("light_passes", r)) return rc;
    const bool groups = r->light_table.n_groups > 0;
    if (groups && !std::isfinite(r->opts.emitter_scale))  // 0 * inf: the specification of a group would be NaN wherever another group is hit
        return fail(CHUNKY_E_STATE, "light_passes: emitter groups are set and CHUNKY_OPT_EMITTER_SCALE is not finite");
    if (int rc = r->light_pass.ensure(kLightImages * aov_image_bytes(r), r->ctx->stream)) return rc;
    if (groups) r->light_groups_rendered = true;
    r->light_pass.last_launches = 0;
    if (n == 0 || T.n_local <= 0) return CHUNKY_OK;
    SceneView S;
    if (int rc = target_scene_view(r, &S)) return rc;
    float* images[kLightImages];
    for (int g = 0; g < kLightImages; g++) images[g] = light_image(r, g);
    int* counter = r->light_pass.counter();
    return first_hit_launches(r, r->light_pass, seeds, n, first_buffer_spp, [&](const PassSeeds& ps) {  // (each continues the running means)
        if (groups)
            HIP_TRY(launch_light_groups(r->kernel_variant, S, r->cam, r->opts, T, ps, images, light_group_images(r), counter, r->ctx->stream, &r->light_pass.choice));
        else
            HIP_TRY(launch_lights(r->kernel_variant, S, r->cam, r->opts, T, ps, images, counter, r->ctx->stream, &r->light_pass.choice));
        return (int)CHUNKY_OK;
    });
}

extern "C" int chunky_render_light_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp) {
    if (n < 0 || (n > 0 && !seeds) || first_buffer_spp < 0) return fail(CHUNKY_E_INVALID, "light_passes: bad arguments");
    return on_first_member("light_passes", r, [&](chunky_render* m, const ShardView& t) { return light_passes(m, t, seeds, n, first_buffer_spp); });
}

extern "C" int chunky_render_light_read(chunky_render* r, int which, float* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_light_read(r->parts[0], which, out, n);
    LOCK_RENDER(r);
    if (which < CHUNKY_LIGHT_SKY || which > CHUNKY_LIGHT_ALL) return fail(CHUNKY_E_INVALID, "light_read: unknown image %d", which);
    const float* src = r->light_pass.images.p ? light_image(r, which) : nullptr;  // null before any pass
    return read_floats("light_read", r, src, out, n, (int64_t)r->width * r->height * 3);
}

extern "C" int chunky_render_light_mix(chunky_render* r, const float w[3], float* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_light_mix(r->parts[0], w, out, n);
    LOCK_RENDER(r);
    if (!w || !std::isfinite(w[0]) || !std::isfinite(w[1]) || !std::isfinite(w[2])) return fail(CHUNKY_E_INVALID, "light_mix: three finite weights are needed");
    const int64_t need = (int64_t)r->width * r->height * 3;
    if (!out || n != need) return fail(CHUNKY_E_INVALID, "light_mix: need %lld floats, got %lld", (long long)need, (long long)n);
    if (!r->light_pass.images.p) return fail(CHUNKY_E_STATE, "light_mix before any light pass");
    if (!r->light_mix.p) HIP_TRY(r->light_mix.alloc(aov_image_bytes(r)));
    HIP_TRY(launch_light_mix(light_image(r, CHUNKY_LIGHT_SKY), light_image(r, CHUNKY_LIGHT_SUN), light_image(r, CHUNKY_LIGHT_EMITTERS), w, (float*)r->light_mix.p, need,
                             r->ctx->stream));
    return read_floats("light_mix", r, r->light_mix.p, out, n, need);
}

extern "C" int chunky_render_light_reset(chunky_render* r) {
    if (r && !r->parts.empty()) return chunky_render_light_reset(r->parts[0]);
    LOCK_RENDER(r);
    if (r->light_pass.images.p) HIP_TRY(hipMemsetAsync(r->light_pass.images.p, 0, kLightImages * aov_image_bytes(r), r->ctx->stream));
    if (r->light_groups.p) HIP_TRY(hipMemsetAsync(r->light_groups.p, 0, (size_t)r->light_table.n_groups * aov_image_bytes(r), r->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_render_light_set_emitter_groups(chunky_render* r, int n_groups, const int32_t* ids, const uint8_t* group_of, int n_ids) {
    if (r && !r->parts.empty()) return chunky_render_light_set_emitter_groups(r->parts[0], n_groups, ids, group_of, n_ids);
    LOCK_RENDER(r);
    LightGroupTable table;
    if (int rc = light_group_table("light_set_emitter_groups", n_groups, ids, group_of, n_ids, (int64_t)r->scene->host_blocks.size(), &table)) return rc;
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // (a pass under way may still read the buffer this call replaces)
    r->light_groups_rendered = false;
    r->light_table = LightGroupTable();
    r->light_groups.release();
    if (n_groups == 0) return CHUNKY_OK;
    const size_t state = light_group_state_bytes(r, n_groups), bytes = state + table.of_block.size();
    HIP_TRY(r->light_groups.alloc(bytes + 4));
    HIP_TRY(hipMemsetAsync(r->light_groups.p, 0, state, r->ctx->stream));
    if (!table.of_block.empty())
        HIP_TRY(hipMemcpyAsync((char*)r->light_groups.p + state, table.of_block.data(), table.of_block.size(), hipMemcpyHostToDevice, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // (the copy's source goes out of use here)
    r->light_table = std::move(table);
    return CHUNKY_OK;
}

// CHUNKY_E_STATE unless groups are set and a pass has run with them
static int light_groups_ready(const char* who, const chunky_render* r) {
    if (r->light_table.n_groups == 0) return fail(CHUNKY_E_STATE, "%s: no emitter groups are set", who);
    if (!r->light_groups_rendered || !r->light_pass.images.p) return fail(CHUNKY_E_STATE, "%s before a light pass with the groups set", who);
    return CHUNKY_OK;
}

extern "C" int chunky_render_light_read_group(chunky_render* r, int group, float* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_light_read_group(r->parts[0], group, out, n);
    LOCK_RENDER(r);
    if (int rc = light_groups_ready("light_read_group", r)) return rc;
    if (group < 0 || group >= r->light_table.n_groups) return fail(CHUNKY_E_INVALID, "light_read_group: group %d of %d", group, r->light_table.n_groups);
    const float* src = (const float*)((const char*)r->light_groups.p + (size_t)group * aov_image_bytes(r));
    return read_floats("light_read_group", r, src, out, n, (int64_t)r->width * r->height * 3);
}

extern "C" int chunky_render_light_mix_groups(chunky_render* r, float w_sky, float w_sun, const float* w_groups, int n_groups, float* out, int64_t n) {
    if (r && !r->parts.empty()) return chunky_render_light_mix_groups(r->parts[0], w_sky, w_sun, w_groups, n_groups, out, n);
    LOCK_RENDER(r);
    if (!w_groups || !std::isfinite(w_sky) || !std::isfinite(w_sun)) return fail(CHUNKY_E_INVALID, "light_mix_groups: finite weights are needed");
    if (n_groups < 0 || n_groups > CHUNKY_LIGHT_MAX_EMITTER_GROUPS) return fail(CHUNKY_E_INVALID, "light_mix_groups: %d group weights", n_groups);
    for (int g = 0; g < n_groups; g++)
        if (!std::isfinite(w_groups[g])) return fail(CHUNKY_E_INVALID, "light_mix_groups: finite weights are needed");
    const int64_t need = (int64_t)r->width * r->height * 3;
    if (!out || n != need) return fail(CHUNKY_E_INVALID, "light_mix_groups: need %lld floats, got %lld", (long long)need, (long long)n);
    if (int rc = light_groups_ready("light_mix_groups", r)) return rc;
    if (n_groups != r->light_table.n_groups) return fail(CHUNKY_E_INVALID, "light_mix_groups: %d weights for %d groups", n_groups, r->light_table.n_groups);
    if (!r->light_mix.p) HIP_TRY(r->light_mix.alloc(aov_image_bytes(r)));
    HIP_TRY(launch_light_group_mix(light_image(r, CHUNKY_LIGHT_SKY), light_image(r, CHUNKY_LIGHT_SUN), (const float*)r->light_groups.p, n_groups, w_sky, w_sun, w_groups,
                                   (float*)r->light_mix.p, need, r->ctx->stream));
    return read_floats("light_mix_groups", r, r->light_mix.p, out, n, need);
}

extern "C" int chunky_render_light_kernel_time(chunky_render* r, float* total_ms, int* launches) {
    return first_hit_kernel_time(r, &chunky_render::light_pass, total_ms, launches);
}

extern "C" int chunky_render_light_kernel_info(chunky_render* r, int32_t out4[4]) {
    return first_hit_kernel_info("light_kernel_info", r, &chunky_render::light_pass, out4);
}
