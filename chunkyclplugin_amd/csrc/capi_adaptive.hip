// capi_adaptive.hip — adaptive sampling on the device (adaptive_spec.h, adaptive.hip); its host twin is adaptive_host.cpp.
#include "adaptive_host.hpp"
#include "adaptive_spec.h"
#include "capi_internal.hpp"

static int adaptive_tiles(const chunky_render* r) { return ((r->width + 15) / 16) * ((r->height + 15) / 16); }

static int adaptive_ensure(chunky_render* r) {
    const size_t np = (size_t)r->width * r->height;
    DevBuf* bufs[5] = {&r->ad_stat, &r->ad_count, &r->ad_flags, &r->ad_tiles, &r->ad_list};
    const size_t bytes[5] = {np * 8, np * 4, np * 2, ((size_t)adaptive_tiles(r) * 2 + 1) * 4, np * 4};
    for (int i = 0; i < 5; i++) {  // each on its own: a call that failed half way left the others in place
        if (bufs[i]->p) continue;
        HIP_TRY(bufs[i]->alloc(bytes[i]));
    }
    if (!r->ad_total_host) HIP_TRY(hipHostMalloc((void**)&r->ad_total_host, sizeof(int32_t), hipHostMallocDefault));
    return CHUNKY_OK;
}

// what an adaptive call needs of the target: one device, the whole image, and render_pool for the scene and options as they are
static int adaptive_state(const char* who, chunky_render* r, SceneView* S) {
    if (r->shard.world > 1) return fail(CHUNKY_E_STATE, "%s: this target holds rank %d of %d of the image, not all of it", who, r->shard.rank, r->shard.world);
    return needs_render_pool(who, r, S);
}

// one launch over the pixel slots of T — the target's own shard, or a list of pixels — folded with the luminance statistic
static int adaptive_fold(chunky_render* r, const SceneView& S, const ShardView& T, const PassSeeds& ps) {
    StagedFold fold;
    fold.kind = StagedFold::stats;
    fold.stat_image = (float*)r->ad_stat.p;
    HIP_TRY(launch_render_fold(r->kernel_variant, S, r->cam, r->opts, T, ps, r->fb, (int*)r->work_counter.p, r->ctx->stream, &r->last_choice,
                               (float*)r->staging.p, nullptr, fold));
    return CHUNKY_OK;
}

// The loop of the specification (adaptive_spec.h ad_step; chunky_adaptive_host_resume is its host twin) on the state r->ad_state
// towards max_spp.  The state is not resumable while it runs; it is again when the loop ends by itself or at a stop.
static int adaptive_run(chunky_render* r, const char* who, const SceneView& S, const int32_t* seeds, int max_spp, const chunky_adaptive_callbacks& cb,
                        chunky_adaptive_summary* summary_out) {
    hipStream_t st = r->ctx->stream;
    const int np = r->width * r->height, n_tiles = adaptive_tiles(r);
    unsigned char* active = (unsigned char*)r->ad_flags.p;
    unsigned char* unconv = active + np;
    int* tile_counts = (int*)r->ad_tiles.p;
    int* tile_offsets = tile_counts + n_tiles;
    int* total = tile_offsets + n_tiles;
    chunky_adaptive_state& s = r->ad_state;
    const chunky_adaptive_params& p = s.params;
    const float t2 = p.threshold * p.threshold;
    r->ad_valid = false;
    r->ad_resumable = false;
    bool stop = false;
    while (!stop && s.passes < max_spp && s.active > 0) {
        const ad_step_t step = ad_step(s.passes, s.last_check, p.min_spp, p.check_interval, max_spp);
        // every pixel still active: the ordinary block mapping; else the active pixels from the list of the last check (a temporary
        // view with world != 1 and tile != 0, the route of shard_gid through T.list)
        ShardView T = r->shard;
        if (s.active < np) T = ShardView{0, 2, 1, s.active, (const int*)r->ad_list.p, s.active};
        int launched = 0;
        bool opened = false;
        if (!step.check_first) {
            // the staging array before the round's timing bracket opens, so that no allocation is timed (T's cap, not r->launch_cap's)
            int cap = 0;
            if (int rc = stage_fold_launches("adaptive", r, T, step.round, &cap)) return rc;
            // a round longer than the launch cap is several launches, with a poll before each
            const int cut = for_each_launch(seeds + s.passes, step.round, s.passes, cap, [&](const PassSeeds& ps, const int32_t*) {
                if (cb.post_render && cb.post_render(cb.user)) {
                    stop = true;
                    return (int)CHUNKY_E_ABORTED;
                }
                if (!opened) {
                    if (int rc = r->ad_clock.open(st)) return rc;
                    opened = true;
                }
                if (int rc = adaptive_fold(r, S, T, ps)) return rc;
                launched += ps.n;
                return (int)CHUNKY_OK;
            });
            if (cut && !stop) return cut;
            s.summary.samples += (int64_t)s.active * launched;
            s.passes += launched;
            if (launched > 0) s.summary.rounds += 1;
        } else {  // the check the run that stopped here did not make (it ended on its own max_spp): a bracket that counts as no round
            if (int rc = r->ad_clock.open(st)) return rc;
            opened = true;
        }
        const bool check = step.check_first || (launched == step.round && ad_check_due(s.passes, p.min_spp, p.check_interval, max_spp) != 0);
        if (check) {
            HIP_TRY(launch_adaptive_check(r->width, r->height, (const float*)r->ad_stat.p, active, unconv, (int*)r->ad_count.p, s.passes, t2, p.floor,
                                          tile_counts, tile_offsets, (int*)r->ad_list.p, total, st));
            HIP_TRY(hipMemcpyAsync(r->ad_total_host, total, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        if (opened) {
            if (int rc = r->ad_clock.close(st, step.check_first ? 0 : 1)) return rc;
            HIP_TRY(hipStreamSynchronize(st));  // once per round: the host loop needs the total
            if (int rc = r->ad_clock.collect()) return rc;  // (finished: its events go back to the pool for the next round)
        }
        if (check) {
            const int n_active = *r->ad_total_host;
            if (n_active < 0 || n_active > s.active) return fail(CHUNKY_E_HIP, "%s: the compaction reported %d active pixels of %d", who, n_active, s.active);
            s.active = n_active;
            s.last_check = s.passes;
            if (s.summary.checks < CHUNKY_ADAPTIVE_MAX_CHECKS) s.summary.active[s.summary.checks] = n_active;
            s.summary.checks += 1;
        }
        if (!stop && !step.check_first && cb.round_done) cb.round_done(cb.user, s.passes, s.active);
        if (check && !stop && cb.post_render && cb.post_render(cb.user)) stop = true;
    }
    HIP_TRY(launch_adaptive_finish(np, active, (int*)r->ad_count.p, s.passes, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.summary.passes = s.passes;
    r->ad_valid = true;
    r->ad_resumable = true;
    if (summary_out) *summary_out = s.summary;
    if (stop) return fail(CHUNKY_E_ABORTED, "%s: stopped by post_render after %d passes", who, s.passes);
    return CHUNKY_OK;
}

extern "C" int chunky_render_adaptive_ex(chunky_render* r, const int32_t* seeds, int max_spp, const chunky_adaptive_params* params,
                                         const chunky_adaptive_callbacks* callbacks, chunky_adaptive_summary* summary_out) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    chunky_adaptive_params p;
    if (int rc = adaptive_params("render_adaptive", params, max_spp, &p)) return rc;
    chunky_adaptive_callbacks cb;
    if (int rc = adaptive_callbacks("render_adaptive_ex", callbacks, &cb)) return rc;
    if (!seeds) return fail(CHUNKY_E_INVALID, "render_adaptive: NULL seeds");
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive: a group's target (the active list lives on one device)");
    LOCK_RENDER(r);
    SceneView S;
    if (int rc = adaptive_state("render_adaptive", r, &S)) return rc;
    if (int rc = adaptive_ensure(r)) return rc;
    hipStream_t st = r->ctx->stream;
    const int np = r->width * r->height;
    r->ad_valid = false;
    r->ad_resumable = false;
    HIP_TRY(hipMemsetAsync(r->fb, 0, (size_t)np * 3 * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(r->ad_stat.p, 0, r->ad_stat.bytes, st));
    HIP_TRY(hipMemsetAsync(r->ad_count.p, 0, r->ad_count.bytes, st));
    HIP_TRY(hipMemsetAsync(r->ad_flags.p, 1, (size_t)np, st));
    adaptive_empty_state(r->width, r->height, p, &r->ad_state);
    return adaptive_run(r, "render_adaptive", S, seeds, max_spp, cb, summary_out);
}

extern "C" int chunky_render_adaptive(chunky_render* r, const int32_t* seeds, int max_spp, const chunky_adaptive_params* params,
                                      chunky_adaptive_summary* summary_out) {
    return chunky_render_adaptive_ex(r, seeds, max_spp, params, nullptr, summary_out);
}

extern "C" int chunky_render_adaptive_resume(chunky_render* r, const int32_t* seeds, int max_spp, const chunky_adaptive_params* params,
                                             const chunky_adaptive_callbacks* callbacks, chunky_adaptive_summary* summary_out) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    chunky_adaptive_params p;
    if (int rc = adaptive_params("render_adaptive_resume", params, INT32_MAX, &p)) return rc;  // (a state stopped before min_spp goes on too)
    chunky_adaptive_callbacks cb;
    if (int rc = adaptive_callbacks("render_adaptive_resume", callbacks, &cb)) return rc;
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive_resume: a group's target (the active list lives on one device)");
    LOCK_RENDER(r);
    SceneView S;
    if (int rc = adaptive_state("render_adaptive_resume", r, &S)) return rc;
    if (!r->ad_resumable)
        return fail(CHUNKY_E_STATE, "render_adaptive_resume: the target holds no adaptive state to continue (none was left, or the framebuffer, the camera, "
                                    "the options, the shard or the buffer changed since)");
    const chunky_adaptive_state& s = r->ad_state;
    if (!same_adaptive_params(p, s.params))
        return fail(CHUNKY_E_STATE, "render_adaptive_resume: the parameters differ from those of the state (threshold %g, floor %g, min_spp %d, check_interval %d)",
                    (double)s.params.threshold, (double)s.params.floor, s.params.min_spp, s.params.check_interval);
    if (max_spp < s.passes) return fail(CHUNKY_E_INVALID, "render_adaptive_resume: max_spp %d is below the %d passes the state holds", max_spp, s.passes);
    if (max_spp == s.passes || s.active == 0) {  // nothing to render
        if (summary_out) *summary_out = s.summary;
        return CHUNKY_OK;
    }
    if (!seeds) return fail(CHUNKY_E_INVALID, "render_adaptive_resume: NULL seeds");
    if (int rc = adaptive_ensure(r)) return rc;
    return adaptive_run(r, "render_adaptive_resume", S, seeds, max_spp, cb, summary_out);
}

extern "C" int chunky_render_adaptive_state(chunky_render* r, chunky_adaptive_state* out, uint8_t* active_out, int64_t n) {
    if (r && !r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive_state: a group's target has no adaptive run");
    LOCK_RENDER(r);
    if (!r->ad_resumable) return fail(CHUNKY_E_STATE, "render_adaptive_state: the target holds no adaptive state to continue");
    if (!out) return fail(CHUNKY_E_INVALID, "render_adaptive_state: NULL output");
    if (out->size < kAdaptiveStateFirst)
        return fail(CHUNKY_E_INVALID, "render_adaptive_state: out->size %zu is smaller than the struct (%zu): set it to sizeof(chunky_adaptive_state)", out->size, kAdaptiveStateFirst);
    if (active_out) {
        if (n != (int64_t)r->width * r->height) return fail(CHUNKY_E_INVALID, "render_adaptive_state: the map has %lld bytes, got %lld", (long long)r->width * r->height, (long long)n);
        HIP_TRY(hipMemcpyAsync(active_out, r->ad_flags.p, (size_t)n, hipMemcpyDeviceToHost, r->ctx->stream));
        HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    }
    give_versioned(r->ad_state, out);
    return CHUNKY_OK;
}

extern "C" int chunky_render_adaptive_restore(chunky_render* r, const chunky_adaptive_state* st, const float* mean, const int32_t* count,
                                              const float* stat, const uint8_t* active) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    if (!st || !mean || !count || !stat || !active) return fail(CHUNKY_E_INVALID, "render_adaptive_restore: NULL argument");
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive_restore: a group's target (the active list lives on one device)");
    LOCK_RENDER(r);
    SceneView S;
    if (int rc = adaptive_state("render_adaptive_restore", r, &S)) return rc;
    chunky_adaptive_state s;
    if (int rc = adaptive_state_valid("render_adaptive_restore", st, count, active, &s)) return rc;
    if (s.width != r->width || s.height != r->height)
        return fail(CHUNKY_E_INVALID, "render_adaptive_restore: a state of %d x %d on a target of %d x %d", s.width, s.height, r->width, r->height);
    if (int rc = adaptive_ensure(r)) return rc;
    hipStream_t stream = r->ctx->stream;
    const size_t np = (size_t)r->width * r->height;
    const int n_tiles = adaptive_tiles(r);
    int* tile_counts = (int*)r->ad_tiles.p;
    int* tile_offsets = tile_counts + n_tiles;
    int* total = tile_offsets + n_tiles;
    r->ad_valid = false;
    r->ad_resumable = false;
    HIP_TRY(hipMemcpyAsync(r->fb, mean, np * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r->ad_count.p, count, np * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r->ad_stat.p, stat, np * 2 * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(r->ad_flags.p, active, np, hipMemcpyHostToDevice, stream));
    // the list of the active pixels, in the order the run that left this map held it: counted, scanned and scattered on the device
    HIP_TRY(launch_adaptive_rebuild(r->width, r->height, (unsigned char*)r->ad_flags.p, tile_counts, tile_offsets, (int*)r->ad_list.p, total, stream));
    HIP_TRY(hipMemcpyAsync(r->ad_total_host, total, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));  // the caller may reuse its arrays on return (not timed: chunky_render_adaptive_kernel_time is about rounds)
    if (*r->ad_total_host != s.active)
        return fail(CHUNKY_E_HIP, "render_adaptive_restore: the device counted %d active pixels, the state holds %d", *r->ad_total_host, s.active);
    r->ad_state = s;
    r->ad_valid = true;
    r->ad_resumable = true;
    return CHUNKY_OK;
}

extern "C" int chunky_render_adaptive_counts(chunky_render* r, int32_t* out, int64_t n) {
    if (r && !r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive_counts: a group's target has no adaptive run");
    LOCK_RENDER(r);
    return read_floats("render_adaptive_counts", r, r->ad_valid ? r->ad_count.p : nullptr, out, n, (int64_t)r->width * r->height);  // (ints)
}

extern "C" int chunky_render_adaptive_noise(chunky_render* r, float* out, int64_t n_floats) {
    if (r && !r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive_noise: a group's target has no adaptive run");
    LOCK_RENDER(r);
    return read_floats("render_adaptive_noise", r, r->ad_valid ? r->ad_stat.p : nullptr, out, n_floats, (int64_t)r->width * r->height * 2);
}

extern "C" int chunky_render_adaptive_kernel_time(chunky_render* r, float* total_ms, int* rounds) {
    if (r && !r->parts.empty()) return fail(CHUNKY_E_STATE, "render_adaptive_kernel_time: a group's target has no adaptive run");
    LOCK_RENDER(r);
    return r->ad_clock.take(total_ms, rounds);
}

extern "C" int chunky_selftest_render_list(chunky_render* r, const int32_t* pixels, int n_pixels, const int32_t* seeds, int n) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    if (n < 0 || n_pixels < 0 || (n > 0 && !seeds) || (n_pixels > 0 && !pixels)) return fail(CHUNKY_E_INVALID, "selftest_render_list: bad arguments");
    if (!r->parts.empty()) return fail(CHUNKY_E_STATE, "selftest_render_list: a group's target");
    LOCK_RENDER(r);
    const int np = r->width * r->height;
    if (n_pixels > np) return fail(CHUNKY_E_INVALID, "selftest_render_list: %d pixels listed, the image has %d", n_pixels, np);
    std::vector<unsigned char> seen((size_t)np, 0);
    for (int i = 0; i < n_pixels; i++) {
        if (pixels[i] < 0 || pixels[i] >= np || seen[pixels[i]]) return fail(CHUNKY_E_INVALID, "selftest_render_list: entry %d (%d) is outside the image or listed twice", i, pixels[i]);
        seen[pixels[i]] = 1;
    }
    SceneView S;
    if (int rc = adaptive_state("selftest_render_list", r, &S)) return rc;
    if (int rc = adaptive_ensure(r)) return rc;
    if (n == 0 || n_pixels == 0) return CHUNKY_OK;
    hipStream_t st = r->ctx->stream;
    r->ad_valid = false;  // the statistic and the list are overwritten
    r->ad_resumable = false;
    HIP_TRY(hipMemsetAsync(r->ad_stat.p, 0, r->ad_stat.bytes, st));
    HIP_TRY(hipMemcpyAsync(r->ad_list.p, pixels, (size_t)n_pixels * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // the caller may reuse its array on return
    const ShardView T{0, 2, 1, n_pixels, (const int*)r->ad_list.p, n_pixels};
    int cap = 0;
    if (int rc = stage_fold_launches("adaptive", r, T, n, &cap)) return rc;
    if (int rc = r->ad_clock.open(st)) return rc;
    if (int rc = for_each_launch(seeds, n, 0, cap, [&](const PassSeeds& ps, const int32_t*) { return adaptive_fold(r, S, T, ps); })) return rc;
    if (int rc = r->ad_clock.close(st)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return r->ad_clock.collect();
}
