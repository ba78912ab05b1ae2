// capi_render.hip — the render target: camera, options, shard, buffer, the pass launcher and its clock, read-back, timing, preview, records.
#include "capi_internal.hpp"

static_assert(sizeof(chunky_hit_record) == sizeof(HitRecord), "record layouts must agree");
static_assert(CHUNKY_MAX_TRACES == kMaxTraces, "trace capacity must agree");

// every member takes its share of the caller's own share (shard_map.hpp member_shard).  All or nothing: a group whose world * members
// does not fit an int, or one member of which would need more slots than an int holds, is refused before any member changes
static int group_apply_shards(chunky_render* r, const ShardView& outer) {
    const int n = (int)r->parts.size();
    std::vector<ShardView> share((size_t)n);
    for (int i = 0; i < n; i++) {
        ShardView& m = share[(size_t)i];
        if (!member_shard(outer, i, n, &m))
            return fail(CHUNKY_E_INVALID, "set_shard: world %d x %d group members does not fit an int", outer.world, n);
        ShardView stored;
        if (!make_shard_view(r->width, r->height, m.rank, m.world, m.tile, &stored))
            return fail(CHUNKY_E_INVALID, "set_shard: rank %d of %d in 16 x 16 blocks of a %d x %d image needs more than 2^31 pixel slots", m.rank, m.world, r->width, r->height);
    }
    for (int i = 0; i < n; i++)
        if (int rc = chunky_render_set_shard(r->parts[(size_t)i], share[(size_t)i].rank, share[(size_t)i].world, share[(size_t)i].tile)) return rc;
    r->outer = outer;
    return CHUNKY_OK;
}

extern "C" int chunky_render_create(chunky_ctx* ctx, chunky_scene* scene, int width, int height, chunky_render** out) {
    if (!ctx || !scene || !out) return fail(CHUNKY_E_INVALID, "chunky_render_create: NULL argument");
    if (scene->ctx != ctx) return fail(CHUNKY_E_INVALID, "scene belongs to another context");
    if (width <= 0 || height <= 0 || (int64_t)width * height > (1 << 30))
        return fail(CHUNKY_E_INVALID, "bad image size %dx%d", width, height);
    if (!ctx->members.empty()) {
        std::lock_guard<std::recursive_mutex> g(ctx->mu);
        if (scene->replicas.size() != ctx->members.size()) return fail(CHUNKY_E_STATE, "chunky_render_create: the scene has been destroyed");
        std::unique_ptr<chunky_render> r(new chunky_render);
        r->ctx = ctx;
        r->scene = scene;
        r->width = width;
        r->height = height;
        int rc = CHUNKY_OK;
        for (size_t i = 0; i < ctx->members.size() && rc == CHUNKY_OK; i++) {
            chunky_render* part = nullptr;
            rc = chunky_render_create(ctx->members[i], scene->replicas[i], width, height, &part);
            if (rc == CHUNKY_OK) r->parts.push_back(part);
        }
        if (rc == CHUNKY_OK) rc = group_apply_shards(r.get(), r->outer);
        if (rc != CHUNKY_OK) {
            for (chunky_render* part : r->parts) (void)chunky_render_destroy(part);
            return rc;
        }
        r->gather_send.resize(ctx->members.size());
        r->gather_recv.resize(ctx->members.size());
        scene->refs++;
        *out = r.release();
        return CHUNKY_OK;
    }
    std::lock_guard<std::recursive_mutex> g(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<chunky_render> r(new chunky_render);
    r->ctx = ctx;
    r->scene = scene;
    r->width = width;
    r->height = height;
    size_t bytes = (size_t)width * height * 3 * sizeof(float);
    HIP_TRY(r->own_fb.alloc(bytes));
    r->fb = (float*)r->own_fb.p;
    HIP_TRY(hipMemsetAsync(r->fb, 0, bytes, ctx->stream));
    // [0] the sample / pixel queue, [2..49] the phase profile, [64..127] render_pool's range counters (render_pool.hip xcd_claim)
    HIP_TRY(r->work_counter.alloc(512));
    HIP_TRY(hipMemsetAsync(r->work_counter.p, 0, 512, ctx->stream));
    r->shard = ShardView{0, 1, 256, width * height};
    scene->refs++;
    *out = r.release();
    return CHUNKY_OK;
}

extern "C" int chunky_render_destroy(chunky_render* r) {
    if (r && !r->parts.empty()) {
        int rc = each_part(r, [&](chunky_render* m_) { return chunky_render_destroy(m_); });
        {
            std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
            for (size_t i = 0; i < r->gather_send.size(); i++) {  // each buffer is freed on the device it lives on
                (void)hipSetDevice(r->ctx->members[i]->device);
                r->gather_send[i].release();
                (void)hipSetDevice(r->ctx->members[0]->device);
                r->gather_recv[i].release();
            }
            scene_unref(r->scene);
        }
        delete r;
        return rc;
    }
    LOCK_RENDER(r);
    (void)hipStreamSynchronize(r->ctx->stream);
    scene_unref(r->scene);
    delete r;
    return CHUNKY_OK;
}

// the frame-dependent words of r's camera, from r's window (the identity while none is set): the target's own size, the CANVAS's
// two floats (the expressions of K/rayTracer.cl:66-67 on the canvas's dimensions) and the window's fields (canvas_window.h)
static void apply_canvas(chunky_render* r) {
    CameraView& c = r->cam;
    const int cw = r->canvas_width ? r->canvas_width : r->width, ch = r->canvas_height ? r->canvas_height : r->height;
    c.width = r->width;
    c.height = r->height;
    c.half_width = (float)(cw / (2.0 * ch));  // K/rayTracer.cl:66
    c.inv_height = (float)(1.0 / ch);         // K/rayTracer.cl:67
    const RtWindow w = rt_make_window(r->width, cw, ch, r->canvas_x0, r->canvas_y0);
    c.x0 = w.x0, c.y0 = w.y0, c.row_skip = w.row_skip, c.gid0 = w.gid0, c.canvas_height = w.canvas_height;
}

extern "C" int chunky_render_set_canvas(chunky_render* r, int canvas_width, int canvas_height, int x0, int y0) {
    if (r && !r->parts.empty()) {
        // every member or none: the checks are the same on each (one size, one camera), so the group's own copy is checked first
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        if (int rc = check_canvas("set_canvas", r->width, r->height, canvas_width, canvas_height, x0, y0, r->parts[0]->have_camera ? r->parts[0]->cam.projector_type : 0))
            return rc;
        return each_part(r, [&](chunky_render* m_) { return chunky_render_set_canvas(m_, canvas_width, canvas_height, x0, y0); });
    }
    LOCK_RENDER(r);
    if (int rc = check_canvas("set_canvas", r->width, r->height, canvas_width, canvas_height, x0, y0, r->have_camera ? r->cam.projector_type : 0)) return rc;
    const bool identity = canvas_width == r->width && canvas_height == r->height;  // (inside the canvas: the offsets are 0)
    r->canvas_width = identity ? 0 : canvas_width;
    r->canvas_height = identity ? 0 : canvas_height;
    r->canvas_x0 = x0, r->canvas_y0 = y0;
    apply_canvas(r);  // (the camera travels by value in the kernel arguments: launches already queued keep the window they had)
    r->ad_resumable = false;  // what a pass renders changes: an adaptive run cannot continue across it
    return CHUNKY_OK;
}

extern "C" int chunky_render_canvas(chunky_render* r, int32_t out4[4]) {
    if (r && !r->parts.empty()) {
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        return chunky_render_canvas(r->parts[0], out4);
    }
    LOCK_RENDER(r);
    if (!out4) return fail(CHUNKY_E_INVALID, "render_canvas: NULL output");
    out4[0] = r->canvas_width ? r->canvas_width : r->width;
    out4[1] = r->canvas_height ? r->canvas_height : r->height;
    out4[2] = r->canvas_x0, out4[3] = r->canvas_y0;
    return CHUNKY_OK;
}

extern "C" int chunky_render_set_camera(chunky_render* r, int projector_type, const float* settings, int64_t n) {
    FAN_RENDER(r, chunky_render_set_camera(m_, projector_type, settings, n));
    LOCK_RENDER(r);
    if (!settings) return fail(CHUNKY_E_INVALID, "set_camera: NULL settings");
    CameraView& c = r->cam;
    if (projector_type == 0) {
        if (n != 15) return fail(CHUNKY_E_INVALID, "set_camera: pinhole needs 15 floats, got %lld", (long long)n);
        memcpy(c.pos, settings, 12);
        memcpy(c.m, settings + 3, 36);
        c.aperture = settings[12];
        c.subject_distance = settings[13];
        c.fov_tan = settings[14];
        c.rays = nullptr;
    } else if (projector_type == -1) {
        int64_t need = (int64_t)r->width * r->height * 6;
        if (n != need) return fail(CHUNKY_E_INVALID, "set_camera: pre-generated rays need %lld floats, got %lld", (long long)need, (long long)n);
        HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // rays may still be read by queued passes
        r->ad_resumable = false;  // (before the table changes: an upload that fails half way has changed it too)
        HIP_TRY(r->rays.upload(settings, (size_t)n * 4, r->ctx->stream));
        c.rays = (const float*)r->rays.p;
    } else if (is_projected_type(projector_type)) {
        if (int rc = check_projected("set_camera", projector_type, settings, n, r->canvas_height ? r->canvas_height : r->height)) return rc;
        memcpy(c.pos, settings, 12);
        memcpy(c.m, settings + 3, 36);
        c.aperture = 0.0f;  // no lens until chunky_render_set_lens
        c.subject_distance = settings[13];  // (CameraView: settings[13] / [14] of a projected camera)
        c.fov_tan = settings[14];
        c.rays = nullptr;
    } else {
        return fail(CHUNKY_E_INVALID, "set_camera: projector type %d is not supported (-1 to 5, 7, 8)", projector_type);
    }
    apply_canvas(r);  // (behind every check: a refused call leaves the camera as it was)
    c.lens_focus = 0.0f;
    c.projector_type = projector_type;
    r->have_camera = true;
    r->ad_resumable = false;  // what a pass renders changes: an adaptive run cannot continue across it
    return CHUNKY_OK;
}

extern "C" int chunky_render_set_lens(chunky_render* r, float aperture, float focus) {
    FAN_RENDER(r, chunky_render_set_lens(m_, aperture, focus));
    LOCK_RENDER(r);
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "set_lens before set_camera");
    if (r->cam.projector_type <= 0)
        return fail(CHUNKY_E_STATE, "set_lens: projector type %d has its own aperture or table; the lens is for the projected cameras", r->cam.projector_type);
    if (int rc = check_lens("set_lens", aperture, focus)) return rc;
    r->cam.aperture = aperture;
    r->cam.lens_focus = aperture > 0.0f ? focus : 0.0f;
    r->ad_resumable = false;  // what a pass renders changes
    return CHUNKY_OK;
}

extern "C" int chunky_render_set_option(chunky_render* r, int option, int32_t value) {
    FAN_RENDER(r, chunky_render_set_option(m_, option, value));
    LOCK_RENDER(r);
    switch (option) {
        case CHUNKY_OPT_DRAW_DEPTH:
            if (value < 0) return fail(CHUNKY_E_INVALID, "draw depth must be >= 0");
            r->opts.draw_depth = value;
            break;
        case CHUNKY_OPT_MAX_DEPTH:
            if (value < 1 || value > 255) return fail(CHUNKY_E_INVALID, "max depth must be in 1..255");
            r->opts.max_depth = value;
            break;
        case CHUNKY_OPT_EMITTER_SCALE: r->opts.emitter_scale = bits_to_float(value); break;
        case CHUNKY_OPT_KERNEL: r->kernel_variant = value; break;
        case CHUNKY_OPT_SUN_SAMPLING:
            if (value < -1 || value > 1) return fail(CHUNKY_E_INVALID, "sun sampling: -1 (as the reference), 0 or 1");
            r->opts.sun_sampling = value;
            break;
        case CHUNKY_OPT_EMITTERS:
            if (value != 0 && value != 1) return fail(CHUNKY_E_INVALID, "emitters: 0 or 1");
            r->opts.emitters = value;
            break;
        case CHUNKY_OPT_BSDF:
            if (value != 0 && value != 1) return fail(CHUNKY_E_INVALID, "bsdf: 0 or 1");
            r->opts.bsdf = value;
            break;
        case CHUNKY_OPT_EMITTER_NEE:
            if (value != 0 && value != 1) return fail(CHUNKY_E_INVALID, "emitter NEE: 0 or 1");
            r->opts.nee = value;
            break;
        case CHUNKY_OPT_BVH_CULL_BEHIND:
            if (value != 0 && value != 1) return fail(CHUNKY_E_INVALID, "BVH cull: 0 or 1");
            r->opts.bvh_cull = value;
            break;
        case CHUNKY_OPT_BIOME_TINT:
            if (value != 0 && value != 1) return fail(CHUNKY_E_INVALID, "biome tint: 0 or 1");
            r->biome_tint = value;
            break;
        default: return fail(CHUNKY_E_INVALID, "unknown option %d", option);
    }
    r->ad_resumable = false;  // (an option was set: a refused call ends nothing)
    return CHUNKY_OK;
}

extern "C" int chunky_render_set_shard(chunky_render* r, int rank, int world, int tile) {
    if (r && !r->parts.empty()) {
        if (world < 1 || rank < 0 || rank >= world || tile < 0) return fail(CHUNKY_E_INVALID, "set_shard: rank %d / world %d / tile %d", rank, world, tile);
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        // (the run length clamped as on a single target below; n_local stays 0: the members hold the slots)
        return group_apply_shards(r, ShardView{rank, world, clamp_tile(r->width, r->height, tile), 0});
    }
    LOCK_RENDER(r);
    if (world < 1 || rank < 0 || rank >= world || tile < 0) return fail(CHUNKY_E_INVALID, "set_shard: rank %d / world %d / tile %d", rank, world, tile);
    // The view is stored with its run length clamped to the pixel count (shard_map.hpp make_shard_view): the device functions never
    // see a larger one, which is what keeps shard_gid's products within an int.
    ShardView t;
    if (!make_shard_view(r->width, r->height, rank, world, tile, &t))
        return fail(CHUNKY_E_INVALID, "set_shard: rank %d of %d in 16 x 16 blocks of a %d x %d image needs more than 2^31 pixel slots", rank, world, r->width, r->height);
    if (r->shard.list) HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // queued launches may still read the old list
    r->block_list.release();
    r->shard = t;
    r->ad_resumable = false;
    r->launch_cap = 0;  // the share changed: so does what a launch can stage
    return CHUNKY_OK;
}

extern "C" int chunky_render_set_device_buffer(chunky_render* r, void* device_ptr) {
    if (r && !r->parts.empty()) return chunky_render_set_device_buffer(r->parts[0], device_ptr);  // the image lives on member 0
    LOCK_RENDER(r);
    r->ad_resumable = false;  // the image an adaptive run would continue stays in the other buffer
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    r->fb = device_ptr ? (float*)device_ptr : (float*)r->own_fb.p;
    return CHUNKY_OK;
}

extern "C" int chunky_render_device_buffer(chunky_render* r, void** device_ptr) {
    if (r && !r->parts.empty()) return chunky_render_device_buffer(r->parts[0], device_ptr);
    LOCK_RENDER(r);
    if (!device_ptr) return fail(CHUNKY_E_INVALID, "NULL out pointer");
    *device_ptr = r->fb;
    return CHUNKY_OK;
}

extern "C" int chunky_render_reset(chunky_render* r) {
    FAN_RENDER(r, chunky_render_reset(m_));
    LOCK_RENDER(r);
    r->ad_resumable = false;
    HIP_TRY(hipMemsetAsync(r->fb, 0, (size_t)r->width * r->height * 3 * sizeof(float), r->ctx->stream));
    return CHUNKY_OK;
}

LaunchClock::~LaunchClock() {
    for (Bracket& b : pending) {
        (void)hipEventDestroy(b.e0);
        (void)hipEventDestroy(b.e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
}

int LaunchClock::open(hipStream_t stream) {
    for (hipEvent_t* e : {&e0, &e1}) {
        if (*e) continue;  // left by a bracket that was never closed
        if (pool->empty()) {
            HIP_TRY(hipEventCreate(e));
        } else {
            *e = pool->back();
            pool->pop_back();
        }
    }
    HIP_TRY(hipEventRecord(e0, stream));
    return CHUNKY_OK;
}

int LaunchClock::close(hipStream_t stream, int weight) {
    HIP_TRY(hipEventRecord(e1, stream));
    pending.push_back(Bracket{e0, e1, weight});
    e0 = e1 = nullptr;
    return CHUNKY_OK;
}

int LaunchClock::collect() {
    for (Bracket& b : pending) {
        float t = 0;
        HIP_TRY(hipEventSynchronize(b.e1));
        HIP_TRY(hipEventElapsedTime(&t, b.e0, b.e1));
        ms += t;
        count += b.weight;
        pool->push_back(b.e0);
        pool->push_back(b.e1);
    }
    pending.clear();
    return CHUNKY_OK;
}

int LaunchClock::take(float* ms_out, int* count_out) {
    if (int rc = collect()) return rc;
    if (ms_out) *ms_out = ms;
    if (count_out) *count_out = count;
    ms = 0;
    count = 0;
    return CHUNKY_OK;
}

// What launch_render is going to run for r's passes over S (launch_plan.hpp), as far as it is known before a launch's pass count is:
// the kernel family, whether a block shard needs the pixel list, the most passes per launch, the answer to the extended options
RenderPlan render_plan(const chunky_render* r, const SceneView& S) {
    return plan_render(r->kernel_variant, scene_facts(S), r->opts, r->cam.projector_type, r->shard, 0, r->work_counter.p != nullptr, false, false);
}

// the extended light-transport options exist in render_pool's default instantiations only: CHUNKY_E_STATE where r's kernel
// option, scene or max depth would send it elsewhere
int check_extended_opts(const char* who, const RenderPlan& plan) {
    if (plan.ext_refusal == ExtRefusal::none) return CHUNKY_OK;
    return fail(CHUNKY_E_STATE, "%s: %s", who, ext_refusal_text(plan.ext_refusal));
}

int target_scene_view(const chunky_render* r, SceneView* S, bool want_emitters) {
    if (int rc = scene_view(r->scene, S, want_emitters)) return rc;
    S->bvh_cull = r->opts.bvh_cull;
    return CHUNKY_OK;
}

int needs_render_pool(const char* who, const chunky_render* r, SceneView* S) {
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "%s before set_camera", who);
    if (int rc = refuse_biome(who, r)) return rc;  // the folds run on the kernels that do not tint by position
    if (int rc = refuse_fog(who, r)) return rc;    // ... and that have no medium
    if (int rc = refuse_glass(who, r)) return rc;  // ... and that let nothing through a translucent block
    if (int rc = target_scene_view(r, S, r->opts.nee != 0)) return rc;
    const RenderPlan plan = render_plan(r, *S);
    if (int rc = check_extended_opts(who, plan)) return rc;
    if (plan.family != KernelFamily::pool)
        return fail(CHUNKY_E_STATE, "%s: the scene or the options send this target to the fallback kernels, which stage no samples", who);
    return CHUNKY_OK;
}

// Biome tints (chunky_scene_set_biome_tints): does r tint by position, and with which map
bool biome_map(const chunky_render* r, BiomeMap* B) {
    const chunky_scene* s = r->scene;
    if (!r->biome_tint || !s->biome.p) return false;
    if (B) *B = BiomeMap{(const int*)s->biome.p, s->biome_x0, s->biome_z0, s->biome_size_x, s->biome_size_z};
    return true;
}
// A call whose images hold colour and whose kernels do not tint by position refuses a target that does: it never renders untinted
int refuse_biome(const char* who, const chunky_render* r) {
    if (!biome_map(r, nullptr)) return CHUNKY_OK;
    return fail(CHUNKY_E_STATE, "%s: not with a biome map on the scene (chunky_scene_set_biome_tints); set CHUNKY_OPT_BIOME_TINT to 0 or remove the map", who);
}

// a device-to-host read-back of exactly `need` 4-byte values on r's stream; src == nullptr: nothing has been rendered into it yet
int read_floats(const char* who, chunky_render* r, const void* src, void* out, int64_t n, int64_t need) {
    if (!out || n != need) return fail(CHUNKY_E_INVALID, "%s: need %lld floats, got %lld", who, (long long)need, (long long)n);
    if (!src) return fail(CHUNKY_E_STATE, "%s before anything was rendered into it", who);
    HIP_TRY(hipMemcpyAsync(out, src, (size_t)n * 4, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return CHUNKY_OK;
}

// The staging array is sized once, before the cut, by the call's first launch: it is the longest, so this equals sizing before every
// launch; and after a halving the cap is the launch that fitted, so every later launch fits as well.  It grows only (launches on the
// stream are ordered, so one array serves them all, whichever call they come from).
int stage_launches(const char* who, chunky_render* r, const ShardView& T, int n, int reserve, int* cap) {
    const int launch = n < *cap ? n : *cap;
    if (r->staging.bytes >= staging_floats(T, r->width, r->height, launch) * sizeof(float)) return CHUNKY_OK;
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));  // queued launches may still write the old array
    r->staging.release();
    size_t free_b = SIZE_MAX, total_b = 0;  // (a reserve is never more than half of what the device has left, stage_passes; unknown: tried)
    if (reserve > launch) {
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = SIZE_MAX;
        (void)hipGetLastError();
    }
    const StagedLaunch got = stage_passes(0, T, r->width, r->height, launch, *cap, reserve, free_b, [&](size_t bytes) {
        if (hipMalloc(&r->staging.p, bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        r->staging.p = nullptr;
        return false;
    });
    r->staging.bytes = got.bytes;
    if (got.passes < launch && launch > 1) *cap = std::max(1, got.passes);  // memory is short: shorter launches instead of a failed render
    if (got.passes < 1)
        return fail(CHUNKY_E_HIP, "%s: cannot allocate %zu bytes for one pass of staged samples", who, staging_floats(T, r->width, r->height, 1) * sizeof(float));
    return CHUNKY_OK;
}

int stage_fold_launches(const char* who, chunky_render* r, const ShardView& T, int n, int* cap) {
    *cap = launch_pass_cap(T, r->width, r->height, kStagingBytes, kMaxPassesPerLaunch);
    if (*cap < 1) return fail(CHUNKY_E_INVALID, "%s: the image is too large to stage one pass", who);
    return stage_launches(who, r, T, n, 0, cap);
}

extern "C" int chunky_render_passes(chunky_render* r, const int32_t* seeds, int n, int first_buffer_spp) {
    FAN_RENDER(r, chunky_render_passes(m_, seeds, n, first_buffer_spp));  // asynchronous on every member: the shares run side by side
    LOCK_RENDER(r);
    if (n < 0 || (n > 0 && !seeds) || first_buffer_spp < 0) return fail(CHUNKY_E_INVALID, "render_passes: bad arguments");
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "render_passes before set_camera");
    SceneView S;
    if (int rc = target_scene_view(r, &S, r->opts.nee != 0)) return rc;
    RenderPlan plan = render_plan(r, S);
    FogParams fog;
    const bool foggy = fog_params_of(r, &fog);
    if (foggy) {  // the fog kernels (launch_plan.hpp plan_fog), or a refusal that says why: never an image of clear air
        const FogPlan f = fog_plan(r, S);
        if (f.refusal != FogRefusal::none) return fail(CHUNKY_E_STATE, "render_passes: %s", fog_refusal_text(f.refusal));
        plan = f.plan;  // (render_pool: no pixel list, launches of up to kMaxPoolPasses)
    }
    GlassParams glass;
    const bool glassy = glass_params_of(r, &glass);
    if (glassy) {  // the glass kernels (launch_plan.hpp plan_glass), or a refusal that says why: never an image with opaque glass
        const GlassPlan g = glass_plan(r, S);
        if (g.refusal != GlassRefusal::none) return fail(CHUNKY_E_STATE, "render_passes: %s", glass_refusal_text(g.refusal));
        plan = g.plan;
    }
    if (int rc = check_extended_opts("render_passes", plan)) return rc;
    BiomeMap biome;
    const bool tinted = !foggy && !glassy && biome_map(r, &biome);
    if (tinted) {  // the kernels that tint by position (launch_plan.hpp plan_biome), or a refusal that says why: never an untinted image
        RenderPlan asked = plan;
        asked.status = PlanStatus::ok;  // (a block shard's pixel list is made below; what a launch cannot carry is refused there)
        const BiomePlan b = plan_biome(asked);
        if (b.refusal != BiomeRefusal::none) return fail(CHUNKY_E_STATE, "render_passes: %s", biome_refusal_text(b.refusal));
        plan.family = b.plan.family;  // (needs_list and most are the fallback families' either way)
    }
    r->ad_resumable = false;  // the call is accepted: it writes the framebuffer (chunky_render_run / _run_ex end it here and in chunky_render_reset)
    if (r->clock.full())
        if (int rc = r->clock.collect()) return rc;
    if (r->shard.n_local <= 0) return CHUNKY_OK;  // this rank (or group member) owns no tile of so small an image: nothing to render
    if (plan.needs_list && !r->shard.list) {
        // a share of 16 x 16 blocks (every group member has one) and a scene / option set render_pool does not take: the
        // fallback kernels render the same pixels from a list
        const std::vector<int32_t> px = block_pixel_list(r->width, r->height, r->shard);
        if (px.empty()) return CHUNKY_OK;
        HIP_TRY(r->block_list.upload(px.data(), px.size() * 4, r->ctx->stream));
        r->shard.list = (const int*)r->block_list.p;
        r->shard.n_list = (int)px.size();
    }
    // render_pool takes up to kMaxPoolPasses per launch, the other kernels what the kernel-argument segment holds
    const int most = plan.most;
    if (r->launch_cap <= 0 || r->launch_cap_most != most) {
        r->launch_cap = std::max(1, launch_pass_cap(r->shard, r->width, r->height, kStagingBytes, most));  // sized by the tiles THIS rank renders
        r->launch_cap_most = most;
    }
    if (int rc = stage_launches("render_passes", r, r->shard, n, r->reserve_passes, &r->launch_cap)) return rc;  // (the cache remembers a halving)
    return for_each_launch(seeds, n, first_buffer_spp, r->launch_cap, [&](const PassSeeds& ps, const int32_t* launch_seeds) {
        const int* seeds_dev = nullptr;
        if (ps.n > kMaxPassesPerLaunch) {  // a long launch: its seeds go to device memory, in stream order behind the launch that read the buffer last
            if (!r->seed_buf.p) {
                HIP_TRY(r->seed_buf.alloc((size_t)kMaxPoolPasses * 4));
            }
            // from a pinned slot of the target's own (the caller may reuse or free `seeds` as soon as this call returns — the JNI
            // glue releases the Java array — and a copy out of pageable memory is only safe if the runtime happens to stage it)
            chunky_render::SeedSlot& slot = r->seed_ring[r->seed_next++ % chunky_render::kSeedSlots];
            if (!slot.host) {  // the event first: a slot is only ever seen with both or with neither
                if (!slot.copied) HIP_TRY(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
                HIP_TRY(hipHostMalloc((void**)&slot.host, (size_t)kMaxPoolPasses * 4, hipHostMallocDefault));
            } else {
                HIP_TRY(hipEventSynchronize(slot.copied));  // the copy that read this slot last (kSeedSlots launches ago)
            }
            memcpy(slot.host, launch_seeds, (size_t)ps.n * 4);
            HIP_TRY(hipMemcpyAsync(r->seed_buf.p, slot.host, (size_t)ps.n * 4, hipMemcpyHostToDevice, r->ctx->stream));
            HIP_TRY(hipEventRecord(slot.copied, r->ctx->stream));
            seeds_dev = (const int*)r->seed_buf.p;
        }
        if (int rc = r->clock.open(r->ctx->stream)) return rc;
        HIP_TRY(launch_render_fold(r->kernel_variant, S, r->cam, r->opts, r->shard, ps, r->fb, (int*)r->work_counter.p, r->ctx->stream, &r->last_choice,
                                   (float*)r->staging.p, seeds_dev, StagedFold{}, tinted ? &biome : nullptr, foggy ? &fog : nullptr,
                                   glassy ? &glass : nullptr));
        return r->clock.close(r->ctx->stream);
    });
}

extern "C" int chunky_render_sync(chunky_render* r) {
    FAN_RENDER(r, chunky_render_sync(m_));
    LOCK_RENDER(r);
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_render_read(chunky_render* r, float* out, int64_t n) {
    if (r && !r->parts.empty()) {
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        const int64_t need = (int64_t)r->width * r->height * 3;
        if (!out || n != need) return fail(CHUNKY_E_INVALID, "render_read: need %lld floats, got %lld", (long long)need, (long long)n);
        if (int rc = group_gather(r)) return rc;
        return chunky_render_read(r->parts[0], out, n);
    }
    LOCK_RENDER(r);
    return read_floats("render_read", r, r->fb, out, n, (int64_t)r->width * r->height * 3);
}

extern "C" int chunky_render_kernel_time(chunky_render* r, float* total_ms, int* launches) {
    if (r && !r->parts.empty()) {  // the members run side by side: the slowest one's total, member 0's launch count
        std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
        float worst = 0;
        for (size_t i = 0; i < r->parts.size(); i++) {
            float ms = 0;
            int n = 0;
            if (int rc = chunky_render_kernel_time(r->parts[i], &ms, &n)) return rc;
            if (ms > worst) worst = ms;
            if (i == 0 && launches) *launches = n;
        }
        if (total_ms) *total_ms = worst;
        return CHUNKY_OK;
    }
    LOCK_RENDER(r);
    return r->clock.take(total_ms, launches);
}

extern "C" int chunky_render_kernel_info(chunky_render* r, int32_t out8[8]) {
    if (r && !r->parts.empty()) return chunky_render_kernel_info(r->parts[0], out8);
    LOCK_RENDER(r);
    if (!out8) return fail(CHUNKY_E_INVALID, "kernel_info: NULL output");
    memset(out8, 0, 8 * sizeof(int32_t));
    out8[0] = r->last_choice.tree;
    out8[1] = r->last_choice.group;
    out8[2] = r->last_choice.bvh;
    out8[3] = r->last_choice.blocks;
    out8[4] = r->last_choice.pool;
    out8[5] = r->last_choice.ext;
    out8[7] = r->last_choice.sorted;
    if (r->last_choice.blocks == 0 && r->have_camera && biome_map(r, nullptr)) {
        // before the first launch of a target that tints by position: the biome instantiation its next launch will run
        SceneView S;
        if (scene_view(r->scene, &S, false) == CHUNKY_OK) {
            const BiomePlan b = plan_biome(render_plan(r, S));
            if (b.plan.status == PlanStatus::ok && b.refusal == BiomeRefusal::none) {
                const bool pool = b.plan.family == KernelFamily::pool;
                out8[0] = b.plan.tree, out8[1] = pool ? 1 : 0, out8[2] = b.plan.bvh ? 1 : 0, out8[4] = pool ? b.plan.park : -1, out8[5] = kChoiceBiome;
            }
        }
    }
    if (r->last_choice.blocks == 0 && r->have_camera && fog_params_of(r, nullptr)) {
        // before the first launch of a target with a fog layer: the fog instantiation its next launch will run
        SceneView S;
        if (scene_view(r->scene, &S, false) == CHUNKY_OK) {
            const FogPlan f = fog_plan(r, S);
            if (f.plan.status == PlanStatus::ok && f.refusal == FogRefusal::none)
                out8[0] = f.plan.tree, out8[1] = 1, out8[2] = f.plan.bvh ? 1 : 0, out8[4] = f.plan.park, out8[5] = kChoiceFog;
        }
    }
    if (r->last_choice.blocks == 0 && r->have_camera && glass_params_of(r, nullptr)) {
        // before the first launch of a target with translucency on: the glass instantiation its next launch will run
        SceneView S;
        if (scene_view(r->scene, &S, false) == CHUNKY_OK) {
            const GlassPlan g = glass_plan(r, S);
            if (g.plan.status == PlanStatus::ok && g.refusal == GlassRefusal::none)
                out8[0] = g.plan.tree, out8[1] = 1, out8[2] = g.plan.bvh ? 1 : 0, out8[4] = g.plan.park, out8[5] = kChoiceGlass;
        }
    }
    if (r->launch_cap > 0) {
        out8[6] = r->launch_cap;  // (of the kernel family that ran last)
    } else {  // before the first launch: what chunky_render_passes is going to decide for this scene and option set
        SceneView S;
        int most = kMaxPassesPerLaunch;
        if (scene_view(r->scene, &S, false) == CHUNKY_OK) most = render_plan(r, S).most;
        out8[6] = std::max(1, launch_pass_cap(r->shard, r->width, r->height, kStagingBytes, most));
    }
    return CHUNKY_OK;
}

extern "C" int chunky_render_phase_stats(chunky_render* r, uint64_t* out24, int reset) {
    if (r && !r->parts.empty()) return chunky_render_phase_stats(r->parts[0], out24, reset);
    LOCK_RENDER(r);
    if (!out24) return fail(CHUNKY_E_INVALID, "phase_stats: NULL output");
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    HIP_TRY(hipMemcpy(out24, (char*)r->work_counter.p + 8, 192, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset((char*)r->work_counter.p + 8, 0, 200));  // (with the word of chunky_render_march_above behind the 24)
    return CHUNKY_OK;
}

extern "C" int chunky_render_march_above(chunky_render* r, uint64_t* out1, int reset) {
    if (r && !r->parts.empty()) return chunky_render_march_above(r->parts[0], out1, reset);
    LOCK_RENDER(r);
    if (!out1) return fail(CHUNKY_E_INVALID, "march_above: NULL output");
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    HIP_TRY(hipMemcpy(out1, (char*)r->work_counter.p + 200, 8, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset((char*)r->work_counter.p + 200, 0, 8));
    return CHUNKY_OK;
}

extern "C" int chunky_render_preview(chunky_render* r, int32_t* argb_out) {
    if (r && !r->parts.empty()) return chunky_render_preview(r->parts[0], argb_out);  // one first-hit pass of the whole image: member 0
    LOCK_RENDER(r);
    if (!argb_out) return fail(CHUNKY_E_INVALID, "preview: NULL output");
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "preview before set_camera");
    SceneView S;
    if (int rc = target_scene_view(r, &S)) return rc;
    DevBuf out;
    size_t bytes = (size_t)r->width * r->height * 4;
    HIP_TRY(out.alloc(bytes));
    BiomeMap biome;
    if (biome_map(r, &biome))
        HIP_TRY(launch_preview_biome(r->kernel_variant, S, biome, r->cam, r->opts, (int*)out.p, r->ctx->stream));
    else
        HIP_TRY(launch_preview(r->kernel_variant, S, r->cam, r->opts, (int*)out.p, r->ctx->stream));
    HIP_TRY(hipMemcpyAsync(argb_out, out.p, bytes, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    return CHUNKY_OK;
}

extern "C" int chunky_render_trace_records(chunky_render* r, int32_t seed, const int32_t* gids, int n,
                                           chunky_hit_record* records, int32_t* counts, float* radiance) {
    if (r && !r->parts.empty()) return chunky_render_trace_records(r->parts[0], seed, gids, n, records, counts, radiance);
    LOCK_RENDER(r);
    if (n < 0 || (n > 0 && (!gids || !records || !counts || !radiance))) return fail(CHUNKY_E_INVALID, "trace_records: bad arguments");
    if (!r->have_camera) return fail(CHUNKY_E_STATE, "trace_records before set_camera");
    if (2 * r->opts.max_depth > kMaxTraces) return fail(CHUNKY_E_STATE, "trace_records holds %d traces per sample: max depth must be <= %d", kMaxTraces, kMaxTraces / 2);
    if (n == 0) return CHUNKY_OK;
    for (int i = 0; i < n; i++)
        if (gids[i] < 0 || gids[i] >= r->width * r->height) return fail(CHUNKY_E_INVALID, "trace_records: gid %d outside the image", gids[i]);
    SceneView S;
    if (int rc = target_scene_view(r, &S)) return rc;
    DevBuf dg, dr, dc, dq;
    hipStream_t st = r->ctx->stream;
    HIP_TRY(dg.upload(gids, (size_t)n * 4, st));
    HIP_TRY(hipMalloc(&dr.p, (size_t)n * kMaxTraces * sizeof(HitRecord)));
    HIP_TRY(hipMalloc(&dc.p, (size_t)n * 4));
    HIP_TRY(hipMalloc(&dq.p, (size_t)n * 12));
    HIP_TRY(hipMemsetAsync(dr.p, 0, (size_t)n * kMaxTraces * sizeof(HitRecord), st));
    BiomeMap biome;
    if (biome_map(r, &biome))
        HIP_TRY(launch_trace_records_biome(r->kernel_variant, S, biome, r->cam, r->opts, seed, (const int*)dg.p, n, (HitRecord*)dr.p, (int*)dc.p, (float*)dq.p, st));
    else
        HIP_TRY(launch_trace_records(r->kernel_variant, S, r->cam, r->opts, seed, (const int*)dg.p, n, (HitRecord*)dr.p, (int*)dc.p, (float*)dq.p, st));
    HIP_TRY(hipMemcpyAsync(records, dr.p, (size_t)n * kMaxTraces * sizeof(HitRecord), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counts, dc.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(radiance, dq.p, (size_t)n * 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CHUNKY_OK;
}
