// capi_internal.hpp — what the capi_*.hip files share: the objects behind include/chunky_hip.h's handles, the lock and fan-out
// macros, and the helpers that cross files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/chunky_hip.h"
#include "capi_error.hpp"
#include "canvas_host.hpp"
#include "capi_host.hpp"
#include "fog_host.hpp"
#include "glass_host.hpp"
#include "kernels.hpp"
#include "lights_host.hpp"
#include "rccl_dyn.hpp"
#include "rt_device.hpp"
#include "scene_records.hpp"
#include "widetree.hpp"

using namespace chunky;

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(CHUNKY_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ------------------------------------------------------------------------------------ context
struct chunky_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::recursive_mutex mu;  // the reference's renderLock
    std::string name;
    void* gamma_table = nullptr;  // 256 floats: the byte thresholds of the GAMMA / ACES tone maps (gamma_thresholds)
    // chunky_group_create: one member context per GPU; this object then only carries the lock and fans calls out
    std::vector<chunky_ctx*> members;
    std::vector<int> peer_status;  // per member: how its read-back copies reach member 0 (chunky_group_peer_status)
    // the read-back exchange of a group (group_gather): one RCCL communicator per member when the collective library could be
    // bound and the members are distinct devices, else empty — `transport` says what the next read-back will use and
    // `transport_detail` why (chunky_group_transport)
    std::vector<ncclComm_t> comms;
    int transport = CHUNKY_TRANSPORT_PEER_COPY;
    std::string transport_detail = "single device: no exchange";
    bool self_exchange = false;  // test rigs (tuning builds, CHUNKY_GROUP_SELF_EXCHANGE=1): member 0's own blocks travel through the exchange too
    int exchange_timeout_ms = 30000;  // how long an RCCL exchange may stay unfinished before its communicators are aborted (group_wait)
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t alloc(size_t n) {  // (contents undefined)
        release();
        const hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    hipError_t upload(const void* src, size_t n, hipStream_t s) {
        if (n != bytes || !p) {
            release();
            hipError_t e = hipMalloc(&p, n ? n : 4);
            if (e != hipSuccess) return e;
            bytes = n;
        }
        if (n == 0) return hipMemsetAsync(p, 0, 4, s);
        hipError_t e = hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        return hipStreamSynchronize(s);  // caller may reuse its array on return (COPY_HOST_PTR)
    }
};

struct chunky_scene {
    chunky_ctx* ctx = nullptr;
    DevBuf octree, blocks, materials, aabbs, quads, trigs, world_bvh, actor_bvh, atlas, sky, wide, block_info, quad_aux;
    DevBuf mat8, aabb_rec, quad_rec;                   // 16-byte-aligned re-layouts of the palettes (rt_device.hpp)
    DevBuf bvh_rec;                                    // both entity BVHs as 64-byte inner nodes, then their triangles as 80-byte records
    size_t tri_off = 0;                                // byte offset of the first triangle record in bvh_rec
    DevBuf emitters;                                   // emitter next-event estimation: {x, y, z, level << 25 | block} per emitter leaf
    std::vector<int32_t> host_octree, host_emitters;
    bool emitters_dirty = true;
    std::vector<int32_t> host_trigs, host_world_bvh, host_actor_bvh;
    int world_root = 0, actor_root = 0;                // first reference of each BVH in bvh_rec / tri_rec (rt_device.hpp)
    bool bvh_dirty = false;
    std::vector<int32_t> host_blocks, host_materials, host_aabbs, host_quads;  // kept to rebuild what is derived from them
    bool derived_dirty = false;                        // block_info, quad_aux, mat8, aabb_rec, quad_rec
    int model_leaf_permille = 0;                       // octree leaves that are model blocks, per thousand leaves that can be hit (scene_view)
    WideTree wide_meta;  // host copy kept so the kind bits can follow the block palette; nlev == 0 when absent
    bool wide_dirty = false;
    int octree_depth = -1;
    int atlas_w = 0, atlas_h = 0, atlas_layers = 0;
    int sky_w = 0, sky_h = 0;
    float sky_intensity = 0;
    int sun[6] = {0, 0, 0, 0, 0, 0};
    bool have_sun = false, world_empty = true, actor_empty = true;
    bool have_world = false, have_actor = false;
    int world_height = 0, actor_height = 0;  // inner-node levels: bounds the to-visit stack (K/bvh.h:38 uses 64)
    // chunky_scene_set_biome_tints: three words per cell of a rectangle of the cell grid (rt_device.hpp BiomeMap); no map: biome.p == nullptr
    DevBuf biome;
    int biome_x0 = 0, biome_z0 = 0, biome_size_x = 0, biome_size_z = 0;
    int refs = 1;  // owner + render targets
    std::vector<chunky_scene*> replicas;  // on a group: the scene's copy on every member (this object holds no data)
};

// Device time of the launches of one kind on a render target: brackets of two events around each launch (or run of launches),
// read and zeroed by the target's *_kernel_time call.  Events come from the target's pool and go back to it when a bracket has
// been collected; a bracket that was opened and never closed (an error return in between) keeps its events for the next open.
constexpr size_t kClockDrain = 4096;  // brackets a clock may hold before the call that adds more collects them first
struct LaunchClock {
    struct Bracket {
        hipEvent_t e0, e1;
        int weight;
    };
    std::vector<hipEvent_t>* pool;
    std::vector<Bracket> pending;
    hipEvent_t e0 = nullptr, e1 = nullptr;  // the open bracket
    float ms = 0;
    int count = 0;
    explicit LaunchClock(std::vector<hipEvent_t>* pool_) : pool(pool_) {}
    LaunchClock(const LaunchClock&) = delete;
    ~LaunchClock();
    bool full() const { return pending.size() > kClockDrain; }
    int open(hipStream_t stream);
    int close(hipStream_t stream, int weight = 1);
    int collect();                      // waits for the closed brackets and adds them to ms / count
    int take(float* ms_out, int* count_out);  // collect, report the totals since the last take, zero them
};

// What one first-hit pass (first_hit_pass.hpp: the AOV's, the mattes', the occlusion and light passes') keeps on a render target
struct FirstHitPass {
    LaunchClock clock;           // the launches' device time (chunky_render_*_kernel_time)
    AovChoice choice{0, 0, 0};   // what the most recent one ran
    int last_launches = 0;       // launches of the most recent *_passes call
    DevBuf images;               // the pass's images, then the kernels' claim counter; null before the first call
    size_t image_bytes = 0;      // bytes of the images, in front of the counter
    // allocated, zeroed, by the first call that needs them
    int ensure(size_t bytes, hipStream_t stream) {
        if (images.p) return CHUNKY_OK;
        HIP_TRY(images.alloc(bytes + 256));
        HIP_TRY(hipMemsetAsync(images.p, 0, bytes + 256, stream));
        image_bytes = bytes;
        return CHUNKY_OK;
    }
    int* counter() const { return (int*)((char*)images.p + image_bytes); }
};

struct chunky_render {
    chunky_ctx* ctx = nullptr;
    chunky_scene* scene = nullptr;
    int width = 0, height = 0;
    // chunky_render_set_canvas: the canvas this target is a window of (0 x 0: none, the target is its own canvas) and the window's corner
    int canvas_width = 0, canvas_height = 0, canvas_x0 = 0, canvas_y0 = 0;
    CameraView cam{};
    bool have_camera = false;
    DevBuf rays;
    RenderOpts opts{256, 5, 13.0f, -1, 1, 0, 0};
    int kernel_variant = 0;
    int biome_tint = 1;  // CHUNKY_OPT_BIOME_TINT: 0 = this target ignores the scene's biome map
    FogSettings fog;     // chunky_render_set_fog: the ground-fog layer of chunky_render_passes; density 0 (default) = none
    GlassSettings glass; // chunky_render_set_translucency: translucent blocks in chunky_render_passes; off by default
    ShardView shard{0, 1, 256, 0};
    DevBuf own_fb, work_counter;
    DevBuf staging;  // render_pool: one launch's samples, [tile of 256 slots][pass][slot][3] floats
    DevBuf block_list;  // block shards under a kernel without the block mapping: this rank's pixels (ShardView::list)
    float* fb = nullptr;
    std::vector<hipEvent_t> free_events;  // the one pool the six clocks below borrow from
    LaunchClock clock{&free_events};      // the render launches (chunky_render_kernel_time)
    KernelChoice last_choice{0, 0, 0, 0, -1, 0};  // what the most recent launch ran (chunky_render_kernel_info)
    int launch_cap = 0;  // most passes one launch carries here (staging size); 0 = not determined yet
    int launch_cap_most = 0;  // ... determined for launches of at most this many passes (kMaxPassesPerLaunch / kMaxPoolPasses)
    DevBuf seed_buf;      // seeds of a launch longer than the kernel-argument segment holds (render_pool)
    int reserve_passes = 0;  // the pass loop is about to climb to launches of this many passes: size the staging array once
    struct SeedSlot {        // pinned host copies of long launches' seeds on their way to seed_buf
        int32_t* host = nullptr;
        hipEvent_t copied = nullptr;
    };
    static constexpr int kSeedSlots = 4;
    SeedSlot seed_ring[kSeedSlots];
    unsigned seed_next = 0;
    // on a group: one target per member (this object holds no device data), the caller's share of the image, and the buffers
    // of the read-back exchange: gather_send[i] on member i's device, gather_recv[i] on member 0's
    std::vector<chunky_render*> parts;
    ShardView outer{0, 1, 0, 0};
    std::vector<DevBuf> gather_send, gather_recv;
    // the denoiser's auxiliary images (chunky_render_aov_passes): aov_pass.images holds albedo then normal, 3 * width * height floats
    // each.  Timing and the last instantiation are kept apart from the render kernels' (chunky_render_kernel_time / _kernel_info do
    // not see AOV launches)
    // chunky_render_aov_passes_ex: alpha, depth (a word per pixel each), position (3), emittance, block id (1 each), allocated (and
    // zeroed) by the first _ex call; its launches share the AOV's counter and record
    DevBuf aov_ex;
    FirstHitPass aov_pass{LaunchClock(&free_events)};
    // chunky_render_matte_passes: matte_pass.images holds 13 planes of width * height int32 (six of ids, six of counts, `other`).
    // matte_work holds a read-out on its way to the host (ranks: 12 planes; extract: one) and matte_set the sorted ids of an extract.
    // Record and counter are its own: the AOV calls do not see them
    DevBuf matte_work, matte_set;
    FirstHitPass matte_pass{LaunchClock(&free_events)};
    int32_t matte_passes = 0;     // passes folded since the last reset
    // chunky_render_occlusion_passes: occlusion_pass.images holds the AO image, then the SUN image (width * height floats each).
    // Record and counter are its own: no other call sees them
    FirstHitPass occlusion_pass{LaunchClock(&free_events)};
    // chunky_render_light_passes: light_pass.images holds the SKY, SUN, EMITTERS and ALL images (3 * width * height floats each).
    // light_mix holds a mix on its way to the host.  Record and counter are its own: no other call sees them
    DevBuf light_mix;
    FirstHitPass light_pass{LaunchClock(&free_events)};
    // chunky_render_light_set_emitter_groups: the table (n_groups == 0: no groups), and on the device the group images, the kernel's
    // per-sample sums and touched words and the table's bytes (capi_lights.hip), allocated by the set call
    LightGroupTable light_table;
    DevBuf light_groups;
    bool light_groups_rendered = false;  // a light pass has run since the groups were set: their images can be read
    // chunky_render_denoise: the filter's workspace (kept between calls) and its timing, apart from the render and AOV launches'
    DevBuf dn_work, dn_out;
    LaunchClock dn_clock{&free_events};  // (a bracket holds all launches of one call: their number is its weight)
    // chunky_render_adaptive: (m, M2) per pixel, the sample counts, the active / unconverged flags (a byte per pixel each), the tile
    // counts and offsets of the compaction with the total behind them, the active list, and the pinned word the total is read from;
    // allocated by the first adaptive call.  Its timing is kept apart from the other launches'
    DevBuf ad_stat, ad_count, ad_flags, ad_tiles, ad_list;
    int32_t* ad_total_host = nullptr;
    bool ad_valid = false;  // an adaptive run has finished: the maps can be read
    // The state chunky_render_adaptive_resume continues (header; the arrays are fb, ad_count, ad_stat and the first half of ad_flags,
    // and ad_list holds the active pixels whenever fewer than all are active).  ad_resumable: the framebuffer, the maps and what a pass
    // renders are as the run that wrote ad_state left them — cleared by every call that writes the framebuffer or changes the
    // camera, the options, the shard or the buffer
    chunky_adaptive_state ad_state{};
    bool ad_resumable = false;
    LaunchClock ad_clock{&free_events};  // one bracket per round
    // chunky_render_robust_*: rb_m bucket images [bucket][pixel][3] (0: no state) and the robust samples folded into them since
    // chunky_render_robust_begin; the resolved image and the trim bytes on their way to the host or to the denoiser, allocated by the
    // first resolve.  Its timing is kept apart from the other launches': one clock for the passes, one for the resolves
    DevBuf rb_buckets, rb_out, rb_trim;
    int rb_m = 0;
    int32_t rb_count = 0;
    LaunchClock rb_clock{&free_events}, rb_resolve_clock{&free_events};
    ~chunky_render() {
        if (ad_total_host) (void)hipHostFree(ad_total_host);
        for (auto e : free_events) (void)hipEventDestroy(e);
        for (SeedSlot& s : seed_ring) {
            if (s.copied) (void)hipEventDestroy(s.copied);
            if (s.host) (void)hipHostFree(s.host);
        }
    }
};

constexpr size_t kStagingBytes = (size_t)8 << 30;  // 8 GiB: 1920x1080 x 256 passes is 6.4 GB (of 288)

// bytes of one AOV image (3 floats per pixel)
static size_t aov_image_bytes(const chunky_render* r) { return (size_t)r->width * r->height * 3 * sizeof(float); }

// ------------------------------------------------------------------------------------ scene
#define LOCK_SCENE(s)                                                        \
    if (!(s) || !(s)->ctx) return fail(CHUNKY_E_INVALID, "NULL scene");      \
    std::lock_guard<std::recursive_mutex> guard_((s)->ctx->mu);              \
    HIP_TRY(hipSetDevice((s)->ctx->device))

// A call on a group's scene is the same call on every replica (under the group's lock: the reference's renderLock).
template <class F>
static int each_replica(chunky_scene* s, F call) {
    std::lock_guard<std::recursive_mutex> g(s->ctx->mu);
    for (chunky_scene* m : s->replicas)
        if (int rc = call(m)) return rc;
    return CHUNKY_OK;
}
#define FAN_SCENE(s, expr) \
    if ((s) && !(s)->replicas.empty()) return each_replica((s), [&](chunky_scene* m_) { return expr; })

// ------------------------------------------------------------------------------------ render
#define LOCK_RENDER(r)                                                       \
    if (!(r) || !(r)->ctx) return fail(CHUNKY_E_INVALID, "NULL render");     \
    std::lock_guard<std::recursive_mutex> guard_((r)->ctx->mu);              \
    HIP_TRY(hipSetDevice((r)->ctx->device))

// A call on a group's render target is the same call on every member's part.
template <class F>
static int each_part(chunky_render* r, F call) {
    std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
    for (chunky_render* m : r->parts)
        if (int rc = call(m)) return rc;
    return CHUNKY_OK;
}
#define FAN_RENDER(r, expr) \
    if ((r) && !(r)->parts.empty()) return each_part((r), [&](chunky_render* m_) { return expr; })

// n passes of a first-hit pass in launches of at most kMaxPassesPerLaunch, each continuing the images: launch(its seeds) returns a CHUNKY_ code
template <class Launch>
static int first_hit_launches(chunky_render* r, FirstHitPass& fp, const int32_t* seeds, int n, int first_buffer_spp, Launch launch) {
    if (fp.clock.full())
        if (int rc = fp.clock.collect()) return rc;
    return for_each_launch(seeds, n, first_buffer_spp, kMaxPassesPerLaunch, [&](const PassSeeds& ps, const int32_t*) {
        if (int rc = fp.clock.open(r->ctx->stream)) return rc;
        if (int rc = launch(ps)) return rc;
        if (int rc = fp.clock.close(r->ctx->stream)) return rc;
        fp.last_launches += 1;
        return (int)CHUNKY_OK;
    });
}

// A first-hit pass on a group's render target: member 0 renders the caller's whole share (as chunky_render_preview does), so the
// images are the one-context images without an exchange (the pass's other entry points forward to member 0).  Runs under the lock.
template <class Passes>
static int on_first_member(const char* who, chunky_render* r, Passes passes) {
    if (!r || !r->ctx) return fail(CHUNKY_E_INVALID, "NULL render");
    std::lock_guard<std::recursive_mutex> g(r->ctx->mu);
    if (r->parts.empty()) return passes(r, r->shard);
    ShardView t;  // the caller's share of the image, all of it on member 0
    if (!make_shard_view(r->width, r->height, r->outer.rank, r->outer.world, r->outer.tile, &t))
        return fail(CHUNKY_E_INVALID, "%s: the group's share needs more than 2^31 pixel slots", who);
    return passes(r->parts[0], t);
}

// ------------------------------------------------------------------------------------ helpers that cross files
#pragma GCC visibility push(hidden)  // internal to the library: none of these is part of its surface
void group_close_rccl(chunky_ctx* g, bool abort);                                       // capi_group.hip
int group_gather(chunky_render* r);
void scene_unref(chunky_scene* s);                                                      // capi_scene.hip
int scene_view(chunky_scene* s, SceneView* v, bool want_emitters = false);
// the scene as r's launches read it: scene_view with r's CHUNKY_OPT_BVH_CULL_BEHIND                  // capi_render.hip
int target_scene_view(const chunky_render* r, SceneView* S, bool want_emitters = false);
// what a call that folds staged samples needs of r from the camera on: render_pool for the scene and options as they are (*S: the scene)
int needs_render_pool(const char* who, const chunky_render* r, SceneView* S);
// r's staging array grown to hold the first launch of n passes over T at *cap passes per launch (pass_schedule.hpp stage_passes);
// *cap comes back lower when memory was short.  The one place staging is allocated
int stage_launches(const char* who, chunky_render* r, const ShardView& T, int n, int reserve, int* cap);
// ... for the calls that fold (the seeds travel in the kernel arguments, no reserve hint, r->launch_cap is not touched): *cap is made here
int stage_fold_launches(const char* who, chunky_render* r, const ShardView& T, int n, int* cap);
RenderPlan render_plan(const chunky_render* r, const SceneView& S);                      // what plan_render decides for r's passes over S
int check_extended_opts(const char* who, const RenderPlan& plan);
bool biome_map(const chunky_render* r, BiomeMap* B);  // r tints by position: its scene has a biome map and CHUNKY_OPT_BIOME_TINT is 1 (then *B is the map)
int refuse_biome(const char* who, const chunky_render* r);  // CHUNKY_E_STATE for a call that does not tint by position while r does
bool fog_params_of(const chunky_render* r, FogParams* F);  // r has a fog layer (then *F holds it as the fog kernels take it)      // capi_fog.hip
int refuse_fog(const char* who, const chunky_render* r);  // CHUNKY_E_STATE for a call that has no fog kernels while r has a layer
// what plan_fog decides for r's passes over S, as render_plan does for a target without fog
FogPlan fog_plan(const chunky_render* r, const SceneView& S);
bool glass_params_of(const chunky_render* r, GlassParams* G);  // r has translucency on (then *G holds it as the glass kernels take it)   // capi_glass.hip
int refuse_glass(const char* who, const chunky_render* r);  // CHUNKY_E_STATE for a call that has no glass kernels while r has translucency on
// what plan_glass decides for r's passes over S
GlassPlan glass_plan(const chunky_render* r, const SceneView& S);
int read_floats(const char* who, chunky_render* r, const void* src, void* out, int64_t n, int64_t need);
int first_hit_kernel_time(chunky_render* r, FirstHitPass chunky_render::*pass, float* total_ms, int* launches);  // capi_aov.hip
int first_hit_kernel_info(const char* who, chunky_render* r, FirstHitPass chunky_render::*pass, int32_t out4[4]);
int device_gamma_table(chunky_ctx* ctx, const float** out);                             // capi_filter.hip
// the denoiser on r's device with r's own AOV images: `color` (3 * width * height floats on that device) filtered into `out` on the host
int render_denoise(chunky_render* r, const DnCoeffs& K, int form, const float* color, float* out);  // capi_denoise.hip
#pragma GCC visibility pop
