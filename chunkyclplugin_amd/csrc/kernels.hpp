// kernels.hpp — host-visible launch interface of the kernel translation units (render_pool.hip, render_fallback.hip,
// aux_kernels.hip, filter.hip, aov.hip, occlusion.hip, lights.hip, matte.hip, denoise.hip, adaptive.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "launch_plan.hpp"  // RenderOpts, the launch limits, pool_tiles: what the launch planner shares with the launchers
#include "pass_schedule.hpp"  // PassSeeds, staging_floats: how passes become launches
#include "shard_map.hpp"  // ShardView, FastDiv: the host arithmetic of the shard-to-pixel map

struct DnCoeffs;  // denoise_spec.h

namespace chunky {

struct SceneView;
struct CameraView;
struct BiomeMap;  // rt_device.hpp
struct FogParams;
struct GlassParams;

constexpr int kMaxTraces = 10;        // 5 path segments x (main + shadow trace)

// Layout shared with include/chunky_hip.h (chunky_hit_record) and oracle/oracle_scene.h.
struct HitRecord {
    int32_t hit;
    int32_t material;
    float distance;
    float normal[3];
    float color[4];
    float emittance;
    float point[3];
};

// What launch_render picked for a launch (chunky_render_kernel_info): the tests assert that the instantiation they
// mean to compare with the oracle is the one that ran.
struct KernelChoice {
    int tree;    // leaf-lookup form: 0 reference layout, -1 generic wide tree, 16 + n dense top over n 3-bit levels
    int group;   // lanes per pixel (render_waves); 0 = render_lanes (one lane per pixel for the whole launch)
    int bvh;     // entity-BVH phases compiled in
    int blocks;  // workgroups launched
    int pool;    // render_pool: paths parked per wave beside the 64 in its lanes; -1 = another kernel
    int ext;     // 1: the extended integrator (CHUNKY_OPT_SUN_SAMPLING / _EMITTERS / _BSDF / _EMITTER_NEE at non-default values); kChoiceBiome: a biome-tint instantiation; kChoiceFog: a ground-fog instantiation (of the extended integrator)
    int sorted;  // render_pool: full cubes and model blocks tested in phases of their own
};
constexpr int kChoiceBiome = 2;  // KernelChoice::ext, and bit 1 of AovChoice::bvh: the launch ran a kernel compiled with CHUNKY_BIOME_TINT
constexpr int kChoiceGlass = 4;  // KernelChoice::ext: the launch ran a kernel compiled with CHUNKY_GLASS (render_pool_glass.hip, render_pool_glass_bvh.hip)
constexpr int kChoiceFog = 3;    // KernelChoice::ext: the launch ran a kernel compiled with CHUNKY_FOG (render_pool_fog.hip, render_pool_fog_bvh.hip)

// compute units of the CURRENT device (cached per device index: members of a group and threads of a host may sit on different GPUs)
inline hipError_t current_device_cus(int* n_cu) {
    static std::atomic<int> cached[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool slot = dev >= 0 && dev < 64;
    int n = slot ? cached[dev].load(std::memory_order_relaxed) : 0;
    if (n == 0) {
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, dev);
        if (e != hipSuccess) return e;
        n = prop.multiProcessorCount;
        if (slot) cached[dev].store(n, std::memory_order_relaxed);
    }
    *n_cu = n;
    return hipSuccess;
}
// A persistent grid: as many workgroups as the device holds at once (its compute units x the kernel's occupancy at this block size
// and LDS), and no more than `want`, what the work can feed
template <class Kernel>
inline hipError_t persistent_grid(Kernel k, int block, size_t lds, long long want, int* grid) {
    int n_cu = 0, occ = 0;
    if (hipError_t e = current_device_cus(&n_cu)) return e;
    if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, block, lds)) return e;
    const long long fits = (long long)n_cu * (occ > 0 ? occ : 1);
    *grid = (int)(fits > want ? want : fits);
    return hipSuccess;
}
// Which kernel a launch runs is decided by plan_render (launch_plan.hpp), here and in the C API alike.
// P.n <= kMaxPassesPerLaunch with the seeds in P.seed, or (render_pool only) up to kMaxPoolPasses with the seeds in seeds_dev
hipError_t launch_render(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                         const PassSeeds& P, float* res, int* work_counter, hipStream_t stream,
                         KernelChoice* chosen = nullptr, float* staging = nullptr, const int* seeds_dev = nullptr);
// What folds the staged samples of a render_pool launch into the target's images, besides fold_kernel's running mean into `res`
// (which every kind keeps, operation for operation):
//   none     fold_kernel alone: launch_render
//   stats    fold_stats_kernel (adaptive.hip): stat_image holds two floats per pixel of the image, the luminance statistic
//   buckets  fold_buckets_kernel<n_buckets> (robust.hip): bucket_images holds n_buckets images [bucket][pixel][3]; the launch's first
//            sample is robust sample `first_index` (robust_spec.h)
struct StagedFold {
    enum Kind : int { none = 0, stats = 1, buckets = 2 } kind = none;
    float* stat_image = nullptr;
    float* bucket_images = nullptr;
    int n_buckets = 0;
    int first_index = 0;
};
// launch_render with the launch's samples folded as `fold` says.  A fold other than `none` is render_pool's only
// (hipErrorNotSupported under the other kernels, which stage no samples); kind == none is launch_render.
// With a biome map (tints by block position) the launch runs what plan_biome (launch_plan.hpp) makes of
// plan_render's plan, on the kernels compiled with CHUNKY_BIOME_TINT (render_pool_biome.hip, render_pool_biome_bvh.hip,
// render_biome.hip); hipErrorNotSupported for what plan_biome refuses, and for a map with a fold other than `none`.
// With `fog` (the ground-fog layer) the launch runs plan_fog's plan on the kernels compiled with CHUNKY_FOG;
// hipErrorNotSupported for what plan_fog refuses — a biome map among it — and for a fold other than `none`.
// With `glass` (translucent blocks) the launch runs plan_glass's plan on the kernels compiled with CHUNKY_GLASS, likewise;
// fog among what plan_glass refuses.
hipError_t launch_render_fold(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                              const PassSeeds& P, float* res, int* work_counter, hipStream_t stream, KernelChoice* chosen,
                              float* staging, const int* seeds_dev, const StagedFold& fold, const BiomeMap* biome = nullptr,
                              const FogParams* fog = nullptr, const GlassParams* glass = nullptr);
// the kernels behind render_pool (render_fallback.hip): render_waves, render_lanes, as `plan` names them
hipError_t launch_fallback(const RenderPlan& plan, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                           const PassSeeds& P, float* res, int* work_counter, hipStream_t stream, KernelChoice* chosen);
// The kernels that tint by position: render_lanes for launch_render_fold, and the twins of launch_trace_records, launch_preview, launch_aov and launch_aov_ex
hipError_t launch_lanes_biome(const RenderPlan& plan, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O,
                              const ShardView& T, const PassSeeds& P, float* res, hipStream_t stream, KernelChoice* chosen);
hipError_t launch_trace_records_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, int seed,
                                      const int* gids_dev, int n, HitRecord* out, int* counts, float* radiance, hipStream_t stream);
hipError_t launch_preview_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, int* argb,
                                hipStream_t stream);
// read-back exchange of a multi-GPU group: pack = true copies the pixels of this shard's slots from the image `fb` to `packed`
// (3 floats per slot, padding slots skipped), pack = false scatters them back into an image
hipError_t launch_gather(bool pack, const ShardView& T, int width, int height, float* fb, float* packed, hipStream_t stream);
// ... and, for the exchange by ncclReduce, zeroes every pixel of `fb` that shard T does not own
hipError_t launch_clear_foreign(const ShardView& T, int width, int height, float* fb, hipStream_t stream);
hipError_t launch_trace_records(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, int seed,
                                const int* gids_dev, int n, HitRecord* out, int* counts, float* radiance,
                                hipStream_t stream);
hipError_t launch_preview(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, int* argb,
                          hipStream_t stream);
// What launch_aov picked for a launch (chunky_render_aov_kernel_info)
struct AovChoice {
    int tree;    // leaf-lookup form, as KernelChoice::tree
    int bvh;     // entity-BVH walk compiled in
    int blocks;  // workgroups launched
};
// AOV passes (aov.hip): P.n <= kMaxPassesPerLaunch; albedo / normal are 3 * width * height floats each, folded in place over the
// pixel slots of shard T; `counter` is one int of device memory the launch claims its work from.
hipError_t launch_aov(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                      float* albedo, float* normal, int* counter, hipStream_t stream, AovChoice* chosen);
// The seven images of chunky_render_aov_passes_ex (aov.hip AovExFold): albedo, normal and position 3 * width * height floats, the
// others width * height words
struct AovExImages {
    float *albedo, *normal, *alpha, *depth, *position, *emittance;
    int* block;
};
// launch_aov with the five first-hit images folded from the same trace
hipError_t launch_aov_ex(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                         const AovExImages& I, int* counter, hipStream_t stream, AovChoice* chosen);
// launch_aov / launch_aov_ex on the kernels that tint by position (aov_biome.hip); AovChoice::bvh then carries kChoiceBiome beside bit 0
hipError_t launch_aov_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, const ShardView& T,
                            const PassSeeds& P, float* albedo, float* normal, int* counter, hipStream_t stream, AovChoice* chosen);
hipError_t launch_aov_ex_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, const ShardView& T,
                               const PassSeeds& P, const AovExImages& I, int* counter, hipStream_t stream, AovChoice* chosen);
// Sun-shadow and ambient-occlusion passes (occlusion.hip): P.n <= kMaxPassesPerLaunch; ao / sun are width * height
// floats each, folded in place over the pixel slots of shard T; ao_distance > 0 (+inf allowed); `counter` as launch_aov's.
hipError_t launch_occlusion(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                            float* ao, float* sun, float ao_distance, int* counter, hipStream_t stream, AovChoice* chosen);
// Light-group passes (lights.hip): P.n <= kMaxPassesPerLaunch; images[CHUNKY_LIGHT_SKY .. CHUNKY_LIGHT_ALL] are
// 3 * width * height floats each, folded in place over the pixel slots of shard T; O.max_depth and O.emitter_scale are the path's;
// `counter` as launch_aov's.
hipError_t launch_lights(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                         float* const images[4], int* counter, hipStream_t stream, AovChoice* chosen);
// out[i] = (w[0] * sky[i] + w[1] * sun[i]) + w[2] * emitters[i] for n floats on the device, without fma
hipError_t launch_light_mix(const float* sky, const float* sun, const float* emitters, const float w[3], float* out, long long n, hipStream_t stream);
// The emitter groups of a render target as the kernel reads them (lights_groups.hip; lights_device.hpp LightGroupOut), all device memory
constexpr int kLightMaxGroups = 8;         // CHUNKY_LIGHT_MAX_EMITTER_GROUPS
constexpr int kChoiceLightGroups = 4;      // bit 2 of AovChoice::bvh: the launch ran lights_groups.hip's kernel
struct LightGroupImages {
    int n_groups;                   // 1 .. kLightMaxGroups
    float* images;                  // n_groups images of 3 * width * height floats
    float* acc;                     // 3 * n_groups floats per pixel, all zero bits or whatever: read only where `touched` says so
    int* touched;                   // a word per pixel, zero between launches
    const unsigned char* of_block;  // n_blocks bytes: the group of block pointer p at [p >> 1]
    int n_blocks;
    int world_group, actor_group;
};
// launch_lights with one more image per emitter group folded from the same walk
hipError_t launch_light_groups(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                               float* const images[4], const LightGroupImages& G, int* counter, hipStream_t stream, AovChoice* chosen);
// out[i] = ((w_sky * sky[i] + w_sun * sun[i]) + w_groups[0] * groups[i]) + w_groups[1] * groups[n + i] ... for n floats, without fma
hipError_t launch_light_group_mix(const float* sky, const float* sun, const float* groups, int n_groups, float w_sky, float w_sun, const float* w_groups,
                                  float* out, long long n, hipStream_t stream);
// ID-matte passes (matte.hip; specification: matte_spec.h): P.n <= kMaxPassesPerLaunch; `planes` is 13 * width * height ints (six planes of
// ids, six of counts, `other`), updated in place over the pixel slots of shard T; `counter` as launch_aov's.  The choice record is the AOV's.
hipError_t launch_matte(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                        int* planes, int* counter, hipStream_t stream, AovChoice* chosen);
// the ranks of every pixel (out_ids, out_coverage: 6 * n_pixels words each, plane-major) and the mask of a set of ids (sorted: ascending,
// each value once, n_set of them on the device; out: n_pixels floats); passes > 0
hipError_t launch_matte_ranks(const int* planes, long long n_pixels, int passes, int* out_ids, float* out_coverage, hipStream_t stream);
hipError_t launch_matte_extract(const int* planes, long long n_pixels, int passes, const int* sorted, int n_set, float* out, hipStream_t stream);
// The À-Trous denoiser (denoise.hip; specification: denoise_spec.h).  color / albedo / normal / out: 3 * width * height floats on the
// device (out may not alias an input); `work`: denoise_work_bytes of device memory, 16-byte aligned, the launch's own while it runs.
// One launch per iteration plus the pack (or demodulation) pass, all on `stream`; *launches receives their number.  `form` picks how taps
// are fetched (all bit-identical).
constexpr int kDenoiseGather = 0;  // the images as they arrive, 3 floats per pixel (the default: the faster of the two)
constexpr int kDenoisePacked = 1;  // 16-byte words per pixel, written by a pack pass
inline size_t denoise_work_bytes(int width, int height) { return (size_t)width * height * 64; }  // enough for either form (packed: two colour planes + two guide planes of float4)
hipError_t launch_denoise(int form, int width, int height, const float* color, const float* albedo, const float* normal, const ::DnCoeffs& K,
                          float* out, void* work, size_t work_bytes, hipStream_t stream, int* launches);
// Adaptive sampling (adaptive.hip; specification: adaptive_spec.h).
// fold_kernel's running mean over the staged samples of n_tiles tiles of shard T, and the Welford update of stat (2 floats per pixel)
hipError_t launch_fold_stats(const float* staging, float* res, float* stat, const ShardView& T, int width, int height, long long n_tiles,
                             int n_passes, int first_spp, hipStream_t stream);
// the check after n passes: unconverged flags (unconv), activity (active; pixels that leave get count = n), then the active pixels in
// whole-image pool-slot order in `list` and their number in *total.  active / unconv: width * height bytes; count / list: width * height
// ints; tile_counts / tile_offsets: one int per 16 x 16 tile; all on the device
hipError_t launch_adaptive_check(int width, int height, const float* stat, unsigned char* active, unsigned char* unconv, int* count, int n,
                                 float t2, float floor_, int* tile_counts, int* tile_offsets, int* list, int* total, hipStream_t stream);
// the list and *total of an activity map that is already final (a restored state): the tiles' active slots counted
// (adaptive_count_kernel), then the scan and the scatter of launch_adaptive_check — the same list, entry for entry; the maps are only read
hipError_t launch_adaptive_rebuild(int width, int height, unsigned char* active, int* tile_counts, int* tile_offsets, int* list, int* total,
                                   hipStream_t stream);
// pixels still active record n
hipError_t launch_adaptive_finish(int n_pixels, const unsigned char* active, int* count, int n, hipStream_t stream);
// Firefly-robust accumulation (robust.hip; specification: robust_spec.h).
// fold_kernel's running mean over the staged samples of n_tiles tiles of shard T, and the update of the n_buckets bucket means
// (buckets: [bucket][pixel][3]) for robust samples first_index ..; hipErrorInvalidValue for a bucket count the specification does not take
hipError_t launch_fold_buckets(const float* staging, float* res, float* buckets, int n_buckets, int first_index, const ShardView& T, int width,
                               int height, long long n_tiles, int n_passes, int first_spp, hipStream_t stream);
// the resolve of every pixel: out 3 * n_pixels floats, trim n_pixels bytes or null; mode RB_MODE_*
hipError_t launch_robust_resolve(const float* buckets, int n_buckets, long long n_pixels, int mode, float gain, float* out, unsigned char* trim,
                                 hipStream_t stream);
// self test: samples [pass][pixel][3] into the staging layout of the whole image (staging zeroed by the caller: padding slots stay 0)
hipError_t launch_robust_stage(const float* samples, float* staging, int width, int height, long long n_tiles, int n_passes, hipStream_t stream);
// thresholds: 256 floats on the device (capi_host.cpp gamma_thresholds) or null = evaluate pow per channel
hipError_t launch_filter(long long n_pixels, float exposure, const double* in, unsigned* out, int type, hipStream_t stream,
                         const float* thresholds = nullptr);
// the same tone map with the alpha byte of pixel p taken from alpha[p] (n_pixels floats on the device): chunky_filter_frame_alpha
hipError_t launch_filter_alpha(long long n_pixels, float exposure, const double* in, const float* alpha, unsigned* out, int type,
                               hipStream_t stream, const float* thresholds);
// tone map self test: gamma_bytes3 (curve 0) / aces_bytes3 (curve 2) against the reference's arithmetic and a search of the
// threshold table, for `count` consecutive float bit patterns
hipError_t launch_gamma_scan(unsigned first, unsigned long long count, int curve, const float* thresholds, unsigned long long* mismatches,
                             float* worst, hipStream_t stream);
// helper-level known answers (aux_kernels.hip helpers_selftest_kernel): rows of 32 floats in, 12 out
hipError_t launch_helpers_selftest(const SceneView& S, int which, int tree, int n, const float* in, float* out, int* tree_used, hipStream_t stream);
hipError_t launch_math_selftest(int which, int n, const float* a, const float* b, float* out, hipStream_t stream);
// projected camera self test (aux_kernels.hip camera_rays_kernel): width * height * 6 floats, origin then direction per pixel.
hipError_t launch_camera_rays_selftest(const CameraView& C, int seed, float* out, hipStream_t stream);
// the shard-to-pixel map (aux_kernels.hip shard_map_kernel).  mode 0: 5 ints per slot 0 .. n - 1 of shard T — pool_slot_gid, the gid /
// x / y of pool_slot_pixel, shard_gid (-1 where it does not apply); mode 1: fast_quotient(a, {m, s}) for n triples (a, m, s) of `in`
hipError_t launch_shard_map_selftest(int mode, const ShardView& T, int width, int height, int n, const unsigned* in, int* out, hipStream_t stream);

}  // namespace chunky
