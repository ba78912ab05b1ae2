// launch_plan.hpp — which render kernel a launch runs, decided in one place: plan_render (launch_plan.cpp) turns the kernel option,
// a handful of scene facts, the render options, the camera kind, the shard and the launch's pass count into a RenderPlan, and the
// kernel translation units only look the plan up in the list of their instantiations (CHUNKY_POOL_INSTANCES and the lists beside
// it, written once, below).  Plain C++17 over ints, no HIP type and no device call: tests/sanitize/launch_plan_sweep.cpp runs the
// planner under AddressSanitizer + UBSan over a stride of every combination of its inputs (tests/test_launch_plan_cpu.py).
// DESIGN.md section 5, "which instantiation runs", is this file as a table.
#pragma once
#include <cstddef>

#include "shard_map.hpp"

// Tunables of the pool kernel that the choice depends on (each measured on the bench; DESIGN.md section 5 has the sweeps).  The -D
// overrides exist for tuning builds (tools/variants.sh) only; they reach every translation unit, this one included.
#ifndef CHUNKY_POOL_WORDS
#define CHUNKY_POOL_WORDS 6   // 16-byte words of a parked path without entity BVHs (7 in tuning builds: 1/d and colour side by side)
#endif
#ifndef CHUNKY_POOL_PARK
#define CHUNKY_POOL_PARK (CHUNKY_POOL_WORDS == 6 ? 64 : 56)   // paths parked per wave (LDS: WORDS x 16 + 8 bytes each; 6 x 4 waves x 64 x 104 B fill 156 of 160 KB)
#endif

namespace chunky {

struct RenderOpts {  // a kernel argument: member order and types are part of every kernel's argument layout
    int draw_depth;       // 256, K/rayTracer.cl:94
    int max_depth;        // 5,   K/rayTracer.cl:107
    float emitter_scale;  // 13,  K/rayTracer.cl:99
    // EXPERIMENTAL light-transport options (specification: oracle/port.c trace_sample_ext).  The
    // defaults are the reference's behaviour and select the reference kernels.
    int sun_sampling;     // -1 as the reference (PackedSun flag bit 0), 0 never, 1 always
    int emitters;         // 1 as the reference; 0 = emittersEnabled false
    int bsdf;             // 1: specular / metal / roughness from material word 5
    int nee;              // 1: emitter next-event estimation
    int bvh_cull;         // 1: CHUNKY_OPT_BVH_CULL_BEHIND (travels to the kernels in SceneView::bvh_cull)
};
inline bool opts_extended(const RenderOpts& O) { return O.sun_sampling != -1 || O.emitters != 1 || O.bsdf != 0 || O.nee != 0; }

constexpr int kBvhStackEntries = 64;  // K/bvh.h:38
// Seeds of the passes one launch runs travel in the kernel-argument segment (4 KB in all); the pass index is 8 bits
constexpr int kMaxPassesPerLaunch = 256;
// render_pool takes longer launches when the staged samples fit (a share of the image on several GPUs: fewer end-of-launch tails):
// the seeds then travel in device memory (launch_render's seeds_dev)
constexpr int kMaxPoolPasses = 1024;
constexpr int kPoolPark = CHUNKY_POOL_PARK;
constexpr size_t kCuLdsBytes = (size_t)160 << 10;  // LDS of a compute unit (gfx950)
constexpr size_t kPoolBvhGroupsPerCu = 5;       // workgroups per CU the entity kernels are sized for (render_pool.hip CHUNKY_POOL_BVH_WAVES)
constexpr int kLaunchBlock = 256;  // threads of a workgroup of every render kernel: four waves

// render_pool's sample tiles of 16 x 16 pixels (path_state.hpp has the order of the slots inside one)
constexpr int kTileLog = 4, kTileEdge = 1 << kTileLog, kSampleTile = kTileEdge * kTileEdge;
// render_pool's tiles of 256 pixel slots: the image's 16 x 16-pixel blocks with one rank (edge blocks padded), the rank's own
// blocks or 256-slot runs with several (path_state.hpp pool_slot_gid)
inline long long pool_tiles(const ShardView& T, int width, int height) {
    if (T.world != 1) return ((long long)T.n_local + kSampleTile - 1) / kSampleTile;  // runs of T.tile pixels, or (T.tile == 0) the rank's blocks
    return (long long)((width + kTileEdge - 1) >> kTileLog) * ((height + kTileEdge - 1) >> kTileLog);
}

// The plain instantiations of render_pool read the atlas, the sky and the record arrays by 32-bit offsets (rt_device.hpp
// CHUNKY_ADDR32_FORMS, which render_pool.hip sets to this for its own kernels and checks against it); -DCHUNKY_ADDR32_FORMS=n:
// experiments, the arrays one at a time
#ifdef CHUNKY_ADDR32_FORMS
constexpr unsigned kPoolAddr32Forms = (unsigned)(CHUNKY_ADDR32_FORMS);
#else
constexpr unsigned kPoolAddr32Forms = 7u;
#endif
// tuning builds (tools/variants.sh): a fixed pool size for the entity kernel, e.g. 8 parked paths at six waves; -1: none
#ifdef CHUNKY_POOL_BVH_PARK
constexpr int kPoolBvhPark = CHUNKY_POOL_BVH_PARK;
#else
constexpr int kPoolBvhPark = -1;
#endif

// A parked path is this many 16-byte words (render_pool.hip pool_pack): 6 without entity BVHs, 8 with them, 9 for the extended integrator
constexpr int pool_words(bool ext, bool bvh) { return ext ? 9 : (bvh ? 8 : CHUNKY_POOL_WORDS); }
// LDS bytes of one wave of render_pool: `park` parked records, a tag and a list word per slot, and with entity BVHs a to-visit
// stack of `depth` entries for every path of the pool.  The kernel carves its LDS with this and the launch sizes it with this:
// a host count that disagreed with the kernel's would have the kernel write past its allocation.
constexpr unsigned pool_wave_lds_bytes(int park, int words, unsigned depth) { return park * 16 * words + park * 8 + (64 + park) * depth * 4; }
// render_waves: the ring of a pixel group (render_fallback.hip)
constexpr int ring_size(int group) { return 2 * group; }

// What the choice reads of a SceneView (rt_device.hpp scene_facts)
struct SceneFacts {
    bool wide;                 // the re-laid-out tree exists (SceneView::wide)
    int wide_nlev;             // its levels
    int wide_bits[6];          // bits per axis of each level (SceneView::wide_bits)
    bool world_bvh_empty, actor_bvh_empty;
    int bvh_stack_entries;
    bool bvh_records;          // the re-laid-out entity records exist (bvh_rec && tri_rec && mat8)
    unsigned addr32;           // SceneView::addr32: the arrays 32-bit offsets reach
    bool sort_blocks;          // model blocks are common (capi_scene.hip scene_view)
    bool block_info;           // SceneView::block_info exists
};

// variant bit 0 set = force the reference-layout octree walk (K/octree.h:81-89 as written)
inline bool use_wide(int variant, const SceneFacts& F) { return F.wide && !(variant & 1); }
// the form of leaf_lookup for a scene: 0 reference layout, 16 + n dense top over n levels of 8x8x8 nodes, -1 any other wide split
int tree_form(int variant, const SceneFacts& F);
// entries per to-visit stack (the reference reserves 64, K/bvh.h:38; here: the height of the taller BVH + 1); 0 without entity BVHs
int stack_entries(const SceneFacts& F);
// LDS bytes of the to-visit stacks of a workgroup of `block` lanes of the kernels that bind a path to a lane
size_t stack_lds_bytes(const SceneFacts& F, int block);

enum class KernelFamily : int { pool = 0, waves = 1, lanes = 2 };  // render_pool; render_waves, render_lanes (render_fallback.hip)
enum class PlanStatus : int { ok = 0, invalid_value = 1, not_supported = 2 };  // hipSuccess, hipErrorInvalidValue, hipErrorNotSupported
// why a launch leaves render_pool: the first of these, in this order, that holds
enum class NotPool : int {
    none = 0,
    lanes_forced,    // variant bit 1: render_lanes
    waves_forced,    // variant bit 3: render_waves
    no_queue,        // no work counter or no staging array
    draw_depth,      // the 6-word parked record counts march steps in 16 bits: a draw depth above 65535 runs render_waves
    max_depth,       // path depth 255 marks a fresh path: max depth above 254
    no_wide_tree,    // the reference-layout walk exists in the plain instantiations only: not with entities, extended options or statistics
    addr32,          // the scene's arrays are too large for the plain instantiations' 32-bit offsets
    bvh_records,     // entity BVHs that could not be re-laid out
    bvh_reference,   // entity BVHs with the reference-layout walk forced (variant bit 0)
};
// what the C API answers to extended light-transport options this plan cannot serve (capi_render.hip check_extended_opts)
enum class ExtRefusal : int { none = 0, default_kernel, wide_tree, max_depth };

struct RenderPlan {
    KernelFamily family;
    int tree;      // leaf-lookup form of the instantiation: 0, -1, 16 - 19
    int park;      // render_pool: paths parked per wave (the instantiation's K); -1 otherwise
    int words;     // render_pool: 16-byte words of a parked path; 0 otherwise
    int group;     // render_pool 1; render_waves: lanes per pixel; render_lanes 0
    int depth;     // entries per to-visit stack; 0 without entity BVHs
    bool bvh, ext, stats, sorted, proj;
    size_t lds;    // dynamic LDS bytes of a workgroup
    int most;      // the most passes a launch may carry
    bool needs_list;  // a shard of 16 x 16 blocks under a kernel that cannot map them: the rank's pixels as a list
    PlanStatus status;
    NotPool why;
    ExtRefusal ext_refusal;
};
// projector_type: CameraView::projector_type; n_passes: of this launch; want_staged_fold: the launch's samples are folded by more than fold_kernel (kernels.hpp StagedFold)
// have_queue_and_staging: the work counter AND the staging array exist.  The two are deliberately one fact: every caller has both or
// neither (the C API allocates them together before any launch), and without either render_lanes runs — render_waves, which needs
// the counter alone, is not chosen for a caller that has the counter but could not stage.
RenderPlan plan_render(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                       bool have_queue_and_staging, bool have_seeds_dev, bool want_staged_fold);
// the message of check_extended_opts for a refusal, with `who` in front
const char* ext_refusal_text(ExtRefusal r);

// The lookup form of the first-hit passes (first_hit_pass.hpp, occlusion.hip, lights.hip): the one render_pool picks for the scene, so that a
// first-hit pass and a render pass of a view read the octree the same way
struct FirstHitPlan {
    int tree;
    bool bvh;
};
FirstHitPlan plan_first_hit(int variant, const SceneFacts& F);

// Biome tints by block position: with a biome map on the scene and CHUNKY_OPT_BIOME_TINT at 1 a launch runs a kernel
// compiled with CHUNKY_BIOME_TINT (rt_device.hpp), and plan_biome maps what plan_render decided onto the instantiations that exist:
//   render_pool, pinhole and pre-generated cameras: tree forms 0, 17, 18 and -1 without entity BVHs (16 and 19 run -1), 17 and -1 with
//   them (18 runs -1); unsorted block tests; kPoolBiomePark parked paths without entity BVHs whatever the rig bits say, the plan's 16 or
//   32 with them (CHUNKY_POOL_BIOME_INSTANCES, CHUNKY_POOL_BIOME_BVH_INSTANCES);
//   render_waves and render_lanes plans: render_lanes (CHUNKY_LANES_INSTANCES), every camera.
// Everything else is refused — BiomePlan::refusal says why, the C API answers CHUNKY_E_STATE with biome_refusal_text — never rendered
// untinted: phase statistics, the extended light-transport options, projected cameras on render_pool.  A plan plan_render refused
// (status != ok) comes back as it is.
constexpr int kPoolBiomePark = kPoolPark;
enum class BiomeRefusal : int { none = 0, stats, extended, projected };
struct BiomePlan {
    RenderPlan plan;
    BiomeRefusal refusal;
};
BiomePlan plan_biome(const RenderPlan& p);
const char* biome_refusal_text(BiomeRefusal r);

// Ground fog: a target with a fog layer (chunky_render_set_fog) runs the EXTENDED family whatever its options say —
// with every light-transport option at its default too — on the kernels compiled with CHUNKY_FOG (rt_device.hpp): render_pool for the
// pinhole and pre-generated cameras, tree forms 17, 18 and -1, 32 parked paths without entity BVHs and 16 with them
// (CHUNKY_POOL_FOG_INSTANCES, CHUNKY_POOL_FOG_BVH_INSTANCES).  plan_fog is plan_render with that family forced.  Everything else is
// refused — FogPlan::refusal says why, the C API answers CHUNKY_E_STATE with fog_refusal_text — and never rendered without fog: a scene
// whose biome map the target applies, phase statistics, the rig bits that pick another walk or kernel, projected cameras (pre-generated
// rays serve every projection), max depth above 254, a scene without a wide tree or whose entity BVHs could not be re-laid out, and
// whatever else sends a launch to the fallback kernels.  A plan plan_render refused (status != ok) comes back with that status.
enum class FogRefusal : int { none = 0, biome, stats, rig_bits, projected, max_depth, wide_tree, bvh_records, not_pool };
struct FogPlan {
    RenderPlan plan;
    FogRefusal refusal;
};
FogPlan plan_fog(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                 bool have_queue_and_staging, bool have_seeds_dev, bool biome_tinted);
const char* fog_refusal_text(FogRefusal r);

// Translucent blocks: a target with translucency on (chunky_render_set_translucency) runs the EXTENDED family whatever
// its options say, on the kernels compiled with CHUNKY_GLASS (rt_device.hpp): plan_fog's instantiations once more — render_pool for the
// pinhole and pre-generated cameras, tree forms 17, 18 and -1, 32 parked paths without entity BVHs and 16 with them
// (CHUNKY_POOL_GLASS_INSTANCES, CHUNKY_POOL_GLASS_BVH_INSTANCES) — with a parked record of kPoolGlassWords 16-byte words: the extended
// integrator's nine, and three for the hit's alpha, the runs, a shadow ray's clip distance and filter and its vertex's normal.
// plan_glass is plan_fog's shape: the same refusals for the same reasons, and one more, a target with a fog layer.
constexpr int kPoolGlassWords = 12;
enum class GlassRefusal : int { none = 0, fog, biome, stats, rig_bits, projected, max_depth, wide_tree, bvh_records, not_pool };
struct GlassPlan {
    RenderPlan plan;
    GlassRefusal refusal;
};
GlassPlan plan_glass(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                     bool have_queue_and_staging, bool have_seeds_dev, bool biome_tinted, bool foggy);
const char* glass_refusal_text(GlassRefusal r);

}  // namespace chunky

// ---------------------------------------------------------------------------------------------
// The instantiations, each list written once: X(TREE, K, STATS, BVH, EXT, SORT) of render_pool, compiled once per namespace
// (chunky:: and chunky::proj::).  render_pool.hip instantiates the plain list, render_pool_bvh.hip the entity list; a plan that
// names none of them is an error (no kernel is substituted).  (The order is the order the compiler emits them in: profiles/
// kernel_resources.json lists them so.)
#define CHUNKY_POOL_INSTANCES(X)                                                \
    /* the extended integrator */                                               \
    X(17, 32, false, false, true, false)                                        \
    X(18, 32, false, false, true, false)                                        \
    X(-1, 32, false, false, true, false)                                        \
    /* phase statistics (variant bit 2), with sorted block tests and without */ \
    X(17, kPoolPark, true, false, false, true)                                  \
    X(-1, kPoolPark, true, false, false, true)                                  \
    X(17, kPoolPark, true, false, false, false)                                 \
    X(-1, kPoolPark, true, false, false, false)                                 \
    /* the pool sizes of the test rigs (variant bits 6-7) */                    \
    X(0, 0, false, false, false, false)                                         \
    X(-1, 0, false, false, false, false)                                        \
    X(0, 32, false, false, false, false)                                        \
    X(-1, 32, false, false, false, false)                                       \
    /* block tests sorted by kind: the re-laid-out tree only */                 \
    X(16, kPoolPark, false, false, false, true)                                 \
    X(17, kPoolPark, false, false, false, true)                                 \
    X(18, kPoolPark, false, false, false, true)                                 \
    X(19, kPoolPark, false, false, false, true)                                 \
    X(-1, kPoolPark, false, false, false, true)                                 \
    /* the default kernels: every tree form */                                  \
    X(0, kPoolPark, false, false, false, false)                                 \
    X(16, kPoolPark, false, false, false, false)                                \
    X(17, kPoolPark, false, false, false, false)                                \
    X(18, kPoolPark, false, false, false, false)                                \
    X(19, kPoolPark, false, false, false, false)                                \
    X(-1, kPoolPark, false, false, false, false)
#ifdef CHUNKY_POOL_BVH_PARK
#define CHUNKY_POOL_BVH_TUNING_INSTANCES(X) X(17, CHUNKY_POOL_BVH_PARK, false, true, false, false) X(-1, CHUNKY_POOL_BVH_PARK, false, true, false, false)
#else
#define CHUNKY_POOL_BVH_TUNING_INSTANCES(X)
#endif
#define CHUNKY_POOL_BVH_INSTANCES(X)                                                                                                   \
    X(17, 16, false, true, true, false)                                                                                                \
    X(18, 16, false, true, true, false)                                                                                                \
    X(-1, 16, false, true, true, false)                                                                                                \
    X(17, 16, true, true, false, false)                                                                                                \
    X(-1, 16, true, true, false, false)                                                                                                \
    X(17, 32, false, true, false, false)                                                                                               \
    X(18, 32, false, true, false, false)                                                                                               \
    X(-1, 32, false, true, false, false)                                                                                               \
    X(17, 16, false, true, false, false)                                                                                               \
    X(18, 16, false, true, false, false)                                                                                               \
    X(-1, 16, false, true, false, false)                                                                                               \
    CHUNKY_POOL_BVH_TUNING_INSTANCES(X)
// X(TREE, G, BVH) of render_waves and X(TREE) of render_lanes (render_fallback.hip): the reference octree layout (0) and the generic
// wide tree (-1) only; a group of 32 lanes per pixel exists without entity BVHs only
#define CHUNKY_WAVES_INSTANCES(X)                                                                                                      \
    X(0, 1, false) X(-1, 1, false) X(0, 1, true) X(-1, 1, true)                                                                        \
    X(0, 8, false) X(-1, 8, false) X(0, 8, true) X(-1, 8, true)                                                                        \
    X(0, 16, false) X(-1, 16, false) X(0, 16, true) X(-1, 16, true)                                                                    \
    X(0, 32, false) X(-1, 32, false)
#define CHUNKY_LANES_INSTANCES(X) X(0) X(-1)
// X(TREE, K, STATS, BVH, EXT, SORT) of render_pool compiled with CHUNKY_BIOME_TINT (render_pool_biome.hip, render_pool_biome_bvh.hip):
// what plan_biome names
#define CHUNKY_POOL_BIOME_INSTANCES(X)                                                                                                 \
    X(0, kPoolBiomePark, false, false, false, false)                                                                                   \
    X(17, kPoolBiomePark, false, false, false, false)                                                                                  \
    X(18, kPoolBiomePark, false, false, false, false)                                                                                  \
    X(-1, kPoolBiomePark, false, false, false, false)
#define CHUNKY_POOL_BIOME_BVH_INSTANCES(X)                                                                                             \
    X(17, 32, false, true, false, false) X(-1, 32, false, true, false, false)                                                          \
    X(17, 16, false, true, false, false) X(-1, 16, false, true, false, false)
// X(TREE, K, STATS, BVH, EXT, SORT) of render_pool compiled with CHUNKY_FOG (render_pool_fog.hip, render_pool_fog_bvh.hip): what plan_fog
// names — the extended instantiations of the plain lists, once more
#define CHUNKY_POOL_FOG_INSTANCES(X)                                                                                                   \
    X(17, 32, false, false, true, false) X(18, 32, false, false, true, false) X(-1, 32, false, false, true, false)
#define CHUNKY_POOL_FOG_BVH_INSTANCES(X)                                                                                               \
    X(17, 16, false, true, true, false) X(18, 16, false, true, true, false) X(-1, 16, false, true, true, false)
// X(TREE, K, STATS, BVH, EXT, SORT) of render_pool compiled with CHUNKY_GLASS (render_pool_glass.hip, render_pool_glass_bvh.hip): what
// plan_glass names
#define CHUNKY_POOL_GLASS_INSTANCES(X)                                                                                                 \
    X(17, 32, false, false, true, false) X(18, 32, false, false, true, false) X(-1, 32, false, false, true, false)
#define CHUNKY_POOL_GLASS_BVH_INSTANCES(X)                                                                                             \
    X(17, 16, false, true, true, false) X(18, 16, false, true, true, false) X(-1, 16, false, true, true, false)
// X(TREE, BVH) of the first-hit kernels (first_hit_pass.hpp first_hit_kernel, occlusion.hip occlusion_kernel, lights.hip light_kernel)
#define CHUNKY_FIRST_HIT_INSTANCES(X)                                                                                                  \
    X(0, true) X(17, true) X(18, true) X(-1, true)                                                                                     \
    X(0, false) X(16, false) X(17, false) X(18, false) X(19, false) X(-1, false)
