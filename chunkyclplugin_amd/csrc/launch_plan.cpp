// launch_plan.cpp — plan_render: the one function that decides which render kernel a launch runs (launch_plan.hpp).  Plain C++17,
// no HIP type; compiled into the library and, with g++ under AddressSanitizer + UBSan, into tests/sanitize/launch_plan_sweep.cpp.
#include "launch_plan.hpp"

namespace chunky {

int tree_form(int variant, const SceneFacts& F) {
    if (!use_wide(variant, F)) return 0;
    int tree = F.wide_nlev <= 4 ? 16 + F.wide_nlev - 1 : -1;
    for (int i = 1; i < F.wide_nlev; i++)
        if (F.wide_bits[i] != 3) tree = -1;
    return tree;
}

static bool has_bvh(const SceneFacts& F) { return !F.world_bvh_empty || !F.actor_bvh_empty; }

int stack_entries(const SceneFacts& F) {
    if (!has_bvh(F)) return 0;
    return F.bvh_stack_entries > 0 && F.bvh_stack_entries < kBvhStackEntries ? F.bvh_stack_entries : kBvhStackEntries;
}

size_t stack_lds_bytes(const SceneFacts& F, int block) { return (size_t)stack_entries(F) * block * sizeof(int); }

// render_pool runs: always without entity BVHs; with them when they could be re-laid out (rt_device.hpp bvh_rec / tri_rec)
// (force_ext: plan_fog's launches run the extended family with every option at its default)
static NotPool why_not_pool(int variant, const SceneFacts& F, const RenderOpts& O, bool have_queue_and_staging, bool force_ext) {
    const bool bvh = has_bvh(F), ext = force_ext || opts_extended(O);
    if (variant & 2) return NotPool::lanes_forced;
    if (variant & 8) return NotPool::waves_forced;
    if (!have_queue_and_staging) return NotPool::no_queue;
    // the 6-word parked record counts march steps in 16 bits (the 8- and 9-word records have a word for them)
    if (!bvh && !ext && O.draw_depth > 65535) return NotPool::draw_depth;
    if (O.max_depth > 254) return NotPool::max_depth;  // (path depth 255 marks a fresh path)
    // a scene without a wide tree (an octree deeper than 15 levels, a block pointer beyond 25 bits: widetree.cpp) runs render_pool's
    // reference-layout walk, which only the plain instantiations have (tree 0 with 0, 32 or 64 parked paths): entity BVHs, the
    // extended options and phase statistics all come with a wide-tree instantiation, so those go to the fallback kernels
    if (!F.wide && (bvh || ext || (variant & 4))) return NotPool::no_wide_tree;
    // the plain instantiations read the atlas, the sky and the records by 32-bit offsets: a scene whose arrays are too large for that
    // (scene_records.cpp addr32_word) runs the fallback kernels; the entity-BVH instantiations read any scene
    if (!bvh && (F.addr32 & kPoolAddr32Forms) != kPoolAddr32Forms) return NotPool::addr32;
    if (bvh && !F.bvh_records) return NotPool::bvh_records;
    if (bvh && (variant & 1)) return NotPool::bvh_reference;
    return NotPool::none;
}

// the extended light-transport options exist in render_pool's default instantiations only
static ExtRefusal ext_refusal(int variant, const SceneFacts& F, const RenderOpts& O, NotPool why, bool force_ext) {
    if (!force_ext && !opts_extended(O)) return ExtRefusal::none;
    if ((variant & (1 | 2 | 4 | 8)) || (has_bvh(F) && !F.bvh_records)) return ExtRefusal::default_kernel;
    if (!F.wide) return ExtRefusal::wide_tree;  // their instantiations walk the re-laid-out tree only (an octree deeper than 15 levels has none)
    // the fallback kernels never read these options: a set render_pool refuses (max depth 255) would render the reference's transport
    if (why != NotPool::none) return ExtRefusal::max_depth;
    return ExtRefusal::none;
}

const char* ext_refusal_text(ExtRefusal r) {
    switch (r) {
        case ExtRefusal::default_kernel: return "the extended light-transport options need the default kernel (CHUNKY_OPT_KERNEL 0)";
        case ExtRefusal::wide_tree: return "the extended light-transport options need an octree the wide re-layout takes (depth <= 15)";
        case ExtRefusal::max_depth: return "the extended light-transport options need max depth <= 254 (CHUNKY_OPT_MAX_DEPTH)";
        default: return "";
    }
}

// render_pool: variant bits 6-7 pick the parked paths per wave, 0 = kPoolPark (default), 1 = none, 2 = 32 (test rigs: the
// reference-layout and the generic tree forms only)
static void plan_pool(RenderPlan& p, int variant, const SceneFacts& F) {
    const bool bvh = p.bvh, ext = p.ext;
    const bool stats = (variant & 4) != 0;
    int tree = tree_form(variant, F);
    int park = kPoolPark;
    switch ((variant >> 6) & 3) {
        case 1: park = 0; break;
        case 2: park = 32; break;
        default: break;
    }
    // Block tests sorted by kind (full cubes / model blocks in phases of their own): for scenes in which model blocks are common
    // (sort_blocks, capi_scene.hip scene_view) — the city gains 2 – 3 %, a scene with hardly any pays 1 % for the bookkeeping; variant
    // bit 8 forces it on, bit 9 off (tests and A/B runs); the plain kernel at its full pool only, and on the re-laid-out tree with
    // the block records: the phases read both
    const bool sorted = ((variant & 256) || F.sort_blocks) && !(variant & 512) && !bvh && !ext && tree != 0 && F.block_info;
    p.sorted = false;
    p.stats = false;
    if (ext) {
        // EXPERIMENTAL light-transport options: their own instantiations, which override the pool-size bits:
        // the 9-word record leaves room for 32 parked paths, 16 beside the to-visit stacks
        if (tree != 17 && tree != 18) tree = -1;
        park = bvh ? 16 : 32;
    } else if (bvh) {
        // every path of the pool owns a to-visit stack in LDS: 32 parked paths when five workgroups per CU still fit, else 16
        // (the entity kernels have the dense tops of one and two levels, else the generic walk)
        if (tree != 17 && tree != 18) tree = -1;
        const size_t lds32 = (size_t)(kLaunchBlock / 64) * pool_wave_lds_bytes(32, pool_words(false, true), (unsigned)p.depth);
        park = kPoolBvhGroupsPerCu * lds32 <= kCuLdsBytes ? 32 : 16;
        if (stats) {  // the statistics kernels: one dense top and the generic walk, 16 parked paths
            if (tree != 17) tree = -1;
            park = 16;
            p.stats = true;
        } else if (kPoolBvhPark >= 0) {  // tuning builds: a fixed pool size, the same two tree forms
            if (tree != 17) tree = -1;
            park = kPoolBvhPark;
        }
    } else if (stats) {
        if (tree != 17) tree = -1;
        park = kPoolPark;
        p.stats = true;
        p.sorted = sorted;
    } else if (park != kPoolPark) {
        if (tree != 0) tree = -1;
    } else if (sorted) {
        if (tree < 16 || tree > 19) tree = -1;
        p.sorted = true;
    } else {
        if (tree != 0 && (tree < 16 || tree > 19)) tree = -1;
    }
    p.tree = tree;
    p.park = park;
    p.words = pool_words(ext, bvh);
    p.group = 1;
    p.lds = (size_t)(kLaunchBlock / 64) * pool_wave_lds_bytes(park, p.words, (unsigned)p.depth);
}

// render_waves unless variant bit 1 asks for render_lanes (or there is no work counter); variant bits 4-5 force render_waves' lanes
// per pixel (1 / 8 / 16).  The fallback kernels exist for the reference octree layout (0) and the generic wide tree (-1) only.
static void plan_fallback(RenderPlan& p, int variant, const SceneFacts& F, int n_local, int n_passes, bool have_queue) {
    p.tree = use_wide(variant, F) ? -1 : 0;
    p.ext = false;
    const size_t stack = stack_lds_bytes(F, kLaunchBlock);
    p.lds = stack;
    if ((variant & 2) || !have_queue) {
        p.family = KernelFamily::lanes;
        p.group = 0;
        return;
    }
    p.family = KernelFamily::waves;
    // lanes per pixel (render_fallback.hip next_sample): 8; 16 or 32 when this GPU owns few pixels (multi-GPU tile split: the fewer
    // pixels per group, the longer the tail of the launch)
    int group = n_local < (3 << 17) ? 32 : (n_local < (3 << 18) ? 16 : 8);
    while (group > 8 && n_passes < 2 * group) group /= 2;  // a group needs a few passes per lane to stay busy
    if (n_passes < 2 * group) group = 1;
    switch ((variant >> 4) & 3) {  // variant bits 4-5 force the group size (tests cover all three)
        case 1: group = 1; break;
        case 2: group = 8; break;
        case 3: group = 16; break;
        default: break;
    }
    if (group == 32 && p.bvh) group = 16;  // (32 lanes per pixel and a to-visit stack per lane: not instantiated)
    p.group = group;
    if (group > 1) p.lds += (size_t)(kLaunchBlock / group) * (2 * ring_size(group) * 16 + 64);
}

static RenderPlan plan_render_as(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                                 bool have_queue_and_staging, bool have_seeds_dev, bool want_staged_fold, bool force_ext) {
    RenderPlan p{};
    p.why = why_not_pool(variant, F, O, have_queue_and_staging, force_ext);
    p.ext_refusal = ext_refusal(variant, F, O, p.why, force_ext);
    const bool pool = p.why == NotPool::none;
    p.family = pool ? KernelFamily::pool : (((variant & 2) || !have_queue_and_staging) ? KernelFamily::lanes : KernelFamily::waves);
    // render_pool takes up to kMaxPoolPasses per launch, the other kernels what the kernel-argument segment holds
    p.most = pool ? kMaxPoolPasses : kMaxPassesPerLaunch;
    // shards of 16 x 16 blocks are mapped by render_pool only: the other kernels take the rank's pixels as a list
    p.needs_list = !pool && T.world != 1 && T.tile == 0;
    p.park = -1;
    p.status = PlanStatus::ok;
    if (pool) {
        if (n_passes > kMaxPoolPasses || (n_passes > kMaxPassesPerLaunch && !have_seeds_dev)) p.status = PlanStatus::invalid_value;
    } else if (want_staged_fold) {
        p.status = PlanStatus::not_supported;  // only render_pool stages samples
    } else if (n_passes > kMaxPassesPerLaunch) {
        p.status = PlanStatus::invalid_value;
    } else if (p.needs_list && !T.list) {
        p.status = PlanStatus::not_supported;
    }
    if (p.status != PlanStatus::ok) return p;  // refused: no kernel is named
    p.bvh = has_bvh(F);
    p.depth = stack_entries(F);
    p.ext = force_ext || opts_extended(O);
    p.proj = pool && projector_type > 0;  // a projected camera: proj::render_pool, same template arguments
    if (pool)
        plan_pool(p, variant, F);
    else
        plan_fallback(p, variant, F, p.needs_list ? T.n_list : T.n_local, n_passes, have_queue_and_staging);
    return p;
}

RenderPlan plan_render(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                       bool have_queue_and_staging, bool have_seeds_dev, bool want_staged_fold) {
    return plan_render_as(variant, F, O, projector_type, T, n_passes, have_queue_and_staging, have_seeds_dev, want_staged_fold, false);
}

FirstHitPlan plan_first_hit(int variant, const SceneFacts& F) {
    const bool bvh = has_bvh(F);
    const int tree = tree_form(variant, F);
    if (tree == 0) return FirstHitPlan{0, bvh};
    if (bvh) return FirstHitPlan{(tree == 17 || tree == 18) ? tree : -1, bvh};  // with entity BVHs the dense tops of one and two levels
    return FirstHitPlan{(tree >= 16 && tree <= 19) ? tree : -1, bvh};
}

// Biome tints: the plan of the kernels compiled with CHUNKY_BIOME_TINT (launch_plan.hpp has the table)
BiomePlan plan_biome(const RenderPlan& in) {
    BiomePlan b{in, BiomeRefusal::none};
    RenderPlan& p = b.plan;
    if (p.status != PlanStatus::ok) return b;  // refused by plan_render: no kernel is named
    if (p.ext) b.refusal = BiomeRefusal::extended;
    else if (p.stats) b.refusal = BiomeRefusal::stats;
    else if (p.proj) b.refusal = BiomeRefusal::projected;
    if (b.refusal != BiomeRefusal::none) return b;
    if (p.family == KernelFamily::pool) {
        if (p.bvh) {
            if (p.tree != 17) p.tree = -1;
            if (p.park != 32) p.park = 16;  // (tuning builds' pool sizes included)
        } else {
            if (p.tree != 0 && p.tree != 17 && p.tree != 18) p.tree = -1;
            p.park = kPoolBiomePark;
        }
        p.sorted = false;
        p.lds = (size_t)(kLaunchBlock / 64) * pool_wave_lds_bytes(p.park, p.words, (unsigned)p.depth);
        return b;
    }
    // render_waves and render_lanes: one lane per pixel; of the LDS the to-visit stacks stay (plan_fallback: the rings lay behind them)
    p.family = KernelFamily::lanes;
    p.group = 0;
    p.lds = (size_t)p.depth * kLaunchBlock * sizeof(int);
    return b;
}

// Ground fog: the extended family, forced, on the kernels compiled with CHUNKY_FOG (launch_plan.hpp has the table)
FogPlan plan_fog(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                 bool have_queue_and_staging, bool have_seeds_dev, bool biome_tinted) {
    FogPlan f{plan_render_as(variant, F, O, projector_type, T, n_passes, have_queue_and_staging, have_seeds_dev, false, true), FogRefusal::none};
    const RenderPlan& p = f.plan;
    if (biome_tinted) f.refusal = FogRefusal::biome;
    else if (variant & 4) f.refusal = FogRefusal::stats;
    else if (variant & (1 | 2 | 8)) f.refusal = FogRefusal::rig_bits;
    else if (projector_type > 0) f.refusal = FogRefusal::projected;
    else if (O.max_depth > 254) f.refusal = FogRefusal::max_depth;
    else if (!F.wide) f.refusal = FogRefusal::wide_tree;
    else if (has_bvh(F) && !F.bvh_records) f.refusal = FogRefusal::bvh_records;
    else if (p.why != NotPool::none || p.ext_refusal != ExtRefusal::none) f.refusal = FogRefusal::not_pool;  // (no work counter, arrays beyond 32-bit offsets)
    // (what is left is a render_pool plan of the extended family — plan_pool: trees 17 / 18 / -1, 32 parked paths, 16 with entity BVHs —
    // or one plan_render refused by its status: a launch too long for its seeds)
    return f;
}

const char* fog_refusal_text(FogRefusal r) {
    switch (r) {
        case FogRefusal::biome: return "fog: not with a biome map on the scene (chunky_scene_set_biome_tints); set CHUNKY_OPT_BIOME_TINT to 0, remove the map or turn fog off";
        case FogRefusal::stats: return "fog: the phase-statistics kernels (CHUNKY_OPT_KERNEL bit 2) have no fog; clear the bit or turn fog off";
        case FogRefusal::rig_bits: return "fog: needs the default kernel (CHUNKY_OPT_KERNEL bits 0, 1 and 3 clear): the fallback kernels and the reference-layout walk have no fog";
        case FogRefusal::projected: return "fog: projected cameras have no fog kernel; pass pre-generated rays (chunky_render_set_rays) or turn fog off";
        case FogRefusal::max_depth: return "fog: needs max depth <= 254 (CHUNKY_OPT_MAX_DEPTH)";
        case FogRefusal::wide_tree: return "fog: needs an octree the wide re-layout takes (depth <= 15)";
        case FogRefusal::bvh_records: return "fog: the scene's entity BVHs could not be re-laid out; the fallback kernels have no fog";
        case FogRefusal::not_pool: return "fog: the scene or the target sends this launch to the fallback kernels, which have no fog";
        default: return "";
    }
}

// Translucent blocks: the extended family, forced, on the kernels compiled with CHUNKY_GLASS and their wider parked record
GlassPlan plan_glass(int variant, const SceneFacts& F, const RenderOpts& O, int projector_type, const ShardView& T, int n_passes,
                     bool have_queue_and_staging, bool have_seeds_dev, bool biome_tinted, bool foggy) {
    GlassPlan g{plan_render_as(variant, F, O, projector_type, T, n_passes, have_queue_and_staging, have_seeds_dev, false, true), GlassRefusal::none};
    RenderPlan& p = g.plan;
    if (foggy) g.refusal = GlassRefusal::fog;
    else if (biome_tinted) g.refusal = GlassRefusal::biome;
    else if (variant & 4) g.refusal = GlassRefusal::stats;
    else if (variant & (1 | 2 | 8)) g.refusal = GlassRefusal::rig_bits;
    else if (projector_type > 0) g.refusal = GlassRefusal::projected;
    else if (O.max_depth > 254) g.refusal = GlassRefusal::max_depth;
    else if (!F.wide) g.refusal = GlassRefusal::wide_tree;
    else if (has_bvh(F) && !F.bvh_records) g.refusal = GlassRefusal::bvh_records;
    else if (p.why != NotPool::none || p.ext_refusal != ExtRefusal::none) g.refusal = GlassRefusal::not_pool;
    if (g.refusal == GlassRefusal::none && p.status == PlanStatus::ok && p.family == KernelFamily::pool) {
        // the glass units' parked record: the launch sizes the LDS with what the kernel carves it with (pool_kernel.inc)
        p.words = kPoolGlassWords;
        p.lds = (size_t)(kLaunchBlock / 64) * pool_wave_lds_bytes(p.park, p.words, (unsigned)p.depth);
    }
    return g;
}

const char* glass_refusal_text(GlassRefusal r) {
    switch (r) {
        case GlassRefusal::fog: return "translucency: not with a fog layer on the target (chunky_render_set_fog); turn fog off (density 0) or translucency off";
        case GlassRefusal::biome: return "translucency: not with a biome map on the scene (chunky_scene_set_biome_tints); set CHUNKY_OPT_BIOME_TINT to 0, remove the map or turn translucency off";
        case GlassRefusal::stats: return "translucency: the phase-statistics kernels (CHUNKY_OPT_KERNEL bit 2) have no translucency; clear the bit or turn translucency off";
        case GlassRefusal::rig_bits: return "translucency: needs the default kernel (CHUNKY_OPT_KERNEL bits 0, 1 and 3 clear): the fallback kernels and the reference-layout walk have no translucency";
        case GlassRefusal::projected: return "translucency: projected cameras have no translucency kernel; pass pre-generated rays (chunky_render_set_rays) or turn translucency off";
        case GlassRefusal::max_depth: return "translucency: needs max depth <= 254 (CHUNKY_OPT_MAX_DEPTH)";
        case GlassRefusal::wide_tree: return "translucency: needs an octree the wide re-layout takes (depth <= 15)";
        case GlassRefusal::bvh_records: return "translucency: the scene's entity BVHs could not be re-laid out; the fallback kernels have no translucency";
        case GlassRefusal::not_pool: return "translucency: the scene or the target sends this launch to the fallback kernels, which have no translucency";
        default: return "";
    }
}

const char* biome_refusal_text(BiomeRefusal r) {
    switch (r) {
        case BiomeRefusal::stats: return "biome tints: the phase-statistics kernels (CHUNKY_OPT_KERNEL bit 2) do not tint by position; set CHUNKY_OPT_BIOME_TINT to 0 or remove the map";
        case BiomeRefusal::extended: return "biome tints: the extended light-transport options do not tint by position; set CHUNKY_OPT_BIOME_TINT to 0 or remove the map";
        case BiomeRefusal::projected: return "biome tints: projected cameras are tinted by render_lanes only (CHUNKY_OPT_KERNEL bit 1); or set CHUNKY_OPT_BIOME_TINT to 0 or remove the map";
        default: return "";
    }
}

}  // namespace chunky
