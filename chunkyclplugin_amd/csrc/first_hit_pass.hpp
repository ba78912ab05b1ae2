// first_hit_pass.hpp — the one kernel behind the passes that fold the FIRST hit of every pass's camera ray into per-pixel images: the
// AOV and AOV-ex passes (aov.hip) and the ID mattes (matte.hip).  Everything here is shared; what a pass has of its own is a Fold.
//
// The sample of pass k at pixel gid is the first trace of reference pass k: RNG state seed + gid, Random_nextState, the camera ray
// (K/rayTracer.cl:55-91), one closestIntersect (K/kernel.h:14-24).
//
// Kernel: a persistent grid sized from the CU count; each wave claims kFirstHitUnit pixel slots at a time — a quarter of one of
// render_pool's 16 x 16 tiles (pool_slot_gid: the same tiles, sub-blocks and shard forms), so the rays of a wave are coherent and
// tiles that are mostly sky do not leave CUs idle.  A lane owns one pixel for every pass of the launch and folds in registers: each
// word of the pass's images is read once and written once per launch.
//
// A Fold is a struct with
//   struct Out             the device pointers of its images (the tail of the launch arguments)
//   (members)              the pixel's running values, in registers
//   waves(bvh)             waves per SIMD the kernel is held to (constexpr)
//   kParts                 whether absorb is told WHICH part of closestIntersect won (an int, first_hit_part) or only whether one did
//   load(a, gid, n_pixels) read the pixel; `a` is the argument pointer of the claim
//   absorb(part, h, r, k, first_spp)  fold the sample of pass k: the trace's answer and record, the camera ray, and the samples
//                          folded before the launch (first_buffer_spp)
//   store(gid, n_pixels)   write the pixel
#pragma once
#include <type_traits>

#include "path_state.hpp"

namespace chunky {

template <class Out>
struct FirstHitArgs {
    SceneView S;
    CameraView C;
    ShardView T;
    PassSeeds P;
    int draw_depth;
    int n_units;   // claims of kFirstHitUnit pixel slots: the rank's tiles x 4
    int* counter;  // next unclaimed unit (zeroed before every launch)
    Out out;
};
constexpr int kFirstHitUnit = 64;  // pixel slots per claim: one wave's worth, a quarter of a 16 x 16 tile (16 x 4 pixels)

// The launch arguments are read through the kernel-argument segment pointer, and that pointer is made opaque again before each stage
// of a pass (the camera ray, the trace, a fold's sky term and its store): the scalars each stage needs are loaded where they are used
// instead of being hoisted out of the loops and kept alive in spilled SGPRs (path_state.hpp fresh_args does the same for render_pool).
template <class Out>
DEV auto first_hit_args() {
    return opaque_args<FirstHitArgs<Out>>();
}

// closestIntersect (path_state.hpp closest_hit) without the hit point, with the entity-BVH walk present only where the scene has
// entities.  PARTS: which part won — 0 nothing, 1 the octree's block, 2 a world-BVH triangle, 3 an actor-BVH triangle (bvh_hit returns
// true only where a triangle passed triangle_hit's `tt < best`, so a later part that answers true has won).  Otherwise a bool, in the
// form the AOV kernels always had: asked for the part and tested against 0, their walks compile to other code (EXPERIMENTS.md R1).
template <int TREE, bool BVH, bool PARTS>
DEV auto first_hit_part(const SceneView& S, f3 o, f3 d, int draw_depth, Hit& h, LdsStack& stack) {
    if constexpr (PARTS) {
        int part = octree_hit<TREE>(S, o, d, draw_depth, h) ? 1 : 0;
        if (BVH) {
            if (!S.world_bvh_empty && bvh_hit(S, S.world_bvh, o, d, h, stack)) part = 2;
            if (!S.actor_bvh_empty && bvh_hit(S, S.actor_bvh, o, d, h, stack)) part = 3;
        }
        return part;
    } else {
        bool hit = octree_hit<TREE>(S, o, d, draw_depth, h);
        if (BVH) {
            if (!S.world_bvh_empty) hit |= bvh_hit(S, S.world_bvh, o, d, h, stack);
            if (!S.actor_bvh_empty) hit |= bvh_hit(S, S.actor_bvh, o, d, h, stack);
        }
        return hit;
    }
}

// PROJ: a projected camera (projector types 1-5, 7, 8, rt_device.hpp projected_ray), instantiated apart so that the other cameras
// keep their code.
template <class Fold, int TREE, bool BVH, bool PROJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(Fold::waves(BVH)))) first_hit_kernel(CHUNKY_KERNEL_ARGS_HEAD FirstHitArgs<typename Fold::Out>) {
    static_assert(sizeof(FirstHitArgs<typename Fold::Out>) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        auto a = first_hit_args<typename Fold::Out>();
        const int width = a->C.width, height = a->C.height, n_pixels = width * height;
        // every lane of the wave is here (the exit below is wave-uniform): lane 0 claims, the others take its value
        int unit = 0;
        if (lane == 0) unit = atomicAdd(a->counter, 1);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a->n_units) break;
        const int gid = pool_slot_gid(arg_copy(&a->T), width, height, unit * kFirstHitUnit + lane);
        if (gid < n_pixels) {  // (not a padding slot)
            Fold f;
            f.load(a, gid, n_pixels);
            const int px = gid % width, py = gid / width;
            const int n_passes = a->P.n, first_spp = a->P.first_spp;
            for (int k = 0; k < n_passes; k++) {
                auto b = first_hit_args<typename Fold::Out>();
                const unsigned seed = (unsigned)b->P.seed[k];
                const CameraView C = arg_copy(&b->C);
                const CanvasPixel cp = canvas_pixel(C, gid, px, py);
                unsigned rng = seed + (unsigned)cp.G;  // K/rayTracer.cl:54-56
                rt_pcg_next(&rng);
                const RayOD r = primary_ray<PROJ>(C, seed, gid, cp, rng, false);
                Hit h;
                h.distance = rt_inf();
                h.material = 0;
                h.normal = mk3(0, 0, 0);
                h.color = f4{0, 0, 0, 0};
                h.emittance = 0;
                h.spec = 0;
                auto t = first_hit_args<typename Fold::Out>();
                const auto part = first_hit_part<TREE, BVH, Fold::kParts>(arg_copy(&t->S), r.o, r.d, t->draw_depth, h, stack);
                f.absorb(part, h, r, k, first_spp);
            }
            f.store(gid, n_pixels);
        }
    }
}

// The instantiation of a first-hit kernel for a tree form and the entity BVHs (launch_plan.hpp plan_first_hit and
// CHUNKY_FIRST_HIT_INSTANCES): pick(tree constant, BVH constant) names the kernel; null when the list has no such form.
template <class Kernel, class Pick>
Kernel first_hit_lookup(const FirstHitPlan& plan, Pick pick) {
#define CHUNKY_FIRST_HIT_CASE(TREE, BVH) \
    if (plan.tree == (TREE) && plan.bvh == (BVH)) return pick(std::integral_constant<int, TREE>(), std::integral_constant<bool, BVH>());
    CHUNKY_FIRST_HIT_INSTANCES(CHUNKY_FIRST_HIT_CASE)
#undef CHUNKY_FIRST_HIT_CASE
    return nullptr;
}

// A launch of a kernel that takes FirstHitArgs<Out> (first_hit_kernel, occlusion.hip's occlusion_kernel): a persistent grid, no more
// workgroups than one claim per wave.  pick(tree constant, BVH constant, PROJ constant) names the instantiation.
// `biome`: the map that heads the arguments of the kernels of a unit compiled with CHUNKY_BIOME_TINT (rt_device.hpp); no other unit reads it.
// (BIOME is part of the two launchers' names: a biome unit's instantiations are functions of their own, never merged with another unit's.)
template <class Out, class Pick, bool BIOME = (CHUNKY_BIOME_TINT != 0)>
hipError_t launch_first_hit_args(Pick pick, int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                                 const PassSeeds& P, const Out& out, int* counter, hipStream_t stream, AovChoice* chosen,
                                 const BiomeMap* biome = nullptr) {
    if (P.n <= 0 || T.n_local <= 0) return hipSuccess;
    if (P.n > kMaxPassesPerLaunch) return hipErrorInvalidValue;
    const FirstHitPlan plan = plan_first_hit(variant, scene_facts(S));
    typedef void (*Kernel)(CHUNKY_KERNEL_ARGS_HEAD FirstHitArgs<Out>);
    if (BIOME && !biome) return hipErrorInvalidValue;
    (void)biome;
    const Kernel k = C.projector_type > 0 ? first_hit_lookup<Kernel>(plan, [&](auto tree, auto bvh) { return pick(tree, bvh, std::true_type()); })
                                          : first_hit_lookup<Kernel>(plan, [&](auto tree, auto bvh) { return pick(tree, bvh, std::false_type()); });
    if (!k) return hipErrorInvalidDeviceFunction;  // a plan outside the list: an error, never another kernel
    const int block = kLaunchBlock;
    const size_t lds = stack_lds_bytes(scene_facts(S), block);
    const long long n_units = pool_tiles(T, C.width, C.height) * (kSampleTile / kFirstHitUnit);
    int grid = 0;
    if (hipError_t e = persistent_grid(k, block, lds, (n_units + block / 64 - 1) / (block / 64), &grid)) return e;
    if (chosen) *chosen = AovChoice{plan.tree, (plan.bvh ? 1 : 0) | (BIOME ? kChoiceBiome : 0), grid};
    hipError_t e = hipMemsetAsync(counter, 0, sizeof(int), stream);
    if (e != hipSuccess) return e;
    FirstHitArgs<Out> A{S, C, T, P, O.draw_depth, (int)n_units, counter, out};
    A.T.list = nullptr;  // (pool_slot_gid maps every shard form itself)
    A.T.n_list = 0;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(block), lds, stream, CHUNKY_LAUNCH_ARGS_HEAD(*biome) A);
    return hipGetLastError();
}

template <class Fold, bool BIOME = (CHUNKY_BIOME_TINT != 0)>
hipError_t launch_first_hit(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                            const typename Fold::Out& out, int* counter, hipStream_t stream, AovChoice* chosen, const BiomeMap* biome = nullptr) {
    return launch_first_hit_args<typename Fold::Out>(
        [](auto tree, auto bvh, auto proj) -> void (*)(CHUNKY_KERNEL_ARGS_HEAD FirstHitArgs<typename Fold::Out>) { return first_hit_kernel<Fold, decltype(tree)::value, decltype(bvh)::value, decltype(proj)::value>; },
        variant, S, C, O, T, P, out, counter, stream, chosen, biome);
}

}  // namespace chunky
