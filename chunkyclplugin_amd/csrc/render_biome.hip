// render_biome.hip — biome tints by block position on the kernels that bind a path to a lane: render_lanes
// (what plan_biome sends the fallback families to), preview_lanes and trace_records_kernel, instantiated once more with
// CHUNKY_BIOME_TINT: the scene's biome map heads their arguments, and a block's material of tint type 1, 2 or 3 multiplies by the
// colour of the block test's cell where the other units multiply by the reference's constants (rt_device.hpp material_eval).
// The pool kernel's instantiations are render_pool_biome.hip's, the AOV kernels' aov_biome.hip's.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#define CHUNKY_BIOME_TINT 1
#include <hip/hip_runtime.h>

#include "lane_kernels.hpp"

namespace chunky {

// render_lanes as plan_biome names it (launch_plan.cpp): the reference octree layout (0) and the generic wide tree (-1), as launch_fallback's
hipError_t launch_lanes_biome(const RenderPlan& plan, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O,
                              const ShardView& T, const PassSeeds& P, float* res, hipStream_t stream, KernelChoice* chosen) {
    if (plan.family != KernelFamily::lanes) return hipErrorInvalidValue;
    const int block = kLaunchBlock;
    const int grid = (T.n_local + block - 1) / block;
    if (grid <= 0 || P.n <= 0) return hipSuccess;
    void (*k)(BiomeMap, SceneView, CameraView, RenderOpts, ShardView, PassSeeds, float*) = nullptr;
#define CHUNKY_LANES_CASE(TREE) \
    if (plan.tree == (TREE)) k = render_lanes<TREE>;
    CHUNKY_LANES_INSTANCES(CHUNKY_LANES_CASE)
#undef CHUNKY_LANES_CASE
    if (!k) return hipErrorInvalidDeviceFunction;  // a plan outside the list: an error, never another kernel
    if (chosen) *chosen = KernelChoice{plan.tree, 0, plan.bvh ? 1 : 0, grid, -1, kChoiceBiome};
    hipLaunchKernelGGL(k, dim3(grid), dim3(block), plan.lds, stream, B, S, C, O, T, P, res);
    return hipGetLastError();
}

hipError_t launch_trace_records_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, int seed,
                                      const int* gids_dev, int n, HitRecord* out, int* counts, float* radiance, hipStream_t stream) {
    const int block = 256;
    const int grid = (n + block - 1) / block;
    if (grid <= 0) return hipSuccess;
    const size_t lds = stack_lds_bytes(scene_facts(S), block);
    if (use_wide(variant, scene_facts(S)))
        hipLaunchKernelGGL(trace_records_kernel<-1>, dim3(grid), dim3(block), lds, stream, B, S, C, O, seed, gids_dev, n, out, counts, radiance);
    else
        hipLaunchKernelGGL(trace_records_kernel<0>, dim3(grid), dim3(block), lds, stream, B, S, C, O, seed, gids_dev, n, out, counts, radiance);
    return hipGetLastError();
}

hipError_t launch_preview_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, int* argb,
                                hipStream_t stream) {
    const int block = 256;
    const int grid = (C.width * C.height + block - 1) / block;
    const size_t lds = stack_lds_bytes(scene_facts(S), block);
    if (use_wide(variant, scene_facts(S)))
        hipLaunchKernelGGL(preview_lanes<-1>, dim3(grid), dim3(block), lds, stream, B, S, C, O, argb);
    else
        hipLaunchKernelGGL(preview_lanes<0>, dim3(grid), dim3(block), lds, stream, B, S, C, O, argb);
    return hipGetLastError();
}

}  // namespace chunky
