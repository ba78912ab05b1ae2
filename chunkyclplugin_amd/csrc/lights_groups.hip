// lights_groups.hip — the light-group kernel with the emitters' share split by block and entity (lights_device.hpp, "Emitter groups";
// chunky_render_light_set_emitter_groups), and the mix over those images.  A unit of its own: lights.hip's instantiations, which run
// whenever no groups are set, stay the code they were.
#include "lights_device.hpp"

namespace chunky {

template <int TREE, bool BVH, bool PROJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(light_waves(BVH)))) light_group_kernel(LightGroupArgs) {
    static_assert(sizeof(LightGroupArgs) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
    typedef LightGroupOut LightOut;  // (the name the body has for the tail of its arguments)
    constexpr bool GROUPS = true;
#include "lights_walk.inc"
}

hipError_t launch_light_groups(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                               float* const images[4], const LightGroupImages& G, int* counter, hipStream_t stream, AovChoice* chosen) {
    if (G.n_groups < 1 || G.n_groups > kLightMaxGroups || G.n_blocks < 0 || !G.images || !G.acc || !G.touched || !G.of_block) return hipErrorInvalidValue;
    const hipError_t e = launch_first_hit_args<LightGroupOut>(
        [](auto tree, auto bvh, auto proj) -> void (*)(LightGroupArgs) { return light_group_kernel<decltype(tree)::value, decltype(bvh)::value, decltype(proj)::value>; },
        variant, S, C, O, T, P,
        LightGroupOut{{images[0], images[1], images[2], images[3]}, O.max_depth, O.emitter_scale, G.n_groups, G.n_blocks, G.images, G.acc, G.touched, G.of_block,
                      G.world_group, G.actor_group},
        counter, stream, chosen);
    if (e == hipSuccess && chosen) chosen->bvh |= kChoiceLightGroups;
    return e;
}

struct LightMixWeights {
    float sky, sun, group[kLightMaxGroups];
};

// out = ((w_sky * SKY + w_sun * SUN) + w[0] * G0) + w[1] * G1 ... per float, in that order (-ffp-contract=off: no fma)
__global__ void __launch_bounds__(256) light_group_mix_kernel(const float* __restrict__ sky, const float* __restrict__ sun, const float* __restrict__ groups,
                                                               int n_groups, LightMixWeights w, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = w.sky * sky[i] + w.sun * sun[i];
#pragma unroll
    for (int g = 0; g < kLightMaxGroups; g++)
        if (g < n_groups) v = v + w.group[g] * groups[(long long)g * n + i];
    out[i] = v;
}

hipError_t launch_light_group_mix(const float* sky, const float* sun, const float* groups, int n_groups, float w_sky, float w_sun, const float* w_groups,
                                  float* out, long long n, hipStream_t stream) {
    if (n_groups < 0 || n_groups > kLightMaxGroups) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    LightMixWeights w{w_sky, w_sun, {0, 0, 0, 0, 0, 0, 0, 0}};
    for (int g = 0; g < n_groups; g++) w.group[g] = w_groups[g];
    hipLaunchKernelGGL(light_group_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sky, sun, groups, n_groups, w, out, n);
    return hipGetLastError();
}

}  // namespace chunky
