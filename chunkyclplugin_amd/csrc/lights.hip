// lights.hip — light groups: the sky's, the sun's and the emitters' share of the beauty image as images of their own, from one walk
// of every path (chunky_render_light_passes).  Specification, the skipped terms and the kernel's body: lights_device.hpp.  This unit
// holds the instantiations for the four images alone; with emitter groups set, lights_groups.hip's run instead.
#include "lights_device.hpp"

namespace chunky {

template <int TREE, bool BVH, bool PROJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(light_waves(BVH)))) light_kernel(LightArgs) {
    static_assert(sizeof(LightArgs) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
    constexpr bool GROUPS = false;
#include "lights_walk.inc"
}

// (first_hit_pass.hpp launch_first_hit_args: the first-hit passes' tree forms and launch arithmetic)
hipError_t launch_lights(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                         float* const images[4], int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit_args<LightOut>(
        [](auto tree, auto bvh, auto proj) -> void (*)(LightArgs) { return light_kernel<decltype(tree)::value, decltype(bvh)::value, decltype(proj)::value>; },
        variant, S, C, O, T, P, LightOut{{images[0], images[1], images[2], images[3]}, O.max_depth, O.emitter_scale}, counter, stream, chosen);
}

// out = (w0 * SKY + w1 * SUN) + w2 * EMITTERS per float, in that order (-ffp-contract=off: no fma)
__global__ void __launch_bounds__(256) light_mix_kernel(const float* __restrict__ sky, const float* __restrict__ sun, const float* __restrict__ emitters,
                                                         float w0, float w1, float w2, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (w0 * sky[i] + w1 * sun[i]) + w2 * emitters[i];
}

hipError_t launch_light_mix(const float* sky, const float* sun, const float* emitters, const float w[3], float* out, long long n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(light_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sky, sun, emitters, w[0], w[1], w[2], out, n);
    return hipGetLastError();
}

}  // namespace chunky
