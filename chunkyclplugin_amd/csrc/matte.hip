// matte.hip — antialiased ID mattes (chunky_render_matte_passes, _ranks, _extract): per pixel six (id, count) slots and an overflow
// word, counted over the first hit of every pass's camera ray.
//
// Specification (the arithmetic is matte_spec.h, which matte_host.cpp compiles too): the sample of pass k at
// pixel gid is the AOV sample (aov.hip) — RNG state seed + gid, Random_nextState, the camera ray, one closestIntersect — and its id
// names the last part of closestIntersect that won: the octree's block, the world BVH, the actor BVH, or the sky.
//
// The kernel is first_hit_pass.hpp's with MatteFold below.  A lane owns its pixel for the launch: it loads the pixel's 13 words once,
// folds every pass in registers (matte_update: a compare-and-select chain over six named pairs) and stores them once.  The planes
// are slot-major, so a wave's loads and stores are whole rows.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "first_hit_pass.hpp"
#include "matte_spec.h"

namespace chunky {

// a pixel's six (id, count) slots off the planes (q: its word in the first, np: words per plane), and its overflow word where OTHER
// (the read-outs do not need it)
template <bool OTHER>
DEV matte_px_t matte_load(const int* __restrict__ q, size_t np) {
    matte_px_t p;
    p.id0 = q[0], p.id1 = q[np], p.id2 = q[2 * np], p.id3 = q[3 * np], p.id4 = q[4 * np], p.id5 = q[5 * np];
    p.c0 = q[6 * np], p.c1 = q[7 * np], p.c2 = q[8 * np], p.c3 = q[9 * np], p.c4 = q[10 * np], p.c5 = q[11 * np];
    p.other = OTHER ? q[12 * np] : 0;
    return p;
}

struct MatteFold {
    struct Out {
        int* planes;  // 13 planes of width * height words: six of ids, six of counts, `other`
    };
    matte_px_t p;
    // Neither the ray nor the hit's colour, normal or emittance outlives the trace, and the pixel's state is 13 integers: five waves per
    // SIMD (at most 96 VGPRs) with and without the BVH walk — 83 to 84 VGPRs without it, 87 to 88 with it, no scratch (AovFold needs
    // four with the walk).  Held to the 80 VGPRs of six waves, the forms without the walk spill 8 - 12 bytes per lane to scratch.
    static constexpr int waves(bool) { return 5; }
    static constexpr bool kParts = true;
    template <class ArgPtr>
    DEV void load(ArgPtr a, int gid, int n_pixels) {
        p = matte_load<true>(a->out.planes + gid, (size_t)n_pixels);
    }
    // the id names the last part of closestIntersect that won
    DEV void absorb(int part, const Hit& h, const RayOD&, int, int) { matte_update(&p, matte_id(part != 0, h.material, part == 2, part == 3)); }
    DEV void store(int gid, int n_pixels) {
        const size_t np = (size_t)n_pixels;
        int* __restrict__ o = first_hit_args<Out>()->out.planes + gid;
        o[0] = p.id0, o[np] = p.id1, o[2 * np] = p.id2, o[3 * np] = p.id3, o[4 * np] = p.id4, o[5 * np] = p.id5;
        o[6 * np] = p.c0, o[7 * np] = p.c1, o[8 * np] = p.c2, o[9 * np] = p.c3, o[10 * np] = p.c4, o[11 * np] = p.c5;
        o[12 * np] = p.other;
    }
};

hipError_t launch_matte(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                        int* planes, int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit<MatteFold>(variant, S, C, O, T, P, MatteFold::Out{planes}, counter, stream, chosen);
}

// ---------------------------------------------------------------------------------------------
// The read-outs: one lane per pixel over the planes.

// ranks: every slot goes to the plane of its rank (matte_ranks: a fixed stable order of six in registers) — the six stores of a lane
// land in six different planes, one each
__global__ void __launch_bounds__(256) matte_ranks_kernel(const int* __restrict__ planes, long long n_pixels, int passes, int* __restrict__ out_ids,
                                                           float* __restrict__ out_coverage) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_pixels) return;
    const size_t np = (size_t)n_pixels;
    const matte_px_t p = matte_load<false>(planes + gid, np);
    const matte_rank_t r = matte_ranks(&p);
    int* __restrict__ oi = out_ids + gid;
    float* __restrict__ oc = out_coverage + gid;
    oi[(size_t)r.r0 * np] = matte_rank_id(p.id0, p.c0), oc[(size_t)r.r0 * np] = matte_coverage(p.c0, passes);
    oi[(size_t)r.r1 * np] = matte_rank_id(p.id1, p.c1), oc[(size_t)r.r1 * np] = matte_coverage(p.c1, passes);
    oi[(size_t)r.r2 * np] = matte_rank_id(p.id2, p.c2), oc[(size_t)r.r2 * np] = matte_coverage(p.c2, passes);
    oi[(size_t)r.r3 * np] = matte_rank_id(p.id3, p.c3), oc[(size_t)r.r3 * np] = matte_coverage(p.c3, passes);
    oi[(size_t)r.r4 * np] = matte_rank_id(p.id4, p.c4), oc[(size_t)r.r4 * np] = matte_coverage(p.c4, passes);
    oi[(size_t)r.r5 * np] = matte_rank_id(p.id5, p.c5), oc[(size_t)r.r5 * np] = matte_coverage(p.c5, passes);
}

// extract: a binary search of the sorted, de-duplicated set per occupied slot
__global__ void __launch_bounds__(256) matte_extract_kernel(const int* __restrict__ planes, long long n_pixels, int passes, const int* __restrict__ sorted,
                                                             int n_set, float* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_pixels) return;
    const matte_px_t p = matte_load<false>(planes + gid, (size_t)n_pixels);
    out[gid] = matte_mask(matte_masked_sum(&p, sorted, n_set), passes);
}

hipError_t launch_matte_ranks(const int* planes, long long n_pixels, int passes, int* out_ids, float* out_coverage, hipStream_t stream) {
    if (n_pixels <= 0) return hipSuccess;
    if (passes <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matte_ranks_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, planes, n_pixels, passes, out_ids, out_coverage);
    return hipGetLastError();
}

hipError_t launch_matte_extract(const int* planes, long long n_pixels, int passes, const int* sorted, int n_set, float* out, hipStream_t stream) {
    if (n_pixels <= 0) return hipSuccess;
    if (passes <= 0 || n_set < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(matte_extract_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, planes, n_pixels, passes, sorted, n_set, out);
    return hipGetLastError();
}

}  // namespace chunky
