// matte.hip — antialiased ID mattes (chunky_render_matte_passes, _ranks, _extract): per pixel six (id, count) slots and an overflow
// word, counted over the first hit of every pass's camera ray.
//
// Specification (the arithmetic is matte_spec.h, which matte_host.cpp compiles too): the sample of pass k at
// pixel gid is the AOV sample (aov.hip) — RNG state seed + gid, Random_nextState, the camera ray, one closestIntersect — and its id
// names the last part of closestIntersect that won: the octree's block, the world BVH, the actor BVH, or the sky.
//
// matte_kernel is a sibling of aov_kernel with the same persistent grid and the same 64-slot claims (pool_slot_gid).  A lane owns
// its pixel for the launch: it loads the pixel's 13 words once, folds every pass in registers (matte_update: a compare-and-select
// chain over six named pairs) and stores them once.  The planes are slot-major, so a wave's loads and stores are whole rows.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "matte_spec.h"
#include "path_state.hpp"

namespace chunky {

struct MatteArgs {
    SceneView S;
    CameraView C;
    ShardView T;
    PassSeeds P;
    int draw_depth;
    int n_units;   // claims of kMatteUnit pixel slots: the rank's tiles x 4
    int* counter;  // next unclaimed unit (zeroed before every launch)
    int* planes;   // 13 planes of width * height words: six of ids, six of counts, `other`
};
static_assert(sizeof(MatteArgs) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
constexpr int kMatteUnit = 64;  // pixel slots per claim: one wave's worth, a quarter of a 16 x 16 tile (as aov.hip kAovUnit)

// closestIntersect (path_state.hpp closest_hit) reporting which part won: 0 nothing, 1 the octree's block, 2 a world-BVH triangle,
// 3 an actor-BVH triangle.  bvh_hit returns true only where a triangle passed triangle_hit's `tt < best`, so a later part that
// answers true has won.
template <int TREE, bool BVH>
DEV int first_hit_part(const SceneView& S, f3 o, f3 d, int draw_depth, Hit& h, LdsStack& stack) {
    int part = octree_hit<TREE>(S, o, d, draw_depth, h) ? 1 : 0;
    if (BVH) {
        if (!S.world_bvh_empty && bvh_hit(S, S.world_bvh, o, d, h, stack)) part = 2;
        if (!S.actor_bvh_empty && bvh_hit(S, S.actor_bvh, o, d, h, stack)) part = 3;
    }
    return part;
}

// the kernel-argument pointer, made opaque before each stage as aov.hip does (the scalars a stage needs are loaded where they are used)
typedef const MatteArgs __attribute__((address_space(4))) * MatteArgPtr;
DEV MatteArgPtr matte_args() {
    MatteArgPtr a = (MatteArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

// Neither the ray nor the hit's colour, normal or emittance outlives the trace, and the pixel's state is 13 integers: five waves per
// SIMD (at most 96 VGPRs) with and without the BVH walk — 83 to 84 VGPRs without it, 87 to 88 with it, no scratch (aov_kernel needs
// four with the walk).  Held to the 80 VGPRs of six waves, the forms without the walk spill 8 - 12 bytes per lane to scratch.
template <int TREE, bool BVH, bool PROJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) matte_kernel(MatteArgs) {
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        MatteArgPtr a = matte_args();
        const int width = a->C.width, height = a->C.height, n_pixels = width * height;
        // every lane of the wave is here (the exit below is wave-uniform): lane 0 claims, the others take its value
        int unit = 0;
        if (lane == 0) unit = atomicAdd(a->counter, 1);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a->n_units) break;
        const int gid = pool_slot_gid(arg_copy(&a->T), width, height, unit * kMatteUnit + lane);
        if (gid < n_pixels) {  // (not a padding slot)
            int* __restrict__ q = a->planes + gid;
            const size_t np = (size_t)n_pixels;
            matte_px_t p;
            p.id0 = q[0], p.id1 = q[np], p.id2 = q[2 * np], p.id3 = q[3 * np], p.id4 = q[4 * np], p.id5 = q[5 * np];
            p.c0 = q[6 * np], p.c1 = q[7 * np], p.c2 = q[8 * np], p.c3 = q[9 * np], p.c4 = q[10 * np], p.c5 = q[11 * np];
            p.other = q[12 * np];
            const int px = gid % width, py = gid / width;
            const int n_passes = a->P.n;
            for (int k = 0; k < n_passes; k++) {
                MatteArgPtr b = matte_args();
                const unsigned seed = (unsigned)b->P.seed[k];
                unsigned rng = seed + (unsigned)gid;  // K/rayTracer.cl:54-56
                rt_pcg_next(&rng);
                const RayOD r = primary_ray<PROJ>(arg_copy(&b->C), seed, gid, rng, false, px, py);
                Hit h;
                h.distance = rt_inf();
                h.material = 0;
                h.normal = mk3(0, 0, 0);
                h.color = f4{0, 0, 0, 0};
                h.emittance = 0;
                h.spec = 0;
                MatteArgPtr t = matte_args();
                const int part = first_hit_part<TREE, BVH>(arg_copy(&t->S), r.o, r.d, t->draw_depth, h, stack);
                matte_update(&p, matte_id(part != 0, h.material, part == 2, part == 3));
            }
            MatteArgPtr w = matte_args();
            int* __restrict__ o = w->planes + gid;
            o[0] = p.id0, o[np] = p.id1, o[2 * np] = p.id2, o[3 * np] = p.id3, o[4 * np] = p.id4, o[5 * np] = p.id5;
            o[6 * np] = p.c0, o[7 * np] = p.c1, o[8 * np] = p.c2, o[9 * np] = p.c3, o[10 * np] = p.c4, o[11 * np] = p.c5;
            o[12 * np] = p.other;
        }
    }
}

// The lookup form, chosen as aov.hip's aov_tree chooses it (the form render_pool runs for the scene): with entity BVHs the dense tops
// of one and two levels, else the generic walk
static int matte_tree(int variant, const SceneView& S, bool bvh) {
    const int tree = tree_form(variant, S);
    if (tree == 0) return 0;
    if (bvh) return (tree == 17 || tree == 18) ? tree : -1;
    return (tree >= 16 && tree <= 19) ? tree : -1;
}

template <bool PROJ>
static void (*matte_instance(int tree, bool bvh))(MatteArgs) {
    if (bvh) {
        switch (tree) {
            case 0: return matte_kernel<0, true, PROJ>;
            case 17: return matte_kernel<17, true, PROJ>;
            case 18: return matte_kernel<18, true, PROJ>;
            default: return matte_kernel<-1, true, PROJ>;
        }
    } else {
        switch (tree) {
            case 0: return matte_kernel<0, false, PROJ>;
            case 16: return matte_kernel<16, false, PROJ>;
            case 17: return matte_kernel<17, false, PROJ>;
            case 18: return matte_kernel<18, false, PROJ>;
            case 19: return matte_kernel<19, false, PROJ>;
            default: return matte_kernel<-1, false, PROJ>;
        }
    }
}

hipError_t launch_matte(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                        int* planes, int* counter, hipStream_t stream, AovChoice* chosen) {
    if (P.n <= 0 || T.n_local <= 0) return hipSuccess;
    if (P.n > kMaxPassesPerLaunch) return hipErrorInvalidValue;
    const bool bvh = !S.world_bvh_empty || !S.actor_bvh_empty;
    const int tree = matte_tree(variant, S, bvh);
    void (*k)(MatteArgs) = C.projector_type > 0 ? matte_instance<true>(tree, bvh) : matte_instance<false>(tree, bvh);
    const int block = 256;
    const size_t lds = stack_lds_bytes(S, block);
    int n_cu = 0, occ = 0;
    hipError_t e = current_device_cus(&n_cu);
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, block, lds);
    if (e != hipSuccess) return e;
    const long long n_units = pool_tiles(T, C.width, C.height) * (kSampleTile / kMatteUnit);
    const long long want = (n_units + block / 64 - 1) / (block / 64);  // no more workgroups than one claim per wave
    long long grid = (long long)n_cu * (occ > 0 ? occ : 1);
    if (grid > want) grid = want;
    if (chosen) *chosen = AovChoice{tree, bvh ? 1 : 0, (int)grid};
    e = hipMemsetAsync(counter, 0, sizeof(int), stream);
    if (e != hipSuccess) return e;
    MatteArgs A{S, C, T, P, O.draw_depth, (int)n_units, counter, planes};
    A.T.list = nullptr;  // (pool_slot_gid maps every shard form itself)
    A.T.n_list = 0;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(block), lds, stream, A);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The read-outs: one lane per pixel over the planes.
DEV matte_px_t matte_load(const int* __restrict__ planes, size_t np, size_t gid) {
    const int* __restrict__ q = planes + gid;
    matte_px_t p;
    p.id0 = q[0], p.id1 = q[np], p.id2 = q[2 * np], p.id3 = q[3 * np], p.id4 = q[4 * np], p.id5 = q[5 * np];
    p.c0 = q[6 * np], p.c1 = q[7 * np], p.c2 = q[8 * np], p.c3 = q[9 * np], p.c4 = q[10 * np], p.c5 = q[11 * np];
    p.other = 0;
    return p;
}

// ranks: every slot goes to the plane of its rank (matte_ranks: a fixed stable order of six in registers) — the six stores of a lane
// land in six different planes, one each
__global__ void __launch_bounds__(256) matte_ranks_kernel(const int* __restrict__ planes, long long n_pixels, int passes, int* __restrict__ out_ids,
                                                           float* __restrict__ out_coverage) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_pixels) return;
    const size_t np = (size_t)n_pixels;
    const matte_px_t p = matte_load(planes, np, (size_t)gid);
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
    const matte_px_t p = matte_load(planes, (size_t)n_pixels, (size_t)gid);
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
