// aov.hip — the denoiser's auxiliary images (chunky_render_aov_passes): albedo and normal of the first surface each camera ray
// hits, folded over passes with the reference's running mean.
//
// Specification: the sample of pass k at pixel gid is the FIRST trace of reference pass k — RNG state
// seed + gid, Random_nextState, the camera ray (K/rayTracer.cl:55-91), one closestIntersect (K/kernel.h:14-24) — so AOV pass k
// sees exactly the camera ray render pass k sees with the same seed.  Hit: albedo = record.color.xyz as closestIntersect leaves
// it (before applyRayColor), normal = record.normal.  Miss: albedo = the radiance of a reference sample whose first trace
// misses (intersectSky with record.emittance = 1 and throughput 1, K/rayTracer.cl:94-97), normal = 0.  Each channel is folded
// with (aov * spp + v) / (spp + 1) in float, in pass order (K/rayTracer.cl:109-112).
//
// Kernel: a persistent grid sized from the CU count; each wave claims 64 pixel slots at a time — a quarter of one of
// render_pool's 16 x 16 tiles (pool_slot_gid: the same tiles, sub-blocks and shard forms), so the rays of a wave are coherent and
// tiles that are mostly sky do not leave CUs idle.  A lane owns one pixel for every pass of the launch and folds both images in
// registers: each AOV word is read once and written once per launch.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "path_state.hpp"

namespace chunky {

struct AovArgs {
    SceneView S;
    CameraView C;
    ShardView T;
    PassSeeds P;
    int draw_depth;
    int n_units;     // claims of kAovUnit pixel slots: the rank's tiles x 4
    int* counter;    // next unclaimed unit (zeroed before every launch)
    float* albedo;   // 3 * width * height floats each
    float* normal;
};
static_assert(sizeof(AovArgs) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
constexpr int kAovUnit = 64;  // pixel slots per claim: one wave's worth, a quarter of a 16 x 16 tile (16 x 4 pixels)

// closestIntersect (path_state.hpp closest_hit) with the entity-BVH walk present only where the scene has entities, and without
// the hit point the AOV does not need
template <int TREE, bool BVH>
DEV bool first_hit(const SceneView& S, f3 o, f3 d, int draw_depth, Hit& h, LdsStack& stack) {
    bool hit = octree_hit<TREE>(S, o, d, draw_depth, h);
    if (BVH) {
        if (!S.world_bvh_empty) hit |= bvh_hit(S, S.world_bvh, o, d, h, stack);
        if (!S.actor_bvh_empty) hit |= bvh_hit(S, S.actor_bvh, o, d, h, stack);
    }
    return hit;
}

// The launch arguments are read through the kernel-argument segment pointer, and that pointer is made opaque again before each
// stage of a pass (the camera ray, the trace, the sky): the scalars each stage needs are loaded where they are used instead of
// being hoisted out of the loops and kept alive in spilled SGPRs (path_state.hpp fresh_args does the same for render_pool).
typedef const AovArgs __attribute__((address_space(4))) * AovArgPtr;
DEV AovArgPtr aov_args() {
    AovArgPtr a = (AovArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

// Five waves per SIMD (at most 96 VGPRs) without the BVH walk; with it, four (at five it would spill to scratch).  PROJ: a projected
// camera (projector types 1-5, 7, 8, rt_device.hpp projected_ray), instantiated apart so that the other cameras keep their code.
template <int TREE, bool BVH, bool PROJ = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BVH ? 4 : 5))) aov_kernel(AovArgs) {
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        AovArgPtr a = aov_args();
        const int width = a->C.width, height = a->C.height, n_pixels = width * height;
        // every lane of the wave is here (the exit below is wave-uniform): lane 0 claims, the others take its value
        int unit = 0;
        if (lane == 0) unit = atomicAdd(a->counter, 1);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a->n_units) break;
        const int gid = pool_slot_gid(arg_copy(&a->T), width, height, unit * kAovUnit + lane);
        if (gid < n_pixels) {  // (not a padding slot)
            float* __restrict__ pa = a->albedo + 3 * (size_t)gid;
            float* __restrict__ pn = a->normal + 3 * (size_t)gid;
            f3 ma = mk3(pa[0], pa[1], pa[2]), mn = mk3(pn[0], pn[1], pn[2]);
            const int px = gid % width, py = gid / width;
            const int n_passes = a->P.n, first_spp = a->P.first_spp;
            for (int k = 0; k < n_passes; k++) {
                AovArgPtr b = aov_args();
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
                f3 c, n;
                AovArgPtr t = aov_args();
                if (first_hit<TREE, BVH>(arg_copy(&t->S), r.o, r.d, t->draw_depth, h, stack)) {
                    c = mk3(h.color.x, h.color.y, h.color.z);
                    n = h.normal;
                } else {
                    // the sample's radiance: 0 + sky (K/rayTracer.cl:94-97)
                    c = mk3(0, 0, 0) + sky_radiance(arg_copy(&aov_args()->S), r.d, mk3(1, 1, 1), 1.0f);
                    n = mk3(0, 0, 0);
                }
                const int spp = first_spp + k;
                const float fs = (float)spp, fs1 = (float)(spp + 1);
                ma = f3{(ma.x * fs + c.x) / fs1, (ma.y * fs + c.y) / fs1, (ma.z * fs + c.z) / fs1};
                mn = f3{(mn.x * fs + n.x) / fs1, (mn.y * fs + n.y) / fs1, (mn.z * fs + n.z) / fs1};
            }
            pa[0] = ma.x;
            pa[1] = ma.y;
            pa[2] = ma.z;
            pn[0] = mn.x;
            pn[1] = mn.y;
            pn[2] = mn.z;
        }
    }
}

// The lookup form: the one launch_render's render_pool picks for the scene (tree_form; with entity BVHs the dense tops of one and
// two levels, else the generic walk), so that an AOV pass and a render pass of a view read the octree the same way.
static int aov_tree(int variant, const SceneView& S, bool bvh) {
    const int tree = tree_form(variant, S);
    if (tree == 0) return 0;
    if (bvh) return (tree == 17 || tree == 18) ? tree : -1;
    return (tree >= 16 && tree <= 19) ? tree : -1;
}

// the instantiation for the tree form and the camera
template <bool PROJ>
static void (*aov_instance(int tree, bool bvh))(AovArgs) {
    if (bvh) {
        switch (tree) {
            case 0: return aov_kernel<0, true, PROJ>;
            case 17: return aov_kernel<17, true, PROJ>;
            case 18: return aov_kernel<18, true, PROJ>;
            default: return aov_kernel<-1, true, PROJ>;
        }
    } else {
        switch (tree) {
            case 0: return aov_kernel<0, false, PROJ>;
            case 16: return aov_kernel<16, false, PROJ>;
            case 17: return aov_kernel<17, false, PROJ>;
            case 18: return aov_kernel<18, false, PROJ>;
            case 19: return aov_kernel<19, false, PROJ>;
            default: return aov_kernel<-1, false, PROJ>;
        }
    }
}

hipError_t launch_aov(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                      float* albedo, float* normal, int* counter, hipStream_t stream, AovChoice* chosen) {
    if (P.n <= 0 || T.n_local <= 0) return hipSuccess;
    if (P.n > kMaxPassesPerLaunch) return hipErrorInvalidValue;
    const bool bvh = !S.world_bvh_empty || !S.actor_bvh_empty;
    const int tree = aov_tree(variant, S, bvh);
    void (*k)(AovArgs) = C.projector_type > 0 ? aov_instance<true>(tree, bvh) : aov_instance<false>(tree, bvh);
    const int block = 256;
    const size_t lds = stack_lds_bytes(S, block);
    int n_cu = 0, occ = 0;
    hipError_t e = current_device_cus(&n_cu);
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, block, lds);
    if (e != hipSuccess) return e;
    const long long n_units = pool_tiles(T, C.width, C.height) * (kSampleTile / kAovUnit);
    const long long want = (n_units + block / 64 - 1) / (block / 64);  // no more workgroups than one claim per wave
    long long grid = (long long)n_cu * (occ > 0 ? occ : 1);
    if (grid > want) grid = want;
    if (chosen) *chosen = AovChoice{tree, bvh ? 1 : 0, (int)grid};
    e = hipMemsetAsync(counter, 0, sizeof(int), stream);
    if (e != hipSuccess) return e;
    AovArgs A{S, C, T, P, O.draw_depth, (int)n_units, counter, albedo, normal};
    A.T.list = nullptr;  // (pool_slot_gid maps every shard form itself)
    A.T.n_list = 0;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(block), lds, stream, A);
    return hipGetLastError();
}

}  // namespace chunky
