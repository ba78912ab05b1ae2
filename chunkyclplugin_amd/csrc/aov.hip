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

// ---------------------------------------------------------------------------------------------
// chunky_render_aov_passes_ex: the same sample, and five more images of its first hit folded beside albedo and
// normal — coverage, the ray parameter, the hit point, the emittance (running means; a miss contributes 0) and the block id (the
// last pass's value; a miss -1).  A sibling kernel with arguments of its own: aov_kernel above keeps its code and its registers.
struct AovExArgs {
    AovArgs A;
    float* alpha;      // width * height floats
    float* depth;      // width * height
    float* position;   // 3 * width * height
    float* emittance;  // width * height
    int* block;        // width * height int32
};
static_assert(sizeof(AovExArgs) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
typedef const AovExArgs __attribute__((address_space(4))) * AovExArgPtr;
DEV AovExArgPtr aov_ex_args() {
    AovExArgPtr a = (AovExArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}
DEV float fold_mean(float m, float fs, float v, float fs1) { return (m * fs + v) / fs1; }

// The ray's origin and direction stay alive across the trace (the hit point is o + d * (distance - kOffset), K/kernel.h:21) and seven
// more running values per lane: four waves per SIMD (at most 128 VGPRs) with and without the BVH walk (held to the 96 of five, the
// forms without it spill 36 - 52 bytes per lane to scratch).
template <int TREE, bool BVH, bool PROJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) aov_ex_kernel(AovExArgs) {
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        AovExArgPtr a = aov_ex_args();
        const int width = a->A.C.width, height = a->A.C.height, n_pixels = width * height;
        int unit = 0;
        if (lane == 0) unit = atomicAdd(a->A.counter, 1);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a->A.n_units) break;
        const int gid = pool_slot_gid(arg_copy(&a->A.T), width, height, unit * kAovUnit + lane);
        if (gid < n_pixels) {  // (not a padding slot)
            float* __restrict__ pa = a->A.albedo + 3 * (size_t)gid;
            float* __restrict__ pn = a->A.normal + 3 * (size_t)gid;
            float* __restrict__ pp = a->position + 3 * (size_t)gid;
            f3 ma = mk3(pa[0], pa[1], pa[2]), mn = mk3(pn[0], pn[1], pn[2]), mp = mk3(pp[0], pp[1], pp[2]);
            float m_alpha = a->alpha[gid], m_depth = a->depth[gid], m_emit = a->emittance[gid];
            int block = a->block[gid];
            const int px = gid % width, py = gid / width;
            const int n_passes = a->A.P.n, first_spp = a->A.P.first_spp;
            for (int k = 0; k < n_passes; k++) {
                AovExArgPtr b = aov_ex_args();
                const unsigned seed = (unsigned)b->A.P.seed[k];
                unsigned rng = seed + (unsigned)gid;  // K/rayTracer.cl:54-56
                rt_pcg_next(&rng);
                const RayOD r = primary_ray<PROJ>(arg_copy(&b->A.C), seed, gid, rng, false, px, py);
                Hit h;
                h.distance = rt_inf();
                h.material = 0;
                h.normal = mk3(0, 0, 0);
                h.color = f4{0, 0, 0, 0};
                h.emittance = 0;
                h.spec = 0;
                f3 c, n, p;
                float v_alpha, v_depth, v_emit;
                AovExArgPtr t = aov_ex_args();
                if (first_hit<TREE, BVH>(arg_copy(&t->A.S), r.o, r.d, t->A.draw_depth, h, stack)) {
                    c = mk3(h.color.x, h.color.y, h.color.z);
                    n = h.normal;
                    p = r.o + r.d * (h.distance - kOffset);  // closest_hit's point
                    v_alpha = 1.0f;
                    v_depth = h.distance;
                    v_emit = h.emittance;
                    block = h.material;
                } else {
                    c = mk3(0, 0, 0) + sky_radiance(arg_copy(&aov_ex_args()->A.S), r.d, mk3(1, 1, 1), 1.0f);
                    n = mk3(0, 0, 0);
                    p = mk3(0, 0, 0);
                    v_alpha = 0.0f;
                    v_depth = 0.0f;
                    v_emit = 0.0f;
                    block = -1;
                }
                const int spp = first_spp + k;
                const float fs = (float)spp, fs1 = (float)(spp + 1);
                ma = f3{fold_mean(ma.x, fs, c.x, fs1), fold_mean(ma.y, fs, c.y, fs1), fold_mean(ma.z, fs, c.z, fs1)};
                mn = f3{fold_mean(mn.x, fs, n.x, fs1), fold_mean(mn.y, fs, n.y, fs1), fold_mean(mn.z, fs, n.z, fs1)};
                mp = f3{fold_mean(mp.x, fs, p.x, fs1), fold_mean(mp.y, fs, p.y, fs1), fold_mean(mp.z, fs, p.z, fs1)};
                m_alpha = fold_mean(m_alpha, fs, v_alpha, fs1);
                m_depth = fold_mean(m_depth, fs, v_depth, fs1);
                m_emit = fold_mean(m_emit, fs, v_emit, fs1);
            }
            pa[0] = ma.x;
            pa[1] = ma.y;
            pa[2] = ma.z;
            pn[0] = mn.x;
            pn[1] = mn.y;
            pn[2] = mn.z;
            pp[0] = mp.x;
            pp[1] = mp.y;
            pp[2] = mp.z;
            AovExArgPtr w = aov_ex_args();
            w->alpha[gid] = m_alpha;
            w->depth[gid] = m_depth;
            w->emittance[gid] = m_emit;
            w->block[gid] = block;
        }
    }
}

template <bool PROJ>
static void (*aov_ex_instance(int tree, bool bvh))(AovExArgs) {
    if (bvh) {
        switch (tree) {
            case 0: return aov_ex_kernel<0, true, PROJ>;
            case 17: return aov_ex_kernel<17, true, PROJ>;
            case 18: return aov_ex_kernel<18, true, PROJ>;
            default: return aov_ex_kernel<-1, true, PROJ>;
        }
    } else {
        switch (tree) {
            case 0: return aov_ex_kernel<0, false, PROJ>;
            case 16: return aov_ex_kernel<16, false, PROJ>;
            case 17: return aov_ex_kernel<17, false, PROJ>;
            case 18: return aov_ex_kernel<18, false, PROJ>;
            case 19: return aov_ex_kernel<19, false, PROJ>;
            default: return aov_ex_kernel<-1, false, PROJ>;
        }
    }
}

hipError_t launch_aov_ex(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                         const AovExImages& I, int* counter, hipStream_t stream, AovChoice* chosen) {
    if (P.n <= 0 || T.n_local <= 0) return hipSuccess;
    if (P.n > kMaxPassesPerLaunch) return hipErrorInvalidValue;
    const bool bvh = !S.world_bvh_empty || !S.actor_bvh_empty;
    const int tree = aov_tree(variant, S, bvh);
    void (*k)(AovExArgs) = C.projector_type > 0 ? aov_ex_instance<true>(tree, bvh) : aov_ex_instance<false>(tree, bvh);
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
    AovExArgs A{AovArgs{S, C, T, P, O.draw_depth, (int)n_units, counter, I.albedo, I.normal}, I.alpha, I.depth, I.position, I.emittance, I.block};
    A.A.T.list = nullptr;  // (pool_slot_gid maps every shard form itself)
    A.A.T.n_list = 0;
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(block), lds, stream, A);
    return hipGetLastError();
}

}  // namespace chunky
