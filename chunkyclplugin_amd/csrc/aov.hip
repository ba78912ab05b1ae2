// aov.hip — the denoiser's auxiliary images (chunky_render_aov_passes): albedo and normal of the first surface each camera ray
// hits, folded over passes with the reference's running mean; and the five further first-hit images of chunky_render_aov_passes_ex.
//
// Specification: the sample of pass k at pixel gid is the FIRST trace of reference pass k (first_hit_pass.hpp,
// which holds the kernel), so AOV pass k sees exactly the camera ray render pass k sees with the same seed.  Hit: albedo =
// record.color.xyz as closestIntersect leaves it (before applyRayColor), normal = record.normal.  Miss: albedo = the radiance of a
// reference sample whose first trace misses (intersectSky with record.emittance = 1 and throughput 1, K/rayTracer.cl:94-97),
// normal = 0.  Each channel is folded with (aov * spp + v) / (spp + 1) in float, in pass order (K/rayTracer.cl:109-112).
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "first_hit_pass.hpp"

namespace chunky {

DEV float fold_mean(float m, float fs, float v, float fs1) { return (m * fs + v) / fs1; }
DEV f3 fold_mean(f3 m, float fs, f3 v, float fs1) { return f3{fold_mean(m.x, fs, v.x, fs1), fold_mean(m.y, fs, v.y, fs1), fold_mean(m.z, fs, v.z, fs1)}; }
DEV f3 load3(const float* p) { return mk3(p[0], p[1], p[2]); }
DEV void store3(float* p, f3 v) { p[0] = v.x, p[1] = v.y, p[2] = v.z; }

// albedo and normal, 3 * width * height floats each
struct AovFold {
    struct Out {
        float *albedo, *normal;
    };
    float *__restrict__ pa, *__restrict__ pn;  // the pixel's words, kept from load to store
    f3 ma, mn;
    // Five waves per SIMD (at most 96 VGPRs) without the BVH walk; with it, four (at five it would spill to scratch).
    static constexpr int waves(bool bvh) { return bvh ? 4 : 5; }
    static constexpr bool kParts = false;
    template <class ArgPtr>
    DEV void load(ArgPtr a, int gid, int) {
        pa = a->out.albedo + 3 * (size_t)gid;
        pn = a->out.normal + 3 * (size_t)gid;
        ma = load3(pa), mn = load3(pn);
    }
    DEV void mean(f3 c, f3 n, float fs, float fs1) { ma = fold_mean(ma, fs, c, fs1), mn = fold_mean(mn, fs, n, fs1); }
    DEV void absorb(bool hit, const Hit& h, const RayOD& r, int k, int first_spp) {
        f3 c, n;
        if (hit) {
            c = mk3(h.color.x, h.color.y, h.color.z);
            n = h.normal;
        } else {
            // the sample's radiance: 0 + sky (K/rayTracer.cl:94-97)
            c = mk3(0, 0, 0) + sky_radiance(arg_copy(&first_hit_args<Out>()->S), r.d, mk3(1, 1, 1), 1.0f);
            n = mk3(0, 0, 0);
        }
        const int spp = first_spp + k;
        mean(c, n, (float)spp, (float)(spp + 1));
    }
    DEV void store(int, int) { store3(pa, ma), store3(pn, mn); }
};

// (aov_biome.hip compiles this file with CHUNKY_BIOME_TINT: the same folds over kernels that tint by position, under names of their own)
#if CHUNKY_BIOME_TINT
hipError_t launch_aov_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, const ShardView& T,
                            const PassSeeds& P, float* albedo, float* normal, int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit<AovFold>(variant, S, C, O, T, P, AovFold::Out{albedo, normal}, counter, stream, chosen, &B);
}
#else
hipError_t launch_aov(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                      float* albedo, float* normal, int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit<AovFold>(variant, S, C, O, T, P, AovFold::Out{albedo, normal}, counter, stream, chosen);
}
#endif

// ---------------------------------------------------------------------------------------------
// chunky_render_aov_passes_ex: the same sample, and five more images of its first hit folded beside albedo and
// normal — coverage, the ray parameter, the hit point, the emittance (running means; a miss contributes 0) and the block id (the
// last pass's value; a miss -1).
struct AovExFold {
    typedef AovExImages Out;
    AovFold plain;
    float* __restrict__ pp;
    f3 mp;
    float m_alpha, m_depth, m_emit;
    int block;
    // The ray's origin and direction stay alive across the trace (the hit point is o + d * (distance - kOffset), K/kernel.h:21) and seven
    // more running values per lane: four waves per SIMD (at most 128 VGPRs) with and without the BVH walk (held to the 96 of five, the
    // forms without it spill 36 - 52 bytes per lane to scratch).
    static constexpr int waves(bool) { return 4; }
    static constexpr bool kParts = false;
    template <class ArgPtr>
    DEV void load(ArgPtr a, int gid, int) {
        plain.pa = a->out.albedo + 3 * (size_t)gid;  // (as plain.load, the three addresses ahead of the loads)
        plain.pn = a->out.normal + 3 * (size_t)gid;
        pp = a->out.position + 3 * (size_t)gid;
        plain.ma = load3(plain.pa), plain.mn = load3(plain.pn), mp = load3(pp);
        m_alpha = a->out.alpha[gid], m_depth = a->out.depth[gid], m_emit = a->out.emittance[gid];
        block = a->out.block[gid];
    }
    // (one branch for all seven samples, as AovFold's for its two: two branches in a row compile to other code, EXPERIMENTS.md R1)
    DEV void absorb(bool hit, const Hit& h, const RayOD& r, int k, int first_spp) {
        f3 c, n, p;
        float v_alpha, v_depth, v_emit;
        if (hit) {
            c = mk3(h.color.x, h.color.y, h.color.z);
            n = h.normal;
            p = r.o + r.d * (h.distance - kOffset);  // closest_hit's point
            v_alpha = 1.0f;
            v_depth = h.distance;
            v_emit = h.emittance;
            block = h.material;
        } else {
            c = mk3(0, 0, 0) + sky_radiance(arg_copy(&first_hit_args<Out>()->S), r.d, mk3(1, 1, 1), 1.0f);
            n = mk3(0, 0, 0);
            p = mk3(0, 0, 0);
            v_alpha = 0.0f;
            v_depth = 0.0f;
            v_emit = 0.0f;
            block = -1;
        }
        const int spp = first_spp + k;
        const float fs = (float)spp, fs1 = (float)(spp + 1);
        plain.mean(c, n, fs, fs1);
        mp = fold_mean(mp, fs, p, fs1);
        m_alpha = fold_mean(m_alpha, fs, v_alpha, fs1);
        m_depth = fold_mean(m_depth, fs, v_depth, fs1);
        m_emit = fold_mean(m_emit, fs, v_emit, fs1);
    }
    DEV void store(int gid, int n_pixels) {
        plain.store(gid, n_pixels);
        store3(pp, mp);
        auto w = first_hit_args<Out>();
        w->out.alpha[gid] = m_alpha;
        w->out.depth[gid] = m_depth;
        w->out.emittance[gid] = m_emit;
        w->out.block[gid] = block;
    }
};

#if CHUNKY_BIOME_TINT
hipError_t launch_aov_ex_biome(int variant, const SceneView& S, const BiomeMap& B, const CameraView& C, const RenderOpts& O, const ShardView& T,
                               const PassSeeds& P, const AovExImages& I, int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit<AovExFold>(variant, S, C, O, T, P, I, counter, stream, chosen, &B);
}
#else
hipError_t launch_aov_ex(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                         const AovExImages& I, int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit<AovExFold>(variant, S, C, O, T, P, I, counter, stream, chosen);
}
#endif

}  // namespace chunky
