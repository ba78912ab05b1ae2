// occlusion.hip — the sun-shadow and ambient-occlusion images of the beauty sample's own rays (chunky_render_occlusion_passes).
//
// Specification: the sample of pass k at pixel gid is the reference's pass-k sample cut off after its first
// bounce trace, in the order sample_path (path_state.hpp) follows: RNG state seed + gid, Random_nextState, the camera ray of the
// target's camera (K/rayTracer.cl:55-91), then up to three closestIntersect calls (K/kernel.h:14-24) with the target's draw depth and
// CHUNKY_OPT_BVH_CULL_BEHIND.  rec[i] is record i of chunky_render_trace_records for that (seed, gid); `sun` is bit 0 of the PackedSun
// flags of the scene (not CHUNKY_OPT_SUN_SAMPLING):
//
//   image             first trace misses   first trace hits
//   CHUNKY_AOV_SUN    1.0f                 sun ? (rec[1].hit ? 0 : 1) : 0
//   CHUNKY_AOV_AO     1.0f                 with b = rec[sun ? 2 : 1]: (b.hit && b.distance < ao_distance) ? 0 : 1
//
// A miss folds 1: a sky pixel is neither shadowed nor occluded, so either image multiplies straight over the beauty image and
// antialiased silhouettes come out right; the mean over the samples that hit is (image - (1 - ALPHA)) / ALPHA with the coverage of
// chunky_render_aov_passes_ex.  Each image is folded with (img * spp + v) / (spp + 1) in float, in pass order, spp = first_spp + k.
//
// The sun trace is the reference's, quirks included (K/rayTracer.cl:101-106): direction normalize(u * v + w) (K/sky.h:86), origin
// rec[0].point with no offset, and the record it works on is a copy of the first hit's, distance included — only occluders nearer
// than the first hit count.  SUN is "the shadow the beauty image has", not a geometric visibility.  With the sun flag off there is no
// sun ray and no RNG draw for it: SUN folds 0 on hits and the bounce takes the two draws right after the camera's.
// The bounce trace is nextPath's (K/kernel.h:46-98): direction diffuse_bounce(rec[0].normal), origin rec[0].point + d * OFFSET, the
// record's distance reset to +inf.  `distance < ao_distance` is one strict float compare: a negative distance (which occurs) counts
// as occluded, a NaN distance as clear.  Where the scene has no entity BVH the kernel starts the record at a bound beyond the radius
// instead of +inf (bounce_reach below), which changes no bit of either image.
//
// Kernel: first_hit_pass.hpp's claim loop, tile and shard mapping, tree-form choice, instance table, LDS stack and launch arithmetic;
// a lane owns one pixel for every pass of the launch.  Inside a claim each lane is a small state machine — PRIMARY, SUN, BOUNCE, DONE —
// around ONE trace site: a lane whose first trace missed starts the camera ray of its next pass while its neighbours trace their sun
// rays, and the wave leaves the loop when every lane has finished its passes.  (Three trace sites in a row would cost the wave its
// slowest lane three times per pass, with the lanes that missed — 40 % of the golden outdoor view — idle for two of them.)  Across a
// trace a lane keeps the two running means, the RNG word, o and d, and the first hit's normal and point; colour, emittance and
// material of every record are dead.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "first_hit_pass.hpp"

namespace chunky {

struct OcclusionOut {
    float *ao, *sun;  // width * height floats each
    float ao_distance;
};
typedef FirstHitArgs<OcclusionOut> OcclusionArgs;

enum : int { OC_PRIMARY = 0, OC_SUN = 1, OC_BOUNCE = 2, OC_DONE = 3 };

// Waves per SIMD the kernel is held to: five (at most 96 VGPRs) with and without the BVH walk.  Compiled for gfx950
// (tools/kernel_resources.py): every form without the walk takes 93 VGPRs, the forms with it 94 - 95 (left at four waves they take 94 -
// 98: two registers from the step); no form uses scratch memory at all.
constexpr int occlusion_waves(bool) { return 5; }

DEV float occlusion_fold(float m, float fs, float v, float fs1) { return (m * fs + v) / fs1; }

// The distance the bounce trace's record starts with where the scene has no entity BVH: a bound S > ao_distance in place of +inf, with
// the same answer to `hit && distance < ao_distance`, bit for bit (DESIGN.md section 16 has the argument).  octree_hit reads the
// record's distance in one place, `dist_march > h.distance`, so the two marches are the same march until dist_march > S; dist_march never
// decreases; and a block test returns no less than -(1 + 2^-23) / m - OFFSET, m the largest |component| of d
// (the test's origin lies inside or in front of the unit cube it tests on every axis, never behind it), so whatever the unbounded march
// finds from there on ends beyond ao_distance.  S = ao_distance + 1.01 / m + 0.01; +inf where that sum does not clear ao_distance by
// the margin in float (a radius above 4096, m = 0, a NaN).  With an entity BVH the bound is not taken: the walk prunes boxes against
// the record's distance, and a pruning decision that differs by an ulp could change which triangles are tested.
DEV float bounce_reach(f3 d, float ao_distance) {
    const float m = rt_fmax(rt_fabs(d.x), rt_fmax(rt_fabs(d.y), rt_fabs(d.z)));
    const float s = ao_distance + (1.01f / m + 0.01f);
    return (ao_distance <= 4096.0f && s > ao_distance) ? s : rt_inf();
}

template <int TREE, bool BVH, bool PROJ>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(occlusion_waves(BVH)))) occlusion_kernel(OcclusionArgs) {
    static_assert(sizeof(OcclusionArgs) <= 4096, "launch arguments must fit the 4 KB kernel-argument segment");
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        auto a = first_hit_args<OcclusionOut>();
        const int width = a->C.width, height = a->C.height, n_pixels = width * height;
        // every lane of the wave is here (both exits below are wave-uniform): lane 0 claims, the others take its value
        int unit = 0;
        if (lane == 0) unit = atomicAdd(a->counter, 1);
        unit = __builtin_amdgcn_readfirstlane(unit);
        if (unit >= a->n_units) break;
        const int gid = pool_slot_gid(arg_copy(&a->T), width, height, unit * kFirstHitUnit + lane);
        const bool mine = gid < n_pixels;  // (not a padding slot)
        const int n_passes = a->P.n, first_spp = a->P.first_spp;
        float m_ao = 0, m_sun = 0;
        int px = 0, py = 0;
        if (mine) {
            m_ao = a->out.ao[gid], m_sun = a->out.sun[gid];
            px = gid % width, py = gid / width;
        }
        int state = mine ? OC_PRIMARY : OC_DONE;  // (a launch carries at least one pass)
        bool start = mine;                        // the lane begins the sample of its pass k
        int k = 0;
        unsigned rng = 0;
        f3 o = mk3(0, 0, 0), d = mk3(0, 0, 0), n0 = mk3(0, 0, 0), p0 = mk3(0, 0, 0);
        float reach = 0, v_sun = 0;  // reach: the distance the next trace's record starts with
        for (;;) {
            if (start) {  // K/rayTracer.cl:54-91
                auto b = first_hit_args<OcclusionOut>();
                const unsigned seed = (unsigned)b->P.seed[k];
                const CameraView C = arg_copy(&b->C);
                const CanvasPixel cp = canvas_pixel(C, gid, px, py);
                rng = seed + (unsigned)cp.G;
                rt_pcg_next(&rng);
                const RayOD r = primary_ray<PROJ>(C, seed, gid, cp, rng, false);
                o = r.o, d = r.d;
                reach = rt_inf();
            }
            if (__ballot(state != OC_DONE) == 0) break;  // every lane has folded its last pass
            // the one trace site: whatever kind of ray each lane has ready
            bool hit = false;
            Hit h;
            h.distance = reach;
            h.material = 0;
            h.normal = mk3(0, 0, 0);
            h.color = f4{0, 0, 0, 0};
            h.emittance = 0;
            h.spec = 0;
            if (state != OC_DONE) {
                auto t = first_hit_args<OcclusionOut>();
                hit = first_hit_part<TREE, BVH, false>(arg_copy(&t->S), o, d, t->draw_depth, h, stack);
            }
            // what the answer means to the lane: each continuation appears once
            bool bounce = false, fold = false;
            float v_ao = 1.0f;
            if (state == OC_PRIMARY) {
                if (!hit) {
                    v_sun = 1.0f;
                    fold = true;
                } else {
                    n0 = h.normal;
                    p0 = o + d * (h.distance - kOffset);  // closest_hit's point
                    auto s = first_hit_args<OcclusionOut>();
                    if (s->S.sun_flags & 1) {
                        // the shadow record is a copy of the main record, distance included, traced from the point with no offset
                        d = sun_sample(arg_copy(&s->S), rng);
                        o = p0;
                        reach = h.distance;
                        state = OC_SUN;
                    } else {
                        v_sun = 0.0f;
                        bounce = true;
                    }
                }
            } else if (state == OC_SUN) {
                v_sun = hit ? 0.0f : 1.0f;
                bounce = true;
            } else if (state == OC_BOUNCE) {
                auto s = first_hit_args<OcclusionOut>();
                v_ao = (hit && h.distance < s->out.ao_distance) ? 0.0f : 1.0f;
                fold = true;
            }
            if (bounce) {  // nextPath
                d = diffuse_bounce(n0, rng);
                o = p0 + d * kOffset;
                reach = BVH ? rt_inf() : bounce_reach(d, first_hit_args<OcclusionOut>()->out.ao_distance);
                state = OC_BOUNCE;
            }
            start = false;
            if (fold) {
                const int spp = first_spp + k;
                const float fs = (float)spp, fs1 = (float)(spp + 1);
                m_ao = occlusion_fold(m_ao, fs, v_ao, fs1);
                m_sun = occlusion_fold(m_sun, fs, v_sun, fs1);
                k += 1;
                start = k < n_passes;
                state = start ? OC_PRIMARY : OC_DONE;
            }
        }
        if (mine) {
            auto w = first_hit_args<OcclusionOut>();
            w->out.ao[gid] = m_ao;
            w->out.sun[gid] = m_sun;
        }
    }
}

// (first_hit_pass.hpp launch_first_hit_args: the first-hit passes' tree forms and launch arithmetic)
hipError_t launch_occlusion(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T, const PassSeeds& P,
                            float* ao, float* sun, float ao_distance, int* counter, hipStream_t stream, AovChoice* chosen) {
    return launch_first_hit_args<OcclusionOut>(
        [](auto tree, auto bvh, auto proj) -> void (*)(OcclusionArgs) { return occlusion_kernel<decltype(tree)::value, decltype(bvh)::value, decltype(proj)::value>; },
        variant, S, C, O, T, P, OcclusionOut{ao, sun, ao_distance}, counter, stream, chosen);
}

}  // namespace chunky
