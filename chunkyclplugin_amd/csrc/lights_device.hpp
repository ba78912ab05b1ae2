// lights_device.hpp — light groups: the sky's, the sun's and the emitters' share of the beauty image as images of their own, from one
// walk of every path (chunky_render_light_passes).  The device code of lights.hip (the four images) and lights_groups.hip (the four
// images and the emitters' share split by block and entity); the kernel's body is lights_walk.inc, included by both.
//
// Specification: the sample of pass k at pixel gid is the reference's whole sample, sample_path
// (path_state.hpp; K/rayTracer.cl:55-107): RNG state seed + gid, Random_nextState, the camera ray of the target's camera, then the
// traces, sun rays (scene sun flag) and bounces up to CHUNKY_OPT_MAX_DEPTH, with the target's draw depth and
// CHUNKY_OPT_BVH_CULL_BEHIND.  Its radiance is a sum of terms that are linear in three scalars, and group g evaluates them with a
// triple of its own:
//
//   image                   sky intensity   sun intensity   emitter scale
//   CHUNKY_LIGHT_SKY        the scene's     0               0
//   CHUNKY_LIGHT_SUN        0               the scene's     0
//   CHUNKY_LIGHT_EMITTERS   0               0               the target's
//   CHUNKY_LIGHT_ALL        the scene's     the scene's     the target's
//
// A group image IS the reference's image under those scalars; the path (geometry, RNG, throughput) never depends on them and is
// walked once.  Per group, in the reference's operation order:
//   at a hit                               radiance += (c * (emittance * scale_g)) * throughput
//   at a miss or an unshadowed sun ray     c = blend * sky_g; if the direction is in the disc c += texel * sun_g;
//                                          radiance += (c * throughput) * e
// with `blend` sky_blend's weighted texel sum before its multiplication by the intensity.  Each image folds with
// (img * spp + v) / (spp + 1) in float, in pass order, spp = first_spp + k.
//
// Terms that are skipped, and why that changes no bit (light_hit_term, light_sky_terms): a group's accumulator starts at +0 and only
// ever has values added to it, so it is never -0, and adding +0 or -0 to it changes nothing.
//   * the hit term of SKY and SUN: colour channels (UNORM8 texels times UNORM8 tints), the emittance (a byte's worth) and the
//     throughput (a product of colours) are finite and non-negative, so (c * (emittance * 0)) * throughput is +0;
//   * the disc's `c += texel * 0` of SKY and EMITTERS: the texel is a finite UNORM8 value, so the product is +0, and c + +0 differs
//     from c only where c is -0 — which the multiplications that follow turn into a +-0 term.
// Everything else that is multiplied by a zero is multiplied literally: `blend * 0` (a NaN direction gives NaN weights, and the
// reference's group image is then NaN) and the products with the throughput and e behind it.
//
// Kernel: first_hit_pass.hpp's claim loop, tile and shard mapping, tree-form choice, instance table, LDS stack and launch arithmetic,
// as occlusion.hip uses them; a lane owns one pixel for every pass of the launch.  Inside a claim each lane is a state machine — MAIN,
// SUN, DONE — around ONE trace site: occlusion_kernel's loop with the path continued to the depth limit.  A lane whose path ended
// starts the camera ray of its next pass while its neighbours are still tracing.  The site runs the octree part of a trace in rounds of
// kLightRound march steps (light_octree_round), so a lane whose trace has ended does not wait for the longest march of the wave.  Across a trace a lane keeps the RNG word, o and d,
// the depth, the throughput, the main hit's normal and distance (the sun record's), and the sample's four group sums; colour, emittance
// and material of every record are dead (a hit rewrites them).  The main hit's point is o itself: the sun ray starts there with no
// offset and the bounce adds d * OFFSET to it.  The running means stay in memory and are read and written where a sample is folded —
// the lane owns its pixel, so nobody else touches those words during the launch — which keeps twelve registers out of the march.
//
// Emitter groups (lights_groups.hip; chunky_render_light_set_emitter_groups): EMITTERS split by what was hit.  Group g's image IS the
// reference's image, with sky and sun intensity 0, of the scene in which every emissive block and entity outside g has emittance 0.
// Per sample its sum receives, in vertex order, the v of light_hit_term at the hits whose id (matte_spec.h matte_id: the last part of
// closestIntersect that won) maps to g, and the `(dark * throughput) * e` of light_sky_terms at every miss and unshadowed sun ray.
// The +0 argument above, restated for emittance 0: a hit of another group adds (c * (0 * scale)) * throughput, which is +-0 for the
// finite scale the host insists on, and the dark term is +-0 unless it is NaN; a sum that starts at +0 is never -0 (x + y is -0 only
// where both are), so skipping the zeros changes no bit.  A NaN dark term is added, as computed, to every group.
// The sums live in memory the lane owns (LightGroupOut::acc, three floats per group and pixel) behind one word of "touched" bits per
// pixel: a hit with non-zero emittance — rare — reads the table, adds to its group's sum and sets the bit; the fold of a sample reads
// the word, folds each group image with the touched sum or +0, and clears it.  No group state is held in registers across the march.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "first_hit_pass.hpp"
#include "matte_spec.h"

namespace chunky {

struct LightOut {
    float* img[4];  // CHUNKY_LIGHT_SKY, _SUN, _EMITTERS, _ALL: 3 * width * height floats each, interleaved like the beauty image
    int max_depth;
    float emitter_scale;
};
typedef FirstHitArgs<LightOut> LightArgs;

struct LightGroupOut {
    float* img[4];
    int max_depth;
    float emitter_scale;
    int n_groups;                  // 1 .. CHUNKY_LIGHT_MAX_EMITTER_GROUPS
    int n_blocks;                  // bytes of of_block
    float* gimg;                   // n_groups images of 3 * width * height floats, one after the other
    float* acc;                    // the sample's group sums: [pixel][group][3]
    int* touched;                  // per pixel: bit g = acc of group g holds this sample's sum (else it counts as +0)
    const unsigned char* of_block; // group of block pointer p at [p >> 1]; a pointer beyond it is group 0
    int world_group, actor_group;  // groups of CHUNKY_MATTE_WORLD_ENTITY and CHUNKY_MATTE_ACTOR_ENTITY
};
typedef FirstHitArgs<LightGroupOut> LightGroupArgs;

enum : int { LT_MAIN = 0, LT_SUN = 1, LT_DONE = 2 };
enum : int { LG_SKY = 0, LG_SUN = 1, LG_EMITTERS = 2, LG_ALL = 3 };

// Waves per SIMD the kernel is held to: four (at most 128 VGPRs).  Compiled for gfx950 (tools/kernel_resources.py): the forms without
// the walk take 121 - 122 VGPRs, the forms with it 125 - 126; no form uses scratch memory at all.  Five waves (96 VGPRs) are out of
// reach: before the trace ran in rounds the kernel took 117 - 121 registers and, held to five waves, spilled 16 - 75 of them to
// scratch — the path state that occlusion_kernel does not carry (throughput, depth, twelve sums) is what that step has no room for.
constexpr int light_waves(bool) { return 4; }

// The sample's radiance, once per group
struct LightSums {
    f3 g[4];
};

// applyRayColor's emitter term (K/kernel.h:33-44).  SKY and SUN skip it: their scale is 0 and the term is +0 (head of the file).
DEV void light_hit_term(LightSums& r, f3 c, float emittance, float scale, f3 throughput) {
    const f3 v = (c * (emittance * scale)) * throughput;
    r.g[LG_EMITTERS] = r.g[LG_EMITTERS] + v;
    r.g[LG_ALL] = r.g[LG_ALL] + v;
}

// intersectSky (K/kernel.h:26-31; rt_device.hpp sky_finish) for the four groups: the disc test and the texel sums are taken once, the
// two intensities applied per group.  ALL is sky_finish itself, operation for operation.
DEV void light_sky_terms(LightSums& r, const SceneView& S, const SkyTexels& q, f3 d, f3 throughput, float e) {
    bool in_disc = false;
    f3 disc = mk3(0, 0, 0);
    const float xu = dot(d, S.su);  // (sky_finish has the argument for the 0.125 gate)
    if ((S.sun_flags & 1) && !(dot(d, S.sw) < 0.5f) && rt_fabs(xu) <= 0.125f) {
        const float width = kSunDiscWidth, width2 = kSunDiscWidth2;
        float a = RT_PI_2_F - rt_acos(xu) + width;
        if (a >= 0 && a < width2) {
            float b = RT_PI_2_F - rt_acos(dot(d, S.sv)) + width;
            if (b >= 0 && b < width2) {
                f4 t = unpack_unorm8(atlas_texel(S, rt_div_const(a, width2), rt_div_const(b, width2), S.sun_tex, S.sun_tex_size));
                disc = mk3(t.x, t.y, t.z);
                in_disc = true;
            }
        }
    }
    const float a = q.a, b = q.b;
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    const f3 blend = mk3(w00 * q.t00.x + w10 * q.t10.x + w01 * q.t01.x + w11 * q.t11.x, w00 * q.t00.y + w10 * q.t10.y + w01 * q.t01.y + w11 * q.t11.y,
                         w00 * q.t00.z + w10 * q.t10.z + w01 * q.t01.z + w11 * q.t11.z);
    const f3 lit = blend * S.sky_intensity;  // c of SKY and, outside the disc, of ALL
    const f3 dark = blend * 0.0f;            // c of EMITTERS and, outside the disc, of SUN: evaluated, not assumed to be 0
    f3 c_all = lit, c_sun = dark;
    if (in_disc) {
        const f3 add = mk3(disc.x * S.sun_intensity, disc.y * S.sun_intensity, disc.z * S.sun_intensity);
        c_all = c_all + add;
        c_sun = c_sun + add;
    }
    r.g[LG_SKY] = r.g[LG_SKY] + (lit * throughput) * e;
    r.g[LG_SUN] = r.g[LG_SUN] + (c_sun * throughput) * e;
    r.g[LG_EMITTERS] = r.g[LG_EMITTERS] + (dark * throughput) * e;
    r.g[LG_ALL] = r.g[LG_ALL] + (c_all * throughput) * e;
}

DEV float light_fold(float m, float fs, float v, float fs1) { return (m * fs + v) / fs1; }

// March steps a lane takes per round of the loop (light_octree_round).  Measured on the headline view at 64 passes (DESIGN.md section
// 17): 8 / 16 / 32 steps 63.5 / 67.3 / 77.2 ms, the whole trace in one go 87.6 ms; 16 is what the test suite ran.
#ifndef CHUNKY_LIGHT_ROUND
#define CHUNKY_LIGHT_ROUND 16
#endif
constexpr int kLightRound = CHUNKY_LIGHT_ROUND;
enum : int { LR_MISS = 0, LR_HIT = 1, LR_GOES_ON = 2 };

// octree_hit (path_state.hpp; K/octree.h:41-109) in rounds of at most kLightRound march steps: the same operations in the same order,
// with the distance marched and the step count kept by the caller between rounds (step == 0: the trace begins, and the entry into the
// world is taken).  From the first bounce on the rays of a wave have nothing in common, and a trace run to its end costs the wave its
// longest march; cut into rounds, a lane whose trace has ended shades and starts its next ray at the next round while the long march
// goes on.  The record's normal is the one field a rejected candidate may leave behind for a later one (K/block.h:59-60): the caller
// keeps it between rounds too.
template <int TREE>
DEV int light_octree_round(const SceneView& S, f3 o, f3 d, int draw_depth, Hit& h, float& dist_march, int& step) {
    const int depth = S.octree_depth;
    f3 inv = rcp3(d);
    f3 off = d * kOffset;
    if (step == 0) {
        dist_march = 0;
        int lx = (int)rt_floor(o.x) >> depth, ly = (int)rt_floor(o.y) >> depth, lz = (int)rt_floor(o.z) >> depth;
        if ((lx != 0) | (ly != 0) | (lz != 0)) {
            float size = (float)(1 << depth);
            float dist = box_quick(0, size, 0, size, 0, size, o, inv);
            if (dist != dist || dist < 0) return LR_MISS;
            dist_march += dist + kOffset;
        }
    }
    const int end = draw_depth - step > kLightRound ? step + kLightRound : draw_depth;
    int i = step, answer = LR_MISS;
    for (;;) {
        // march to the next leaf that can be hit: a loop of its own, so that the lanes that have found theirs wait at its end and the
        // block tests of the wave run together, once, instead of one lane's test stalling every march step of the others
        bool candidate = false;
        f3 pos = o, po = o;
        int bx = 0, by = 0, bz = 0, level = 0, data = 0;
        for (;;) {
            if (i >= end) {
                answer = end < draw_depth ? LR_GOES_ON : LR_MISS;
                break;
            }
            if (dist_march > h.distance) break;
            pos = o + d * dist_march;
            po = pos + off;
            bx = (int)rt_floor(po.x), by = (int)rt_floor(po.y), bz = (int)rt_floor(po.z);
            if (((bx | by | bz) >> depth) != 0) break;  // any coordinate outside [0, 2^depth)
            int kind;
            leaf_lookup<TREE>(S, bx, by, bz, data, level, kind);
            if (kind < 2) {  // not air (ray->material is always 0, K/octree.h:92) and able to intersect
                candidate = true;
                break;
            }
            const int lx = bx >> level, ly = by >> level, lz = bz >> level;
            dist_march += box_exit((float)(lx << level), (float)((lx + 1) << level), (float)(ly << level), (float)((ly + 1) << level),
                                   (float)(lz << level), (float)((lz + 1) << level), po, inv) + kOffset;
            i++;
        }
        if (!candidate) break;
        const float dist = block_hit(S, data, bx, by, bz, pos, d, inv, h);
        if (dist == dist) {
            h.distance = dist_march + dist;
            h.material = data;
            answer = LR_HIT;
            break;
        }
        const int lx = bx >> level, ly = by >> level, lz = bz >> level;
        dist_march += box_exit((float)(lx << level), (float)((lx + 1) << level), (float)(ly << level), (float)((ly + 1) << level),
                               (float)(lz << level), (float)((lz + 1) << level), po, inv) + kOffset;
        i++;
    }
    step = i;
    return answer;
}

// closestIntersect (first_hit_pass.hpp first_hit_part) with the octree part in rounds: the entity BVHs are walked in the round the
// octree part ends in, against the record that part leaves.  IDS (the emitter groups): a hit's record leaves with its id in h.material
// (matte_spec.h matte_id) — the block pointer the octree part wrote, or the entity id of the BVH that won last; nothing else reads a
// record's material after a trace.
template <int TREE, bool BVH, bool IDS>
DEV int light_trace_round(const SceneView& S, f3 o, f3 d, int draw_depth, Hit& h, float& dist_march, int& step, LdsStack& stack) {
    int answer = light_octree_round<TREE>(S, o, d, draw_depth, h, dist_march, step);
    if (BVH && answer != LR_GOES_ON) {
        bool hit = answer == LR_HIT;
        if (IDS) {
            if (!S.world_bvh_empty && bvh_hit(S, S.world_bvh, o, d, h, stack)) hit = true, h.material = MATTE_WORLD_ENTITY;
            if (!S.actor_bvh_empty && bvh_hit(S, S.actor_bvh, o, d, h, stack)) hit = true, h.material = MATTE_ACTOR_ENTITY;
        } else {
            if (!S.world_bvh_empty) hit |= bvh_hit(S, S.world_bvh, o, d, h, stack);
            if (!S.actor_bvh_empty) hit |= bvh_hit(S, S.actor_bvh, o, d, h, stack);
        }
        answer = hit ? LR_HIT : LR_MISS;
    }
    return answer;
}

// The emitter groups' share of the kernel body (lights_walk.inc): three steps that are nothing where GROUPS is false.
// the group of a hit's id (lights_host.cpp light_group_of)
DEV int light_group_of(const LightGroupOut& out, int id) {
    if (id == MATTE_WORLD_ENTITY) return out.world_group;
    if (id == MATTE_ACTOR_ENTITY) return out.actor_group;
    const int k = id >> 1;
    return id >= 0 && k < out.n_blocks ? (int)out.of_block[k] : 0;
}

// sum of group g of pixel gid += v (the pixel is the lane's own for the whole launch)
DEV void light_group_add(const LightGroupOut& out, int gid, int g, f3 v) {
    int* t = out.touched + gid;
    float* p = out.acc + ((size_t)gid * (size_t)out.n_groups + (size_t)g) * 3;
    const int bits = *t;
    f3 s = mk3(0, 0, 0);
    if ((bits >> g) & 1) s = mk3(p[0], p[1], p[2]);
    s = s + v;
    p[0] = s.x, p[1] = s.y, p[2] = s.z;
    *t = bits | (1 << g);
}

// at a main hit, behind light_hit_term: the same v to the group of the hit's id (h.material: light_trace_round)
template <bool GROUPS>
DEV void light_groups_hit(int gid, const Hit& h, f3 c, f3 throughput) {
    if constexpr (GROUPS) {
        if (h.emittance != 0) {  // (else the term is +-0: head of the file)
            auto u = first_hit_args<LightGroupOut>();
            const LightGroupOut out = arg_copy(&u->out);
            light_group_add(out, gid, light_group_of(out, h.material), (c * (h.emittance * out.emitter_scale)) * throughput);
        }
    }
}

// at a miss or an unshadowed sun ray, behind light_sky_terms: the term EMITTERS received, to every group — unless it is +-0 in every
// channel, which it is whenever the direction did not make the weights NaN
template <bool GROUPS>
DEV void light_groups_unlit(int gid, const SkyTexels& q, f3 throughput, float e) {
    if constexpr (GROUPS) {
        const float a = q.a, b = q.b;
        const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
        const f3 blend = mk3(w00 * q.t00.x + w10 * q.t10.x + w01 * q.t01.x + w11 * q.t11.x, w00 * q.t00.y + w10 * q.t10.y + w01 * q.t01.y + w11 * q.t11.y,
                             w00 * q.t00.z + w10 * q.t10.z + w01 * q.t01.z + w11 * q.t11.z);
        const f3 unlit = ((blend * 0.0f) * throughput) * e;
        if (unlit.x != unlit.x || unlit.y != unlit.y || unlit.z != unlit.z) {
            auto u = first_hit_args<LightGroupOut>();
            const LightGroupOut out = arg_copy(&u->out);
            for (int g = 0; g < out.n_groups; g++) light_group_add(out, gid, g, unlit);
        }
    }
}

// at the fold of a sample, behind the four images: every group image folds every pass, with +0 where the sample never reached the group
template <bool GROUPS>
DEV void light_groups_fold(int gid, int n_pixels, float fs, float fs1) {
    if constexpr (GROUPS) {
        auto u = first_hit_args<LightGroupOut>();
        const LightGroupOut out = arg_copy(&u->out);
        const int bits = out.touched[gid];
        const float* acc = out.acc + (size_t)gid * (size_t)out.n_groups * 3;
        float* p = out.gimg + 3 * (size_t)gid;
        for (int g = 0; g < out.n_groups; g++, acc += 3, p += 3 * (size_t)n_pixels) {
            f3 s = mk3(0, 0, 0);
            if ((bits >> g) & 1) s = mk3(acc[0], acc[1], acc[2]);
            const float m0 = p[0], m1 = p[1], m2 = p[2];
            p[0] = light_fold(m0, fs, s.x, fs1);
            p[1] = light_fold(m1, fs, s.y, fs1);
            p[2] = light_fold(m2, fs, s.z, fs1);
        }
        if (bits) out.touched[gid] = 0;
    }
}

}  // namespace chunky
