// render_pool.hip — the hot path: render_pool (a persistent grid whose waves each run a pool of 64 + K path state machines
// phase by phase — MARCH / BLOCK / SHADE, plus the entity-BVH walk — voted over the pool, samples claimed per XCD) and
// fold_kernel (the running mean of K/rayTracer.cl:109-112 over the staged samples, in pass order); the read-back exchange
// of a multi-GPU group; launch_render, which runs what launch_plan.cpp planned.  DESIGN.md section 5 describes the kernel.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include <cstdlib>

// This unit's kernels read the atlas, the sky and the record arrays by 32-bit offsets off scalar bases (rt_device.hpp load_at; launch_render
// starts them only for scenes whose SceneView::addr32 allows all three: launch_plan.cpp).  render_pool_bvh.hip, which includes this file, does not: the
// entity-BVH instantiations keep the 64-bit addresses.  (-DCHUNKY_ADDR32_FORMS=n: experiments, the arrays one at a time.)
#if !defined(CHUNKY_POOL_BVH_TU) && !defined(CHUNKY_ADDR32_FORMS)
#define CHUNKY_ADDR32_FORMS 7
#endif
// ... and they form a tree node's in-node index ahead of the wait for the entry above it (path_state.hpp leaf_lookup; EXPERIMENTS 7.4)
#if !defined(CHUNKY_POOL_BVH_TU) && !defined(CHUNKY_MARCH_HOIST)
#define CHUNKY_MARCH_HOIST 1
#endif

#include "path_state.hpp"
#include "pool_walk.hpp"
#if CHUNKY_FOG
#include "fog_spec.h"
#endif
#if CHUNKY_GLASS
#include "glass_spec.h"
#endif

#ifndef CHUNKY_STAGING_STORE
#define CHUNKY_STAGING_STORE 0  // how finished samples reach the staging array: 0 = non-temporal (measured best), 1-3: see the deposit site
#endif
#ifndef CHUNKY_BLOCK_CONTINUES
#define CHUNKY_BLOCK_CONTINUES 1  // the block test starts the shadow ray or bounce where it hits (block_continues below); 0 (tuning builds): every trace that ends goes to SHADE
#endif
#ifndef CHUNKY_MARCH_CAP
#define CHUNKY_MARCH_CAP 1  // an upward ray's march ends above the highest leaf that can be hit (path_state.hpp march_step); 0 (tuning builds): at the world's edge only
#endif

namespace chunky {

// SHADE of the EXTENDED integrator: oracle/port.c trace_sample_ext, operation for operation, as a
// state machine over the kind of trace that just ended (L.tkind: 0 the path's ray, 1 the sun shadow ray, 2 the emitter
// shadow ray).  Returns ST_SETUP (a ray is ready to be traced) or ST_NEXT (the path is finished).
template <int TREE, bool BVH>
DEV int shade_phase_ext(const SceneView& S, const RenderOpts& O, LaneState& L) {
    const bool hit = BVH ? L.trace_hit : L.oct_hit;
    const int kind = L.tkind;
#if CHUNKY_GLASS
    // Translucent blocks (tests/glass_port.c trace_sample_glass operation for operation).  In these units a shadow
    // ray is traced as a main ray is — L.shadow stays false: the nearest hit, written to the record — so that it can be crossed in order;
    // what the vertex still needs of its record, the normal, waits in L.n_vertex, and the ray's clip distance in L.clip.
    const f3 n = kind == 0 ? L.h.normal : L.n_vertex;
    constexpr bool kShadowFlag = false;
    const GlassParams G = glass_params();
    if (hit && glass_translucent(L.h.color.w, G.opaque_alpha, (int)L.crossings, G.max_crossings)) {
        const float a = L.h.color.w;
        // a main ray draws: below a the hit is a surface vertex as ever; a shadow ray draws nothing and always crosses
        const bool crosses = kind == 0 ? !(rt_pcg_float(&L.rng) < a) : true;
        if (crosses) {
            if (kind == 0) {
                L.throughput = L.throughput * mk3(glass_tc(a, L.h.color.x), glass_tc(a, L.h.color.y), glass_tc(a, L.h.color.z));
            } else {
                L.pend = L.pend * mk3(glass_fs(a, L.h.color.x), glass_fs(a, L.h.color.y), glass_fs(a, L.h.color.z));
                L.clip = L.clip - L.h.distance;
            }
            // the ray is inside the hit's run from here on, if the octree part of the trace won (an entity triangle leaves the run alone)
            if (L.oct_hit && (!BVH || L.h.distance == L.bvh_dist)) L.rm = L.cand_data;
            glass_restart(L.o.x, L.o.y, L.o.z, L.d.x, L.d.y, L.d.z, L.h.distance, L.h.normal.x, L.h.normal.y, L.h.normal.z, &L.o.x, &L.o.y, &L.o.z);
            L.crossings += 1;
            L.h.distance = kind == 0 ? rt_inf() : L.clip;
            return ST_SETUP;  // the same direction, the same kind of trace, the same depth
        }
    }
    if (kind != 0) L.o = L.o_vertex;  // a shadow ray has ended: back at the vertex (a crossing moved the origin)
#else
    const f3 n = L.h.normal;
    constexpr bool kShadowFlag = true;
#endif
    int next = 0;  // 1 sun sampling, 2 emitter sampling, 3 diffuse bounce, 4 specular bounce (ray already set)
#if CHUNKY_FOG
    // Ground fog (tests/fog_port.c trace_sample_fog operation for operation): free flight at the end of every main-ray
    // trace, hit or miss, ahead of everything else; a medium vertex is a vertex of its own kind — L.medium says so across its shadow trace.
    const FogParams F = fog_params();
    bool medium = kind == 1 && L.medium;
    if (kind == 0) {
        float ta, tb, len;
        if (fog_interval(L.o.y, L.d.x, L.d.y, L.d.z, hit ? L.h.distance : rt_inf(), F.y_min, F.y_max, &ta, &tb, &len)) {
            const float s = fog_free_flight(rt_pcg_float(&L.rng), F.sigma);
            if (s < (tb - ta) * len) {
                medium = true;
                L.o = L.o + L.d * (ta + s / len);
                L.throughput = L.throughput * mk3(F.color[0], F.color[1], F.color[2]);
                L.after_nee = false;
                L.h.distance = rt_inf();  // (the shadow record keeps the record's distance: nothing clips the sun ray of a vertex in mid-air)
            }
        }
    }
    L.medium = false;
    if (medium) {
        if (kind == 0) {
            const bool sun_on = O.sun_sampling < 0 ? (S.sun_flags & 1) != 0 : O.sun_sampling != 0;
            if (sun_on) {
                L.d = sun_sample(S, L.rng);
                L.h.emittance = FOG_PHASE_WEIGHT * fog_segment_transmittance(F.sigma, F.y_min, F.y_max, L.o.y, L.d.x, L.d.y, L.d.z, rt_inf());
                L.medium = true;
                L.tkind = 1;
                L.shadow = true;
                return ST_SETUP;
            }
        } else if (!hit) {
            L.radiance = L.radiance + sky_radiance(S, L.d, L.throughput, L.h.emittance);
        }
        const float x1 = rt_pcg_float(&L.rng), x2 = rt_pcg_float(&L.rng);
        fog_sphere(x1, x2, &L.d.x, &L.d.y, &L.d.z);  // (no origin offset: there is no surface to leave)
    } else
#endif
    if (kind == 0) {
        if (!hit) {
            L.radiance = L.radiance + sky_radiance(S, L.d, L.throughput, 1.0f);
            return ST_NEXT;
        }
        const f3 d_in = L.d;
#if CHUNKY_GLASS
        L.n_vertex = n;      // a surface vertex: its shadow rays and its bounce start inside the run it was reached through
        L.rm_vertex = L.rm;
#endif
        L.o = L.o + L.d * (L.h.distance - kOffset);  // rec.point
#if CHUNKY_GLASS
        L.o_vertex = L.o;
#endif
        const f3 base = L.throughput;
        const f3 c = mk3(L.h.color.x, L.h.color.y, L.h.color.z);
        const f3 thr_d = base * c;
        // port.c hit_is_listed: after a vertex that sampled the emitter list a hit loses its emittance only if the list holds it — the
        // octree part of the trace won (with entity BVHs: no triangle came nearer, so the record's distance is still the one
        // rbvh_begin copied to bvh_dist), the block is a full cube, its material has flag 2 clear and a non-zero emittance byte.
        // (L.cand_data is the block the trace ended at; the palette reads sit behind a non-zero emittance: a rare path.)
        bool listed = false;
        if (L.after_nee && L.h.emittance != 0 && (!BVH || (L.oct_hit && L.h.distance == L.bvh_dist))) {
            const int block = L.cand_data;
            if (S.blocks[block] == 1) {
                const int* m = S.materials + S.blocks[block + 1];
                listed = !(m[0] & 2) && (m[4] & 0xFF) != 0;
            }
        }
        if (O.emitters && !listed) L.radiance = L.radiance + (c * (L.h.emittance * O.emitter_scale)) * thr_d;
        L.after_nee = false;
        bool specular = false;
        float metal = 0, rough = 0;
        if (O.bsdf) {
            const float spec = rt_unorm8((unsigned)L.h.spec & 0xFFu);
            metal = rt_unorm8(((unsigned)L.h.spec >> 8) & 0xFFu);
            rough = rt_unorm8(((unsigned)L.h.spec >> 16) & 0xFFu);
            const float ps = rt_fmax(spec, metal);
            if (ps > 0) specular = rt_pcg_float(&L.rng) < ps;
        }
        if (specular) {
            L.throughput = mk3(base.x * (c.x * metal + (1 - metal)), base.y * (c.y * metal + (1 - metal)), base.z * (c.z * metal + (1 - metal)));
            f3 refl = d_in - n * (2 * dot(d_in, n));
            if (rough > 0) {
                const float x1 = rt_pcg_float(&L.rng), x2 = rt_pcg_float(&L.rng);
                const f3 dd = cosine_direction(n, x1, x2);
                refl = normalize(dd * rough + refl * (1 - rough));
                const float rn = dot(refl, n);
                if (rn < 0) refl = refl - n * (2 * rn);
            }
            L.d = refl;
            L.o = L.o + refl * kOffset;
            next = 4;
        } else {
            L.throughput = thr_d;
            next = 1;
        }
    } else if (kind == 1) {
#if CHUNKY_GLASS
        // (the record's emittance is a crossed hit's by now: |dot(d, n)| again, from the operands it was made from)
        if (!hit) L.radiance = L.radiance + sky_radiance(S, L.d, L.throughput, rt_fabs(dot(L.d, n))) * L.pend;
#else
        if (!hit) L.radiance = L.radiance + sky_radiance(S, L.d, L.throughput, L.h.emittance);
#endif
        next = 2;
    } else {
        if (!hit) L.radiance = L.radiance + L.pend;  // (with translucent blocks: through the filter, crossing by crossing)
        next = 3;
    }
    if (next == 1) {  // Sun_sampleDirection + shadow ray (K/sky.h:68-93, K/rayTracer.cl:101-106): the record keeps its distance
        const bool sun_on = O.sun_sampling < 0 ? (S.sun_flags & 1) != 0 : O.sun_sampling != 0;
        if (sun_on) {
            L.d = sun_sample(S, L.rng);
            L.h.emittance = rt_fabs(dot(L.d, n));
#if CHUNKY_FOG
            // (to infinity, whatever distance the shadow record keeps)
            L.h.emittance = L.h.emittance * fog_segment_transmittance(F.sigma, F.y_min, F.y_max, L.o.y, L.d.x, L.d.y, L.d.z, rt_inf());
#endif
            L.tkind = 1;
            L.shadow = kShadowFlag;
#if CHUNKY_GLASS
            L.clip = L.h.distance;  // the record's distance, kept (K/rayTracer.cl:101-106)
            L.pend = mk3(1, 1, 1);  // the sun ray's filter
            L.crossings = 0;
            L.rm = L.rm_vertex;
#endif
            return ST_SETUP;
        }
        next = 2;
    }
    if (next == 2) {
        next = 3;
        // not at the last vertex: the bounce ray that would find the same light implicitly is never traced there
        if (O.nee && O.emitters && S.n_emitters > 0 && (int)L.depth + 1 < O.max_depth) {
            const float xk = rt_pcg_float(&L.rng), xf = rt_pcg_float(&L.rng), xu = rt_pcg_float(&L.rng), xv = rt_pcg_float(&L.rng);
            int k = (int)(xk * (float)S.n_emitters);
            if (k > S.n_emitters - 1) k = S.n_emitters - 1;
            int face = (int)(xf * 6.0f);
            if (face > 5) face = 5;
            const int4 em = S.emitters[k];
            const int level = (em.w >> 25) & 15, block = em.w & 0x1FFFFFF;
            const float size = (float)(1 << level);
            const float a = xu * size, b = xv * size;
            const float fa = a - rt_floor(a), fb = b - rt_floor(b);
            const float ex = (float)em.x, ey = (float)em.y, ez = (float)em.z;
            f3 pe, nf;
            float tu, tv;
            switch (face) {
                case 0: pe = mk3(ex, ey + a, ez + b); nf = mk3(-1, 0, 0); tu = 1 - fb; tv = fa; break;
                case 1: pe = mk3(ex + size, ey + a, ez + b); nf = mk3(1, 0, 0); tu = fb; tv = fa; break;
                case 2: pe = mk3(ex + a, ey, ez + b); nf = mk3(0, -1, 0); tu = fa; tv = 1 - fb; break;
                case 3: pe = mk3(ex + a, ey + size, ez + b); nf = mk3(0, 1, 0); tu = fa; tv = fb; break;
                case 4: pe = mk3(ex + a, ey + b, ez); nf = mk3(0, 0, -1); tu = fa; tv = fb; break;
                default: pe = mk3(ex + a, ey + b, ez + size); nf = mk3(0, 0, 1); tu = 1 - fa; tv = fb; break;
            }
            const f3 l = pe - L.o;
            const float d2 = dot(l, l);
            const float dist = rt_sqrt(d2);
            const f3 dir = l * rcp_exact(dist);
            const float cs = dot(dir, n), cl = -dot(dir, nf);
            L.after_nee = true;
            if (cs > 0 && cl > 0 && dist > 0.002f) {
                Hit er = L.h;
                if (material_sample(S, S.blocks[block + 1], tu, tv, er) && er.emittance > 0) {
                    const float w = (cs * cl) / (RT_PI_F * d2) * (6.0f * (float)S.n_emitters * (size * size));
                    const f3 ce = mk3(er.color.x, er.color.y, er.color.z);
                    const f3 le = ce * (ce * (er.emittance * O.emitter_scale));
                    L.pend = L.throughput * (le * w);
#if CHUNKY_FOG
                    L.pend = L.pend * fog_segment_transmittance(F.sigma, F.y_min, F.y_max, L.o.y, dir.x, dir.y, dir.z, dist);
#endif
                    L.d = dir;
                    L.h.distance = dist - 0.001f;  // anything nearer than the emitter's face hides it
                    L.tkind = 2;
                    L.shadow = kShadowFlag;
#if CHUNKY_GLASS
                    L.clip = L.h.distance;
                    L.crossings = 0;
                    L.rm = L.rm_vertex;
#endif
                    return ST_SETUP;
                }
            }
        }
    }
    if (next == 3) {
        const float x1 = rt_pcg_float(&L.rng), x2 = rt_pcg_float(&L.rng);
        L.d = cosine_direction(n, x1, x2);
        L.o = L.o + L.d * kOffset;
    }
    L.depth += 1;
    L.h.distance = rt_inf();
    L.tkind = 0;
    L.shadow = false;
#if CHUNKY_GLASS
    L.crossings = 0;
    L.rm = L.rm_vertex;  // (whatever a shadow ray did to it is discarded)
#endif
    return (int)L.depth < O.max_depth ? ST_SETUP : ST_NEXT;
}
// ---------------------------------------------------------------------------------------------
// render_pool — the wave-scheduled path state machine with a POOL of paths per wave.
//
// render_waves binds a path to a lane for its whole life, so the phase a wave executes only ever serves the lanes
// that happen to wait in it (39 / 27 / 35 of 64 for MARCH / BLOCK / SHADE on the benchmark view).  Here a wave owns
// 64 + K paths: 64 in its lanes' registers and K parked in LDS (32 dwords each: everything LaneState carries between
// phases).  Before a phase runs, lanes whose path waits for another phase swap it for a parked path that waits for
// this one, so the phase executes for (almost) every lane as long as the pool holds 64 such paths; nothing is shared
// between waves and nothing waits on another wave.  The vote is over the pool, not the lanes.
//
// A work item is one SAMPLE (pass, pixel), claimed from a global counter in pass-major order; its radiance goes to a
// staging array [pass][pixel][3] and fold_kernel applies the running mean of K/rayTracer.cl:109-112 in pass order
// afterwards — the same float recurrence in the same order, so the image is bit-identical, and the pixel groups, LDS
// rings and hand-over rounds of render_waves (15 % of its time) do not exist here.
// A lane (or parked slot) that holds no path and wants a sample is "fresh": state ST_SHADE — the SHADE branch serves it — with
// the path depth 255 (kFreshDepth; plan_render sends max_depth above 254 to the other kernels).  The states a path can be in
// between two phase executions are then 0 MARCH, 1 BLOCK, 2 SHADE, 3 DONE (+ ST_BVH / ST_LEAF with entity BVHs, + ST_MODEL where full
// cubes and model blocks are tested in phases of their own: SORT): the state IS its
// class, the census is one compare per class, and the vote and the swap need no classification (round 6: a fresh path used to be
// a state of its own, 12, and every iteration classified both state vectors through a chain of compares and branches).
constexpr unsigned kFreshDepth = 255u;

struct PoolLds {
    uint4* park;  // [WORDS][K]: 16-byte word g of slot s at park[g * K + s] (consecutive lanes, consecutive 16 bytes)
    int* tags;    // [K] state of the path parked in slot s
    int* list;    // [K] scratch: the slots taking part in a swap, by rank
};

template <bool BVH>
DEV int phase_class(int st) {
    return BVH && st >= ST_BVH ? 5 : st;  // (ST_MARCH 0, ST_BLOCK 1, ST_SHADE 2, ST_DONE 3; the entity walk's states are one class)
}

// A parked path is WORDS 16-byte words.  6 words without entity BVHs (1/d and the distance marched share their registers, and so
// their word, with the hit's colour and emittance: pool_pack; the march-step count shares word 0 with the flags —
// plan_render sends draw depths above 65535 to render_waves — and the candidate block takes the place of the BVH cursor's
// word); 8 with them; 9 for the extended integrator.  The flag bits sit where LaneState's bit-fields have them.
template <int WORDS>
DEV void pool_pack(const LaneState& L, uint4 (&v)[WORDS]) {
    constexpr bool SHORT = WORDS <= 7;         // no entity BVHs: the march-step count shares word 0 with the flags, the candidate block takes the cursor's place
    constexpr int H = SHORT ? 5 : 6;  // first of the two words of the main record
    const unsigned misc = (unsigned)L.depth | ((unsigned)L.shadow << 8) | ((unsigned)L.oct_hit << 9) | ((unsigned)L.trace_hit << 10) |
                          ((unsigned)L.cand_level << 11) | ((unsigned)L.bvh_which << 15) |
                          (SHORT ? (unsigned)L.steps << 16 : ((unsigned)L.pid << 16) | ((unsigned)L.tkind << 24) | ((unsigned)L.after_nee << 26))
#if CHUNKY_FOG
                          | ((unsigned)L.medium << 27)
#endif
#if CHUNKY_GLASS
                          | ((unsigned)L.crossings << 27)
#endif
        ;
#if CHUNKY_GLASS
    static_assert(WORDS == kPoolGlassWords, "the glass units park the twelve-word record only");
    v[8] = make_uint4(__float_as_uint(L.h.color.w), (unsigned)L.rm, (unsigned)L.rm_vertex, __float_as_uint(L.clip));
    v[9] = make_uint4(__float_as_uint(L.n_vertex.x), __float_as_uint(L.n_vertex.y), __float_as_uint(L.n_vertex.z), __float_as_uint(L.o_vertex.x));
    v[10] = make_uint4(__float_as_uint(L.o_vertex.y), __float_as_uint(L.o_vertex.z), 0u, 0u);
#endif
    if (WORDS > 8) v[WORDS - 1] = make_uint4(__float_as_uint(L.pend.x), __float_as_uint(L.pend.y), __float_as_uint(L.pend.z), (unsigned)L.h.spec);
    v[0] = make_uint4((unsigned)L.sidx, L.rng, misc, SHORT ? (unsigned)L.cand_data : (unsigned)L.steps);
    v[1] = make_uint4(__float_as_uint(L.radiance.x), __float_as_uint(L.radiance.y), __float_as_uint(L.radiance.z), __float_as_uint(L.throughput.x));
    v[2] = make_uint4(__float_as_uint(L.throughput.y), __float_as_uint(L.throughput.z), __float_as_uint(L.o.x), __float_as_uint(L.o.y));
    v[3] = make_uint4(__float_as_uint(L.o.z), __float_as_uint(L.d.x), __float_as_uint(L.d.y), __float_as_uint(L.d.z));
    if (WORDS == 6) {
        // Six words: the march's values (1/d, the distance marched) and the hit's colour and emittance are never alive together — from the
        // start of a trace to its end colour and emittance are dead (a hit rewrites them before SHADE reads them; a shadow ray's
        // emittance, |dot(sun direction, normal)|, is evaluated by shade_phase where it is read), from the end of a trace to the start of
        // the next one 1/d and the distance marched are dead (trace_setup sets both) — so the kernel keeps a hit's colour and emittance
        // in the registers of 1/d and the distance marched between the block test that hit and SHADE (block_phase<SHARE> writes them
        // there, march_registers_to_hit names them for SHADE), and a parked path has no word for them.
        v[4] = make_uint4(__float_as_uint(L.inv.x), __float_as_uint(L.inv.y), __float_as_uint(L.inv.z), __float_as_uint(L.dist_march));
        v[5] = make_uint4(__float_as_uint(L.h.distance), __float_as_uint(L.h.normal.x), __float_as_uint(L.h.normal.y), __float_as_uint(L.h.normal.z));
        return;
    }
    v[4] = make_uint4(__float_as_uint(L.inv.x), __float_as_uint(L.inv.y), __float_as_uint(L.inv.z), __float_as_uint(L.dist_march));
    if (WORDS > 7) v[5] = make_uint4((unsigned)L.bvh_cur, (unsigned)L.bvh_top, __float_as_uint(L.bvh_dist), (unsigned)L.cand_data);
    v[H] = make_uint4(__float_as_uint(L.h.distance), __float_as_uint(L.h.normal.x), __float_as_uint(L.h.normal.y), __float_as_uint(L.h.normal.z));
    v[H + 1] = make_uint4(__float_as_uint(L.h.color.x), __float_as_uint(L.h.color.y), __float_as_uint(L.h.color.z), __float_as_uint(L.h.emittance));
}
template <int WORDS>
DEV void pool_unpack(LaneState& L, const uint4 (&v)[WORDS]) {
    constexpr bool SHORT = WORDS <= 7;
    constexpr int H = SHORT ? 5 : 6;
    if (WORDS > 8) {
        L.pend = mk3(__uint_as_float(v[WORDS - 1].x), __uint_as_float(v[WORDS - 1].y), __uint_as_float(v[WORDS - 1].z));
        L.h.spec = (int)v[WORDS - 1].w;
    }
    L.sidx = (int)v[0].x; L.rng = v[0].y;
    L.depth = v[0].z & 0xFFu; L.shadow = (v[0].z >> 8) & 1u; L.oct_hit = (v[0].z >> 9) & 1u; L.trace_hit = (v[0].z >> 10) & 1u;
    L.cand_level = (v[0].z >> 11) & 15u; L.bvh_which = (v[0].z >> 15) & 1u;
    if (SHORT) {
        L.steps = (int)(v[0].z >> 16);
        L.cand_data = (int)v[0].w;
    } else {
        L.pid = (int)((v[0].z >> 16) & 0xFFu); L.tkind = (v[0].z >> 24) & 3u; L.after_nee = (v[0].z >> 26) & 1u;
#if CHUNKY_FOG
        L.medium = (v[0].z >> 27) & 1u;
#endif
#if CHUNKY_GLASS
        L.crossings = (v[0].z >> 27) & 31u;
        L.rm = (int)v[8].y; L.rm_vertex = (int)v[8].z; L.clip = __uint_as_float(v[8].w);
        L.n_vertex = mk3(__uint_as_float(v[9].x), __uint_as_float(v[9].y), __uint_as_float(v[9].z));
        L.o_vertex = mk3(__uint_as_float(v[9].w), __uint_as_float(v[10].x), __uint_as_float(v[10].y));
#endif
        L.steps = (int)v[0].w;
        L.bvh_cur = (int)v[5].x; L.bvh_top = (int)v[5].y; L.bvh_dist = __uint_as_float(v[5].z);
        L.cand_data = (int)v[5].w;
    }
    L.radiance = mk3(__uint_as_float(v[1].x), __uint_as_float(v[1].y), __uint_as_float(v[1].z));
    L.throughput = mk3(__uint_as_float(v[1].w), __uint_as_float(v[2].x), __uint_as_float(v[2].y));
    L.o = mk3(__uint_as_float(v[2].z), __uint_as_float(v[2].w), __uint_as_float(v[3].x));
    L.d = mk3(__uint_as_float(v[3].y), __uint_as_float(v[3].z), __uint_as_float(v[3].w));
    L.inv = mk3(__uint_as_float(v[4].x), __uint_as_float(v[4].y), __uint_as_float(v[4].z));
    L.dist_march = __uint_as_float(v[4].w);
    if (WORDS == 6) {
        L.h.distance = __uint_as_float(v[5].x);
        L.h.normal = mk3(__uint_as_float(v[5].y), __uint_as_float(v[5].z), __uint_as_float(v[5].w));
        return;
    }
    L.h.distance = __uint_as_float(v[H].x);
    L.h.normal = mk3(__uint_as_float(v[H].y), __uint_as_float(v[H].z), __uint_as_float(v[H].w));
#if CHUNKY_GLASS
    L.h.color = f4{__uint_as_float(v[H + 1].x), __uint_as_float(v[H + 1].y), __uint_as_float(v[H + 1].z), __uint_as_float(v[8].x)};  // the hit's alpha survives parking
#else
    L.h.color = f4{__uint_as_float(v[H + 1].x), __uint_as_float(v[H + 1].y), __uint_as_float(v[H + 1].z), 0.0f};
#endif
    L.h.emittance = __uint_as_float(v[H + 1].w);
}

// The six-word record's register sharing (pool_pack): a block test that ended the trace has left the hit's colour and emittance where
// 1/d and the distance marched were (path_state.hpp block_phase<SHARE>), SHADE reads them from there.  (After a shadow ray's hit, or a
// trace that ended in the march, what it finds there is read by nobody.)
DEV void march_registers_to_hit(LaneState& L) {
    L.h.color = f4{L.inv.x, L.inv.y, L.inv.z, 0.0f};
    L.h.emittance = L.dist_march;
}

// LDS traffic between the lanes of ONE wave: the hardware executes a wave's LDS instructions in order; the fence keeps
// the compiler from moving accesses of different lanes to the same word across it.
DEV void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Lanes whose path does not wait for phase X trade it for a parked path that does (as many as both sides have).
// Lanes that hold nothing any more (ST_DONE) give their place up first.  Returns the number of swaps.
//
// The state tags of the parked paths live in registers (`ptag` of lane j = tag of slot j).  Partners find each other by
// rank through two small LDS arrays — slot and tag of the r-th parked path that comes in, tag of the r-th lane path that
// goes out — written by everybody first and read after ONE fence; then each swapping lane reads its partner's eight
// 16-byte groups in one burst and writes its own over them.
template <int K, int WORDS = 8>
DEV int pool_swap(PoolLds P, LaneState& L, int& st, int& ptag, int X, int lane) {
    constexpr bool BVH = WORDS >= 8;  // (the extended integrator's 9-word record, and the glass units' 12-word one, carry the walk's fields too; 6 / 7 words: no entity BVHs)
    // who trades, as lane masks in scalar registers (mask algebra on the scalar unit; the vector unit only compares)
    constexpr LaneMask kSlots = K >= 64 ? ~0ull : ((1ull << K) - 1ull);            // lane j < K speaks for parked slot j
    const LaneMask m_done = __ballot(st == ST_DONE);
    const LaneMask m_goes = __ballot(phase_class<BVH>(st) != X);                   // (ST_DONE is a class of its own: included)
    const LaneMask m_in = __ballot(phase_class<BVH>(ptag) == X) & kSlots;
    const int n_out = (int)__popcll(m_goes), n_in = (int)__popcll(m_in);
    const int n = n_out < n_in ? n_out : n_in;
    if (n == 0) return 0;  // wave-uniform
    const int r_in = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m_in >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_in, 0u));
    int r_out;
    if (m_done == 0) {  // (wave-uniform) the usual case: lanes go out in lane order
        r_out = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m_goes >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_goes, 0u));
    } else {            // the last moments of a launch: lanes that hold nothing any more give their place up first
        const bool done = st == ST_DONE;
        const LaneMask m_mine = done ? m_done : (m_goes & ~m_done);
        r_out = (done ? 0 : (int)__popcll(m_done)) + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m_mine >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_mine, 0u));
    }
    const bool comes = in_mask(m_in) && r_in < n, goes = in_mask(m_goes) && r_out < n;
    if (comes) P.list[r_in] = lane | (ptag << 8);  // slot and tag of the r-th path that comes in
    if (goes) P.tags[r_out] = st;                  // tag of the r-th path that goes out
    wave_lds_fence();
    if (comes) ptag = P.tags[r_in];
    if (goes) {
        const int e = P.list[r_out];
        const int s = e & 0xFF;
        uint4 mine[WORDS], theirs[WORDS];
        pool_pack<WORDS>(L, mine);
        // one LDS exchange per 8 bytes: the parked record and the lane's registers trade places in place
#pragma unroll
        for (int g = 0; g < WORDS; g++) {
            unsigned long long* q = (unsigned long long*)&P.park[g * K + s];
            const unsigned long long lo = __hip_atomic_exchange(q, (unsigned long long)mine[g].x | ((unsigned long long)mine[g].y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            const unsigned long long hi = __hip_atomic_exchange(q + 1, (unsigned long long)mine[g].z | ((unsigned long long)mine[g].w << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            theirs[g] = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        }
        st = e >> 8;
        pool_unpack<WORDS>(L, theirs);
    }
    wave_lds_fence();  // the next swap's readers (other lanes) come after these writes
    return n;
}
// Tunables of the pool kernel (each measured on the bench; DESIGN.md section 5 has the sweeps).  The -D overrides exist
// for tuning builds (tools/variants.sh) only.
#ifndef CHUNKY_POOL_WAVES
#define CHUNKY_POOL_WAVES 6   // waves per SIMD: a march step waits on two dependent tree reads, every wave counts
#endif
#ifndef CHUNKY_POOL_BVH_WAVES
#define CHUNKY_POOL_BVH_WAVES 5
#endif
// (CHUNKY_POOL_WORDS and CHUNKY_POOL_PARK, which the choice of instantiation depends on: launch_plan.hpp)
#ifndef CHUNKY_POOL_REFILL
#define CHUNKY_POOL_REFILL 20 // leave the march loop to refill once this many lanes are free and parked marchers exist (round 6, with the new leave rule: 16 / 20 / 24 = 7 504 / 7 526 / 7 510 headline, 4 170 / 4 140 / 4 075 indoor)
#endif
#ifndef CHUNKY_WALK_LEAVE
#define CHUNKY_WALK_LEAVE 24  // leave the entity-BVH walk once this many lanes have finished theirs
#endif
#ifndef CHUNKY_STAY_FEW_PARKED
#define CHUNKY_STAY_FEW_PARKED 12  // "hardly any marcher parked" (see the march's leave rule)
#endif
#ifndef CHUNKY_STAY_LONGER
#define CHUNKY_STAY_LONGER 16      // ... how many lanes emptier the march then runs before the wave leaves it
#endif
constexpr int kPoolRefill = CHUNKY_POOL_REFILL, kWalkLeave = CHUNKY_WALK_LEAVE;
#ifndef CHUNKY_STAY_LONGER_BVH
#define CHUNKY_STAY_LONGER_BVH 6   // ... in the kernels with entity BVHs (16 / 10 / 6 / 0 lanes: entities 225.5 / 227 / 225.6 / 223, the city with its entities 851 / 898 / 921 / 914)
#endif
constexpr int kStayFewParked = CHUNKY_STAY_FEW_PARKED, kStayLonger = CHUNKY_STAY_LONGER, kStayLongerBvh = CHUNKY_STAY_LONGER_BVH;
#ifndef CHUNKY_W_MODEL
#define CHUNKY_W_MODEL 4
#endif
#ifndef CHUNKY_MODEL_FIRE
#define CHUNKY_MODEL_FIRE 560  // model blocks are tested once (how many wait) x (iterations since they last were) reaches this
#endif
constexpr int kWModel = CHUNKY_W_MODEL, kModelFire = CHUNKY_MODEL_FIRE;
constexpr int kWWalk = 1;          // vote weight of the walk against kWMarch / kWBlock / kWShade = 4: the walkers are the pool's standing crowd
constexpr int kSampleBatch = 256;  // sample indices a wave claims per atomic (measured: 64 -20 %, 128 -5 %, 512 -0.1 %, 1024 -1.3 %)

// Samples are handed out per XCD.  Each of the eight XCDs has its own L2, and workgroup b of a launch runs on XCD b % 8 (read
// from the hardware: HW_REG_XCC_ID).  The launch's samples — tile-major, so a contiguous range is a stripe of the image with
// all its passes — are cut into kXcdRanges equal ranges with a counter each; a wave starts in a range of the XCD it runs on
// and, when that has run dry (sky stripes finish long before terrain stripes), goes on with the range that follows, where its
// neighbours already are.  The waves that share an L2 — and the paths that share a wave's pool — thus work on neighbouring
// tiles of one stripe, rays of one kind, while the chip as a whole is spread over the image.  Which wave renders a sample
// has no influence on its value.  Measured on the bench (one counter: 5.55 Gsamples/s): eight stripes 5.92; going on with
// the fullest range instead of the next 5.77; tile groups dealt round-robin to the XCDs instead of stripes: groups of 1-8
// tiles -0.6 ... +0.9 %, 16-240 tiles +3 %.
constexpr int kXcdRanges = 8;  // one range per XCD (16 / 32 / 64 ranges measured -0.3 / -0.9 / -1.7 %)
constexpr int kXcdCounters = 64;  // the range counters sit at work_counter[64 ...] (behind the claim counter and the 25 profile words)
DEV int xcd_id() {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return (int)(x & 7u);
}
// the range a wave starts in: the XCD's ranges are consecutive, its workgroups take them in turn
DEV int xcd_first_range() { return xcd_id(); }
struct XcdClaim {
    int q;               // the range this wave draws from; kXcdRanges + the ranges found empty so far, once its first one is
    unsigned next, end;  // claimed and not yet handed out: samples [next, end) of the launch
};
// samples of range x: [x * stripe, min((x + 1) * stripe, n_samples)); stripe is a multiple of kSampleBatch
DEV unsigned xcd_range_size(unsigned x, unsigned stripe, unsigned n_samples) {
    const unsigned lo = x * stripe;
    return lo >= n_samples ? 0u : (n_samples - lo < stripe ? n_samples - lo : stripe);
}
// Every lane with `need` gets a sample index: < n_samples a sample, kClaimNone nothing this time (the tail of a batch: the
// lane asks again), kClaimDone no samples left anywhere.  Convergent.
constexpr unsigned kClaimNone = 0xFFFFFFFEu, kClaimDone = 0xFFFFFFFFu;
DEV unsigned xcd_claim(int* counters, XcdClaim& c, int& tried, bool need, unsigned stripe, unsigned n_samples) {
    const unsigned long long mask = __ballot(need);
    if (mask == 0) return kClaimNone;
    const unsigned n_need = (unsigned)__popcll(mask);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    const unsigned rem = c.end - c.next;
    unsigned sidx = kClaimNone;
    if (need && rank < rem) sidx = c.next + rank;
    c.next += n_need < rem ? n_need : rem;
    if (n_need > rem) {
        bool got = false;
        while (tried < kXcdRanges) {
            int b = 0;
            if (need && rank == 0) b = atomicAdd(counters + c.q, kSampleBatch);
            const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane(__shfl(b, __ffsll((long long)mask) - 1));
            const unsigned n_q = xcd_range_size((unsigned)c.q, stripe, n_samples);
            if (base < n_q) {
                c.next = (unsigned)c.q * stripe + base;
                c.end = c.next + (n_q - base < (unsigned)kSampleBatch ? n_q - base : (unsigned)kSampleBatch);
                got = true;
                break;
            }
            c.q = c.q + 1 == kXcdRanges ? 0 : c.q + 1;  // this range is empty for good: on to the next
            tried += 1;
        }
        if (!got) {
            if (need && rank >= rem) sidx = kClaimDone;
            c.next = c.end = 0u;
        } else {
            const unsigned mine = c.next + (rank - rem);
            if (need && rank >= rem && mine < c.end) sidx = mine;
            c.next = c.next + (n_need - rem) < c.end ? c.next + (n_need - rem) : c.end;
        }
    }
    return sidx;
}

// stats (STATS = true), same layout as render_waves: [0..8] executions / lanes / cycles of MARCH, BLOCK (and the entity-BVH
// walk), SHADE; [9..11] wave lifetimes; [12] swap rounds, [13] paths swapped; [14..] parts of SHADE.
// The march loop of one entry into MARCH: steps while `stay` lanes or more are marching.  Who found a candidate accumulates in
// `to_block`; `data` / `level` are the leaf every lane looked at last.
// CAP: upward rays end their march above the highest leaf that can be hit (path_state.hpp march_step); `above` counts, in the profiling
// build, the lane-steps that the cap ends or would end.
template <int TREE, bool GUARD, bool STATS, bool CAP>
DEV void march_loop(const SceneView& Sm, const RenderOpts& Om, LaneState& L, LaneMask& marching, LaneMask& to_block, int& data, int& level,
                    int& nm, int stay, const LaneMask* far_masks, unsigned long long* prof, int* entry = nullptr, unsigned long long* above = nullptr) {
    const unsigned edge = world_edge(Sm);
    const int ybias = CAP ? march_ybias(Sm, L, edge) : 0;  // one more register for the length of the loop; not part of a parked path
    do {
        if (STATS) {
            prof[0] += 1;
            prof[1] += (unsigned long long)nm;
        }
        LaneMask cand, live;
        march_step<TREE, GUARD, CAP>(Sm, Om, L, marching, cand, live, data, level, edge, far_masks, entry, ybias, STATS ? above : nullptr);
        to_block |= cand;
        marching = live & ~cand;
        nm = __popcll(marching);
    } while (nm >= stay);
}

// BLOCK starts the shadow ray or the bounce where its test hits.  A trace that ends goes to SHADE, but for a hit SHADE only colours the
// throughput, draws the two numbers of the sun direction or the bounce and runs trace_setup: no sky, no deposit, no new sample — and the
// whole wave executes SHADE for it.  So the block test (the plain kernels: no entity BVHs, not the extended integrator) runs that
// continuation itself, path_continue.inc and trace_setup, for every lane whose test just reported a hit and whose path is
// known to go on: a main ray's hit (the shadow ray) and a shadow ray's hit (the bounce).  A bounce that reaches the depth limit ends
// the path — known from the depth alone, before a number is drawn — and stays SHADE's, as does every miss, the deposit and the
// hand-out of samples.  The lane leaves as a marcher (or, as from SHADE's trace_setup, for SHADE when the new ray misses the world).
// A path runs the same helpers on the same values in the same order, its own RNG draws included: the image does not change, only which
// lanes run together — one SHADE visit, one loop iteration and one swap round less per hit.
// Only in scenes with the sun on (S.sun_flags & 1, wave-uniform: the word comes with the block test's own scene words).  With the sun
// off a vertex has one trace, and in a closed room the paths of a wave go BLOCK -> SHADE -> MARCH together, 63.6 lanes per execution
// and no swap in between; taking the hits over there splits every fifth lane off (the bounce at the depth limit) and the march runs
// emptier: the indoor room lost 5.6 % (EXPERIMENTS 8.1), so such scenes keep the flow in which every trace that ends goes to SHADE.
// The other scene and option words are read here, behind the test, through fresh_args: none of them lives in the loop's SGPRs.
// (So of the included text the branch "a main ray's hit bounces" never runs here: a main ray's hit always starts the shadow ray.)
// -DCHUNKY_BLOCK_CONTINUES=0 (tuning builds, tools/variants.sh; the default is set at the top of this file) restores that flow everywhere.
template <int END, int WORDS>
DEV void block_continues(const SceneView& Sb, LaneState& L, int& st) {  // for the lanes the block test just ran for: st is what it returned
    static_assert(END == ST_SHADE, "the plain kernels only: with entity BVHs a trace does not end at the octree");
    if (!(Sb.sun_flags & 1)) return;
    asm volatile("; chunky-mark block-continues" : "+v"(st));  // (opaque: nothing below is started above the test)
    const bool hit_now = st == END;
    WaveArgPtr A = fresh_args();
    const SceneView S = arg_copy(&A->S);
    const RenderOpts O = arg_copy(&A->O);
    const bool main_trace = !L.shadow;
    // (a shadow ray is started whatever the depth; a bounce makes the depth L.depth + 1, which SHADE checks against the limit)
    // (the sun flag is on here — the early return above — and is named again all the same: without it one proj:: instantiation spills 8 bytes)
    const bool takes = hit_now && ((main_trace && (S.sun_flags & 1)) || (int)L.depth + 1 < O.max_depth);
    if (takes) {
        // the hit's colour and emittance are consumed first: with the six-word record they sit where trace_setup writes 1/d and the distance
        if (WORDS == 6) march_registers_to_hit(L);
        bool finished = false;  // (stays false: a shadow ray never ends a path, and the bounce is below the depth limit)
#include "path_continue.inc"
        st = trace_setup<END, false>(S, L);
    }
}

// Between two phases of the kernel's loop: the phase chosen, as a value the optimiser cannot see through (no instruction) — it cannot
// tell any more that the phases exclude each other, so it does not merge them back into one chain of alternatives (pool_kernel.inc).
// The comment it leaves in the compiled kernel says which phase's code ends there (tools/isa_copies.py, tools/isa_scratch.py).
#define CHUNKY_PHASE_END(X, name) asm volatile("; chunky-mark phase-end " name : "+s"(X))

// The hot kernel, twice (pool_kernel.inc): render_pool for pinhole and pre-generated rays, proj::render_pool for the projected
// cameras (projector types 1-5, 7, 8).  A compile-time choice, as SORT is: a branch on the projector type inside the kernel would cost
// the pinhole path registers it does not have.
#define CHUNKY_POOL_PROJ false
#include "pool_kernel.inc"
#undef CHUNKY_POOL_PROJ
namespace proj {
#define CHUNKY_POOL_PROJ true
#include "pool_kernel.inc"
#undef CHUNKY_POOL_PROJ
}  // namespace proj
// The instantiation a plan names (launch_plan.hpp: the lists are written there, once), of either kernel; null when the list has none.
// The entity-BVH instantiations are compiled in a translation unit of their own, render_pool_bvh.hip: this file again, up to here, with
// CHUNKY_IEEE_FORMS (rt_short_forms.h) — those kernels keep the compiler's divisions and roots.  This unit instantiates no kernel with
// BVH = true, that one none with BVH = false.
// The instantiations that tint by position (CHUNKY_BIOME_TINT, rt_device.hpp: the biome map heads their arguments) are compiled in two
// more units, render_pool_biome.hip and render_pool_biome_bvh.hip: this file up to here once more, for the pinhole and pre-generated cameras.
typedef void (*PoolKernel)(WaveArgs);
typedef void (*PoolBiomeKernel)(BiomeMap, WaveArgs);
PoolBiomeKernel pool_kernel_biome(const RenderPlan& p);
PoolBiomeKernel pool_kernel_biome_bvh(const RenderPlan& p);
// The instantiations with the ground-fog layer (CHUNKY_FOG, rt_device.hpp: the layer's parameters head their arguments; shade_phase_ext
// above) are compiled in two more units again, render_pool_fog.hip and render_pool_fog_bvh.hip: the extended integrator, pinhole and
// pre-generated cameras.
typedef void (*PoolFogKernel)(FogParams, WaveArgs);
PoolFogKernel pool_kernel_fog(const RenderPlan& p);
PoolFogKernel pool_kernel_fog_bvh(const RenderPlan& p);
// The instantiations with translucent blocks (CHUNKY_GLASS, rt_device.hpp: the two parameters head their arguments; shade_phase_ext above and
// the march's run rule, path_state.hpp march_step) are compiled in two more units, render_pool_glass.hip and render_pool_glass_bvh.hip:
// the extended integrator, pinhole and pre-generated cameras, the twelve-word parked record.
typedef void (*PoolGlassKernel)(GlassParams, WaveArgs);
PoolGlassKernel pool_kernel_glass(const RenderPlan& p);
PoolGlassKernel pool_kernel_glass_bvh(const RenderPlan& p);
#if CHUNKY_GLASS
#define CHUNKY_POOL_GLASS_CASE(TREE, K, STATS, BVH, EXT, SORT)                                                                   \
    if (p.tree == (TREE) && p.park == (K) && p.stats == (STATS) && p.bvh == (BVH) && p.ext == (EXT) && p.sorted == (SORT) && !p.proj) \
        return render_pool<TREE, K, STATS, BVH, EXT, SORT>;
#ifdef CHUNKY_POOL_BVH_TU
PoolGlassKernel pool_kernel_glass_bvh(const RenderPlan& p) {
    CHUNKY_POOL_GLASS_BVH_INSTANCES(CHUNKY_POOL_GLASS_CASE)
    return nullptr;
}
#else
PoolGlassKernel pool_kernel_glass(const RenderPlan& p) {
    if (p.bvh) return pool_kernel_glass_bvh(p);
    CHUNKY_POOL_GLASS_INSTANCES(CHUNKY_POOL_GLASS_CASE)
    return nullptr;
}
#endif
}  // namespace chunky
#elif CHUNKY_FOG
#define CHUNKY_POOL_FOG_CASE(TREE, K, STATS, BVH, EXT, SORT)                                                                    \
    if (p.tree == (TREE) && p.park == (K) && p.stats == (STATS) && p.bvh == (BVH) && p.ext == (EXT) && p.sorted == (SORT) && !p.proj) \
        return render_pool<TREE, K, STATS, BVH, EXT, SORT>;
#ifdef CHUNKY_POOL_BVH_TU
PoolFogKernel pool_kernel_fog_bvh(const RenderPlan& p) {
    CHUNKY_POOL_FOG_BVH_INSTANCES(CHUNKY_POOL_FOG_CASE)
    return nullptr;
}
#else
PoolFogKernel pool_kernel_fog(const RenderPlan& p) {
    if (p.bvh) return pool_kernel_fog_bvh(p);
    CHUNKY_POOL_FOG_INSTANCES(CHUNKY_POOL_FOG_CASE)
    return nullptr;
}
#endif
}  // namespace chunky
#elif CHUNKY_BIOME_TINT
#define CHUNKY_POOL_BIOME_CASE(TREE, K, STATS, BVH, EXT, SORT)                                                                   \
    if (p.tree == (TREE) && p.park == (K) && p.stats == (STATS) && p.bvh == (BVH) && p.ext == (EXT) && p.sorted == (SORT) && !p.proj) \
        return render_pool<TREE, K, STATS, BVH, EXT, SORT>;
#ifdef CHUNKY_POOL_BVH_TU
PoolBiomeKernel pool_kernel_biome_bvh(const RenderPlan& p) {
    CHUNKY_POOL_BIOME_BVH_INSTANCES(CHUNKY_POOL_BIOME_CASE)
    return nullptr;
}
#else
PoolBiomeKernel pool_kernel_biome(const RenderPlan& p) {
    if (p.bvh) return pool_kernel_biome_bvh(p);
    CHUNKY_POOL_BIOME_INSTANCES(CHUNKY_POOL_BIOME_CASE)
    return nullptr;
}
#endif
}  // namespace chunky
#else  // CHUNKY_BIOME_TINT
#define CHUNKY_POOL_CASE(TREE, K, STATS, BVH, EXT, SORT)                                                                        \
    if (p.tree == (TREE) && p.park == (K) && p.stats == (STATS) && p.bvh == (BVH) && p.ext == (EXT) && p.sorted == (SORT))      \
        return p.proj ? proj::render_pool<TREE, K, STATS, BVH, EXT, SORT> : render_pool<TREE, K, STATS, BVH, EXT, SORT>;
PoolKernel pool_kernel_bvh(const RenderPlan& p);
#ifdef CHUNKY_POOL_BVH_TU
PoolKernel pool_kernel_bvh(const RenderPlan& p) {
    CHUNKY_POOL_BVH_INSTANCES(CHUNKY_POOL_CASE)
    return nullptr;
}
}  // namespace chunky
#else
static_assert(kPoolAddr32Forms == (unsigned)(CHUNKY_ADDR32_FORMS), "the planner sends scenes here by the address forms these kernels have");
static PoolKernel pool_kernel(const RenderPlan& p) {
    if (p.bvh) return pool_kernel_bvh(p);
    CHUNKY_POOL_INSTANCES(CHUNKY_POOL_CASE)
    return nullptr;
}

// The running mean of K/rayTracer.cl:109-112 over the staged samples of a launch, strictly in pass order: one thread per
// pixel and channel, reads coalesced across pixels ([pass][slot][3]).
__global__ void __launch_bounds__(256) fold_kernel(const float* __restrict__ staging, float* __restrict__ res, ShardView T, int n_pixels,
                                                    int width, long long n_slots, int n_passes, int first_spp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 3ll * n_slots) return;
    const int slot = (int)(t / 3), c = (int)(t - 3ll * slot);
    const int gid = pool_slot_gid(T, width, n_pixels / width, slot);
    if (gid >= n_pixels) return;
    float mean = res[3 * (size_t)gid + c];
    // sample (sub-block, pass, i) sits at index (sub-block * n_passes + pass) * kSubBlock + i
    const size_t sub = (size_t)slot / kSubBlock, i = (size_t)slot % kSubBlock;
    const float* p = staging + 3 * (sub * (size_t)n_passes * kSubBlock + i) + c;
#pragma unroll 8
    for (int k = 0; k < n_passes; k++) {
        const int spp = first_spp + k;
        // (plain loads: a thread's consecutive passes share cache lines)
        mean = (mean * (float)spp + p[(size_t)k * (3 * kSubBlock)]) / (float)(spp + 1);
    }
    res[3 * (size_t)gid + c] = mean;
}

// Read-back exchange of a multi-GPU group (capi_group.hip group_gather): the pixels of the slots of shard T, 3 floats per slot
// in slot order, out of the image (PACK) or back into one.  Slot -> pixel is pool_slot_gid, as in the kernels that rendered
// them; padding slots carry nothing.
template <bool PACK>
__global__ void __launch_bounds__(256) gather_kernel(ShardView T, int width, int height, float* __restrict__ fb, float* __restrict__ packed) {
    const int slot = (int)(blockIdx.x * 256 + threadIdx.x);
    if (slot >= T.n_local) return;
    const int gid = pool_slot_gid(T, width, height, slot);
    if (gid >= width * height) return;
    float* a = fb + 3 * (size_t)gid;
    float* b = packed + 3 * (size_t)slot;
    if (PACK) {
        b[0] = a[0]; b[1] = a[1]; b[2] = a[2];
    } else {
        a[0] = b[0]; a[1] = b[1]; a[2] = b[2];
    }
}
// The exchange by ncclReduce (capi_group.hip group_gather_reduce) sums zero-padded framebuffers: this clears the pixels shard T does
// not own — same ownership rule as shard_gid / pool_slot_gid (runs of T.tile pixel indices, or 16 x 16 blocks, dealt round-robin).
__global__ void __launch_bounds__(256) clear_foreign_kernel(ShardView T, int width, int height, float* __restrict__ fb) {
    const int gid = (int)(blockIdx.x * 256 + threadIdx.x);
    if (gid >= width * height || T.world == 1) return;
    int unit;
    if (T.tile != 0) {
        unit = gid / T.tile;
    } else {
        const int y = gid / width, x = gid - y * width;
        unit = (y >> kTileLog) * ((width + kTileEdge - 1) >> kTileLog) + (x >> kTileLog);
    }
    if (unit % T.world == T.rank) return;
    float* a = fb + 3 * (size_t)gid;
    a[0] = 0.0f; a[1] = 0.0f; a[2] = 0.0f;
}
// ------------------------------------------------------------------------------------ launchers
// render_pool + fold_kernel, as planned: look the kernel up, size the persistent grid, fill the arguments, launch, fold.
static hipError_t launch_pool(const RenderPlan& plan, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                              const PassSeeds& P, float* res, int* work_counter, hipStream_t stream, KernelChoice* chosen,
                              float* staging, const int* seeds_dev, const StagedFold& fold = StagedFold{}, const BiomeMap* biome = nullptr,
                              const FogParams* fog = nullptr, const GlassParams* glass = nullptr) {
    // (biome: a plan of plan_biome's, run by the instantiation that takes the map ahead of the same arguments; fog: a plan of plan_fog's,
    // glass: a plan of plan_glass's, likewise)
    const PoolKernel k = biome || fog || glass ? nullptr : pool_kernel(plan);
    const PoolBiomeKernel kb = biome && !fog && !glass ? pool_kernel_biome(plan) : nullptr;
    const PoolFogKernel kf = fog && !biome && !glass ? pool_kernel_fog(plan) : nullptr;
    const PoolGlassKernel kg = glass && !biome && !fog ? pool_kernel_glass(plan) : nullptr;
    if (!k && !kb && !kf && !kg) return hipErrorInvalidDeviceFunction;  // a plan outside the list: an error, never another kernel
    const int block = kLaunchBlock, park = plan.park;
    const long long n_tiles = pool_tiles(T, C.width, C.height);
    const long long n_samples = n_tiles * kSampleTile * P.n;  // tiles at the image's edges are padded
    // a wave keeps 64 + park paths in flight: no more workgroups than the samples can feed
    const long long want = (n_samples + (long long)(block / 64) * (64 + park) - 1) / ((long long)(block / 64) * (64 + park));
    int grid = 0;  // (for an empty share or no passes `want`, and so the grid, is <= 0: nothing is launched, below)
    if (hipError_t e = kg ? persistent_grid(kg, block, plan.lds, want, &grid)
                          : (kf ? persistent_grid(kf, block, plan.lds, want, &grid)
                                : (kb ? persistent_grid(kb, block, plan.lds, want, &grid) : persistent_grid(k, block, plan.lds, want, &grid))))
        return e;
    if (T.n_local <= 0 || P.n <= 0) return hipSuccess;  // (behind the device queries: a call on a broken device fails whatever it renders)
    if (chosen) *chosen = KernelChoice{plan.tree, 1, plan.bvh ? 1 : 0, grid, park, kg ? kChoiceGlass : (kf ? kChoiceFog : (kb ? kChoiceBiome : (plan.ext ? 1 : 0))), plan.sorted ? 1 : 0};
    hipError_t e = hipMemsetAsync(work_counter, 0, sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(work_counter + kXcdCounters, 0, kXcdRanges * sizeof(int), stream);  // the per-XCD sample ranges (xcd_claim)
    if (e != hipSuccess) return e;
    const WaveArgs A = make_wave_args(S, C, O, T, P, work_counter, res, (unsigned long long*)(work_counter + 2), (unsigned)plan.depth, staging, (unsigned)n_samples,
                                      (unsigned)((n_tiles + kXcdRanges - 1) / kXcdRanges * kSampleTile * P.n), fast_div((unsigned)P.n * (unsigned)kSubBlock),
                                      fast_div((unsigned)((C.width + kTileEdge - 1) >> kTileLog)), seeds_dev);
    if (kg)
        hipLaunchKernelGGL(kg, dim3(grid), dim3(block), plan.lds, stream, *glass, A);
    else if (kf)
        hipLaunchKernelGGL(kf, dim3(grid), dim3(block), plan.lds, stream, *fog, A);
    else if (kb)
        hipLaunchKernelGGL(kb, dim3(grid), dim3(block), plan.lds, stream, *biome, A);
    else
        hipLaunchKernelGGL(k, dim3(grid), dim3(block), plan.lds, stream, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (fold.kind == StagedFold::stats) {  // adaptive sampling: the same running mean, and the pixels' luminance statistic from the same read
        return launch_fold_stats(staging, res, fold.stat_image, T, C.width, C.height, n_tiles, P.n, P.first_spp, stream);
    }
    if (fold.kind == StagedFold::buckets) {  // robust accumulation: the same running mean, and the pixels' bucket means from the same read
        return launch_fold_buckets(staging, res, fold.bucket_images, fold.n_buckets, fold.first_index, T, C.width, C.height, n_tiles, P.n, P.first_spp, stream);
    }
    const long long threads = 3ll * n_tiles * kSampleTile;
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, (const float*)staging, res, T,
                       C.width * C.height, C.width, n_tiles * kSampleTile, P.n, P.first_spp);
    return hipGetLastError();
}
hipError_t launch_render(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                         const PassSeeds& P, float* res, int* work_counter, hipStream_t stream, KernelChoice* chosen,
                         float* staging, const int* seeds_dev) {
    return launch_render_fold(variant, S, C, O, T, P, res, work_counter, stream, chosen, staging, seeds_dev, StagedFold{});
}
hipError_t launch_render_fold(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, const ShardView& T,
                              const PassSeeds& P, float* res, int* work_counter, hipStream_t stream, KernelChoice* chosen,
                              float* staging, const int* seeds_dev, const StagedFold& fold, const BiomeMap* biome, const FogParams* fog,
                              const GlassParams* glass) {
    if (biome && fold.kind != StagedFold::none) return hipErrorNotSupported;  // the folds run on the kernels that do not tint by position
    if (glass) {  // translucent blocks: plan_glass's plan on the glass instantiations, or nothing (the C API has refused the rest with the reason)
        if (fold.kind != StagedFold::none) return hipErrorNotSupported;
        const GlassPlan g = plan_glass(variant, scene_facts(S), O, C.projector_type, T, P.n, work_counter && staging, seeds_dev != nullptr, biome != nullptr, fog != nullptr);
        if (g.plan.status == PlanStatus::invalid_value) return hipErrorInvalidValue;
        if (g.plan.status != PlanStatus::ok || g.refusal != GlassRefusal::none) return hipErrorNotSupported;
        return launch_pool(g.plan, S, C, O, T, P, res, work_counter, stream, chosen, staging, P.n > kMaxPassesPerLaunch ? seeds_dev : nullptr, fold, nullptr, nullptr, glass);
    }
    if (fog) {  // ground fog: plan_fog's plan on the fog instantiations, or nothing (the C API has refused the rest with the reason)
        if (fold.kind != StagedFold::none) return hipErrorNotSupported;
        const FogPlan f = plan_fog(variant, scene_facts(S), O, C.projector_type, T, P.n, work_counter && staging, seeds_dev != nullptr, biome != nullptr);
        if (f.plan.status == PlanStatus::invalid_value) return hipErrorInvalidValue;
        if (f.plan.status != PlanStatus::ok || f.refusal != FogRefusal::none) return hipErrorNotSupported;
        return launch_pool(f.plan, S, C, O, T, P, res, work_counter, stream, chosen, staging, P.n > kMaxPassesPerLaunch ? seeds_dev : nullptr, fold, nullptr, fog);
    }
    RenderPlan plan = plan_render(variant, scene_facts(S), O, C.projector_type, T, P.n, work_counter && staging, seeds_dev != nullptr, fold.kind != StagedFold::none);
    switch (plan.status) {
        case PlanStatus::invalid_value: return hipErrorInvalidValue;
        case PlanStatus::not_supported: return hipErrorNotSupported;
        default: break;
    }
    if (biome) {  // a scene with a biome map: plan_render's plan as plan_biome maps it
        const BiomePlan b = plan_biome(plan);
        if (b.refusal != BiomeRefusal::none) return hipErrorNotSupported;  // (the C API has refused it with the reason before it came here)
        plan = b.plan;
    }
    if (plan.family == KernelFamily::pool)
        return launch_pool(plan, S, C, O, T, P, res, work_counter, stream, chosen, staging, P.n > kMaxPassesPerLaunch ? seeds_dev : nullptr, fold, biome);
    ShardView F = T;
    if (plan.needs_list) F.n_local = T.n_list;  // a shard of 16 x 16 blocks: the fallback kernels take the rank's pixels as a list
    if (biome) return launch_lanes_biome(plan, S, *biome, C, O, F, P, res, stream, chosen);
    return launch_fallback(plan, S, C, O, F, P, res, work_counter, stream, chosen);
}

hipError_t launch_gather(bool pack, const ShardView& T, int width, int height, float* fb, float* packed, hipStream_t stream) {
    if (T.n_local <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((T.n_local + 255) / 256);
    if (pack)
        hipLaunchKernelGGL(gather_kernel<true>, dim3(grid), dim3(256), 0, stream, T, width, height, fb, packed);
    else
        hipLaunchKernelGGL(gather_kernel<false>, dim3(grid), dim3(256), 0, stream, T, width, height, fb, packed);
    return hipGetLastError();
}

hipError_t launch_clear_foreign(const ShardView& T, int width, int height, float* fb, hipStream_t stream) {
    const long long n = (long long)width * height;
    if (n <= 0 || T.world == 1) return hipSuccess;
    hipLaunchKernelGGL(clear_foreign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, T, width, height, fb);
    return hipGetLastError();
}

}  // namespace chunky
#endif  // CHUNKY_POOL_BVH_TU
#endif  // CHUNKY_BIOME_TINT
