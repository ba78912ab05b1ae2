/* glass_port.c — the CPU specification of translucent blocks (include/chunky_hip.h "translucent blocks").
 *
 * TEST INFRASTRUCTURE ONLY, like oracle/port.c, which this file includes whole and leaves untouched: every port_* entry point exists
 * here too (tests/glass_spec.py wraps the library in oracle.binding.PortLib), and the glass entry points are added:
 *   glass_set                 the setting (on = 0: off)
 *   glass_render_passes /     port_render_passes / port_render_gids with trace_sample_glass in the place of trace_sample_ext; with the
 *   glass_render_gids         feature off they ARE those two (tests/test_glass_cpu.py demands equal bits)
 *   glass_helpers             row-wise known answers of csrc/glass_spec.h
 *   glass_census_*            what the samples met: see GlassCensus
 * trace_sample_glass is trace_sample_ext's loop (the extended integrator, whatever the options: with every option at its default it
 * computes what trace_sample computes) with the rules of DESIGN.md section 22: its own octree march with the run rule — port.c's, with
 * the reference's "the ray is inside this block" hook (K/octree.h:92) put to use — crossings of the path's own ray, and shadow rays that
 * are traced hit by hit, nearest first.  The arithmetic is csrc/glass_spec.h, the header the kernels compile.  Built with the flags of
 * oracle/Makefile's `port` rule. */
#include "../oracle/port.c"

#include "../chunkyclplugin_amd/csrc/glass_spec.h"

typedef struct {
    int on;
    float opaque_alpha;
    int max_crossings;
} Glass;
static Glass g_glass = {0, GLASS_OPAQUE_ALPHA_DEFAULT, GLASS_MAX_CROSSINGS_DEFAULT};
void glass_set(int on, float opaque_alpha, int max_crossings) {
    g_glass.on = on;
    g_glass.opaque_alpha = opaque_alpha;
    g_glass.max_crossings = max_crossings;
}

/* the census (all zero while the feature is off) */
typedef struct {
    int64_t main_crossings;    /* crossings of a path's own ray */
    int64_t reflect_vertices;  /* translucent hits of a path's own ray whose draw made them surface vertices */
    int64_t sun_crossings;     /* crossings of sun shadow rays */
    int64_t emitter_crossings; /* crossings of emitter shadow rays */
    int64_t rm_skipped;        /* leaves that can be hit, stepped through because they hold the block of the ray's run */
    int64_t rm_resets;         /* runs ended by a leaf that cannot be hit */
    int64_t capped;            /* hits below opaque_alpha made opaque by the cap */
    int64_t tri_crossings;     /* crossings (of any ray) of an entity triangle */
    int64_t rehits;            /* crossings whose next hit is the same thing — the same block, or a triangle after a triangle — within 4 kOffset */
    int64_t crossings;         /* all crossings: main + sun + emitter */
} GlassCensus;
#define N_GLASS_CENSUS ((int)(sizeof(GlassCensus) / sizeof(int64_t)))
static GlassCensus g_glass_census;
static int g_glass_census_on = 0;
static _Thread_local GlassCensus* t_glass = 0;
#define GLASS_COUNT(field) do { if (t_glass) t_glass->field += 1; } while (0)
int glass_census_count(void) { return N_GLASS_CENSUS; }
void glass_census_enable(int on) { g_glass_census_on = on; }
void glass_census_reset(void) { memset(&g_glass_census, 0, sizeof g_glass_census); }
void glass_census_read(int64_t* out) { memcpy(out, &g_glass_census, sizeof g_glass_census); }
static void glass_census_merge(const GlassCensus* c) {
    const int64_t* s = (const int64_t*)c;
    int64_t* d = (int64_t*)&g_glass_census;
    for (int i = 0; i < N_GLASS_CENSUS; i++) {
#ifdef _OPENMP
#pragma omp atomic
#endif
        d[i] += s[i];
    }
}

/* a leaf that can be hit: a block of the palette with a model (what the wide tree's builder leaves unmarked: csrc/widetree.cpp) */
static int glass_can_hit(const OracleScene* s, int data) {
    if (data == 0 || data == ANY_TYPE) return 0;
    const int type = s->block_palette[data];
    return type == 1 || type == 2 || type == 3;
}

/* octree_intersect (K/octree.h:41-109) with the run rule: p->ray_material is the block of the run the ray is inside (0: none) */
static int glass_octree_intersect(const OracleScene* s, Path* p, Record* rec, int draw_depth) {
    const int32_t* tree = s->octree;
    int depth = s->octree_depth;
    v3 o = p->origin, d = p->direction;
    float dist_march = 0;
    v3 inv = V3(1 / d.x, 1 / d.y, 1 / d.z);
    v3 off = scale3(d, OFFSET);
    int lx = ifloor(o.x) >> depth, ly = ifloor(o.y) >> depth, lz = ifloor(o.z) >> depth;
    if ((lx != 0) | (ly != 0) | (lz != 0)) {
        float size = (float)(1 << depth);
        Box world = {0, size, 0, size, 0, size};
        float dist = box_quick(&world, o, inv);
        if (rt_isnan(dist) || dist < 0) return 0;
        dist_march += dist + OFFSET;
    }
    for (int i = 0; i < draw_depth; i++) {
        if (dist_march > rec->distance) return 0;
        v3 pos = add3(o, scale3(d, dist_march));
        v3 po = add3(pos, off);
        int bx = ifloor(po.x), by = ifloor(po.y), bz = ifloor(po.z);
        if (((bx >> depth) != 0) | ((by >> depth) != 0) | ((bz >> depth) != 0)) return 0;
        COUNT(steps, 1);
        int level = depth;
        int data = tree[0];
        while (data > 0) {
            level--;
            data = tree[data + ((((bx >> level) & 1) << 2) | (((by >> level) & 1) << 1) | ((bz >> level) & 1))];
        }
        data = -data;
        lx = bx >> level; ly = by >> level; lz = bz >> level;
        if (!glass_can_hit(s, data)) {
            if (p->ray_material != 0) GLASS_COUNT(rm_resets);
            p->ray_material = 0; /* the run ends */
        } else if (data == p->ray_material) {
            GLASS_COUNT(rm_skipped); /* inside the run: stepped through */
        } else {
            float dist = intersect_block(s, data, bx, by, bz, rec, pos, d, inv);
            if (!rt_isnan(dist)) {
                rec->distance = dist_march + dist;
                rec->material = data;
                return 1;
            }
        }
        Box leaf = {(float)(lx << level), (float)((lx + 1) << level), (float)(ly << level),
                    (float)((ly + 1) << level), (float)(lz << level), (float)((lz + 1) << level)};
        dist_march += box_exit(&leaf, po, inv) + OFFSET;
    }
    return 0;
}

/* closest_intersect (K/kernel.h:14-24) over that march */
static int glass_closest_intersect(const OracleScene* s, Path* p, Record* rec, int draw_depth) {
    COUNT(traces, 1);
    int hit = 0;
    const int oct = glass_octree_intersect(s, p, rec, draw_depth);
    hit |= oct;
    const int world = bvh_intersect(s, s->world_bvh, p, rec);
    hit |= world;
    const int actor = bvh_intersect(s, s->actor_bvh, p, rec);
    hit |= actor;
    rec->octree_won = oct && !world && !actor;
    if (hit) rec->point = add3(p->origin, scale3(p->direction, rec->distance - OFFSET));
    return hit;
}

/* what a crossing does to the ray, whatever its kind: the run, the origin */
static void glass_cross(Path* q, const Record* r) {
    if (r->octree_won) q->ray_material = r->material;
    else GLASS_COUNT(tri_crossings);
    GLASS_COUNT(crossings);
    glass_restart(q->origin.x, q->origin.y, q->origin.z, q->direction.x, q->direction.y, q->direction.z, r->distance, r->normal.x, r->normal.y,
                  r->normal.z, &q->origin.x, &q->origin.y, &q->origin.z);
}
/* the census of re-hits: the hit `r` follows a crossing of (won, material) */
static void glass_rehit(int crossed, int crossed_won, int crossed_material, const Record* r) {
    if (!crossed || !(r->distance < 4 * OFFSET)) return;
    if (crossed_won ? (r->octree_won && r->material == crossed_material) : !r->octree_won) GLASS_COUNT(rehits);
}

/* A shadow ray from q (its run: q.ray_material) whose record `sh` holds the clip distance: 1 when its light arrives, 0 when an opaque
 * hit — or a translucent one at the cap — blocks it.  *filter comes in as (1, 1, 1) for a sun ray and as the light itself (pend) for
 * an emitter ray, and is multiplied by fs crossing by crossing.  No random draw. */
static int glass_shadow(const OracleScene* s, const Glass* G, Path q, Record sh, v3* filter, int emitter_ray) {
    int crossings = 0, crossed = 0, crossed_won = 0, crossed_material = 0;
    float clip = sh.distance;
    for (;;) {
        if (!glass_closest_intersect(s, &q, &sh, g_draw_depth)) return 1;
        glass_rehit(crossed, crossed_won, crossed_material, &sh);
        const float a = sh.color.w;
        if (!glass_translucent(a, G->opaque_alpha, crossings, G->max_crossings)) {
            if (a < G->opaque_alpha) GLASS_COUNT(capped);
            return 0;
        }
        *filter = mul3(*filter, V3(glass_fs(a, sh.color.x), glass_fs(a, sh.color.y), glass_fs(a, sh.color.z)));
        clip = clip - sh.distance;
        if (emitter_ray) GLASS_COUNT(emitter_crossings); else GLASS_COUNT(sun_crossings);
        crossed = 1, crossed_won = sh.octree_won, crossed_material = sh.material;
        glass_cross(&q, &sh);
        crossings += 1;
        sh.distance = clip;
    }
}

/* One sample.  Random draws: at a translucent hit of the path's own ray [1: cross or reflect]; then the order of trace_sample_ext's
 * comment block. */
static v3 trace_sample_glass(const OracleScene* s, const Sun* sun, const Ext* x, const Glass* G, int seed, int gid) {
    Path p;
    Record rec;
    path_init(&p, &rec);
    unsigned state = (unsigned)seed + (unsigned)gid;
    rt_pcg_next(&state);
    primary_ray(s, gid, &state, &p, 0);
    COUNT(samples, 1);
    const int sun_on = x->sun_sampling < 0 ? (sun->flags & 1) : x->sun_sampling;
    int after_nee = 0;
    int crossings = 0, crossed = 0, crossed_won = 0, crossed_material = 0; /* of the ray in flight */
    for (;;) {
        int hit = glass_closest_intersect(s, &p, &rec, g_draw_depth);
        if (hit) glass_rehit(crossed, crossed_won, crossed_material, &rec);
        crossed = 0;
        /* ---- a translucent hit: before anything else ---- */
        if (hit && glass_translucent(rec.color.w, G->opaque_alpha, crossings, G->max_crossings)) {
            const float a = rec.color.w;
            if (!(rt_pcg_float(&state) < a)) {
                /* the ray crosses: no emission, after_nee and the depth unchanged */
                GLASS_COUNT(main_crossings);
                p.throughput = mul3(p.throughput, V3(glass_tc(a, rec.color.x), glass_tc(a, rec.color.y), glass_tc(a, rec.color.z)));
                crossed = 1, crossed_won = rec.octree_won, crossed_material = rec.material;
                glass_cross(&p, &rec);
                crossings += 1;
                rec.distance = rt_inf();
                continue;
            }
            GLASS_COUNT(reflect_vertices);
        } else if (hit && rec.color.w < G->opaque_alpha) {
            GLASS_COUNT(capped);
        }
        /* ---- from here on: trace_sample_ext, its shadow rays traced by glass_shadow ---- */
        if (!hit) {
            rec.emittance = 1;
            intersect_sky(s, sun, &p, &rec);
            break;
        }
        COUNT(hits, 1);
        const int rm_vertex = p.ray_material; /* the run the vertex was reached through: its shadow rays and its bounce start inside it */
        const v3 base = p.throughput;
        const v3 c = V3(rec.color.x, rec.color.y, rec.color.z);
        const v3 thr_d = mul3(base, c);
        const v3 point = rec.point, n = rec.normal;
        const int listed = after_nee && rec.emittance != 0 && hit_is_listed(s, &rec);
        if (x->emitters && !listed)
            p.color = add3(p.color, mul3(scale3(c, rec.emittance * g_emitter_scale), thr_d));
        after_nee = 0;
        int specular = 0;
        float metal = 0, rough = 0;
        if (x->bsdf) {
            const float spec = rt_unorm8((unsigned)rec.spec & 0xFF);
            metal = rt_unorm8(((unsigned)rec.spec >> 8) & 0xFF);
            rough = rt_unorm8(((unsigned)rec.spec >> 16) & 0xFF);
            const float ps = rt_fmax(spec, metal);
            if (ps > 0) specular = rt_pcg_float(&state) < ps;
        }
        if (specular) {
            p.throughput = V3(base.x * (c.x * metal + (1 - metal)), base.y * (c.y * metal + (1 - metal)), base.z * (c.z * metal + (1 - metal)));
            const v3 d = p.direction;
            v3 refl = sub3(d, scale3(n, 2 * dot3(d, n)));
            if (rough > 0) {
                float x1 = rt_pcg_float(&state), x2 = rt_pcg_float(&state);
                v3 dd = cosine_direction(n, x1, x2);
                refl = normalize3(add3(scale3(dd, rough), scale3(refl, 1 - rough)));
                float rn = dot3(refl, n);
                if (rn < 0) refl = sub3(refl, scale3(n, 2 * rn));
            }
            p.direction = refl;
            p.origin = add3(point, scale3(refl, OFFSET));
        } else {
            p.throughput = thr_d;
            p.origin = point;
            if (sun_on) {
                Sun on = *sun;
                on.flags |= 1;
                sun_sample_direction(&on, &p, &rec, &state);
                Record shadow = rec; /* (its distance: the record's, kept — K/rayTracer.cl:101-106) */
                shadow.point = rec.normal;
                v3 filter = V3(1, 1, 1);
                if (glass_shadow(s, G, p, shadow, &filter, 0)) {
                    /* intersect_sky's sum (K/kernel.h:26-31) with the weight the record was given, through the filter */
                    Record sky = rec;
                    sky_intersect(s, &p, &sky);
                    sun_intersect(s, sun, &p, &sky);
                    const v3 cs = V3(sky.color.x, sky.color.y, sky.color.z);
                    p.color = add3(p.color, mul3(scale3(mul3(cs, p.throughput), rec.emittance), filter));
                }
            }
            if (x->nee && x->emitters && g_n_emitters > 0 && p.ray_depth + 1 < g_max_depth) {
                const float xk = rt_pcg_float(&state), xf = rt_pcg_float(&state), xu = rt_pcg_float(&state), xv = rt_pcg_float(&state);
                int k = (int)(xk * (float)g_n_emitters);
                if (k > g_n_emitters - 1) k = g_n_emitters - 1;
                int face = (int)(xf * 6.0f);
                if (face > 5) face = 5;
                const int32_t* em = g_emitters + 4 * k;
                const int level = (em[3] >> 25) & 15, block = em[3] & 0x1FFFFFF;
                const float size = (float)(1 << level);
                const float a = xu * size, b = xv * size;
                const float fa = a - rt_floor(a), fb = b - rt_floor(b);
                const float ex = (float)em[0], ey = (float)em[1], ez = (float)em[2];
                v3 pe, nf;
                float tu, tv;
                switch (face) {
                    case 0: pe = V3(ex, ey + a, ez + b); nf = V3(-1, 0, 0); tu = 1 - fb; tv = fa; break;
                    case 1: pe = V3(ex + size, ey + a, ez + b); nf = V3(1, 0, 0); tu = fb; tv = fa; break;
                    case 2: pe = V3(ex + a, ey, ez + b); nf = V3(0, -1, 0); tu = fa; tv = 1 - fb; break;
                    case 3: pe = V3(ex + a, ey + size, ez + b); nf = V3(0, 1, 0); tu = fa; tv = fb; break;
                    case 4: pe = V3(ex + a, ey + b, ez); nf = V3(0, 0, -1); tu = fa; tv = fb; break;
                    default: pe = V3(ex + a, ey + b, ez + size); nf = V3(0, 0, 1); tu = 1 - fa; tv = fb; break;
                }
                const v3 l = sub3(pe, point);
                const float d2 = dot3(l, l);
                const float dist = rt_sqrt(d2);
                const v3 dir = scale3(l, 1 / dist);
                const float cs = dot3(dir, n), cl = -dot3(dir, nf);
                if (cs > 0 && cl > 0 && dist > 0.002f) {
                    Record er;
                    memset(&er, 0, sizeof er);
                    if (material_sample(s, s->block_palette[block + 1], &er, tu, tv) && er.emittance > 0) {
                        Path q = p;
                        q.origin = point;
                        q.direction = dir;
                        q.ray_material = rm_vertex;
                        Record sh = rec;
                        sh.distance = dist - 0.001f;
                        const float w = (cs * cl) / (RT_PI_F * d2) * (6.0f * (float)g_n_emitters * (size * size));
                        const v3 ce = V3(er.color.x, er.color.y, er.color.z);
                        const v3 le = mul3(ce, scale3(ce, er.emittance * g_emitter_scale));
                        v3 pend = mul3(thr_d, scale3(le, w));
                        if (glass_shadow(s, G, q, sh, &pend, 1)) p.color = add3(p.color, pend);
                    }
                }
                after_nee = 1;
            }
            float x1 = rt_pcg_float(&state), x2 = rt_pcg_float(&state);
            p.direction = cosine_direction(n, x1, x2);
            p.origin = add3(point, scale3(p.direction, OFFSET));
        }
        p.ray_material = rm_vertex; /* (the shadow rays worked on copies) */
        crossings = 0;
        p.ray_depth += 1;
        rec.distance = rt_inf();
        if (!(p.ray_depth < g_max_depth)) break;
    }
    return p.color;
}

static v3 glass_sample(const OracleScene* s, const Sun* sun, const Glass* G, int seed, int gid) {
    if (G->on) return trace_sample_glass(s, sun, &g_ext, G, seed, gid);
    return ext_active() ? trace_sample_ext(s, sun, &g_ext, seed, gid) : trace_sample(s, sun, seed, gid, 0, 0);
}

/* port_render_passes, with the setting */
int glass_render_passes(const OracleScene* s, const int32_t* seeds, int n_passes, int first_spp, int64_t gid_begin, int64_t gid_end, float* res,
                        int threads) {
    Sun sun = sun_new(s->sun);
    if (threads < 1) threads = 1;
    for (int k = 0; k < n_passes; k++) {
        int seed = seeds[k], spp = first_spp + k;
#pragma omp parallel num_threads(threads)
        {
            Counters local;
            GlassCensus census;
            memset(&local, 0, sizeof local);
            memset(&census, 0, sizeof census);
            t_ctr = g_count_enabled ? &local : 0;
            t_glass = g_glass_census_on ? &census : 0;
            const Sun my_sun = sun;
            const OracleScene my_scene = *s;
            const Glass my_glass = g_glass;
#pragma omp for schedule(dynamic, 256)
            for (int64_t gid = gid_begin; gid < gid_end; gid++) {
                v3 c = glass_sample(&my_scene, &my_sun, &my_glass, seed, (int)gid);
                float* px = res + 3 * gid;
                px[0] = (px[0] * spp + c.x) / (spp + 1);
                px[1] = (px[1] * spp + c.y) / (spp + 1);
                px[2] = (px[2] * spp + c.z) / (spp + 1);
            }
            if (g_count_enabled) counters_merge(&local);
            if (g_glass_census_on) glass_census_merge(&census);
            t_ctr = 0;
            t_glass = 0;
        }
    }
    return 0;
}

/* port_render_gids, with the setting */
int glass_render_gids(const OracleScene* s, const int32_t* seeds, int n_passes, int first_spp, const int32_t* gids, int64_t n_gids, float* res,
                      int threads) {
    Sun sun = sun_new(s->sun);
    if (threads < 1) threads = 1;
#pragma omp parallel num_threads(threads)
    {
        Counters local;
        GlassCensus census;
        memset(&local, 0, sizeof local);
        memset(&census, 0, sizeof census);
        t_ctr = g_count_enabled ? &local : 0;
        t_glass = g_glass_census_on ? &census : 0;
        const Sun my_sun = sun;
        const OracleScene my_scene = *s;
        const Glass my_glass = g_glass;
#pragma omp for schedule(dynamic, 64)
        for (int64_t i = 0; i < n_gids; i++) {
            int gid = gids[i];
            float* px = res + 3 * (int64_t)gid;
            float m0 = px[0], m1 = px[1], m2 = px[2];
            for (int k = 0; k < n_passes; k++) {
                int spp = first_spp + k;
                v3 c = glass_sample(&my_scene, &my_sun, &my_glass, seeds[k], gid);
                m0 = (m0 * spp + c.x) / (spp + 1);
                m1 = (m1 * spp + c.y) / (spp + 1);
                m2 = (m2 * spp + c.z) / (spp + 1);
            }
            px[0] = m0;
            px[1] = m1;
            px[2] = m2;
        }
        if (g_count_enabled) counters_merge(&local);
        if (g_glass_census_on) glass_census_merge(&census);
        t_ctr = 0;
        t_glass = 0;
    }
    return 0;
}

/* Known answers of csrc/glass_spec.h, row-wise: n rows of 12 floats in, 4 floats out.
 *   which 0  glass_translucent: in {a, opaque_alpha, crossings, max_crossings}; out {0 / 1}
 *   which 1  glass_tc: in {a, c}; out {tc}
 *   which 2  glass_fs: in {a, c}; out {fs}
 *   which 3  glass_restart: in {o.xyz, d.xyz, distance, n.xyz}; out {o'.xyz} */
void glass_helpers(int which, int n, const float* in_rows, float* out_rows) {
    for (int i = 0; i < n; i++) {
        const float* a = in_rows + 12 * i;
        float* o = out_rows + 4 * i;
        o[0] = o[1] = o[2] = o[3] = 0;
        switch (which) {
            case 0: o[0] = (float)glass_translucent(a[0], a[1], (int)a[2], (int)a[3]); break;
            case 1: o[0] = glass_tc(a[0], a[1]); break;
            case 2: o[0] = glass_fs(a[0], a[1]); break;
            case 3: glass_restart(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], &o[0], &o[1], &o[2]); break;
            default: break;
        }
    }
}
