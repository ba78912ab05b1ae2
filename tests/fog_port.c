/* fog_port.c — the CPU specification of the ground-fog layer (include/chunky_hip.h "ground fog").
 *
 * TEST INFRASTRUCTURE ONLY, like oracle/port.c, which this file includes whole and leaves untouched: every port_* entry point exists
 * here too (tests/fog_spec.py wraps the library in oracle.binding.PortLib), and the fog entry points are added:
 *   fog_set                 the layer (density 0: off)
 *   fog_render_passes /     port_render_passes / port_render_gids with trace_sample_fog in the place of trace_sample_ext; with the
 *   fog_render_gids         layer off they ARE those two (tests/test_fog_cpu.py demands equal bits)
 *   fog_helpers             row-wise known answers of csrc/fog_spec.h
 *   fog_census_*            what the samples met: see FogCensus
 * trace_sample_fog is trace_sample_ext's loop (the extended integrator, whatever the options: with every option at its default it
 * computes what trace_sample computes) with the rules of DESIGN.md section 21; the arithmetic is csrc/fog_spec.h, the header the
 * kernels compile.  Built with the flags of oracle/Makefile's `port` rule. */
#include "../oracle/port.c"

#include "../chunkyclplugin_amd/csrc/fog_spec.h"

typedef struct {
    float sigma, y_min, y_max;
    v3 color;
} Fog;
static Fog g_fog = {0, 0, 0, {0, 0, 0}};
void fog_set(float density, float y_min, float y_max, float r, float g, float b) {
    g_fog.sigma = density;
    g_fog.y_min = y_min;
    g_fog.y_max = y_max;
    g_fog.color = V3(r, g, b);
}

/* the census (all zero while the layer is off) */
typedef struct {
    int64_t segments;      /* main-ray segments that met the slab (one free-flight draw each) */
    int64_t medium;        /* medium vertices */
    int64_t medium_sun;    /* sun shadow rays started at a medium vertex */
    int64_t surface_sun;   /* sun shadow rays started at a surface vertex whose weight the slab lowered (transmittance < 1) */
    int64_t emitter;       /* emitter samples whose light the slab lowered (transmittance < 1) */
    int64_t parallel;      /* main-ray segments with d.y == 0 */
} FogCensus;
#define N_FOG_CENSUS ((int)(sizeof(FogCensus) / sizeof(int64_t)))
static FogCensus g_fog_census;
static int g_fog_census_on = 0;
static _Thread_local FogCensus* t_fog = 0;
#define FOG_COUNT(field) do { if (t_fog) t_fog->field += 1; } while (0)
int fog_census_count(void) { return N_FOG_CENSUS; }
void fog_census_enable(int on) { g_fog_census_on = on; }
void fog_census_reset(void) { memset(&g_fog_census, 0, sizeof g_fog_census); }
void fog_census_read(int64_t* out) { memcpy(out, &g_fog_census, sizeof g_fog_census); }
static void fog_census_merge(const FogCensus* c) {
    const int64_t* s = (const int64_t*)c;
    int64_t* d = (int64_t*)&g_fog_census;
    for (int i = 0; i < N_FOG_CENSUS; i++) {
#ifdef _OPENMP
#pragma omp atomic
#endif
        d[i] += s[i];
    }
}

static float fog_t_sun(const Fog* f, v3 o, v3 d) { /* the slab's transmittance from o towards d, to infinity */
    return fog_segment_transmittance(f->sigma, f->y_min, f->y_max, o.y, d.x, d.y, d.z, rt_inf());
}

/* One sample.  Random draws per main segment: [1 free flight, if the segment meets the slab]; at a medium vertex [2 sun if on] 2 sphere;
 * otherwise the order of trace_sample_ext's comment block. */
static v3 trace_sample_fog(const OracleScene* s, const Sun* sun, const Ext* x, const Fog* f, int seed, int gid) {
    Path p;
    Record rec;
    path_init(&p, &rec);
    unsigned state = (unsigned)seed + (unsigned)gid;
    rt_pcg_next(&state);
    primary_ray(s, gid, &state, &p, 0);
    COUNT(samples, 1);
    const int fog_on = f->sigma > 0;
    const int sun_on = x->sun_sampling < 0 ? (sun->flags & 1) : x->sun_sampling;
    int after_nee = 0;
    for (;;) {
        int hit = closest_intersect(s, &p, &rec, g_draw_depth);
        /* ---- free flight: at the end of every main-ray trace, hit or miss, before anything else ---- */
        int medium = 0;
        float t_medium = 0;
        if (fog_on) {
            float ta, tb, len;
            if (p.direction.y == 0) FOG_COUNT(parallel);
            if (fog_interval(p.origin.y, p.direction.x, p.direction.y, p.direction.z, hit ? rec.distance : rt_inf(), f->y_min, f->y_max, &ta, &tb, &len)) {
                FOG_COUNT(segments);
                const float sf = fog_free_flight(rt_pcg_float(&state), f->sigma);
                if (sf < (tb - ta) * len) {
                    medium = 1;
                    t_medium = ta + sf / len;
                }
            }
        }
        if (medium) {
            /* ---- the medium vertex: no emission, no specular lobe, no emitter sampling ---- */
            FOG_COUNT(medium);
            p.origin = add3(p.origin, scale3(p.direction, t_medium));
            p.throughput = mul3(p.throughput, f->color);
            after_nee = 0;
            rec.distance = rt_inf(); /* the shadow record keeps the record's distance (K/rayTracer.cl:101-106): nothing clips this sun ray */
            if (sun_on) {
                Sun on = *sun;
                on.flags |= 1;
                FOG_COUNT(medium_sun);
                sun_sample_direction(&on, &p, &rec, &state);
                Record shadow = rec;
                shadow.point = rec.normal;
                shadow.emittance = FOG_PHASE_WEIGHT * fog_t_sun(f, p.origin, p.direction); /* in place of |dot(d, n)| */
                if (!closest_intersect(s, &p, &shadow, g_draw_depth)) intersect_sky(s, sun, &p, &shadow);
            }
            {
                float x1 = rt_pcg_float(&state), x2 = rt_pcg_float(&state);
                fog_sphere(x1, x2, &p.direction.x, &p.direction.y, &p.direction.z); /* no origin offset */
            }
            p.ray_depth += 1;
            rec.distance = rt_inf();
            if (!(p.ray_depth < g_max_depth)) break;
            continue;
        }
        /* ---- from here on: trace_sample_ext, with the two shadow-ray factors ---- */
        if (!hit) {
            rec.emittance = 1;
            intersect_sky(s, sun, &p, &rec);
            break;
        }
        COUNT(hits, 1);
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
                Record shadow = rec;
                shadow.point = rec.normal;
                if (fog_on) { /* |dot(d, n)| x the slab's transmittance to infinity, NOT clipped by the distance the record keeps */
                    const float t_sun = fog_t_sun(f, p.origin, p.direction);
                    if (t_sun < 1) FOG_COUNT(surface_sun);
                    shadow.emittance = shadow.emittance * t_sun;
                }
                if (!closest_intersect(s, &p, &shadow, g_draw_depth)) intersect_sky(s, sun, &p, &shadow);
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
                        Record sh = rec;
                        sh.distance = dist - 0.001f;
                        const float w = (cs * cl) / (RT_PI_F * d2) * (6.0f * (float)g_n_emitters * (size * size));
                        const v3 ce = V3(er.color.x, er.color.y, er.color.z);
                        const v3 le = mul3(ce, scale3(ce, er.emittance * g_emitter_scale));
                        v3 pend = mul3(thr_d, scale3(le, w));
                        if (fog_on) { /* the transmittance over [0, dist], fixed when the ray is set up */
                            const float t_em = fog_segment_transmittance(f->sigma, f->y_min, f->y_max, point.y, dir.x, dir.y, dir.z, dist);
                            if (t_em < 1) FOG_COUNT(emitter);
                            pend = scale3(pend, t_em);
                        }
                        if (!closest_intersect(s, &q, &sh, g_draw_depth)) p.color = add3(p.color, pend);
                    }
                }
                after_nee = 1;
            }
            float x1 = rt_pcg_float(&state), x2 = rt_pcg_float(&state);
            p.direction = cosine_direction(n, x1, x2);
            p.origin = add3(point, scale3(p.direction, OFFSET));
        }
        p.ray_depth += 1;
        rec.distance = rt_inf();
        if (!(p.ray_depth < g_max_depth)) break;
    }
    return p.color;
}

/* port_render_passes, with the layer */
int fog_render_passes(const OracleScene* s, const int32_t* seeds, int n_passes, int first_spp, int64_t gid_begin, int64_t gid_end, float* res,
                      int threads) {
    Sun sun = sun_new(s->sun);
    if (threads < 1) threads = 1;
    for (int k = 0; k < n_passes; k++) {
        int seed = seeds[k], spp = first_spp + k;
#pragma omp parallel num_threads(threads)
        {
            Counters local;
            FogCensus census;
            memset(&local, 0, sizeof local);
            memset(&census, 0, sizeof census);
            t_ctr = g_count_enabled ? &local : 0;
            t_fog = g_fog_census_on ? &census : 0;
            const Sun my_sun = sun;
            const OracleScene my_scene = *s;
            const Fog my_fog = g_fog;
#pragma omp for schedule(dynamic, 256)
            for (int64_t gid = gid_begin; gid < gid_end; gid++) {
                v3 c = trace_sample_fog(&my_scene, &my_sun, &g_ext, &my_fog, seed, (int)gid);
                float* px = res + 3 * gid;
                px[0] = (px[0] * spp + c.x) / (spp + 1);
                px[1] = (px[1] * spp + c.y) / (spp + 1);
                px[2] = (px[2] * spp + c.z) / (spp + 1);
            }
            if (g_count_enabled) counters_merge(&local);
            if (g_fog_census_on) fog_census_merge(&census);
            t_ctr = 0;
            t_fog = 0;
        }
    }
    return 0;
}

/* port_render_gids, with the layer */
int fog_render_gids(const OracleScene* s, const int32_t* seeds, int n_passes, int first_spp, const int32_t* gids, int64_t n_gids, float* res,
                    int threads) {
    Sun sun = sun_new(s->sun);
    if (threads < 1) threads = 1;
#pragma omp parallel num_threads(threads)
    {
        Counters local;
        FogCensus census;
        memset(&local, 0, sizeof local);
        memset(&census, 0, sizeof census);
        t_ctr = g_count_enabled ? &local : 0;
        t_fog = g_fog_census_on ? &census : 0;
        const Sun my_sun = sun;
        const OracleScene my_scene = *s;
        const Fog my_fog = g_fog;
#pragma omp for schedule(dynamic, 64)
        for (int64_t i = 0; i < n_gids; i++) {
            int gid = gids[i];
            float* px = res + 3 * (int64_t)gid;
            float m0 = px[0], m1 = px[1], m2 = px[2];
            for (int k = 0; k < n_passes; k++) {
                int spp = first_spp + k;
                v3 c = trace_sample_fog(&my_scene, &my_sun, &g_ext, &my_fog, seeds[k], gid);
                m0 = (m0 * spp + c.x) / (spp + 1);
                m1 = (m1 * spp + c.y) / (spp + 1);
                m2 = (m2 * spp + c.z) / (spp + 1);
            }
            px[0] = m0;
            px[1] = m1;
            px[2] = m2;
        }
        if (g_count_enabled) counters_merge(&local);
        if (g_fog_census_on) fog_census_merge(&census);
        t_ctr = 0;
        t_fog = 0;
    }
    return 0;
}

/* Known answers of csrc/fog_spec.h, row-wise: n rows of 8 floats in, 4 floats out.
 *   which 0  fog_interval: in {o.y, d.x, d.y, d.z, t_end, y_min, y_max}; out {non-empty (0 / 1), ta, tb, len}
 *   which 1  fog_transmittance: in {tau}; out {T}
 *   which 2  fog_segment_transmittance: in {o.y, d.x, d.y, d.z, t_end, y_min, y_max, sigma}; out {T}
 *   which 3  fog_free_flight: in {u, sigma}; out {s}
 *   which 4  fog_sphere: in {x1, x2}; out {d.x, d.y, d.z} */
void fog_helpers(int which, int n, const float* in_rows, float* out_rows) {
    for (int i = 0; i < n; i++) {
        const float* a = in_rows + 8 * i;
        float* o = out_rows + 4 * i;
        o[0] = o[1] = o[2] = o[3] = 0;
        switch (which) {
            case 0: o[0] = (float)fog_interval(a[0], a[1], a[2], a[3], a[4], a[5], a[6], &o[1], &o[2], &o[3]); break;
            case 1: o[0] = fog_transmittance(a[0]); break;
            case 2: o[0] = fog_segment_transmittance(a[7], a[5], a[6], a[0], a[1], a[2], a[3], a[4]); break;
            case 3: o[0] = fog_free_flight(a[0], a[1]); break;
            case 4: fog_sphere(a[0], a[1], &o[0], &o[1], &o[2]); break;
            default: break;
        }
    }
}
