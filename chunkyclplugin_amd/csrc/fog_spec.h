/* fog_spec.h — the arithmetic of the ground-fog layer (include/chunky_hip.h, "ground fog"), compiled by the
 * kernels (render_pool_fog.hip, render_pool_fog_bvh.hip) and by the CPU specification (tests/fog_port.c) from this one text.
 *
 * The medium: homogeneous, isotropically scattering, density sigma > 0 per block of path length, inside the slab y_min <= y < y_max
 * (octree coordinates), single-scattering colour in [0, 1]^3.  This is the project's own specification; the reference has no medium.
 *
 * Plain C99 over rt_math.h.  Every operation is one exactly rounded binary32 or binary64 operation (the units that include this header
 * are compiled with -ffp-contract=off); logarithm and exponential are rt_log2_d / rt_exp2_d, which the device and the host evaluate
 * to the same bits (the hardware's v_log_f32 / v_exp_f32 have no CPU counterpart).  Every function is total: for finite or infinite
 * arguments none returns a NaN, an empty interval has transmittance exactly 1 and an infinite optical depth exactly 0. */
#ifndef CHUNKY_FOG_SPEC_H
#define CHUNKY_FOG_SPEC_H
#include "rt_math.h"

/* The part of the ray o + t d, 0 <= t < t_end, that lies in the slab: 1 and [*ta, *tb) when there is one, else 0.  *len = |d|, the
 * physical length of a unit of t (primary directions are not unit vectors: K/rayTracer.cl normalises in `preview` only), so the
 * segment is (*tb - *ta) * *len blocks long.
 *   d.y == 0:  [0, t_end) when y_min <= o.y < y_max, else empty;
 *   otherwise: t0 = (y_min - o.y) / d.y, t1 = (y_max - o.y) / d.y, ta = max(min(t0, t1), 0), tb = min(max(t0, t1), t_end).
 * Empty unless ta < tb — and empty for a direction of length 0 (or one whose length is not a number), which covers no distance: the
 * rule that keeps span x length from ever being 0 x inf. */
RT_FN int fog_interval(float oy, float dx, float dy, float dz, float t_end, float y_min, float y_max, float* ta, float* tb, float* len) {
    const float l = rt_sqrt(rt_dot3(dx, dy, dz, dx, dy, dz));
    float a, b;
    *len = l;
    if (dy == 0.0f) {
        a = 0.0f;
        b = (y_min <= oy && oy < y_max) ? t_end : 0.0f;
    } else {
        const float t0 = (y_min - oy) / dy, t1 = (y_max - oy) / dy;
        a = rt_fmax(rt_fmin(t0, t1), 0.0f);
        b = rt_fmin(rt_fmax(t0, t1), t_end);
    }
    *ta = a;
    *tb = b;
    return (a < b) && (l > 0.0f);
}

/* optical depth of `span` units of t along a direction of length `len` */
RT_FN float fog_tau(float sigma, float span, float len) { return sigma * (span * len); }

/* exp(-tau): 1 for tau <= 0 (and for a NaN), 0 for tau = +inf; 2^(-tau log2 e) in binary64, the exponent kept inside rt_exp2_d's
 * domain (2^-200 rounds to the binary32 zero, as every exp(-tau) below it does), rounded once to binary32 */
RT_FN float fog_transmittance(float tau) {
    double t;
    if (!(tau > 0.0f)) return 1.0f;
    t = (double)tau * -1.4426950408889634;
    t = t < -200.0 ? -200.0 : t;
    return (float)rt_exp2_d(t);
}

/* transmittance of the slab along o + t d, 0 <= t < t_end (t_end = +inf: to infinity) */
RT_FN float fog_segment_transmittance(float sigma, float y_min, float y_max, float oy, float dx, float dy, float dz, float t_end) {
    float ta, tb, len;
    if (!fog_interval(oy, dx, dy, dz, t_end, y_min, y_max, &ta, &tb, &len)) return 1.0f;
    return fog_transmittance(fog_tau(sigma, tb - ta, len));
}

/* free-flight distance s = -ln(1 - u) / sigma for a draw u of rt_pcg_float (a multiple of 2^-24 in [0, 1): 1 - u is exact, in
 * [2^-24, 1], a normal number): -ln2 log2(1 - u) in binary64, rounded to binary32 and kept from going below 0 (rt_log2_d is good to
 * about 2^-44 absolute, so log2(1) comes out as a few 2^-43 and not as 0), then ONE binary32 division */
RT_FN float fog_free_flight(float u, float sigma) {
    const double l2 = rt_log2_d((double)(1.0f - u));
    return rt_fmax((float)(-0.6931471805599453 * l2), 0.0f) / sigma;
}

/* uniform direction on the unit sphere from two draws: z = 1 - 2 x1, r = sqrt(max(0, 1 - z^2)), phi = 2 pi x2; (r cos phi, r sin phi, z) */
RT_FN void fog_sphere(float x1, float x2, float* dx, float* dy, float* dz) {
    const float z = 1.0f - 2.0f * x1;
    const float r = rt_sqrt(rt_fmax(0.0f, 1.0f - z * z));
    const float phi = 2 * RT_PI_F * x2;
    float sp, cp;
    rt_sincos(phi, &sp, &cp);
    *dx = r * cp;
    *dy = r * sp;
    *dz = z;
}

/* the sun shadow ray's weight at a medium vertex: the isotropic phase function 1 / (4 pi) in the convention in which a diffuse
 * surface's |cos theta| stands for Lambert's cos theta / pi times pi */
#define FOG_PHASE_WEIGHT 0.25f

#endif /* CHUNKY_FOG_SPEC_H */
