/* glass_spec.h — the arithmetic of translucent blocks (include/chunky_hip.h, "translucent blocks"), compiled by the
 * kernels (render_pool_glass.hip, render_pool_glass_bvh.hip) and by the CPU specification (tests/glass_port.c) from this one text.
 *
 * A hit of colour c and alpha a (Hit::color as material_eval leaves it, after the tint multiply) is TRANSLUCENT when a < opaque_alpha
 * and the ray has crossed fewer than max_crossings translucent hits; a NaN alpha is opaque.  This is the project's own specification;
 * the reference drops alpha behind its test (K/material.h:50-54).
 *
 * Plain C99 over rt_math.h.  Every operation is one exactly rounded binary32 operation (the units that include this header are
 * compiled with -ffp-contract=off).  Every function is total: finite arguments give finite results — a product that would overflow
 * is held at the largest finite number — and no argument, infinite or NaN, gives a NaN. */
#ifndef CHUNKY_GLASS_SPEC_H
#define CHUNKY_GLASS_SPEC_H
#include "rt_math.h"

#define GLASS_OPAQUE_ALPHA_DEFAULT 0.99f /* 0xFF arrives as 255/256 or, tinted, (255/256)^2 = 0.9922: both stay opaque */
#define GLASS_MAX_CROSSINGS_DEFAULT 8
#define GLASS_MAX_CROSSINGS_LIMIT 31 /* the counter has five bits */
#define GLASS_FLT_MAX 3.4028234663852886e38f

/* x, kept finite and a number: NaN -> 0, beyond +-FLT_MAX -> +-FLT_MAX */
RT_FN float glass_finite(float x) {
    if (x != x) return 0.0f;
    return x > GLASS_FLT_MAX ? GLASS_FLT_MAX : (x < -GLASS_FLT_MAX ? -GLASS_FLT_MAX : x);
}

/* is a hit of alpha a translucent for a ray that has crossed `crossings` translucent hits (a NaN compares false: opaque) */
RT_FN int glass_translucent(float a, float opaque_alpha, int crossings, int max_crossings) {
    return (a < opaque_alpha) && (crossings < max_crossings);
}

/* the filter of a main ray that crosses, per channel: (1 - a) + a c — "more paint, more colour" */
RT_FN float glass_tc(float a, float c) { return glass_finite((1.0f - a) + a * c); }

/* the filter of a shadow ray, per channel: (1 - a) tc */
RT_FN float glass_fs(float a, float c) { return glass_finite((1.0f - a) * glass_tc(a, c)); }

/* Where a crossing restarts: p = o + d distance, n_f = the hit normal turned against d (n if dot(d, n) <= 0, else -n),
 * o' = p - n_f (2 kOffset): a step through the surface; a zero normal gives o' = p. */
#define GLASS_RESTART_STEP 0.0002f /* 2 kOffset (K/constants.h:5) */
RT_FN void glass_restart(float ox, float oy, float oz, float dx, float dy, float dz, float distance, float nx, float ny, float nz,
                         float* px, float* py, float* pz) {
    const float s = rt_dot3(dx, dy, dz, nx, ny, nz) <= 0.0f ? GLASS_RESTART_STEP : -GLASS_RESTART_STEP;
    *px = glass_finite((ox + dx * distance) - nx * s);
    *py = glass_finite((oy + dy * distance) - ny * s);
    *pz = glass_finite((oz + dz * distance) - nz * s);
}

#endif /* CHUNKY_GLASS_SPEC_H */
