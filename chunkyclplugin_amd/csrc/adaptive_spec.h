/* adaptive_spec.h — the arithmetic of adaptive sampling (include/chunky_hip.h, "adaptive sampling"), compiled
 * by the kernels (adaptive.hip) and by the host (adaptive_host.cpp chunky_adaptive_host) from this one text.
 *
 * Every operation below is one exactly rounded float operation (+, -, *, /, a conversion of a small integer, a comparison); the
 * translation units that include this header are compiled with -ffp-contract=off, so no multiply-add pair is fused, and the
 * device and the host produce the same bits. */
#pragma once
#include "rt_math.h"

/* running mean of K/rayTracer.cl:109-112 for the sample of pass `spp` (counted from 0): fold_kernel's operations */
RT_FN float ad_mean(float mean, float sample, int spp) { return (mean * (float)spp + sample) / (float)(spp + 1); }

/* luminance of a sample (Rec. 709 weights as floats) */
RT_FN float ad_luma(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }

/* Welford's update of (m, M2) with the luminance y of pass k (counted from 0) */
RT_FN void ad_welford(float y, int k, float* m, float* M2) {
    const float d = y - *m;
    *m = *m + d / (float)(k + 1);
    *M2 = *M2 + d * (y - *m);
}

RT_FN int ad_finite(float v) { return rt_fabs(v) < rt_inf(); } /* false for NaN */

/* The convergence test after n passes: 1 when the pixel is unconverged.  t2 = threshold * threshold (one float product, made on the
 * host).  A pixel whose m or M2 is not finite is converged. */
RT_FN int ad_unconverged(float m, float M2, int n, float t2, float floor_) {
    if (!ad_finite(m) || !ad_finite(M2)) return 0;
    const float b = m > floor_ ? m : floor_;
    const float lim = ((t2 * ((float)n * (float)(n - 1))) * b) * b;
    return M2 > lim;
}

/* 1 when a check is due after n passes: n = min_spp + j * check_interval for an integer j >= 0, and n < max_spp (a check after the
 * last pass could change nothing: every pixel still active records max_spp either way) */
RT_FN int ad_check_due(int n, int min_spp, int check_interval, int max_spp) {
    return n >= min_spp && n < max_spp && (n - min_spp) % check_interval == 0;
}

/* ---- continuing a run (include/chunky_hip.h, "adaptive sampling that stops and continues").  The check points are the grid
 * min_spp + j * check_interval, j >= 0. */

/* the largest grid point <= n, 0 when there is none */
RT_FN int ad_grid_floor(int n, int min_spp, int check_interval) {
    return n < min_spp ? 0 : n - (n - min_spp) % check_interval;
}

/* the grid point before the grid point g, 0 when g is the first */
RT_FN int ad_grid_before(int g, int min_spp, int check_interval) { return g - check_interval >= min_spp ? g - check_interval : 0; }

/* 1 when n is a grid point */
RT_FN int ad_on_grid(int n, int min_spp, int check_interval) { return n >= min_spp && (n - min_spp) % check_interval == 0; }

/* One step of the loop, for a state of `passes` passes whose last check ran at `last_check` (0 = none yet), towards max_spp:
 *   check_first  1 when the check at `passes` is due under this max_spp and has not been run — the run that stopped here ended on its
 *                own max_spp, where no check is made.  The caller runs it, sets last_check = passes and asks again.
 *   round        otherwise the passes of the next round: up to the next grid point or to max_spp, whichever comes first (a state off
 *                the grid takes a short round); 0 when passes >= max_spp.  The round's check is due iff ad_check_due(passes + round).
 * From the empty state (0, 0) this is the loop of a single run: min_spp passes, then check_interval at a time. */
typedef struct ad_step_t {
    int check_first, round;
} ad_step_t;

RT_FN ad_step_t ad_step(int passes, int last_check, int min_spp, int check_interval, int max_spp) {
    ad_step_t s;
    s.check_first = ad_check_due(passes, min_spp, check_interval, max_spp) && last_check != passes;
    s.round = 0;
    if (s.check_first || passes >= max_spp) return s;
    const int left = max_spp - passes; /* (distances, not end points: no sum here can pass INT_MAX) */
    const int to_grid = passes < min_spp ? min_spp - passes : check_interval - (passes - min_spp) % check_interval;
    s.round = to_grid < left ? to_grid : left;
    return s;
}
