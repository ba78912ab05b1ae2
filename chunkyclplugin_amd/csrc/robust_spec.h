/* robust_spec.h — the arithmetic of firefly-robust accumulation (include/chunky_hip.h, "firefly-robust accumulation"; DESIGN.md
 * section 20), compiled by the kernels (robust.hip) and by the host (robust_host.cpp) from this one text.
 *
 * The method is a median of means with an adaptive trim.  The idea follows Buisine, Delepoulle and Renaud, "Firefly removal in Monte
 * Carlo rendering with adaptive Median of meaNs" (2021); the formulas below are this project's own specification, written without
 * that paper at hand, and do not claim to reproduce it.
 *
 * Every operation below is one exactly rounded float operation (+, *, /, a conversion of a small integer, a comparison, the
 * truncation of a float in [0, 7) to int); the translation units that include this header are compiled with -ffp-contract=off, so
 * no multiply-add pair is fused, and the device and the host produce the same bits.
 *
 * M, the number of buckets, is a template argument (odd, 3 .. 15; h = (M - 1) / 2): every loop is fully unrolled and every index
 * into the M values is a constant, so that on the device the values stay in registers. */
#pragma once
#include "adaptive_spec.h" /* ad_mean: the running mean a bucket is updated with */

#define RB_MODE_MEAN 0   /* CHUNKY_ROBUST_MEAN:   t = 0, the mean of the bucket means */
#define RB_MODE_MEDIAN 1 /* CHUNKY_ROBUST_MEDIAN: t = h, the median of the bucket means */
#define RB_MODE_GINI 2   /* CHUNKY_ROBUST_GINI:   t from the Gini coefficient of the bucket means */
#define RB_MIN_BUCKETS 3
#define RB_MAX_BUCKETS 15

#if defined(__clang__)
#define RB_UNROLL _Pragma("unroll")
#else
#define RB_UNROLL _Pragma("GCC unroll 16")
#endif

/* 1 for a bucket count the specification takes */
RT_FN int rb_buckets_ok(int m) { return m >= RB_MIN_BUCKETS && m <= RB_MAX_BUCKETS && (m & 1) == 1; }

/* Robust sample j (counted from 0 since the state began) goes to bucket j % M as that bucket's sample j / M:
 * mean_b = ad_mean(mean_b, s, j / M). */

/* Ascending sort by the fixed odd-even transposition network: rounds r = 0 .. M - 1, round r compares the pairs (i, i + 1) for
 * i = r & 1, (r & 1) + 2, ...; a pair is swapped iff x[i + 1] < x[i].  A NaN never swaps: the order is then defined but arbitrary. */
template <int M>
RT_FN void rb_sort(float (&x)[M]) {
    RB_UNROLL
    for (int r = 0; r < M; r++) {
        RB_UNROLL
        for (int i = r & 1; i + 1 < M; i += 2) {
            const float a = x[i], b = x[i + 1];
            const bool swap = b < a;
            x[i] = swap ? b : a;
            x[i + 1] = swap ? a : b;
        }
    }
}

/* The Gini coefficient of the sorted values: S = x0 + x1 + ..., W = sum (2 i - M + 1) x_i, both added left to right;
 * G = W / (M S) where 0 < S < inf, else 0 (a NaN in S gives 0). */
template <int M>
RT_FN float rb_gini(const float (&x)[M]) {
    float S = x[0];
    float W = (float)(1 - M) * x[0];
    RB_UNROLL
    for (int i = 1; i < M; i++) {
        S = S + x[i];
        W = W + (float)(2 * i - M + 1) * x[i];
    }
    return (S > 0.0f && S < rt_inf()) ? W / ((float)M * S) : 0.0f;
}

/* Values trimmed from each end, 0 .. h */
template <int M>
RT_FN int rb_trim(float G, int mode, float gain) {
    const int h = (M - 1) / 2;
    if (mode == RB_MODE_MEAN) return 0;
    if (mode == RB_MODE_MEDIAN) return h;
    const float p = (G * (float)(h + 1)) * gain;
    return !(p > 0.0f) ? 0 : (p >= (float)h ? h : (int)p);
}

/* (x_t + x_{t+1} + ... + x_{M-1-t}) / (float)(M - 2 t), added left to right (constant indices: the sum is selected, not indexed) */
template <int M>
RT_FN float rb_trimmed_mean(const float (&x)[M], int t) {
    float acc = x[0];
    RB_UNROLL
    for (int i = 1; i < M; i++) acc = i == t ? x[i] : ((i > t && i <= M - 1 - t) ? acc + x[i] : acc);
    return acc / (float)(M - 2 * t);
}

/* The resolve of one channel of one pixel: x holds its M bucket means in any order and is sorted in place; *t_out receives the trim */
template <int M>
RT_FN float rb_resolve(float (&x)[M], int mode, float gain, int* t_out) {
    rb_sort<M>(x);
    const int t = rb_trim<M>(rb_gini<M>(x), mode, gain);
    *t_out = t;
    return rb_trimmed_mean<M>(x, t);
}
