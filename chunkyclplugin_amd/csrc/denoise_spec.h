/* denoise_spec.h — the per-pixel arithmetic of the edge-avoiding À-Trous denoiser (Dammertz et al. 2010), defined once for the
 * host loop (denoise_host.cpp chunky_denoise_host) and the kernels (denoise.hip), in the role camera_proj.h plays for the cameras.
 *
 * Everything here is made of exactly rounded binary32 operations (+ - * / rint, fma only where written as rt_fma), compiled with
 * -ffp-contract=off on both sides, so a pixel has the same bits wherever it is evaluated and however its taps are fetched.
 *
 * Inputs per pixel: colour C, albedo A, normal N (3 floats each).  With eps = 2^-10 and m = max(A, eps) per channel:
 *   demodulate   D0 = C / m                     (flag bit 0; otherwise D0 = C)
 *   iteration i  step s = 1 << i, taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner, taps outside the image skipped;
 *                h = k[|dx|] k[|dy|], k = {3/8, 1/4, 1/16};  dc, dn, da = sums over channels of squared differences of D, N, A;
 *                x = (dc c_i + dn c_n) + da c_a;  w = h dn_exp(x);  a tap whose D(q) has a non-finite channel, or whose x is not
 *                finite, has weight 0;  D'(p) = (sum w D(q)) / (sum w), sums in tap order;  D'(p) = D(p) when D(p) has a non-finite
 *                channel or sum w = 0
 *   remodulate   out = D m                      (flag bit 0)
 * and two rules that keep one bad pixel from spreading and the result independent of NaN payloads: a pixel whose input colour has a
 * non-finite channel comes back as its input colour, bit for bit; any other NaN in the output is the canonical quiet NaN.
 */
#ifndef CHUNKY_DENOISE_SPEC_H
#define CHUNKY_DENOISE_SPEC_H

#include "rt_math.h"

#define DN_EPS 0x1p-10f
#define DN_MAX_ITERATIONS 8

RT_FN int dn_finite(float v) { return rt_fabs(v) < rt_inf(); } /* false for NaN */
RT_FN int dn_finite3(const float* v) { return dn_finite(v[0]) & dn_finite(v[1]) & dn_finite(v[2]); }

/* e^(-x) for x >= 0 (x beyond 128 counts as 128: the result is 0 from 103.98 on).  k = rint(-x log2 e), r = -x - k ln 2 in two
 * parts (k C1 is exact: C1 has 9 significant bits, |k| < 2^8), e^r = 1 + r + r^2 P(r) on |r| <= ln2 / 2 (the Cephes expf
 * polynomial), then 2^k through the exponent bits in two factors so that a subnormal result is rounded once, by the last
 * multiplication.  dn_exp(0) = 1 exactly; never negative, never NaN; at most 1 ULP from e^(-x) (tests/test_denoise_cpu.py). */
RT_FN float dn_exp(float x) {
    const float t = -rt_fmin(x, 128.0f);
    const float kf = rt_rint(t * 1.44269504088896341f);
    float r = rt_fma(kf, -0.693359375f, t);
    r = rt_fma(kf, 2.12194440e-4f, r);
    const float z = r * r;
    float p = rt_fma(r, 1.9875691500e-4f, 1.3981999507e-3f);
    p = rt_fma(p, r, 8.3334519073e-3f);
    p = rt_fma(p, r, 4.1665795894e-2f);
    p = rt_fma(p, r, 1.6666665459e-1f);
    p = rt_fma(p, r, 5.0000001201e-1f);
    const float y = rt_fma(p, z, r) + 1.0f;
    const int k = (int)kf;       /* -185 .. 0 */
    const int k1 = k >> 1;       /* floor(k / 2) */
    const int k2 = k - k1;
    return (y * rt_u2f((unsigned)(k1 + 127) << 23)) * rt_u2f((unsigned)(k2 + 127) << 23);
}

RT_FN float dn_guard(float a) { return rt_fmax(a, DN_EPS); } /* max(A, eps); a NaN albedo counts as eps */

/* One pixel of one iteration.  F.load(x, y, d, n, a) delivers D, N and A of pixel (x, y) — from planar images, packed words or a
 * tile, which changes no bit.  (px, py) lies inside the image. */
template <class Fetch>
RT_FN void dn_filter_pixel(const Fetch& F, int px, int py, int width, int height, int step, float c_i, float c_n, float c_a, float* out) {
    float dp[3], np[3], ap[3];
    F.load(px, py, dp, np, ap);
    float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = py + step * dy;
        if (qy < 0 || qy >= height) continue;
        const float ky = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = px + step * dx;
            if (qx < 0 || qx >= width) continue;
            const float kx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
            const float h = kx * ky; /* exact: 9, 6, 4, 3/2, 1 or 1/4 over 64 */
            float dq[3], nq[3], aq[3];
            F.load(qx, qy, dq, nq, aq);
            const float e0 = dq[0] - dp[0], e1 = dq[1] - dp[1], e2 = dq[2] - dp[2];
            const float f0 = nq[0] - np[0], f1 = nq[1] - np[1], f2 = nq[2] - np[2];
            const float g0 = aq[0] - ap[0], g1 = aq[1] - ap[1], g2 = aq[2] - ap[2];
            const float dc = (e0 * e0 + e1 * e1) + e2 * e2;
            const float dn = (f0 * f0 + f1 * f1) + f2 * f2;
            const float da = (g0 * g0 + g1 * g1) + g2 * g2;
            const float x = (dc * c_i + dn * c_n) + da * c_a;
            const int ok = dn_finite3(dq) & dn_finite(x);
            const float w = ok ? h * dn_exp(ok ? x : 0.0f) : 0.0f;
            sw = sw + w;
            s0 = s0 + w * (ok ? dq[0] : 0.0f);
            s1 = s1 + w * (ok ? dq[1] : 0.0f);
            s2 = s2 + w * (ok ? dq[2] : 0.0f);
        }
    }
    const int keep = !dn_finite3(dp) || !(sw > 0.0f);
    out[0] = keep ? dp[0] : s0 / sw;
    out[1] = keep ? dp[1] : s1 / sw;
    out[2] = keep ? dp[2] : s2 / sw;
}

/* D0 of a pixel */
RT_FN void dn_demodulate(const float* c, const float* a, int demodulate, float* d) {
    d[0] = demodulate ? c[0] / dn_guard(a[0]) : c[0];
    d[1] = demodulate ? c[1] / dn_guard(a[1]) : c[1];
    d[2] = demodulate ? c[2] / dn_guard(a[2]) : c[2];
}

/* the output of a pixel from its last D, its albedo and its input colour c */
RT_FN void dn_finish(const float* d, const float* a, const float* c, int demodulate, float* out) {
    const int pass = !dn_finite3(c);
    for (int k = 0; k < 3; k++) {
        float v = demodulate ? d[k] * dn_guard(a[k]) : d[k];
        v = v != v ? rt_nan() : v;
        out[k] = pass ? c[k] : v;
    }
}

/* the coefficients of iteration i, computed once on the host in float: c_i = 4^i / sigma_color^2 (the colour sigma halves each
 * iteration), c_n = 1 / sigma_normal^2, c_a = 1 / sigma_albedo^2 */
struct DnCoeffs {
    int iterations, demodulate;
    float c_i[DN_MAX_ITERATIONS], c_n, c_a;
};
static inline int dn_coeffs(int iterations, float sigma_color, float sigma_normal, float sigma_albedo, int demodulate, DnCoeffs* k) {
    k->iterations = iterations;
    k->demodulate = demodulate;
    k->c_n = 1.0f / (sigma_normal * sigma_normal);
    k->c_a = 1.0f / (sigma_albedo * sigma_albedo);
    int ok = k->c_n > 0.0f && k->c_n < __builtin_inff() && k->c_a > 0.0f && k->c_a < __builtin_inff();
    for (int i = 0; i < DN_MAX_ITERATIONS; i++) {
        k->c_i[i] = (float)(1 << (2 * i)) / (sigma_color * sigma_color);
        if (i < iterations) ok = ok && k->c_i[i] > 0.0f && k->c_i[i] < __builtin_inff();
    }
    return ok;
}

#endif /* CHUNKY_DENOISE_SPEC_H */
