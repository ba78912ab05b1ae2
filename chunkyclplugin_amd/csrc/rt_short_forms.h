/* rt_short_forms.h — device-only short forms of `1.0f / x`, `sqrtf(x)` and `x / constant` for gfx950.
 *
 * The compiler's IEEE expansions carry the scaling that denormal operands and results need (v_div_scale / v_div_fmas /
 * v_div_fixup: 11 VALU for a division; a scale-up test, scale-down and class select around the root's residual test: 15 VALU),
 * on every execution.  Here a lane whose operand is inside a range takes the unscaled core of the same computation — the
 * hardware's 1-ulp estimate, then one residual correction with fused multiply-adds — and a wave in which ANY lane is outside the
 * range takes the compiler's operation for all of its lanes, behind a wave-uniform branch, so the usual path holds no expansion.
 *
 * Nothing here is argued to be exact: the sweeps of math_selftest_kernel (aux_kernels.hip, `which` 40-43;
 * tests/test_gpu_exact_divsqrt.py) compare each form on the device with the compiled operation for all 2^32 bit patterns of x,
 * NaNs included, and find no difference.
 *
 * CHUNKY_IEEE_FORMS, defined by a translation unit ahead of every include, makes the four entry points (rcp_exact, rcp_exact3,
 * rt_sqrt_short, rt_div_const) the compiler's operations again, on every path: the results are the same bit for bit, the code is the
 * code from before these forms.  render_pool_bvh.hip sets it: the entity-BVH kernels, which spend their time in the BVH walk, were
 * measurably slower with the short forms around it (EXPERIMENTS 7.3).
 *
 * Read by HIP translation units only (rt_math.h includes it under __HIPCC__ and calls it under __HIP_DEVICE_COMPILE__): the host
 * checkers and the oracle's build never see this file, and host code never runs it.
 */
#ifndef CHUNKY_RT_SHORT_FORMS_H
#define CHUNKY_RT_SHORT_FORMS_H

#define RT_SHORT static __device__ inline __attribute__((always_inline))

RT_SHORT unsigned rt_bits(float f) { return __builtin_bit_cast(unsigned, f); }
/* true when any lane of the wave that is executing holds `p` */
RT_SHORT bool rt_any_lane(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }
/* The operand of a slow path goes through this first: an empty volatile statement cannot be executed speculatively, so the compiler
 * keeps the branch around the expansion (without it, it computes both forms on every execution and selects). */
RT_SHORT float rt_slow_operand(float x) {
    asm volatile("; chunky-mark exact-slow-path" : "+v"(x));
    return x;
}

/* ---- 1.0f / x ----------------------------------------------------------------------------------------------------------------
 * In range: 2^-126 <= |x| < 2^126 (x and 1/x both normal; 0, denormals, infinities and NaNs fail one of the two compares).
 * y = v_rcp(x), then one residual correction y += y * (1 - x * y).
 * (The test compares floats, |x| as a source modifier: the same test on the bit pattern needs a register for the shifted pattern,
 * and in render_pool<17, 64>, which stands at its limit of 80, that one register cost seven spilled ones.) */
RT_SHORT bool rt_rcp_outside(float x) { return !(__builtin_fabsf(x) >= 0x1p-126f && __builtin_fabsf(x) < 0x1p126f); }
RT_SHORT float rt_rcp_core(float x) {
    const float y = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, y, 1.0f);
    return __builtin_fmaf(y, e, y);
}
/* == 1.0f / x for every bit pattern of x */
RT_SHORT float rcp_exact(float x) {
#ifdef CHUNKY_IEEE_FORMS
    return 1.0f / x;
#endif
    float y = rt_rcp_core(x);
    if (rt_any_lane(rt_rcp_outside(x))) y = 1.0f / rt_slow_operand(x);
    return y;
}
/* three at once, one merged test and one slow path */
RT_SHORT void rcp_exact3(float x, float y, float z, float* rx, float* ry, float* rz) {
#ifdef CHUNKY_IEEE_FORMS
    *rx = 1.0f / x;
    *ry = 1.0f / y;
    *rz = 1.0f / z;
    return;
#endif
    float a = rt_rcp_core(x), b = rt_rcp_core(y), c = rt_rcp_core(z);
    if (rt_any_lane(rt_rcp_outside(x) || rt_rcp_outside(y) || rt_rcp_outside(z))) {
        a = 1.0f / rt_slow_operand(x);
        b = 1.0f / rt_slow_operand(y);
        c = 1.0f / rt_slow_operand(z);
    }
    *rx = a;
    *ry = b;
    *rz = c;
}

/* ---- sqrtf(x) ----------------------------------------------------------------------------------------------------------------
 * In range: 2^-96 <= x <= the largest finite float (positive, normal, and far enough from the denormals that the residual
 * x - s * s is exact: the compiler's own form scales up below 2^-96), tested on the bit pattern with one unsigned compare.
 * s = v_sqrt(x), h = v_rsq(x) / 2, then one correction s += (x - s * s) * h. */
RT_SHORT bool rt_sqrt_outside(float x) { return rt_bits(x) - 0x0F800000u > 0x6FFFFFFFu; }
/* == __builtin_sqrtf(x) for every bit pattern of x */
RT_SHORT float rt_sqrt_short(float x) {
#ifdef CHUNKY_IEEE_FORMS
    return __builtin_sqrtf(x);
#endif
    float s = __builtin_amdgcn_sqrtf(x);
    const float h = 0.5f * __builtin_amdgcn_rsqf(x);
    const float r = __builtin_fmaf(-s, s, x);
    s = __builtin_fmaf(r, h, s);
    if (rt_any_lane(rt_sqrt_outside(x))) s = __builtin_sqrtf(rt_slow_operand(x));
    return s;
}

/* ---- x / c, c a compile-time constant -------------------------------------------------------------------------------------------
 * In range: 2^-100 <= |x| < 2^100 (the quotient and the residual stay normal for constants between 2^-3 and 2^3; -0, whose
 * residual would come out as +0, is outside).  q = x * rc, r = x - c * q, q += r * rc with rc = RN(1 / c), folded by the
 * compiler.  One sweep per constant (rt_device.hpp kSkyTwoPi, kSunDiscWidth2): no other constant may use this. */
RT_SHORT bool rt_divc_outside(float x) { return !(__builtin_fabsf(x) >= 0x1p-100f && __builtin_fabsf(x) < 0x1p100f); }
RT_SHORT float rt_div_const(float x, const float c) {
#ifdef CHUNKY_IEEE_FORMS
    return x / c;
#endif
    const float rc = 1.0f / c;
    float q = x * rc;
    const float r = __builtin_fmaf(-c, q, x);
    q = __builtin_fmaf(r, rc, q);
    if (rt_any_lane(rt_divc_outside(x))) q = rt_slow_operand(x) / c;
    return q;
}

#endif
