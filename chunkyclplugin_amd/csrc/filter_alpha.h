/* filter_alpha.h — the alpha byte of chunky_filter_frame_alpha: min(255, (uint)(clamp(a, 0, 1) * 255.0f + 0.5f)), 0 for a NaN.  One
 * definition for both sides: filter_alpha_kernel (filter.hip) and the host instrument chunky_filter_alpha_bytes (capi_host.cpp)
 * compile it, both without FMA contraction. */
#ifndef CHUNKY_FILTER_ALPHA_H
#define CHUNKY_FILTER_ALPHA_H

#include "rt_math.h"

RT_FN unsigned rt_alpha_byte(float a) {
    a = a > 0.0f ? (a < 1.0f ? a : 1.0f) : 0.0f; /* a NaN fails the first comparison: 0 */
    const unsigned u = (unsigned)(a * 255.0f + 0.5f); /* in [0.5, 255.5]: the cast is defined */
    return u > 255u ? 255u : u;
}

#endif /* CHUNKY_FILTER_ALPHA_H */
