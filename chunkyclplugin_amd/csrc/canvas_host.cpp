// canvas_host.cpp — a render target as a window of a larger canvas (chunky_render_set_canvas): what can be
// decided without a device.  Plain C++: no device code, no HIP type.
#include "canvas_host.hpp"

#include "../../include/chunky_hip.h"
#include "canvas_window.h"
#include "capi_error.hpp"

// 64-bit throughout: every argument is a caller's int, and the sums and the product below leave an int long before they are refused
int check_canvas(const char* who, int width, int height, int canvas_width, int canvas_height, int x0, int y0, int projector_type) {
    if (width <= 0 || height <= 0) return fail(CHUNKY_E_INVALID, "%s: bad window size %dx%d", who, width, height);
    if (canvas_width <= 0 || canvas_height <= 0) return fail(CHUNKY_E_INVALID, "%s: bad canvas size %dx%d", who, canvas_width, canvas_height);
    if (x0 < 0 || y0 < 0) return fail(CHUNKY_E_INVALID, "%s: negative offset (%d, %d)", who, x0, y0);
    if ((int64_t)x0 + width > canvas_width || (int64_t)y0 + height > canvas_height)
        return fail(CHUNKY_E_INVALID, "%s: a %dx%d window at (%d, %d) does not lie inside the %dx%d canvas", who, width, height, x0, y0, canvas_width,
                    canvas_height);
    if ((int64_t)canvas_width * canvas_height > INT32_MAX)
        return fail(CHUNKY_E_INVALID, "%s: a %dx%d canvas has more than 2^31 - 1 pixels (a canvas index is an int)", who, canvas_width, canvas_height);
    if (projector_type == CHUNKY_PROJ_ODS_STACKED && canvas_height % 2 != 0)
        return fail(CHUNKY_E_INVALID, "%s: the stacked ODS image needs an even canvas height, got %d", who, canvas_height);
    return CHUNKY_OK;
}

extern "C" int chunky_canvas_check(int width, int height, int canvas_width, int canvas_height, int x0, int y0, int projector_type) {
    return check_canvas("canvas_check", width, height, canvas_width, canvas_height, x0, y0, projector_type);
}

extern "C" int chunky_selftest_canvas_pixel(int width, int height, int canvas_width, int canvas_height, int x0, int y0, int32_t g, int32_t out3[3]) {
    if (int rc = check_canvas("canvas_pixel", width, height, canvas_width, canvas_height, x0, y0, 0)) return rc;
    if (!out3) return fail(CHUNKY_E_INVALID, "canvas_pixel: NULL output");
    if (g < 0 || (int64_t)g >= (int64_t)width * height) return fail(CHUNKY_E_INVALID, "canvas_pixel: index %d outside the window", g);
    const RtWindow w = rt_make_window(width, canvas_width, canvas_height, x0, y0);
    const RtCanvasPixel p = rt_canvas_pixel(g, g % width, g / width, w.x0, w.y0, w.row_skip, w.gid0);
    out3[0] = p.G, out3[1] = p.X, out3[2] = p.Y;
    return CHUNKY_OK;
}
