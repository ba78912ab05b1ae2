/* canvas_window.h — a render target as a window of a larger canvas (chunky_render_set_canvas).  Plain C: the
 * kernels (rt_device.hpp canvas_pixel), the host twin of the projected cameras (capi_host.cpp) and the device-free checker
 * (canvas_host.cpp) share the one definition of where a window pixel lies on its canvas.
 *
 * A target of width x height at (x0, y0) of a canvas_width x canvas_height canvas: window pixel (px, py), local index
 * g = py * width + px, is canvas pixel (X, Y) = (x0 + px, y0 + py), canvas index G = Y * canvas_width + X.  With
 * row_skip = canvas_width - width and gid0 = y0 * canvas_width + x0 that is G = g + py * row_skip + gid0: integers throughout (an
 * offset is never folded into a float), and nothing leaves an int for a window inside a canvas of at most INT32_MAX pixels —
 * py * row_skip < canvas_width * canvas_height, and G is a pixel of the canvas.  The identity window (canvas == target, offsets 0)
 * has row_skip = gid0 = x0 = y0 = 0: G = g, X = px, Y = py. */
#ifndef CHUNKY_CANVAS_WINDOW_H
#define CHUNKY_CANVAS_WINDOW_H

#include "rt_math.h"

typedef struct {
    int x0, y0;        /* the window's corner on the canvas */
    int row_skip;      /* canvas_width - width */
    int gid0;          /* y0 * canvas_width + x0: the canvas index of window pixel (0, 0) */
    int canvas_height; /* (the canvas's width reaches the kernels in half_width alone) */
} RtWindow;

typedef struct {
    int G, X, Y;
} RtCanvasPixel;

RT_FN RtCanvasPixel rt_canvas_pixel(int g, int px, int py, int x0, int y0, int row_skip, int gid0) {
    RtCanvasPixel p;
    p.G = g + py * row_skip + gid0;
    p.X = px + x0;
    p.Y = py + y0;
    return p;
}

/* the fields of a window the checker has accepted (canvas_host.cpp check_canvas) */
RT_FN RtWindow rt_make_window(int width, int canvas_width, int canvas_height, int x0, int y0) {
    RtWindow w;
    w.x0 = x0;
    w.y0 = y0;
    w.row_skip = canvas_width - width;
    w.gid0 = y0 * canvas_width + x0;
    w.canvas_height = canvas_height;
    return w;
}

#endif /* CHUNKY_CANVAS_WINDOW_H */
