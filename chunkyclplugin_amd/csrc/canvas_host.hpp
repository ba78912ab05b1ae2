// canvas_host.hpp — the device-free checks of chunky_render_set_canvas (canvas_host.cpp).  Plain C++: no HIP type.
#pragma once
#include <cstdint>

#pragma GCC visibility push(hidden)
// CHUNKY_OK when a width x height target may be the window at (x0, y0) of a canvas_width x canvas_height canvas under a camera of
// projector_type (any value set_camera takes; only CHUNKY_PROJ_ODS_STACKED matters: an even canvas height), else CHUNKY_E_INVALID
// with the reason as the thread's last error
int check_canvas(const char* who, int width, int height, int canvas_width, int canvas_height, int x0, int y0, int projector_type);
#pragma GCC visibility pop
