// glass_host.hpp — the device-free part of translucent blocks (chunky_render_set_translucency): what a target keeps
// of the setting and the check of a caller's chunky_translucency (glass_host.cpp).  Plain C++: no HIP type.
#pragma once
#include <cstddef>
#include <cstdint>

struct chunky_translucency;  // include/chunky_hip.h

#pragma GCC visibility push(hidden)
// a target's setting; off (the default): every hit is opaque, as in the reference
struct GlassSettings {
    bool enabled = false;
    float opaque_alpha = 0.99f;
    int max_crossings = 8;
    bool on() const { return enabled; }
};
// CHUNKY_OK and *out (when not NULL) the setting `t` asks for — off for NULL — else CHUNKY_E_INVALID with the reason as the thread's
// last error and *out untouched: a size that is neither this header's, nor larger with nothing but zero bytes behind it; opaque_alpha
// outside (0, 1] or not a number; max_crossings outside [1, 31]
int check_translucency(const char* who, const chunky_translucency* t, GlassSettings* out);
#pragma GCC visibility pop
