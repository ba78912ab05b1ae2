// fog_host.hpp — the device-free part of the ground-fog layer (chunky_render_set_fog): what a target keeps of it
// and the check of a caller's chunky_fog (fog_host.cpp).  Plain C++: no HIP type.
#pragma once
#include <cstddef>
#include <cstdint>

struct chunky_fog;  // include/chunky_hip.h

#pragma GCC visibility push(hidden)
// a target's layer; density 0: fog is off (the default)
struct FogSettings {
    float density = 0.0f, y_min = 0.0f, y_max = 0.0f;
    float color[3] = {0.0f, 0.0f, 0.0f};
    bool on() const { return density > 0.0f; }
};
// CHUNKY_OK and *out (when not NULL) the layer `fog` asks for — off for NULL or density 0 — else CHUNKY_E_INVALID with the reason as
// the thread's last error and *out untouched: a size that is neither this header's, nor larger with nothing but zero bytes behind it;
// a non-finite member; density < 0; y_min >= y_max; a colour component outside [0, 1]
int check_fog(const char* who, const chunky_fog* fog, FogSettings* out);
#pragma GCC visibility pop
