// render_pool_fog.hip — the ground-fog instantiations of render_pool without entity BVHs (render_pool.hip pool_kernel_fog): that file
// again with CHUNKY_FOG (rt_device.hpp) — the layer's parameters head the kernels' arguments, and the extended integrator's SHADE
// (shade_phase_ext) draws a free flight at the end of every main-ray trace (fog_spec.h).  Address forms and march
// as the plain kernels' (CHUNKY_ADDR32_FORMS 7).
#define CHUNKY_FOG 1
#include "render_pool.hip"
