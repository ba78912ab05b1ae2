// render_pool_glass.hip — the instantiations of render_pool with translucent blocks, without entity BVHs (render_pool.hip
// pool_kernel_glass): that file again with CHUNKY_GLASS (rt_device.hpp) — the two parameters head the kernels' arguments, the march steps
// through the run a ray is inside (path_state.hpp march_step), the extended integrator's SHADE (shade_phase_ext) lets a ray cross a
// translucent hit (glass_spec.h), and a parked path is twelve words.  Address forms as the plain kernels'
// (CHUNKY_ADDR32_FORMS 7).
#define CHUNKY_GLASS 1
#include "render_pool.hip"
