// render_pool_biome.hip — the biome-tint instantiations of render_pool without entity BVHs (render_pool.hip pool_kernel_biome): that file
// again with CHUNKY_BIOME_TINT (rt_device.hpp) — the scene's biome map heads the kernels' arguments, and a block's material of tint type
// 1, 2 or 3 multiplies by the colour of the block test's cell.  Address forms and march as the plain kernels' (CHUNKY_ADDR32_FORMS 7).
#define CHUNKY_BIOME_TINT 1
#include "render_pool.hip"
