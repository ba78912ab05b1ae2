// aov_biome.hip — the biome-tint instantiations of the AOV and AOV-ex first-hit kernels (launch_aov_biome, launch_aov_ex_biome): aov.hip
// again, compiled with CHUNKY_BIOME_TINT (rt_device.hpp) — the kernels take the scene's biome map as their first argument and tint
// grass, foliage and water by the block test's cell, so the albedo a denoiser is guided by is the albedo the beauty pass renders.
#define CHUNKY_BIOME_TINT 1
#include "aov.hip"
