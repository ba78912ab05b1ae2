// render_pool_fog_bvh.hip — the ground-fog instantiations of render_pool with entity BVHs (render_pool.hip pool_kernel_fog_bvh):
// render_pool_bvh.hip's setting (the compiler's divisions and roots, 64-bit addresses for every scene array) with CHUNKY_FOG.
#define CHUNKY_FOG 1
#define CHUNKY_IEEE_FORMS 1
#define CHUNKY_POOL_BVH_TU 1
#include "render_pool.hip"
