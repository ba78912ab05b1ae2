// render_pool_glass_bvh.hip — the instantiations of render_pool with translucent blocks and entity BVHs (render_pool.hip
// pool_kernel_glass_bvh): render_pool_bvh.hip's setting (the compiler's divisions and roots, 64-bit addresses for every scene array)
// with CHUNKY_GLASS.
#define CHUNKY_GLASS 1
#define CHUNKY_IEEE_FORMS 1
#define CHUNKY_POOL_BVH_TU 1
#include "render_pool.hip"
