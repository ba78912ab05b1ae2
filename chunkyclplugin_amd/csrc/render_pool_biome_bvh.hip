// render_pool_biome_bvh.hip — the biome-tint instantiations of render_pool with entity BVHs (render_pool.hip pool_kernel_biome_bvh):
// render_pool_bvh.hip's setting (the compiler's divisions and roots, 64-bit addresses for every scene array) with CHUNKY_BIOME_TINT.
// Entity triangles have no cell: they keep the reference's constant tints.
#define CHUNKY_BIOME_TINT 1
#define CHUNKY_IEEE_FORMS 1
#define CHUNKY_POOL_BVH_TU 1
#include "render_pool.hip"
