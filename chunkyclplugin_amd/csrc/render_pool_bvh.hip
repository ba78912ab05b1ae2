// render_pool_bvh.hip — the entity-BVH instantiations of render_pool (render_pool.hip pool_kernel_bvh), compiled with the compiler's own
// divisions and square roots in place of the short exact forms of rt_short_forms.h, and (CHUNKY_POOL_BVH_TU) with 64-bit addresses for
// every scene array.  Same results bit for bit; these kernels, whose time goes to the BVH walk, were measurably slower with the short
// forms in the code around it (EXPERIMENTS 7.3), so they keep the code they had (7.4).
#define CHUNKY_IEEE_FORMS 1
#define CHUNKY_POOL_BVH_TU 1
#include "render_pool.hip"
