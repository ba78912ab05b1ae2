// lane_kernels.hpp — the kernels that bind one path to one lane and walk it as K/rayTracer.cl writes it (path_state.hpp sample_path,
// closest_hit): render_lanes (render_fallback.hip: one lane owns one pixel for all the passes of a launch), trace_records_kernel and
// preview_lanes (aux_kernels.hip).  Templates only: each of those units instantiates its own, and render_biome.hip instantiates all
// three once more with CHUNKY_BIOME_TINT (rt_device.hpp), where CHUNKY_KERNEL_ARGS_HEAD puts the biome map ahead of their arguments.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#pragma once
#include "path_state.hpp"

namespace chunky {

template <int TREE>
__global__ void __launch_bounds__(256) render_lanes(CHUNKY_KERNEL_ARGS_HEAD SceneView S, CameraView C, RenderOpts O, ShardView T, PassSeeds P,
                                                     float* __restrict__ res) {
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= T.n_local) return;
    int gid = shard_gid(T, local);
    if (gid >= C.width * C.height) return;
    float* px = res + 3 * (size_t)gid;
    f3 mean = mk3(px[0], px[1], px[2]);
    for (int k = 0; k < P.n; k++) {
        f3 c = sample_path<false, TREE>(S, C, O, P.seed[k], gid, stack, nullptr, nullptr);
        int spp = P.first_spp + k;
        float fs = (float)spp, fs1 = (float)(spp + 1);
        mean = f3{(mean.x * fs + c.x) / fs1, (mean.y * fs + c.y) / fs1, (mean.z * fs + c.z) / fs1};
    }
    px[0] = mean.x;
    px[1] = mean.y;
    px[2] = mean.z;
}

template <int TREE>
__global__ void __launch_bounds__(256) trace_records_kernel(CHUNKY_KERNEL_ARGS_HEAD SceneView S, CameraView C, RenderOpts O, int seed,
                                                             const int* __restrict__ gids, int n,
                                                             HitRecord* __restrict__ out, int* __restrict__ counts,
                                                             float* __restrict__ radiance) {
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    HitRecord local[kMaxTraces];
    int cnt = 0;
    f3 c = sample_path<true, TREE>(S, C, O, seed, gids[i], stack, local, &cnt);
    for (int k = 0; k < cnt; k++) out[(size_t)i * kMaxTraces + k] = local[k];
    counts[i] = cnt;
    radiance[3 * i] = c.x;
    radiance[3 * i + 1] = c.y;
    radiance[3 * i + 2] = c.z;
}

// preview — K/rayTracer.cl:115-217
template <int TREE>
__global__ void __launch_bounds__(256) preview_lanes(CHUNKY_KERNEL_ARGS_HEAD SceneView S, CameraView C, RenderOpts O, int* __restrict__ argb) {
    extern __shared__ int lds[];
    LdsStack stack{lds + threadIdx.x, (int)blockDim.x};
    int gid = blockIdx.x * blockDim.x + threadIdx.x;
    int W = C.width, H = C.height;
    if (gid >= W * H) return;
    // the crosshair is the canvas's (K/rayTracer.cl:146-150 on the canvas pixel and the canvas's size; a target that is no window: its own)
    const CanvasPixel cp = canvas_pixel(C, gid);
    const int px = cp.X, py = cp.Y;
    W += C.row_skip, H = C.canvas_height;
    if ((px == W / 2 && (py >= H / 2 - 5 && py <= H / 2 + 5)) || (py == H / 2 && (px >= W / 2 - 5 && px <= W / 2 + 5))) {
        argb[gid] = (int)0xFFFFFFFFu;
        return;
    }
    unsigned rng = 0;
    rt_pcg_next(&rng);
    const RayOD pr = primary_ray_any(C, 0u, gid, cp, rng, true);  // a projected camera: the rays of seed 0
    const f3 o = pr.o, d = pr.d;
    Hit h;
    h.distance = rt_inf();
    h.material = 0;
    h.normal = mk3(0, 0, 0);
    h.color = f4{0, 0, 0, 0};
    h.emittance = 0;
    f3 point;
    f4 c;
    if (closest_hit<TREE>(S, o, d, O.draw_depth, h, point, stack)) {
        float shading = dot(h.normal, mk3(0.25f, 0.866f, 0.433f));
        shading = rt_fmax(0.3f, shading);
        c = f4{h.color.x * shading, h.color.y * shading, h.color.z * shading, 0};
    } else {
        c = sky_color(S, d);
        sun_disc(S, d, c);
    }
    int r = (int)rt_floor(rt_clamp(rt_sqrt(c.x) * 255.0f, 0.0f, 255.0f));
    int g = (int)rt_floor(rt_clamp(rt_sqrt(c.y) * 255.0f, 0.0f, 255.0f));
    int b = (int)rt_floor(rt_clamp(rt_sqrt(c.z) * 255.0f, 0.0f, 255.0f));
    argb[gid] = (int)(0xFF000000u | ((unsigned)r << 16) | ((unsigned)g << 8) | (unsigned)b);
}

}  // namespace chunky
