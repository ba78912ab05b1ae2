// aux_kernels.hip — kernels beside the hot path: trace_records (per-trace hit records for the parity tests), preview
// (K/rayTracer.cl:115-217) and the self tests (rt_math.h contract; helper-level known answers).
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "path_state.hpp"
#include "lane_kernels.hpp"  // trace_records_kernel, preview_lanes
#include "pool_walk.hpp"

namespace chunky {

constexpr int kSweepFirst = 40, kSweepRecord = 60;

// Device evaluation of the rt_math.h contract, compared bit-for-bit with the host by the tests.
__global__ void math_selftest_kernel(int which, int n, const float* __restrict__ a, const float* __restrict__ b,
                                     float* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b[i], r = 0;
    switch (which) {
        case 0: r = rt_sin(x); break;
        case 1: r = rt_cos(x); break;
        case 2: r = rt_asin(x); break;
        case 3: r = rt_acos(x); break;
        case 4: r = rt_atan2(x, y); break;
        case 5: r = rt_fmod1(x); break;
        case 6: r = rt_fmin(x, y); break;
        case 7: r = rt_fmax(x, y); break;
        case 8: r = rt_sqrt(x); break;
        case 9: r = x / y; break;
        case 10: r = rt_rlen3(x, y, x); break;
        case 11: r = rt_dot3(x, y, x, y, x, y); break;
        case 12: r = rt_floor(x); break;
        case 13: r = (float)(int)x; break;
        case 14: r = (float)((double)((unsigned)(int)x & 0xFF) / 255.0); break;
        case 15: r = (float)(-0.5 + (double)(x * y)); break;
        case 16: r = rt_pow(x, y); break;
        case 18: r = (float)floor_to_int(x); break;
        case 17: r = (float)((double)x * (double)y); break;
        // the short exact forms (rt_short_forms.h) and, odd numbers, the compiled IEEE operations they stand for
        case 20: r = rcp_exact(x); break;
        case 21: r = 1.0f / x; break;
        case 22: r = rt_sqrt(x); break;
        case 23: r = __builtin_sqrtf(x); break;
        case 24: r = rt_div_const(x, kSkyTwoPi); break;
        case 25: r = x / kSkyTwoPi; break;
        case 26: r = rt_div_const(x, kSunDiscWidth2); break;
        case 27: r = x / kSunDiscWidth2; break;
        case 28: { const f3 q = rcp3(mk3(x, y, x)); r = (i & 1) ? q.y : q.x; break; }  // (odd rows: 1 / b)
        default: break;
    }
    out[i] = r;
}

// Sweeps (`which` >= kSweepFirst): a short form against the compiled operation over a run of bit patterns, bits compared (NaNs
// included).  a[0] holds the first pattern and b[0] the number of patterns per thread, both as bit patterns; thread i takes
// first + k * n + i for k < count, so that a wave's lanes hold neighbouring patterns, and n * count = 2^32 covers every float once.
// out (as unsigned, zeroed by the launcher): [0] mismatches, [1] mismatches recorded so far, [2 ..] the first kSweepRecord
// mismatching patterns that got a slot.  40-43 are the forms the kernels use, 50 a form that must fail.
template <class NEW, class REF>
DEV void sweep_patterns(int i, int n, unsigned first, unsigned count, unsigned* out, NEW form, REF ieee) {
    unsigned bad = 0;
    for (unsigned k = 0; k < count; ++k) {
        const unsigned u = first + k * (unsigned)n + (unsigned)i;
        const float x = __uint_as_float(u);
        if (__float_as_uint(form(x)) != __float_as_uint(ieee(x))) {
            ++bad;
            const unsigned slot = atomicAdd(&out[1], 1u);
            if (slot < (unsigned)kSweepRecord) out[2 + slot] = u;
        }
    }
    if (bad) atomicAdd(&out[0], bad);
}
__global__ void math_sweep_kernel(int which, int n, const float* __restrict__ a, const float* __restrict__ b, unsigned* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned first = __float_as_uint(a[0]), count = __float_as_uint(b[0]);
    const auto rcp = [](float x) { return 1.0f / x; };
    const auto root = [](float x) { return __builtin_sqrtf(x); };
    switch (which) {
        case 40: sweep_patterns(i, n, first, count, out, [](float x) { return rcp_exact(x); }, rcp); break;
        case 41: sweep_patterns(i, n, first, count, out, [](float x) { return rt_sqrt(x); }, root); break;
        case 42: sweep_patterns(i, n, first, count, out, [](float x) { return rt_div_const(x, kSkyTwoPi); }, [](float x) { return x / kSkyTwoPi; }); break;
        case 43: sweep_patterns(i, n, first, count, out, [](float x) { return rt_div_const(x, kSunDiscWidth2); }, [](float x) { return x / kSunDiscWidth2; }); break;
        case 50: sweep_patterns(i, n, first, count, out, [](float x) { return rt_rcp_outside(x) ? 1.0f / x : __builtin_amdgcn_rcpf(x); }, rcp); break;  // the control: the bare estimate is NOT 1 / x
        default: break;
    }
}

// Helper-level known answers (chunky_selftest_helpers): the device functions the kernels are made of, one call per input
// row, against tests/golden/helpers.npz — the answers of the reference object's own exported helpers (oracle/ref_shim.cpp
// ref_helpers has the row layouts and the `which` numbering, K/primitives.h:30-409, K/sky.h:42-106, K/kernel.h:46-98,
// K/block.h:30-118, K/octree.h:41-109, K/bvh.h:22-113).  18 = the world-BVH walk as render_pool performs it (rwalk_step on
// the aligned records, to-visit stacks in LDS), same rows and answers as 15.
constexpr int kHelperIn = 32, kHelperOut = 12;
struct ScratchStack {
    int a[kBvhStackEntries];
    DEV void push(int slot, int v) { a[slot] = v; }
    DEV int pop(int slot) { return a[slot]; }
};
template <int TREE>
__global__ void __launch_bounds__(64) helpers_selftest_kernel(SceneView S, int which, int n, const float* __restrict__ in_rows,
                                                              float* __restrict__ out_rows) {
    extern __shared__ int lds[];
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n) return;
    const float* in = in_rows + (size_t)r * kHelperIn;
    float out[kHelperOut];
    for (int k = 0; k < kHelperOut; k++) out[k] = 0;
    Hit h;
    h.distance = rt_inf();
    h.material = 0;
    h.normal = mk3(0, 0, 0);
    h.color = f4{0, 0, 0, 0};
    h.emittance = 0;
    h.spec = 0;
    const f3 a6 = mk3(in[6], in[7], in[8]), a9 = mk3(in[9], in[10], in[11]);
    switch (which) {
        case 0: out[0] = box_quick(in[0], in[1], in[2], in[3], in[4], in[5], a6, rcp3(a9)); break;
        case 1: out[0] = box_exit(in[0], in[1], in[2], in[3], in[4], in[5], a6, rcp3(a9)); break;
        case 2: case 3: {
            const f3 inv = which == 2 ? rcp3(mk3(in[12], in[13], in[14])) : rcp3(a9);
            const Slabs sl = which == 2 ? slabs(0, 1, 0, 1, 0, 1, a6, inv) : slabs(in[0], in[1], in[2], in[3], in[4], in[5], a6, inv);
            const float tn = slab_near(sl), tf = slab_far(sl);
            if (tf < tn) {
                out[0] = rt_nan();
            } else {
                const Face f = which == 2 ? face_unit(sl, tn, a6 + a9 * tn) : face_map2(sl, tn, a6 + a9 * tn);
                out[0] = tn; out[1] = f.n.x; out[2] = f.n.y; out[3] = f.n.z; out[4] = f.u; out[5] = f.v;
            }
            break;
        }
        case 4: {
            const f3 pos = mk3(in[4], in[5], in[6]), dir = mk3(in[7], in[8], in[9]);
            out[0] = block_hit(S, __float_as_int(in[0]), (int)in[1], (int)in[2], (int)in[3], pos, dir, rcp3(dir), h);
            out[1] = h.normal.x; out[2] = h.normal.y; out[3] = h.normal.z;
            out[4] = h.color.x; out[5] = h.color.y; out[6] = h.color.z; out[7] = h.color.w; out[8] = h.emittance;
            break;
        }
        case 6: {
            f3 nn = mk3(0, 0, 0);
            float u = 0, v = 0;
            int mat = 0;
            out[0] = triangle_hit((const int*)in, in[26], mk3(in[20], in[21], in[22]), mk3(in[23], in[24], in[25]), nn, u, v, mat);
            out[1] = nn.x; out[2] = nn.y; out[3] = nn.z; out[4] = u; out[5] = v; out[6] = __int_as_float(mat);
            break;
        }
        case 7: {
            unsigned rng = (unsigned)__float_as_int(in[0]);
            const f3 d = sun_sample(S, rng);
            out[0] = d.x; out[1] = d.y; out[2] = d.z;
            out[3] = rt_fabs(dot(d, mk3(in[1], in[2], in[3])));  // record.emittance, K/sky.h:90 (sample_path / shade_phase write it the same way)
            out[4] = __int_as_float((int)rng);
            break;
        }
        case 8: {
            f4 c = f4{in[3], in[4], in[5], in[6]};
            const f4 before = c;
            sun_disc(S, mk3(in[0], in[1], in[2]), c);
            out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;  // (alpha: the kernels never read it; the test compares x, y, z)
            out[4] = (c.x != before.x || c.y != before.y || c.z != before.z) ? 1.0f : 0.0f;
            break;
        }
        case 9: {
            const f4 c = sky_color(S, mk3(in[0], in[1], in[2]));
            out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
            break;
        }
        case 10: {
            unsigned rng = (unsigned)__float_as_int(in[0]);
            const f3 d = diffuse_bounce(mk3(in[1], in[2], in[3]), rng);
            const f3 o = mk3(in[4], in[5], in[6]) + d * kOffset;
            out[0] = d.x; out[1] = d.y; out[2] = d.z; out[3] = o.x; out[4] = o.y; out[5] = o.z; out[6] = __int_as_float((int)rng);
            break;
        }
        case 11: {
            const f4 c = unpack_unorm8(atlas_texel(S, in[0], in[1], __float_as_int(in[2]), __float_as_int(in[3])));
            out[0] = c.x; out[1] = c.y; out[2] = c.z; out[3] = c.w;
            break;
        }
        case 12: {
            out[0] = material_sample(S, __float_as_int(in[0]), in[1], in[2], h) ? 1.0f : 0.0f;
            out[1] = h.color.x; out[2] = h.color.y; out[3] = h.color.z; out[4] = h.color.w; out[5] = h.emittance;
            break;
        }
        case 14: case 15: case 18: {
            const f3 o = mk3(in[0], in[1], in[2]), d = mk3(in[3], in[4], in[5]);
            bool hit = false;
            if (which == 14) {
                hit = octree_hit<TREE>(S, o, d, 256, h);
            } else if (which == 15) {
                ScratchStack stack;
                h.distance = in[6];
                hit = bvh_hit(S, S.world_bvh, o, d, h, stack);
            } else {
                LaneState L;
                L.o = o; L.d = d; L.inv = rcp3(d);
                L.h = h;
                L.h.distance = in[6];
                L.shadow = false; L.oct_hit = false; L.trace_hit = false;
                L.bvh_dist = in[6];
                L.pid = (int)threadIdx.x;
                SceneView W = S;
                W.actor_bvh_empty = 1;  // the world BVH alone, like row 15
                PathStacks K{lds, (int)blockDim.x};
                int st = rbvh_enter(W, L, 0);
                while (st == ST_BVH) st = rwalk_step(W, L, K);
                hit = L.trace_hit;
                h = L.h;
            }
            int k = 0;
            out[k++] = hit ? 1.0f : 0.0f;
            out[k++] = h.distance;
            if (which == 14) out[k++] = __int_as_float(h.material);
            out[k++] = h.normal.x; out[k++] = h.normal.y; out[k++] = h.normal.z;
            out[k++] = h.color.x; out[k++] = h.color.y; out[k++] = h.color.z; out[k++] = h.color.w;
            out[k++] = h.emittance;
            break;
        }
        default: break;
    }
    for (int k = 0; k < kHelperOut; k++) out_rows[(size_t)r * kHelperOut + k] = out[k];
}
hipError_t launch_trace_records(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, int seed,
                                const int* gids_dev, int n, HitRecord* out, int* counts, float* radiance,
                                hipStream_t stream) {
    const int block = 256;
    int grid = (n + block - 1) / block;
    if (grid <= 0) return hipSuccess;
    if (use_wide(variant, scene_facts(S)))
        hipLaunchKernelGGL(trace_records_kernel<-1>, dim3(grid), dim3(block), stack_lds_bytes(scene_facts(S), block), stream, S, C, O,
                           seed, gids_dev, n, out, counts, radiance);
    else
        hipLaunchKernelGGL(trace_records_kernel<0>, dim3(grid), dim3(block), stack_lds_bytes(scene_facts(S), block), stream, S, C, O,
                           seed, gids_dev, n, out, counts, radiance);
    return hipGetLastError();
}

hipError_t launch_preview(int variant, const SceneView& S, const CameraView& C, const RenderOpts& O, int* argb,
                          hipStream_t stream) {
    const int block = 256;
    int grid = (C.width * C.height + block - 1) / block;
    if (use_wide(variant, scene_facts(S)))
        hipLaunchKernelGGL(preview_lanes<-1>, dim3(grid), dim3(block), stack_lds_bytes(scene_facts(S), block), stream, S, C, O, argb);
    else
        hipLaunchKernelGGL(preview_lanes<0>, dim3(grid), dim3(block), stack_lds_bytes(scene_facts(S), block), stream, S, C, O, argb);
    return hipGetLastError();
}

// chunky_selftest_camera_rays: the projected camera's ray of every pixel for one seed, as the render kernels compute it, in the
// layout of the pre-generated table (origin, direction; K/camera.h:8-11)
__global__ void __launch_bounds__(256) camera_rays_kernel(CameraView C, unsigned seed, float* __restrict__ out) {
    const int gid = (int)(blockIdx.x * 256 + threadIdx.x);
    if (gid >= C.width * C.height) return;
    const RayOD r = projected_ray(C, seed, canvas_pixel(C, gid));
    float* o = out + 6 * (size_t)gid;
    o[0] = r.o.x; o[1] = r.o.y; o[2] = r.o.z;
    o[3] = r.d.x; o[4] = r.d.y; o[5] = r.d.z;
}
hipError_t launch_camera_rays_selftest(const CameraView& C, int seed, float* out, hipStream_t stream) {
    const long long n = (long long)C.width * C.height;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, C, (unsigned)seed, out);
    return hipGetLastError();
}

// chunky_selftest_shard_map: the slot -> pixel functions every image-writing kernel goes through, one thread per slot, as the
// kernels call them — slots at and beyond T.n_local included (the padding of a launch's last tile).  Nothing is indexed by a gid:
// the five results of slot i go to out[5 * i ...].  shard_gid is evaluated where the kernels evaluate it (a run shard or one rank,
// below n_local); -1 elsewhere.
__global__ void __launch_bounds__(256) shard_map_kernel(ShardView T, int width, int height, int n, FastDiv by_bw, int* __restrict__ out) {
    const int slot = (int)(blockIdx.x * 256 + threadIdx.x);
    if (slot >= n) return;
    const SlotPixel px = pool_slot_pixel(T, width, height, slot, by_bw);
    int* o = out + 5 * (size_t)slot;
    o[0] = pool_slot_gid(T, width, height, slot);
    o[1] = px.gid; o[2] = px.x; o[3] = px.y;
    o[4] = (slot < T.n_local && (T.world == 1 || T.tile != 0)) ? shard_gid(T, slot) : -1;
}
// ... and the division by a launch constant: out[i] = fast_quotient(a, {m, s}) for the triples (a, m, s) of `in` — the pairs (m, s)
// made on the host by fast_div, as a launch's are
__global__ void __launch_bounds__(256) fast_quotient_kernel(int n, const unsigned* __restrict__ in, int* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const unsigned* t = in + 3 * (size_t)i;
    out[i] = (int)fast_quotient(t[0], FastDiv{t[1], (int)t[2]});
}
hipError_t launch_shard_map_selftest(int mode, const ShardView& T, int width, int height, int n, const unsigned* in, int* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (mode == 0) {
        ShardView V = T;
        V.list = nullptr;  // (the block mapping and the run formula only: no list is read)
        V.n_list = 0;
        hipLaunchKernelGGL(shard_map_kernel, grid, block, 0, stream, V, width, height, n, fast_div((unsigned)((width + kTileEdge - 1) >> kTileLog)), out);
        return hipGetLastError();
    }
    if (mode != 1 || !in) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fast_quotient_kernel, grid, block, 0, stream, n, in, out);
    return hipGetLastError();
}

hipError_t launch_math_selftest(int which, int n, const float* a, const float* b, float* out, hipStream_t stream) {
    if (which >= kSweepFirst) {
        if (n < kSweepRecord + 2) return hipErrorInvalidValue;  // (out has n words)
        const hipError_t e = hipMemsetAsync(out, 0, (size_t)n * 4, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(math_sweep_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, which, n, a, b, (unsigned*)out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(math_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, which, n, a, b, out);
    return hipGetLastError();
}

// `tree`: 0 the reference layout, 1 the wide tree in the form the render kernels would pick for this scene (row 14 only)
hipError_t launch_helpers_selftest(const SceneView& S, int which, int tree, int n, const float* in, float* out, int* tree_used, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (which == 18 && !(S.bvh_rec && S.tri_rec && S.mat8)) return hipErrorNotSupported;
    int t = tree ? tree_form(0, scene_facts(S)) : 0;
    typedef void (*Kernel)(SceneView, int, int, const float*, float*);
    Kernel k;
    switch (t) {
        case 0: k = helpers_selftest_kernel<0>; break;
        case 16: k = helpers_selftest_kernel<16>; break;
        case 17: k = helpers_selftest_kernel<17>; break;
        case 18: k = helpers_selftest_kernel<18>; break;
        default: t = -1; k = helpers_selftest_kernel<-1>; break;
    }
    if (tree_used) *tree_used = t;
    const int entries = S.bvh_stack_entries > 0 && S.bvh_stack_entries < kBvhStackEntries ? S.bvh_stack_entries : kBvhStackEntries;
    const size_t lds = which == 18 ? (size_t)entries * 64 * sizeof(int) : 0;
    hipLaunchKernelGGL(k, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, stream, S, which, n, in, out);
    return hipGetLastError();
}


}  // namespace chunky
