// denoise.hip — the edge-avoiding À-Trous denoiser on the device (chunky_denoise_frame, chunky_render_denoise).
//
// Specification: denoise_spec.h.  Every kernel below evaluates dn_filter_pixel of that header; they differ
// only in how a tap's colour, normal and albedo reach the lane, which changes no bit.  One launch per iteration (an iteration reads
// taps up to 2 << i pixels away, so it needs all of the previous one), ping-pong between two colour buffers of the workspace.
//
// Two forms are built (EXPERIMENTS.md, denoiser):
//   gather  one thread per pixel, lanes along x, the three images as they arrive (3 floats per pixel each): a tap is nine
//           global_load_dword whose lanes are 12 bytes apart.  The default: it measured 19 % faster than the packed form.
//   packed  a pack pass writes three planes of 16-byte words per pixel — {D0.xyz, 0}, {N.xyz, A.x}, {A.yz, 0, 0}; the demodulation
//           is folded into it — and an iteration fetches a tap with three global_load_dwordx4, each a coalesced 1 KB per wave; the
//           colour plane is the ping-pong buffer, the guide planes are written once.  The last iteration folds the remodulation
//           and writes the caller's 3-float layout.  Kept selectable (flags bits 8-9) as the measured alternative.
// A wave covers 64 consecutive pixels of one row (block 64 x 4), so the row test of a tap is wave-uniform and only the waves at the
// left and right image edges diverge on the column test.
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "denoise_spec.h"
#include "kernels.hpp"

namespace chunky {

constexpr int kDnBlockX = 64, kDnBlockY = 4;

struct DnPlanarFetch {  // 3 floats per pixel in each of three images
    const float* __restrict__ d;
    const float* __restrict__ n;
    const float* __restrict__ a;
    int width;
    __device__ __forceinline__ void load(int x, int y, float* dq, float* nq, float* aq) const {
        const size_t o = 3 * ((size_t)y * width + x);
        dq[0] = d[o]; dq[1] = d[o + 1]; dq[2] = d[o + 2];
        nq[0] = n[o]; nq[1] = n[o + 1]; nq[2] = n[o + 2];
        aq[0] = a[o]; aq[1] = a[o + 1]; aq[2] = a[o + 2];
    }
};

struct DnPackedFetch {  // three planes of float4 per pixel
    const float4* __restrict__ d;
    const float4* __restrict__ g0;
    const float4* __restrict__ g1;
    int width;
    __device__ __forceinline__ void load(int x, int y, float* dq, float* nq, float* aq) const {
        const size_t o = (size_t)y * width + x;
        const float4 c = d[o], u = g0[o], v = g1[o];
        dq[0] = c.x; dq[1] = c.y; dq[2] = c.z;
        nq[0] = u.x; nq[1] = u.y; nq[2] = u.z;
        aq[0] = u.w; aq[1] = v.x; aq[2] = v.y;
    }
};

struct DnIterArgs {
    int width, height, step, demodulate;
    float c_i, c_n, c_a;
};

// gather: D0 = C / max(A, eps) as an image of its own (only with the demodulation flag)
__global__ void __launch_bounds__(256) dn_demod_kernel(long long n_pixels, const float* __restrict__ color, const float* __restrict__ albedo, float* __restrict__ d0) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    float d[3];
    dn_demodulate(color + 3 * i, albedo + 3 * i, 1, d);
    d0[3 * i] = d[0];
    d0[3 * i + 1] = d[1];
    d0[3 * i + 2] = d[2];
}

// gather: one iteration; LAST writes the output (remodulated, bad input pixels passed through) instead of the next D
template <bool LAST>
__global__ void __launch_bounds__(256) dn_gather_kernel(DnIterArgs K, const float* __restrict__ d, const float* __restrict__ normal, const float* __restrict__ albedo,
                                                        const float* __restrict__ color, float* __restrict__ out) {
    const int px = (int)(blockIdx.x * kDnBlockX + threadIdx.x), py = (int)(blockIdx.y * kDnBlockY + threadIdx.y);
    if (px >= K.width || py >= K.height) return;
    float r[3];
    dn_filter_pixel(DnPlanarFetch{d, normal, albedo, K.width}, px, py, K.width, K.height, K.step, K.c_i, K.c_n, K.c_a, r);
    const size_t o = 3 * ((size_t)py * K.width + px);
    if (LAST) {
        const float a[3] = {albedo[o], albedo[o + 1], albedo[o + 2]}, c[3] = {color[o], color[o + 1], color[o + 2]};
        float f[3];
        dn_finish(r, a, c, K.demodulate, f);
        r[0] = f[0]; r[1] = f[1]; r[2] = f[2];
    }
    out[o] = r[0];
    out[o + 1] = r[1];
    out[o + 2] = r[2];
}

// packed: the three planes from the caller's images, demodulation folded in
__global__ void __launch_bounds__(256) dn_pack_kernel(long long n_pixels, int demodulate, const float* __restrict__ color, const float* __restrict__ albedo,
                                                      const float* __restrict__ normal, float4* __restrict__ d0, float4* __restrict__ g0, float4* __restrict__ g1) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float a[3] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]};
    float d[3];
    dn_demodulate(color + 3 * i, a, demodulate, d);
    d0[i] = make_float4(d[0], d[1], d[2], 0.0f);
    g0[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], a[0]);
    g1[i] = make_float4(a[1], a[2], 0.0f, 0.0f);
}

// packed: one iteration; LAST writes 3 floats per pixel to `out`, otherwise a float4 per pixel to `next`
template <bool LAST>
__global__ void __launch_bounds__(256) dn_packed_kernel(DnIterArgs K, const float4* __restrict__ d, const float4* __restrict__ g0, const float4* __restrict__ g1,
                                                        const float* __restrict__ color, float4* __restrict__ next, float* __restrict__ out) {
    const int px = (int)(blockIdx.x * kDnBlockX + threadIdx.x), py = (int)(blockIdx.y * kDnBlockY + threadIdx.y);
    if (px >= K.width || py >= K.height) return;
    float r[3];
    dn_filter_pixel(DnPackedFetch{d, g0, g1, K.width}, px, py, K.width, K.height, K.step, K.c_i, K.c_n, K.c_a, r);
    const size_t p = (size_t)py * K.width + px;
    if (LAST) {
        const float4 u = g0[p], v = g1[p];
        const float a[3] = {u.w, v.x, v.y}, c[3] = {color[3 * p], color[3 * p + 1], color[3 * p + 2]};
        float f[3];
        dn_finish(r, a, c, K.demodulate, f);
        out[3 * p] = f[0];
        out[3 * p + 1] = f[1];
        out[3 * p + 2] = f[2];
    } else {
        next[p] = make_float4(r[0], r[1], r[2], 0.0f);
    }
}

hipError_t launch_denoise(int form, int width, int height, const float* color, const float* albedo, const float* normal, const DnCoeffs& K, float* out,
                          void* work, size_t work_bytes, hipStream_t stream, int* launches) {
    if (width <= 0 || height <= 0 || K.iterations < 1 || K.iterations > DN_MAX_ITERATIONS) return hipErrorInvalidValue;
    const long long n = (long long)width * height;
    if (work_bytes < denoise_work_bytes(width, height)) return hipErrorInvalidValue;
    const dim3 block(kDnBlockX, kDnBlockY), grid((unsigned)((width + kDnBlockX - 1) / kDnBlockX), (unsigned)((height + kDnBlockY - 1) / kDnBlockY));
    if (grid.y > 65535u * 16u) return hipErrorInvalidValue;
    const unsigned flat = (unsigned)((n + 255) / 256);
    int count = 0;
    if (form == kDenoiseGather) {
        float* buf[2] = {(float*)work, (float*)work + 3 * n};
        const float* cur = color;
        if (K.demodulate) {
            hipLaunchKernelGGL(dn_demod_kernel, dim3(flat), dim3(256), 0, stream, n, color, albedo, buf[1]);
            cur = buf[1];
            count++;
        }
        for (int i = 0; i < K.iterations; i++) {
            const DnIterArgs A{width, height, 1 << i, K.demodulate, K.c_i[i], K.c_n, K.c_a};
            if (i == K.iterations - 1) {
                hipLaunchKernelGGL(dn_gather_kernel<true>, grid, block, 0, stream, A, cur, normal, albedo, color, out);
            } else {
                float* dst = buf[i & 1];
                hipLaunchKernelGGL(dn_gather_kernel<false>, grid, block, 0, stream, A, cur, normal, albedo, color, dst);
                cur = dst;
            }
            count++;
        }
    } else if (form == kDenoisePacked) {
        float4* buf[2] = {(float4*)work, (float4*)work + n};
        float4* g0 = (float4*)work + 2 * n;
        float4* g1 = (float4*)work + 3 * n;
        hipLaunchKernelGGL(dn_pack_kernel, dim3(flat), dim3(256), 0, stream, n, K.demodulate, color, albedo, normal, buf[0], g0, g1);
        count++;
        for (int i = 0; i < K.iterations; i++) {
            const DnIterArgs A{width, height, 1 << i, K.demodulate, K.c_i[i], K.c_n, K.c_a};
            if (i == K.iterations - 1)
                hipLaunchKernelGGL(dn_packed_kernel<true>, grid, block, 0, stream, A, buf[i & 1], g0, g1, color, (float4*)nullptr, out);
            else
                hipLaunchKernelGGL(dn_packed_kernel<false>, grid, block, 0, stream, A, buf[i & 1], g0, g1, color, buf[(i + 1) & 1], (float*)nullptr);
            count++;
        }
    } else {
        return hipErrorInvalidValue;
    }
    if (launches) *launches = count;
    return hipGetLastError();
}

}  // namespace chunky
