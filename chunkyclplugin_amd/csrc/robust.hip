// robust.hip — the kernels of firefly-robust accumulation (chunky_render_robust_*; specification: robust_spec.h).
//
//   fold_buckets_kernel<M>    fold_kernel's running mean over the staged samples of a launch, and from the same read the update of
//                             the pixel's M bucket means: one thread per pixel slot and channel, as fold_kernel.  The M means stay in
//                             registers: register k holds bucket (first index + k) % M, so that pass k of every run of M passes meets
//                             register k — the pass loop is unrolled by M and no index into the means depends on a run-time value
//   robust_resolve_kernel<M>  per pixel: the sort network, the Gini coefficient, the trim and the trimmed mean of each channel, fully
//                             unrolled; writes the image and, where asked, the pixel's trim byte
//   robust_stage_kernel       self test: per-pass samples [pass][pixel][3] into the staging layout of a whole image
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "path_state.hpp"
#include "robust_spec.h"

namespace chunky {

// Layout and addressing of the staging array are fold_kernel's ([sub-block][pass][slot in sub-block][3]), and so are the operations on
// `res` and their order: the beauty image is the one fold_kernel leaves.  buckets: [bucket][pixel][3].  first_index: the robust sample
// count before this launch.
template <int M>
__global__ void __launch_bounds__(256) fold_buckets_kernel(const float* __restrict__ staging, float* __restrict__ res, float* __restrict__ buckets,
                                                            ShardView T, int n_pixels, int width, long long n_slots, int n_passes, int first_spp,
                                                            int first_index) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 3ll * n_slots) return;
    const int slot = (int)(t / 3), c = (int)(t - 3ll * slot);
    const int gid = pool_slot_gid(T, width, n_pixels / width, slot);
    if (gid >= n_pixels) return;
    const size_t at = 3 * (size_t)gid + c, plane = 3 * (size_t)n_pixels;
    float mean = res[at];
    const int r0 = first_index % M;
    float b[M];
#pragma unroll
    for (int k = 0; k < M; k++) {
        const int bucket = r0 + k < M ? r0 + k : r0 + k - M;
        b[k] = buckets[(size_t)bucket * plane + at];
    }
    const size_t sub = (size_t)slot / kSubBlock, i = (size_t)slot % kSubBlock;
    const float* p = staging + 3 * (sub * (size_t)n_passes * kSubBlock + i) + c;
    for (int base = 0; base < n_passes; base += M) {
#pragma unroll
        for (int k = 0; k < M; k++) {
            if (base + k < n_passes) {  // (the tail of the last run)
                const float s = p[(size_t)(base + k) * (3 * kSubBlock)];
                mean = ad_mean(mean, s, first_spp + base + k);
                b[k] = ad_mean(b[k], s, (first_index + base + k) / M);
            }
        }
    }
    res[at] = mean;
#pragma unroll
    for (int k = 0; k < M; k++) {
        const int bucket = r0 + k < M ? r0 + k : r0 + k - M;
        buckets[(size_t)bucket * plane + at] = b[k];
    }
}

template <int M>
__global__ void __launch_bounds__(256) robust_resolve_kernel(const float* __restrict__ buckets, int n_pixels, int mode, float gain,
                                                              float* __restrict__ out, unsigned char* __restrict__ trim) {
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_pixels) return;
    const size_t plane = 3 * (size_t)n_pixels;
    int most = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float x[M];
#pragma unroll
        for (int k = 0; k < M; k++) x[k] = buckets[(size_t)k * plane + 3 * (size_t)p + c];
        int t;
        out[3 * (size_t)p + c] = rb_resolve<M>(x, mode, gain, &t);
        most = t > most ? t : most;
    }
    if (trim) trim[p] = (unsigned char)most;
}

__global__ void __launch_bounds__(256) robust_stage_kernel(const float* __restrict__ samples, float* __restrict__ staging, int width, int height,
                                                            long long n_slots, int n_passes) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_slots) return;
    const int slot = (int)t;
    const ShardView whole{0, 1, 256, width * height};
    const int gid = pool_slot_gid(whole, width, height, slot);
    if (gid >= width * height) return;  // (padding slots: the array was zeroed)
    const size_t sub = (size_t)slot / kSubBlock, i = (size_t)slot % kSubBlock;
    float* q = staging + 3 * (sub * (size_t)n_passes * kSubBlock + i);
    for (int k = 0; k < n_passes; k++) {
        const float* s = samples + 3 * ((size_t)k * width * height + gid);
        float* d = q + (size_t)k * (3 * kSubBlock);
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
}

// ------------------------------------------------------------------------------------ launchers
#define CHUNKY_ROBUST_M(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15)

hipError_t launch_fold_buckets(const float* staging, float* res, float* buckets, int n_buckets, int first_index, const ShardView& T, int width,
                               int height, long long n_tiles, int n_passes, int first_spp, hipStream_t stream) {
    const long long n_slots = n_tiles * kSampleTile;
    if (!rb_buckets_ok(n_buckets) || first_index < 0) return hipErrorInvalidValue;
    if (n_slots <= 0 || n_passes <= 0) return hipSuccess;
    const dim3 grid((unsigned)((3 * n_slots + 255) / 256));
    switch (n_buckets) {
#define CHUNKY_ROBUST_CASE(M_)                                                                                                                   \
    case M_:                                                                                                                                     \
        hipLaunchKernelGGL(fold_buckets_kernel<M_>, grid, dim3(256), 0, stream, staging, res, buckets, T, width * height, width, n_slots, n_passes, \
                           first_spp, first_index);                                                                                              \
        break;
        CHUNKY_ROBUST_M(CHUNKY_ROBUST_CASE)
#undef CHUNKY_ROBUST_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_robust_resolve(const float* buckets, int n_buckets, long long n_pixels, int mode, float gain, float* out, unsigned char* trim,
                                 hipStream_t stream) {
    if (!rb_buckets_ok(n_buckets) || n_pixels > (1ll << 30)) return hipErrorInvalidValue;
    if (n_pixels <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_pixels + 255) / 256));
    switch (n_buckets) {
#define CHUNKY_ROBUST_CASE(M_)                                                                                                     \
    case M_:                                                                                                                       \
        hipLaunchKernelGGL(robust_resolve_kernel<M_>, grid, dim3(256), 0, stream, buckets, (int)n_pixels, mode, gain, out, trim); \
        break;
        CHUNKY_ROBUST_M(CHUNKY_ROBUST_CASE)
#undef CHUNKY_ROBUST_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_robust_stage(const float* samples, float* staging, int width, int height, long long n_tiles, int n_passes, hipStream_t stream) {
    const long long n_slots = n_tiles * kSampleTile;
    if (n_slots <= 0 || n_passes <= 0) return hipSuccess;
    hipLaunchKernelGGL(robust_stage_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, samples, staging, width, height, n_slots,
                       n_passes);
    return hipGetLastError();
}

}  // namespace chunky
