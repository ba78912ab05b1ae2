// adaptive.hip — the kernels of adaptive sampling (chunky_render_adaptive; specification: adaptive_spec.h).
//
//   fold_stats_kernel      fold_kernel's running mean over the staged samples of a launch plus the Welford update of the pixel's
//                          luminance statistic, in one read of the staging array: one thread per pixel slot (luminance needs the
//                          three channels of a sample together)
//   adaptive_check_kernel  the convergence test, one thread per pixel: writes the unconverged flags
//   adaptive_tile_kernel   one workgroup per 16 x 16 tile of pixel slots, in the order of pool_slot_gid with one rank.  <false>: a
//                          pixel stays active iff a pixel of its 3 x 3 neighbourhood is unconverged (those that leave record n_p),
//                          and the tile's active slots are counted with wave ballots; <true>: the active slots are written to the
//                          list at the tile's offset plus the ballot's prefix (mbcnt) — no atomic decides a position, so the list is
//                          the same on every run and stays in whole-image slot order (four consecutive entries are mostly one
//                          2 x 2 block: the 256 samples a wave of render_pool claims stay coherent rays)
//   adaptive_scan_kernel   exclusive scan over the tile counts (one workgroup: a 1920 x 1080 image has 8 160 tiles) and the total
//   adaptive_finish_kernel pixels still active at the end record the passes rendered
//   adaptive_count_kernel  the tile counts of an activity map that is already final (a restored state): with the scan and the scatter
//                          it rebuilds the list
//
// Compiled with -ffp-contract=off (see rt_device.hpp).
#include <hip/hip_runtime.h>

#include "adaptive_spec.h"
#include "path_state.hpp"

namespace chunky {

// Layout and addressing are fold_kernel's ([sub-block][pass][slot in sub-block][3]).  A thread reads the 12 contiguous bytes of its
// sample per pass (4-byte aligned only: slot i of a sub-block starts at byte 12 i, so a 16-byte load does not apply); a wave's 64
// slots are 16 sub-blocks of 48 contiguous bytes each, the same lines fold_kernel's 192 threads touch for those slots.
__global__ void __launch_bounds__(256) fold_stats_kernel(const float* __restrict__ staging, float* __restrict__ res, float* __restrict__ stat,
                                                          ShardView T, int n_pixels, int width, long long n_slots, int n_passes, int first_spp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_slots) return;
    const int slot = (int)t;
    const int gid = pool_slot_gid(T, width, n_pixels / width, slot);
    if (gid >= n_pixels) return;
    float* px = res + 3 * (size_t)gid;
    float* sp = stat + 2 * (size_t)gid;
    float r = px[0], g = px[1], b = px[2];
    float m = sp[0], M2 = sp[1];
    const size_t sub = (size_t)slot / kSubBlock, i = (size_t)slot % kSubBlock;
    const float* p = staging + 3 * (sub * (size_t)n_passes * kSubBlock + i);
#pragma unroll 4
    for (int k = 0; k < n_passes; k++) {
        const int spp = first_spp + k;
        const float* s = p + (size_t)k * (3 * kSubBlock);
        const float s0 = s[0], s1 = s[1], s2 = s[2];
        r = ad_mean(r, s0, spp);
        g = ad_mean(g, s1, spp);
        b = ad_mean(b, s2, spp);
        ad_welford(ad_luma(s0, s1, s2), spp, &m, &M2);
    }
    px[0] = r; px[1] = g; px[2] = b;
    sp[0] = m; sp[1] = M2;
}

__global__ void __launch_bounds__(256) adaptive_check_kernel(const float* __restrict__ stat, const unsigned char* __restrict__ active,
                                                              unsigned char* __restrict__ unconv, int n_pixels, int n, float t2, float floor_) {
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= n_pixels) return;
    unconv[p] = (unsigned char)(active[p] && ad_unconverged(stat[2 * (size_t)p], stat[2 * (size_t)p + 1], n, t2, floor_));
}

template <bool SCATTER>
__global__ void __launch_bounds__(256) adaptive_tile_kernel(int width, int height, const unsigned char* __restrict__ unconv, unsigned char* __restrict__ active,
                                                             int* __restrict__ count, int n, int* __restrict__ tile_counts,
                                                             const int* __restrict__ tile_offsets, int* __restrict__ list) {
    __shared__ int wave_count[4];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int slot = (int)(blockIdx.x * 256 + threadIdx.x);
    const ShardView whole{0, 1, 256, width * height};
    const int gid = pool_slot_gid(whole, width, height, slot);
    bool a = false;
    if (gid < width * height && active[gid]) {
        a = true;
        if (!SCATTER) {
            const int y = gid / width, x = gid - y * width;
            const int x0 = x > 0 ? x - 1 : x, x1 = x < width - 1 ? x + 1 : x, y0 = y > 0 ? y - 1 : y, y1 = y < height - 1 ? y + 1 : y;
            int any = 0;
            for (int yy = y0; yy <= y1; yy++)
                for (int xx = x0; xx <= x1; xx++) any |= unconv[(size_t)yy * width + xx];
            if (!any) {  // the pixel leaves: its state is final
                a = false;
                active[gid] = 0;
                count[gid] = n;
            }
        }
    }
    const unsigned long long mask = __ballot(a);
    if (lane == 0) wave_count[wave] = (int)__builtin_popcountll(mask);
    __syncthreads();
    if (!SCATTER) {
        if (threadIdx.x == 0) tile_counts[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
    } else if (a) {
        int base = tile_offsets[blockIdx.x];
        for (int w = 0; w < wave; w++) base += wave_count[w];
        const int prefix = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        list[base + prefix] = gid;
    }
}

// The counting half of adaptive_tile_kernel<false> for an activity map that is already final (chunky_render_adaptive_restore): a
// tile's active slots, nothing tested and nothing written to the maps.  Followed by adaptive_scan_kernel and
// adaptive_tile_kernel<true> it rebuilds the list a run held after the check that left this map, entry for entry.
__global__ void __launch_bounds__(256) adaptive_count_kernel(int width, int height, const unsigned char* __restrict__ active, int* __restrict__ tile_counts) {
    __shared__ int wave_count[4];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int slot = (int)(blockIdx.x * 256 + threadIdx.x);
    const ShardView whole{0, 1, 256, width * height};
    const int gid = pool_slot_gid(whole, width, height, slot);
    const bool a = gid < width * height && active[gid] != 0;
    const unsigned long long mask = __ballot(a);
    if (lane == 0) wave_count[wave] = (int)__builtin_popcountll(mask);
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

__global__ void __launch_bounds__(1024) adaptive_scan_kernel(const int* __restrict__ counts, int* __restrict__ offsets, int n_tiles, int* __restrict__ total) {
    __shared__ int wave_sum[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int running = 0;
    for (int base = 0; base < n_tiles; base += 1024) {
        const int i = base + tid;
        const int v = i < n_tiles ? counts[i] : 0;
        int x = v;  // inclusive scan inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wave_sum[wave] = x;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < 16; w++) {
            before += w < wave ? wave_sum[w] : 0;
            all += wave_sum[w];
        }
        if (i < n_tiles) offsets[i] = running + before + x - v;
        running += all;
        __syncthreads();
    }
    if (tid == 0) *total = running;
}

__global__ void __launch_bounds__(256) adaptive_finish_kernel(const unsigned char* __restrict__ active, int* __restrict__ count, int n_pixels, int n) {
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p < n_pixels && active[p]) count[p] = n;
}

// ------------------------------------------------------------------------------------ launchers
hipError_t launch_fold_stats(const float* staging, float* res, float* stat, const ShardView& T, int width, int height, long long n_tiles,
                             int n_passes, int first_spp, hipStream_t stream) {
    const long long n_slots = n_tiles * kSampleTile;
    if (n_slots <= 0 || n_passes <= 0) return hipSuccess;
    hipLaunchKernelGGL(fold_stats_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, staging, res, stat, T, width * height,
                       width, n_slots, n_passes, first_spp);
    return hipGetLastError();
}

hipError_t launch_adaptive_check(int width, int height, const float* stat, unsigned char* active, unsigned char* unconv, int* count, int n,
                                 float t2, float floor_, int* tile_counts, int* tile_offsets, int* list, int* total, hipStream_t stream) {
    const int n_pixels = width * height;
    const int n_tiles = ((width + kTileEdge - 1) >> kTileLog) * ((height + kTileEdge - 1) >> kTileLog);
    hipLaunchKernelGGL(adaptive_check_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, stat, (const unsigned char*)active,
                       unconv, n_pixels, n, t2, floor_);
    hipLaunchKernelGGL(adaptive_tile_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, stream, width, height, (const unsigned char*)unconv,
                       active, count, n, tile_counts, (const int*)tile_offsets, list);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, (const int*)tile_counts, tile_offsets, n_tiles, total);
    hipLaunchKernelGGL(adaptive_tile_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, stream, width, height, (const unsigned char*)unconv,
                       active, count, n, tile_counts, (const int*)tile_offsets, list);
    return hipGetLastError();
}

hipError_t launch_adaptive_rebuild(int width, int height, unsigned char* active, int* tile_counts, int* tile_offsets, int* list, int* total,
                                   hipStream_t stream) {
    const int n_tiles = ((width + kTileEdge - 1) >> kTileLog) * ((height + kTileEdge - 1) >> kTileLog);
    hipLaunchKernelGGL(adaptive_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, width, height, (const unsigned char*)active, tile_counts);
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, (const int*)tile_counts, tile_offsets, n_tiles, total);
    // (the scatter reads neither unconv nor count, and writes only the list)
    hipLaunchKernelGGL(adaptive_tile_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, stream, width, height, (const unsigned char*)nullptr, active,
                       (int*)nullptr, 0, tile_counts, (const int*)tile_offsets, list);
    return hipGetLastError();
}

hipError_t launch_adaptive_finish(int n_pixels, const unsigned char* active, int* count, int n, hipStream_t stream) {
    hipLaunchKernelGGL(adaptive_finish_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, active, count, n_pixels, n);
    return hipGetLastError();
}

}  // namespace chunky
