// tools/ubench_imul.hip — what do the integer multiplies and 64-bit shift-adds of address arithmetic cost to issue on gfx950?
//
//   hipcc --offload-arch=gfx950 -O3 -o build/ubench_imul tools/ubench_imul.hip && build/ubench_imul > profiles/r10_imul_rates.txt
//
// A scene array indexed with a sign-extended int or a size_t product compiles to v_mul_lo_u32, v_mad_u64_u32, v_mad_i64_i32 and
// v_lshl_add_u64; the same address as a 32-bit offset is v_mad_u32_u24, v_lshl_add_u32 and v_add_u32 (EXPERIMENTS 7.4,
// tools/isa_addr.py).  For each of the seven this program times, with s_memtime around it, a stream of 1 024 issues per wave — independent
// (eight destinations in rotation, no instruction reads another's result) and dependent (each reads the one before) — at one wave
// and at six waves per SIMD: 256 x 256 threads is one wave on every SIMD of 256 CUs, six times as many workgroups six.  (Where the
// dispatcher puts workgroups is its business: the figures are the median over all waves of a launch.)  Printed per instruction: a
// wave's cycles per issue, and at six waves those cycles / 6 — the SIMD's issue cost when other waves fill the gaps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));            \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

typedef unsigned long long u64;
constexpr int kIssues = 1024, kBlock = 32;  // 32 issues per asm statement, 32 statements

#define X8(f) f(0) f(1) f(2) f(3) f(4) f(5) f(6) f(7)
#define X32(f) X8(f) X8(f) X8(f) X8(f)
#define OUT8(t) "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7])

// independent forms: destination %d (0 .. 7), sources %8 %9 (32-bit) and %10 (64-bit)
#define I_MUL_LO(d) "v_mul_lo_u32 %" #d ", %8, %9\n"
#define I_MAD_U64(d) "v_mad_u64_u32 %" #d ", vcc, %8, %9, %10\n"
#define I_MAD_I64(d) "v_mad_i64_i32 %" #d ", vcc, %8, %9, %10\n"
#define I_LSHL_ADD_U64(d) "v_lshl_add_u64 %" #d ", %10, 2, %10\n"
#define I_MAD_U24(d) "v_mad_u32_u24 %" #d ", %8, %9, %8\n"
#define I_LSHL_ADD_U32(d) "v_lshl_add_u32 %" #d ", %8, 2, %9\n"
#define I_ADD_U32(d) "v_add_u32 %" #d ", %8, %9\n"
// dependent forms: %0 is read and written (32- or 64-bit), sources %1 %2
#define D_MUL_LO(d) "v_mul_lo_u32 %0, %0, %1\n"
#define D_MAD_U64(d) "v_mad_u64_u32 %0, vcc, %1, %2, %0\n"
#define D_MAD_I64(d) "v_mad_i64_i32 %0, vcc, %1, %2, %0\n"
#define D_LSHL_ADD_U64(d) "v_lshl_add_u64 %0, %0, 1, %0\n"
#define D_MAD_U24(d) "v_mad_u32_u24 %0, %0, %1, %2\n"
#define D_LSHL_ADD_U32(d) "v_lshl_add_u32 %0, %0, 1, %1\n"
#define D_ADD_U32(d) "v_add_u32 %0, %0, %1\n"

__device__ inline u64 now() {
    u64 t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

enum { MUL_LO, MAD_U64, MAD_I64, LSHL_ADD_U64, MAD_U24, LSHL_ADD_U32, ADD_U32, N_OPS };
static const char* kNames[N_OPS] = {"v_mul_lo_u32", "v_mad_u64_u32", "v_mad_i64_i32", "v_lshl_add_u64", "v_mad_u32_u24", "v_lshl_add_u32", "v_add_u32"};

// cycles[wave] = s_memtime ticks of kIssues issues of OP in one wave; sink keeps the results alive
template <int OP, bool DEP>
__global__ __launch_bounds__(256) void stream(u64* __restrict__ cycles, unsigned* __restrict__ sink, unsigned seed) {
    unsigned a = threadIdx.x * 2654435761u + seed, b = (threadIdx.x | 1u) + seed;
    u64 c = ((u64)a << 32) | b;
    unsigned t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u64 w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned x = a;
    u64 y = c;
    const u64 t0 = now();
#pragma unroll 1
    for (int i = 0; i < kIssues / kBlock; i++) {
        if (!DEP) {
            if (OP == MUL_LO) asm volatile(X32(I_MUL_LO) : OUT8(t) : "v"(a), "v"(b), "v"(c));
            if (OP == MAD_U64) asm volatile(X32(I_MAD_U64) : OUT8(w) : "v"(a), "v"(b), "v"(c) : "vcc");
            if (OP == MAD_I64) asm volatile(X32(I_MAD_I64) : OUT8(w) : "v"(a), "v"(b), "v"(c) : "vcc");
            if (OP == LSHL_ADD_U64) asm volatile(X32(I_LSHL_ADD_U64) : OUT8(w) : "v"(a), "v"(b), "v"(c));
            if (OP == MAD_U24) asm volatile(X32(I_MAD_U24) : OUT8(t) : "v"(a), "v"(b), "v"(c));
            if (OP == LSHL_ADD_U32) asm volatile(X32(I_LSHL_ADD_U32) : OUT8(t) : "v"(a), "v"(b), "v"(c));
            if (OP == ADD_U32) asm volatile(X32(I_ADD_U32) : OUT8(t) : "v"(a), "v"(b), "v"(c));
        } else {
            if (OP == MUL_LO) asm volatile(X32(D_MUL_LO) : "+v"(x) : "v"(b), "v"(a));
            if (OP == MAD_U64) asm volatile(X32(D_MAD_U64) : "+v"(y) : "v"(a), "v"(b) : "vcc");
            if (OP == MAD_I64) asm volatile(X32(D_MAD_I64) : "+v"(y) : "v"(a), "v"(b) : "vcc");
            if (OP == LSHL_ADD_U64) asm volatile(X32(D_LSHL_ADD_U64) : "+v"(y) : "v"(a), "v"(b));
            if (OP == MAD_U24) asm volatile(X32(D_MAD_U24) : "+v"(x) : "v"(b), "v"(a));
            if (OP == LSHL_ADD_U32) asm volatile(X32(D_LSHL_ADD_U32) : "+v"(x) : "v"(b), "v"(a));
            if (OP == ADD_U32) asm volatile(X32(D_ADD_U32) : "+v"(x) : "v"(b), "v"(a));
        }
    }
    const u64 t1 = now();
    unsigned r = x ^ (unsigned)y ^ (unsigned)(y >> 32);
#pragma unroll
    for (int k = 0; k < 8; k++) r ^= t[k] ^ (unsigned)w[k] ^ (unsigned)(w[k] >> 32);
    const unsigned wave = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;  // < gridDim.x * 4: the size of `cycles`
    if ((threadIdx.x & 63) == 0) cycles[wave] = t1 - t0;
    if (r == 0x12345u) sink[0] = r;  // (practically never: the store only keeps r alive)
}

template <int OP, bool DEP>
static double median_cycles(int waves_per_simd, u64* d_cycles, unsigned* d_sink) {
    const int grid = 256 * waves_per_simd, waves = grid * 4;
    hipLaunchKernelGGL((stream<OP, DEP>), dim3(grid), dim3(256), 0, 0, d_cycles, d_sink, 1u);  // warm-up: the code is in the instruction cache
    hipLaunchKernelGGL((stream<OP, DEP>), dim3(grid), dim3(256), 0, 0, d_cycles, d_sink, 2u);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<u64> h(waves);
    CK(hipMemcpy(h.data(), d_cycles, (size_t)waves * 8, hipMemcpyDeviceToHost));
    std::nth_element(h.begin(), h.begin() + waves / 2, h.end());
    return (double)h[waves / 2] / kIssues;
}

template <int OP>
static void report(u64* d_cycles, unsigned* d_sink) {
    const double i1 = median_cycles<OP, false>(1, d_cycles, d_sink), d1 = median_cycles<OP, true>(1, d_cycles, d_sink);
    const double i6 = median_cycles<OP, false>(6, d_cycles, d_sink), d6 = median_cycles<OP, true>(6, d_cycles, d_sink);
    printf("{\"instruction\": \"%s\", \"ticks_per_issue\": {\"1_wave_independent\": %.2f, \"1_wave_dependent\": %.2f, \"6_waves_independent\": %.2f, "
           "\"6_waves_dependent\": %.2f}, \"simd_ticks_per_issue_at_6_waves\": {\"independent\": %.2f, \"dependent\": %.2f}}\n",
           kNames[OP], i1, d1, i6, d6, i6 / 6, d6 / 6);
}

int main() {
    u64* d_cycles;
    unsigned* d_sink;
    CK(hipMalloc(&d_cycles, (size_t)256 * 6 * 4 * 8));  // the largest launch: 256 * 6 workgroups of four waves
    CK(hipMalloc(&d_sink, 64));
    printf("{\"note\": \"s_memtime ticks per issue of one wave64 instruction, median over the waves of a launch; %d issues per wave\"}\n", kIssues);
    report<MUL_LO>(d_cycles, d_sink);
    report<MAD_U64>(d_cycles, d_sink);
    report<MAD_I64>(d_cycles, d_sink);
    report<LSHL_ADD_U64>(d_cycles, d_sink);
    report<MAD_U24>(d_cycles, d_sink);
    report<LSHL_ADD_U32>(d_cycles, d_sink);
    report<ADD_U32>(d_cycles, d_sink);
    CK(hipFree(d_cycles));
    CK(hipFree(d_sink));
    return 0;
}
