// Micro-benchmark: the Levenshtein lane core with match masks from per-lane REGISTER tables read with v_perm_b32
// (strsim_lane_ptab.h) against the bit-fill masks (lev_myers32_snap, strsim_lane_core.h), everything in registers, at 4 and 5
// waves per SIMD and rounds of 8 / 16 / 32 columns on gfx950.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ipolars-strsim_amd/csrc bench_support/micro/core_ptab.hip -o bench_support/micro/core_ptab && bench_support/micro/core_ptab
// Prints cycles of SIMD time per iteration (= per 64 pairs of that many columns, plane build and table build included) and
// checks that both cores return the same distances.  The column bound is a kernel argument (an SGPR, as in k_lane_stage).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "strsim_lane_ptab.h"

template <int CORE>
__global__ __launch_bounds__(64) void k(uint32_t *out, unsigned long long *clk, uint32_t seed, int iters, uint32_t cols)
{
    using namespace strsim;
    uint32_t wa[8], wb[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        wa[d] = (seed * (2 * d + 3) + threadIdx.x * 0x01010101u) & 0x1F1F1F1Fu;
        wb[d] = (seed * (2 * d + 5) + threadIdx.x * 0x01000193u) & 0x1F1F1F1Fu;
    }
    const uint32_t tmax = wave_uniform(cols), tmin = tmax - 3u, lt = tmin + (threadIdx.x & 3u);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    uint32_t acc = 0;
#pragma unroll 1
    for (int i = 0; i < iters; ++i) {
        uint32_t P[5];
        build_planes<5>(wb, P);
        const uint32_t dist = CORE == 1 ? lev_myers32_snap<5>(wa, lt, tmin, tmax, P, 32u) : lev_myers32_ptab<5>(wa, lt, tmin, tmax, P, 32u);
        acc += dist;
        wa[0] ^= dist & 0x1Fu; // the next iteration depends on this one
        wb[7] = (wb[7] + dist) & 0x1F1F1F1Fu;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * 64 + threadIdx.x] = acc;
    if (threadIdx.x == 0) { clk[2 * blockIdx.x] = t1 - t0; clk[2 * blockIdx.x + 1] = r1 - r0; }
}

template <int CORE>
static double run(int cus, int w, uint32_t cols, uint32_t *first)
{
    const int blocks = cus * 4 * w; // one wave per block
    uint32_t *d;
    unsigned long long *c;
    (void)hipMalloc(&d, (size_t)blocks * 64 * 4);
    (void)hipMalloc(&c, (size_t)blocks * 16);
    const int iters = 4000;
    hipLaunchKernelGGL(k<CORE>, dim3(blocks), dim3(64), 0, 0, d, c, 12345u, 200, cols);
    (void)hipDeviceSynchronize();
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a);
    hipLaunchKernelGGL(k<CORE>, dim3(blocks), dim3(64), 0, 0, d, c, 12345u, iters, cols);
    (void)hipEventRecord(b);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    unsigned long long *h = new unsigned long long[2 * blocks];
    (void)hipMemcpy(h, c, (size_t)blocks * 16, hipMemcpyDeviceToHost);
    uint32_t ho[64];
    (void)hipMemcpy(ho, d, sizeof ho, hipMemcpyDeviceToHost);
    uint32_t sum = 0;
    for (int i = 0; i < 64; ++i) sum = sum * 31u + ho[i];
    *first = sum;
    double cyc = 0, rt = 0;
    for (int i = 0; i < blocks; ++i) { cyc += (double)h[2 * i]; rt += (double)h[2 * i + 1]; }
    cyc /= blocks; rt /= blocks;
    const double ghz = cyc / rt * 0.1;
    const double per_iter = ms * 1e-3 * ghz * 1e9 / ((double)iters * w);
    printf("core %s columns=%2u waves/SIMD=%d: %.3f ms, clock %.2f GHz, %.0f cycles of SIMD time per iteration (64 pairs)\n",
           CORE == 1 ? "bit-fill" : "ptab    ", cols, w, ms, ghz, per_iter);
    delete[] h;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    (void)hipFree(d); (void)hipFree(c);
    return per_iter;
}

int main()
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) { printf("no device\n"); return 1; }
    const int cus = p.multiProcessorCount;
    int differ = 0;
    for (int w : {4, 5})
        for (uint32_t cols : {8u, 12u, 16u, 32u}) {
            uint32_t s1, s2;
            const double c1 = run<1>(cus, w, cols, &s1);
            const double c2 = run<2>(cus, w, cols, &s2);
            printf("   results %s (%08x %08x), ptab / bit-fill = %.3f\n", s1 == s2 ? "agree" : "DIFFER", s1, s2, c2 / c1);
            differ += s1 != s2;
        }
    return differ ? 2 : 0;
}
