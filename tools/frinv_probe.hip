// What the running-product scan of csrc/frscan.hip is measured against, and what its one inversion costs (tools/, not
// product code; tools/frscan_timing.py builds and runs it).  Build:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value tools/frinv_probe.hip -o tools/frinv_probe
// Usage: frinv_probe <log2 n> [<log2 n> ..]; one line of key=value pairs per measurement.
//   per_lane     a lane per element computing a^(r-2): 254 squarings and 126 products, and the two conversions of standard I/O
//   one_lane     the same chain in ONE lane of one wave: the latency of the scan's single inversion were it a launch of its own
//   round_trip   the alternative: 32 bytes to the host, Fr::inv there, 32 bytes back, the stream drained twice
//   mul_rate     Fr::mul (field.hpp, 8 x 32-bit) with operands in registers, every SIMD busy: products per second
#include "../rapidsnark-old_amd/csrc/field.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <vector>
using namespace zk;

__device__ __forceinline__ Fr inv_chain(const Fr &a) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FrParams::P[i];
    e[0] -= 2;
    Fr result = Fr::one(), base = a;
#pragma unroll 1
    for (int i = 0; i < 254; i++) {
        if (e[0] & 1u) result = Fr::mul(result, base);
        base = Fr::sqr(base);
#pragma unroll
        for (int q = 0; q < 7; q++) e[q] = (e[q] >> 1) | (e[q + 1] << 31);
        e[7] >>= 1;
    }
    return result;
}

__global__ __launch_bounds__(256) void k_inverse_per_lane(Fr *out, const Fr *__restrict__ in, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = Fr::from_mont(inv_chain(Fr::to_mont(in[i])));
}

__global__ __launch_bounds__(64) void k_inverse_one_lane(Fr *out, const Fr *__restrict__ in) {
    if (threadIdx.x == 0) out[0] = inv_chain(in[0]);
}

__global__ __launch_bounds__(256) void k_mul_rate(Fr *out, const Fr *__restrict__ in, uint32_t iters) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    Fr a = in[t & 1023u], y = in[(t + 7u) & 1023u];
    for (uint32_t i = 0; i < iters; i++) {
        a = Fr::mul(a, y);
        y.v[0] ^= i & 3u;
    }
    out[t] = a;
}

template <class F>
static double median_ms(F launch, int reps = 5) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    launch();
    hipDeviceSynchronize();
    std::vector<double> t;
    for (int r = 0; r < reps; r++) {
        hipEventRecord(e0, 0);
        launch();
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main(int argc, char **argv) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) {
        printf("no device\n");
        return 1;
    }
    const int cus = prop.multiProcessorCount;
    uint64_t nmax = 1024;
    for (int a = 1; a < argc; a++) nmax = std::max<uint64_t>(nmax, 1ull << atoi(argv[a]));
    std::vector<uint32_t> h(nmax * 8);
    for (size_t i = 0; i < h.size(); i++) h[i] = (uint32_t)(i * 2654435761u) >> ((i & 7) == 7 ? 4 : 0);      // below 2^252 < r
    Fr *in, *out;
    if (hipMalloc(&in, nmax * sizeof(Fr)) != hipSuccess || hipMalloc(&out, std::max<uint64_t>(nmax, (uint64_t)cus * 8 * 256) * sizeof(Fr)) != hipSuccess) {
        printf("allocation failed\n");
        return 1;
    }
    hipMemcpy(in, h.data(), nmax * sizeof(Fr), hipMemcpyHostToDevice);

    const uint32_t iters = 2000;
    for (int wps = 1; wps <= 8; wps *= 2) {
        const int blocks = cus * wps;              // a block = 4 waves = one a SIMD
        const double ms = median_ms([&] { hipLaunchKernelGGL(k_mul_rate, dim3(blocks), dim3(256), 0, 0, out, in, iters); });
        printf("mul_rate waves_per_simd=%d products_per_s=%.4g\n", wps, (double)blocks * 256 * iters / (ms * 1e-3));
    }
    printf("one_lane ms=%.4f\n", median_ms([&] { hipLaunchKernelGGL(k_inverse_one_lane, dim3(1), dim3(64), 0, 0, out, in); }));
    {
        Fr x, y;
        std::vector<double> t;
        for (int r = 0; r < 6; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            hipMemcpyAsync(&x, in, sizeof x, hipMemcpyDeviceToHost, 0);
            hipStreamSynchronize(0);
            y = Fr::inv(x);
            hipMemcpyAsync(out, &y, sizeof y, hipMemcpyHostToDevice, 0);
            hipStreamSynchronize(0);
            t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(t.begin() + 1, t.end());             // the first is the warm-up
        printf("round_trip ms=%.4f\n", t[1 + 2]);
    }
    for (int a = 1; a < argc; a++) {
        const uint64_t n = 1ull << atoi(argv[a]);
        const double ms = median_ms([&] { hipLaunchKernelGGL(k_inverse_per_lane, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, out, in, n); });
        printf("per_lane n=%llu ms=%.4f\n", (unsigned long long)n, ms);
    }
    // a^-1 a = 1 for the first element of the last run
    Fr a, b;
    hipMemcpy(&a, in, sizeof a, hipMemcpyDeviceToHost);
    hipMemcpy(&b, out, sizeof b, hipMemcpyDeviceToHost);
    const Fr one = Fr::from_mont(Fr::mul(Fr::to_mont(a), Fr::to_mont(b)));
    printf("check %s\n", argc > 1 && one.v[0] == 1 && (one.v[1] | one.v[7]) == 0 ? "ok" : (argc > 1 ? "FAILED" : "skipped"));
    return 0;
}
