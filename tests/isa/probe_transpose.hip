// Probe for tests/test_gpu_transpose_probe.py: blk::transpose64 as the product's kernels use it -- one workgroup of 16 waves,
// every wave with its own RW-word region of the LDS -- on blocks whose 16 x 4096 values are all distinct.  Each wave transposes its
// 64 x 64 block and transposes it back; the host checks both images exactly (the routine only moves data).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "srx_block.hpp"

using namespace srx;

constexpr int NWAVE = 16, BLK = 64 * 64;

extern "C" __global__ void __launch_bounds__(64 * NWAVE) k_probe_t64(const float *__restrict__ in, float *__restrict__ out_t, float *__restrict__ out_back)
{
    __shared__ __attribute__((aligned(16))) float lds[NWAVE * blk::RW];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int base = wave * BLK;  // < NWAVE * BLK: every access below stays inside the three NWAVE * BLK buffers
    float a[64], r[64];
#pragma unroll
    for (int i = 0; i < 64; i++)
        a[i] = in[base + i * 64 + lane];
    blk::transpose64(a, r, lds + wave * blk::RW, lane);
#pragma unroll
    for (int i = 0; i < 64; i++)
        out_t[base + i * 64 + lane] = r[i];
    blk::transpose64(r, a, lds + wave * blk::RW, lane);
#pragma unroll
    for (int i = 0; i < 64; i++)
        out_back[base + i * 64 + lane] = a[i];
}

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            std::printf("%s: %s\n", #x, hipGetErrorString(e_));                        \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

int main()
{
    const size_t n = (size_t)NWAVE * BLK;
    std::vector<float> h(n), t(n), b(n);
    for (size_t i = 0; i < n; i++)
        h[i] = (float)(i + 1);  // < 2^24: exact and distinct
    float *d_in, *d_t, *d_b;
    CHECK(hipMalloc(&d_in, n * sizeof(float)));
    CHECK(hipMalloc(&d_t, n * sizeof(float)));
    CHECK(hipMalloc(&d_b, n * sizeof(float)));
    CHECK(hipMemcpy(d_in, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    CHECK(hipMemset(d_t, 0, n * sizeof(float)));
    CHECK(hipMemset(d_b, 0, n * sizeof(float)));
    hipLaunchKernelGGL(k_probe_t64, dim3(1), dim3(64 * NWAVE), 0, 0, d_in, d_t, d_b);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(t.data(), d_t, n * sizeof(float), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), d_b, n * sizeof(float), hipMemcpyDeviceToHost));
    long bad_t = 0, bad_b = 0;
    for (int w = 0; w < NWAVE; w++)
        for (int i = 0; i < 64; i++)
            for (int l = 0; l < 64; l++) {
                // r[i] at lane l is element (l, i) of the block
                if (t[(size_t)w * BLK + i * 64 + l] != h[(size_t)w * BLK + l * 64 + i]) {
                    if (bad_t++ < 8)
                        std::printf("transpose: wave %d out[%d][%d] = %.0f, want %.0f\n", w, i, l, t[(size_t)w * BLK + i * 64 + l], h[(size_t)w * BLK + l * 64 + i]);
                }
                if (b[(size_t)w * BLK + i * 64 + l] != h[(size_t)w * BLK + i * 64 + l]) {
                    if (bad_b++ < 8)
                        std::printf("back: wave %d out[%d][%d] = %.0f, want %.0f\n", w, i, l, b[(size_t)w * BLK + i * 64 + l], h[(size_t)w * BLK + i * 64 + l]);
                }
            }
    hipFree(d_in), hipFree(d_t), hipFree(d_b);
    std::printf("transpose probe: %d waves, %ld wrong transposed, %ld wrong after the way back\n", NWAVE, bad_t, bad_b);
    if (bad_t || bad_b)
        return 1;
    std::printf("transpose probe OK\n");
    return 0;
}
