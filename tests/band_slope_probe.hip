// band_interval_slope (csrc/ttm_band_image.h) on the device, for tests/test_band_slopes.py: reads quadruples {x_lo, x_hi, y_lo, y_hi}
// of doubles from a file, writes one slope per quadruple to another.  Compiled with the library's flags (no contraction).
//     band_slope_probe IN OUT
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ttm_band_image.h"

__global__ void k_slope_probe(const double* __restrict__ q, long long n, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = band_interval_slope(q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
}

#define CHECK(call)                                                                   \
    do {                                                                              \
        const hipError_t e_ = (call);                                                 \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const long long n = bytes / 32;
    std::vector<double> in((size_t)4 * n), res((size_t)n);
    if (n < 1 || fread(in.data(), 32, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    double *dq = nullptr, *dout = nullptr;
    CHECK(hipMalloc(&dq, (size_t)32 * n));
    CHECK(hipMalloc(&dout, (size_t)8 * n));
    CHECK(hipMemcpy(dq, in.data(), (size_t)32 * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_slope_probe, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, 0, dq, n, dout);
    CHECK(hipGetLastError());
    CHECK(hipMemcpy(res.data(), dout, (size_t)8 * n, hipMemcpyDeviceToHost));
    CHECK(hipFree(dq));
    CHECK(hipFree(dout));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(res.data(), 8, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    return 0;
}
