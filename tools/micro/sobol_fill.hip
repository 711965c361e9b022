// Microbenchmark (tuning aid, not part of the product): launch shapes of the Sobol' reference-draw fill around the routines the
// library runs (csrc/ttm_rng.h: sobol_low, sobol_high, normal_quantile) - 1 / 2 / 4 / 8 aligned blocks of 256 rows per workgroup,
// 1 .. 16 columns per workgroup - beside the Philox fill on the same buffer and, for the floor of each part, the same grid with
// the stores alone (constants), the points alone (the integer half and the conversion, no quantile), the quantile alone (one
// store per thread) and a quantile that branches between its two pieces instead of selecting.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/micro/sobol_fill.hip -o tools/micro/sobol_fill
//   tools/micro/sobol_fill [rows = 1000000] [columns = 40]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../triangular_transport_toolbox_amd/csrc/ttm_rng.h"

using namespace ttm;

__device__ __forceinline__ double horner7(const double* c, double t) {
    double s = c[7];
    for (int k = 6; k >= 0; --k) s = fma(s, t, c[k]);
    return s;
}

// AS 241 as published: a branch per piece, a division in each, the library functions
__device__ __forceinline__ double normal_quantile_branch(double u) {
    const double A[8] = {3.3871328727963666080e0,  1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                         4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3};
    const double B[8] = {1.0,                      4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3,
                         2.1213794301586595867e+4, 3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3};
    const double C[8] = {1.42343711074968357734e0,  4.63033784615654529590e0,  5.76949722146069140550e0,  3.64784832476320460504e0,
                         1.27045825245236838258e0,  2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4};
    const double D[8] = {1.0,                       2.05319162663775882187e0,  1.67638483018380384940e0,  6.89767334985100004550e-1,
                         1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9};
    const double q = u - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * horner7(A, r) / horner7(B, r);
    }
    const double r = sqrt(-log(fmin(u, 1.0 - u))) - 1.6;
    return copysign(horner7(C, r) / horner7(D, r), q);
}

// MODE 0: the library's arithmetic; 1: stores only; 2: points only; 3: quantile only (one store per thread); 4: the branching quantile
template <int ROWS, int MODE>
__global__ __launch_bounds__(256) void k_fill(double* __restrict__ Z, int64_t ldz, int64_t N, int ncols, int tile, const uint32_t* __restrict__ dirs,
                                              const uint32_t* __restrict__ shift, int64_t row0) {
    __shared__ uint32_t s_low[SOBOL_TILE][SOBOL_LOW], s_high[SOBOL_TILE][ROWS];
    const int t = (int)threadIdx.x, j0 = (int)blockIdx.y * tile;
    const int nc = ncols - j0 < tile ? ncols - j0 : tile;
    const int64_t blk = row0 / (256 * ROWS) + (int64_t)blockIdx.x;
    if (t < nc * SOBOL_LOW) {
        s_low[t / SOBOL_LOW][t % SOBOL_LOW] = dirs[(int64_t)(j0 + t / SOBOL_LOW) * SOBOL_BITS + t % SOBOL_LOW];
    } else if (t >= 128 && t - 128 < nc * ROWS) {
        const int c = (t - 128) / ROWS, r = (t - 128) % ROWS;
        s_high[c][r] = sobol_high(dirs + (int64_t)(j0 + c) * SOBOL_BITS, shift[j0 + c], (uint32_t)(blk * ROWS + r));
    }
    __syncthreads();
    double acc = 0.0;
    for (int c = 0; c < nc; ++c) {
        double* col = Z + (int64_t)(j0 + c) * ldz;
        const uint32_t low = sobol_low(s_low[c], (uint32_t)t);
        double u[ROWS], z[ROWS];
        for (int r = 0; r < ROWS; ++r) u[r] = ((double)(low ^ s_high[c][r]) + 0.5) * (1.0 / 1073741824.0);
        if (MODE == 0 || MODE == 3) normal_quantiles<ROWS>(u, z);
        else
            for (int r = 0; r < ROWS; ++r) z[r] = MODE == 1 ? 1.0 + c : MODE == 2 ? u[r] : normal_quantile_branch(u[r]);
        for (int r = 0; r < ROWS; ++r) {
            const uint32_t n = ((((uint32_t)blk * ROWS + r) << SOBOL_LOW) | (uint32_t)t) - (uint32_t)row0;
            if (MODE == 3) acc += z[r];
            else if (n < (uint32_t)N) col[n] = z[r];
        }
    }
    if (MODE == 3 && (int64_t)blockIdx.x * 256 + t < N) Z[(int64_t)j0 * ldz + (int64_t)blockIdx.x * 256 + t] = acc;
}

__global__ __launch_bounds__(256) void k_philox(double* __restrict__ Z, int64_t ldz, int64_t N, int ncols, int64_t row0) {
    normal_fill_pair(Z, ldz, N, ncols, 0, 5, 0, row0, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

struct Shape { const char* name; int rows, mode, tile; int64_t row0; };        // rows 0: the Philox fill, tile = its column groups

static double* Z;
static uint32_t *dirs, *shift;
static int64_t ldz, N;
static int ncols;

template <int ROWS, int MODE>
static void launch(int tile, int64_t row0) {
    const int64_t span = 256 * ROWS, gx = (row0 + N - 1) / span - row0 / span + 1;
    hipLaunchKernelGGL((k_fill<ROWS, MODE>), dim3((unsigned)gx, (unsigned)((ncols + tile - 1) / tile)), dim3(256), 0, 0, Z, ldz, N, ncols, tile, dirs,
                       shift, row0);
}

static void run(const Shape& s) {
    const int tile = std::min(s.tile, ncols);
    if (s.rows == 0) {
        const int64_t np = ((s.row0 + N - 1) >> 1) - (s.row0 >> 1) + 1;
        hipLaunchKernelGGL(k_philox, dim3((unsigned)((np + 255) / 256), (unsigned)tile), dim3(256), 0, 0, Z, ldz, N, ncols, s.row0);
    } else if (s.mode == 1) launch<4, 1>(tile, s.row0);
    else if (s.mode == 2) launch<4, 2>(tile, s.row0);
    else if (s.mode == 3) launch<4, 3>(tile, s.row0);
    else if (s.mode == 4) launch<4, 4>(tile, s.row0);
    else if (s.rows == 1) launch<1, 0>(tile, s.row0);
    else if (s.rows == 2) launch<2, 0>(tile, s.row0);
    else if (s.rows == 8) launch<8, 0>(tile, s.row0);
    else launch<4, 0>(tile, s.row0);
}

int main(int argc, char** argv) {
    N = argc > 1 ? atoll(argv[1]) : 1000000;
    ncols = argc > 2 ? atoi(argv[2]) : 40;
    ldz = N + 2 + (N & 1);
    if (N < 1 || N > (1 << 29) || ncols < 1 || ncols > 4096) { printf("rows in [1, 2^29], columns in [1, 4096]\n"); return 1; }
    std::vector<uint32_t> h((size_t)ncols * (SOBOL_BITS + 1));
    uint32_t x = 12345u;                                                          // any table does for the timing: 30-bit words
    for (auto& w : h) { x = x * 1664525u + 1013904223u; w = x >> 2; }
    if (hipMalloc(&Z, (size_t)ldz * ncols * 8) != hipSuccess || hipMalloc(&dirs, h.size() * 4) != hipSuccess) { printf("no device memory\n"); return 1; }
    shift = dirs + (size_t)ncols * SOBOL_BITS;
    hipMemcpy(dirs, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    const Shape shapes[] = {
        {"philox, 5 column groups (the library's)", 0, 0, 5, 0},
        {"sobol 4 x 256 rows, 1 column / workgroup", 4, 0, 1, 0},   {"sobol 4 x 256 rows, 2 columns", 4, 0, 2, 0},
        {"sobol 4 x 256 rows, 4 columns", 4, 0, 4, 0},              {"sobol 4 x 256 rows, 8 columns", 4, 0, 8, 0},
        {"sobol 4 x 256 rows, 16 columns", 4, 0, 16, 0},            {"sobol 1 x 256 rows, 8 columns", 1, 0, 8, 0},
        {"sobol 2 x 256 rows, 8 columns", 2, 0, 8, 0},              {"sobol 8 x 256 rows, 8 columns", 8, 0, 8, 0},
        {"sobol 4 x 256 rows, 8 columns, row0 = 1", 4, 0, 8, 1},    {"stores alone, 4 x 256, 8 columns", 4, 1, 8, 0},
        {"points alone, 4 x 256, 8 columns", 4, 2, 8, 0},           {"quantile alone, 4 x 256, 8 columns", 4, 3, 8, 0},
        {"branching quantile, 4 x 256, 8 columns", 4, 4, 8, 0},
    };
    const int ns = (int)(sizeof(shapes) / sizeof(shapes[0])), rounds = 7, per = 20;
    std::vector<std::vector<float>> ms(ns);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int s = 0; s < ns; ++s) for (int i = 0; i < 3; ++i) run(shapes[s]);                             // warm-up of every shape
    for (int i = 0; i < 300; ++i) run(shapes[0]);                                                        // a busy chip holds its clock
    if (hipDeviceSynchronize() != hipSuccess) { printf("a launch failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    for (int r = 0; r < rounds; ++r)
        for (int s = 0; s < ns; ++s) {
            run(shapes[s]);
            hipEventRecord(e0);
            for (int i = 0; i < per; ++i) run(shapes[s]);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float t;
            hipEventElapsedTime(&t, e0, e1);
            ms[s].push_back(t / per);
        }
    if (hipDeviceSynchronize() != hipSuccess) { printf("a launch failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    printf("rows %lld, columns %d, %.1f MB written; median (min .. max) of %d rounds of %d launches\n", (long long)N, ncols, 8e-6 * N * ncols, rounds, per);
    for (int s = 0; s < ns; ++s) {
        std::sort(ms[s].begin(), ms[s].end());
        const double med = ms[s][rounds / 2];
        printf("%-44s %.4f ms (%.4f .. %.4f)  %.2f TB/s\n", shapes[s].name, med, ms[s].front(), ms[s].back(), 8e-9 * N * ncols / med);
    }
    hipFree(Z); hipFree(dirs);
    return 0;
}
