// Microbenchmark (tuning aid, not part of the product): launch shapes of the reference-draw fill around the thread body the
// library runs (csrc/ttm_rng.h: normal_fill_pair) - workgroups of 64 / 256 / 1024 threads, the columns walked by one thread or
// spread over blockIdx.y, the 16-byte store path (even row0) against the 8-byte one (odd row0) - and, for the floor of each
// half, the same grid with the stores alone (constants) and with the arithmetic alone (one store per thread).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/micro/normal_fill.hip -o tools/micro/normal_fill
//   tools/micro/normal_fill [rows = 1000000] [columns = 40]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../triangular_transport_toolbox_amd/csrc/ttm_rng.h"

using namespace ttm;

// MODE 0: the library's body; 1: stores only; 2: arithmetic only
template <int BLOCK, int MODE>
__global__ __launch_bounds__(BLOCK) void k_fill(double* __restrict__ Z, int64_t ldz, int64_t N, int ncols, uint64_t seed, uint32_t draw, int64_t row0) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (MODE == 0) {
        normal_fill_pair(Z, ldz, N, ncols, 0, seed, draw, row0, i, (int)blockIdx.y, (int)gridDim.y);
        return;
    }
    const int64_t n0 = 2 * i;
    if (n0 + 1 >= N) return;
    double acc = 0.0;
    for (int j = blockIdx.y; j < ncols; j += gridDim.y) {
        if (MODE == 1) {
            store_pair(Z + (int64_t)j * ldz + n0, 1.0 + j, 2.0 + j);
        } else {
            double z0, z1;
            normal_pair(seed, draw, (uint32_t)j, (uint64_t)i, z0, z1);
            acc += z0 * z1;
        }
    }
    if (MODE == 2) Z[(int64_t)blockIdx.y * ldz + n0] = acc;
}

struct Shape { const char* name; int block, mode, gy; int64_t row0; };

template <int BLOCK, int MODE>
static void launch(double* Z, int64_t ldz, int64_t N, int ncols, int gy, int64_t row0) {
    const int64_t np = ((row0 + N - 1) >> 1) - (row0 >> 1) + 1;
    hipLaunchKernelGGL((k_fill<BLOCK, MODE>), dim3((unsigned)((np + BLOCK - 1) / BLOCK), (unsigned)gy), dim3(BLOCK), 0, 0, Z, ldz, N, ncols,
                       (uint64_t)5, (uint32_t)0, row0);
}

static void run(const Shape& s, double* Z, int64_t ldz, int64_t N, int ncols) {
    const int gy = s.gy < 1 ? ncols : std::min(s.gy, ncols);
    if (s.block == 64) launch<64, 0>(Z, ldz, N, ncols, gy, s.row0);
    else if (s.block == 1024) launch<1024, 0>(Z, ldz, N, ncols, gy, s.row0);
    else if (s.mode == 1) launch<256, 1>(Z, ldz, N, ncols, gy, s.row0);
    else if (s.mode == 2) launch<256, 2>(Z, ldz, N, ncols, gy, s.row0);
    else launch<256, 0>(Z, ldz, N, ncols, gy, s.row0);
}

int main(int argc, char** argv) {
    const int64_t N = argc > 1 ? atoll(argv[1]) : 1000000;
    const int ncols = argc > 2 ? atoi(argv[2]) : 40;
    const int64_t ldz = N + 2 + (N & 1);                                 // (room for the odd-row0 window)
    double* Z = nullptr;
    if (hipMalloc(&Z, (size_t)ldz * ncols * 8) != hipSuccess) { printf("no device memory\n"); return 1; }
    const Shape shapes[] = {
        {"256 threads, columns in the thread", 256, 0, 1, 0},       {"256 threads, 2 column groups", 256, 0, 2, 0},
        {"256 threads, 4 column groups", 256, 0, 4, 0},             {"256 threads, 8 column groups", 256, 0, 8, 0},
        {"256 threads, a block row per column", 256, 0, 0, 0},      {"64 threads, columns in the thread", 64, 0, 1, 0},
        {"64 threads, 4 column groups", 64, 0, 4, 0},               {"1024 threads, columns in the thread", 1024, 0, 1, 0},
        {"1024 threads, 4 column groups", 1024, 0, 4, 0},           {"256 threads, odd row0 (8-byte stores)", 256, 0, 1, 1},
        {"256 threads, odd row0, 4 column groups", 256, 0, 4, 1},   {"stores alone, 256 threads", 256, 1, 1, 0},
        {"arithmetic alone, 256 threads", 256, 2, 1, 0},            {"arithmetic alone, 4 column groups", 256, 2, 4, 0},
    };
    const int ns = (int)(sizeof(shapes) / sizeof(shapes[0])), rounds = 7, per = 20;
    std::vector<std::vector<float>> ms(ns);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int s = 0; s < ns; ++s) for (int i = 0; i < 3; ++i) run(shapes[s], Z, ldz, N, ncols);          // warm-up of every shape
    for (int i = 0; i < 300; ++i) run(shapes[0], Z, ldz, N, ncols);                                      // a busy chip holds its clock
    if (hipDeviceSynchronize() != hipSuccess) { printf("a launch failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    for (int r = 0; r < rounds; ++r)
        for (int s = 0; s < ns; ++s) {
            run(shapes[s], Z, ldz, N, ncols);
            hipEventRecord(e0);
            for (int i = 0; i < per; ++i) run(shapes[s], Z, ldz, N, ncols);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            float t;
            hipEventElapsedTime(&t, e0, e1);
            ms[s].push_back(t / per);
        }
    printf("rows %lld, columns %d, %.1f MB written; median (min .. max) of %d rounds of %d launches\n", (long long)N, ncols, 8e-6 * N * ncols, rounds, per);
    for (int s = 0; s < ns; ++s) {
        std::sort(ms[s].begin(), ms[s].end());
        const double med = ms[s][rounds / 2];
        printf("%-42s %.4f ms (%.4f .. %.4f)  %.2f TB/s\n", shapes[s].name, med, ms[s].front(), ms[s].back(), 8e-9 * N * ncols / med);
    }
    hipFree(Z);
    return 0;
}
