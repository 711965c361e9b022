// ttm_rng.h - counter-based normal deviates for the observation-noise draws of the device-resident EnTF loop
// (example_06.py:286-288 draws them with np.random: synthetic input, any generator will do - this one is stateless, so a
// draw depends only on (seed, stream, row) and the filter is reproducible whatever the launch geometry) and for the
// reference draws of a fitted map (ttm_normal_fill: normal_pair, two deviates per block).
// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw 2011) + Box-Muller on two 53-bit uniforms.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/ttm.h"
#include "ttm_vec.h"

namespace ttm {

TTM_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// standard normal deviate number `row` of stream `stream` under `seed`
TTM_HD double normal_deviate(uint64_t seed, uint32_t stream, uint64_t row) {
    uint32_t r[4];
    philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), stream, 0x5EEDu, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const double u1 = ((double)((((uint64_t)r[0] << 32) | r[1]) >> 11) + 0.5) * (1.0 / 9007199254740992.0);   // (0, 1)
    const double u2 = ((double)((((uint64_t)r[2] << 32) | r[3]) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586477 * u2);
}

// The reference draws of a fitted map (ttm_normal_fill): BOTH Box-Muller branches of one Philox block, the standard normal
// deviates of global rows 2p and 2p + 1 of column `col` of draw `draw` (< 2^31) under `seed`.  The counter layout is the
// contract: {lo32(p), hi32(p), col, 0x80000000 | draw}, key {lo32(seed), hi32(seed)} - the set top bit of the
// fourth word keeps these blocks apart from normal_deviate's (0x5EED there), the uniforms are formed as there.
TTM_HD void normal_pair(uint64_t seed, uint32_t draw, uint32_t col, uint64_t p, double& z0, double& z1) {
    uint32_t r[4];
    philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), col, 0x80000000u | draw, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const double u1 = ((double)((((uint64_t)r[0] << 32) | r[1]) >> 11) + 0.5) * (1.0 / 9007199254740992.0);   // (0, 1)
    const double u2 = ((double)((((uint64_t)r[2] << 32) | r[3]) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    const double R = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(6.283185307179586477 * u2, &s, &c);
    z0 = R * c;
    z1 = R * s;
}

// What one thread of k_normal_fill does: pair number i of the window of global rows [row0, row0 + N) - the window's first
// pair is row0 / 2, so with an odd row0 the first thread owns one row of the window and, with the other parity of the end,
// so does the last - in the columns j0, j0 + jstep, ... < ncols.  A pair with both rows in the window at a 16-byte aligned
// address is one 16-byte store; every other one goes out as one or two guarded 8-byte stores.
TTM_HD void normal_fill_pair(double* Zsoa, int64_t ldz, int64_t N, int ncols, int col0, uint64_t seed, uint32_t draw, int64_t row0,
                             int64_t i, int j0, int jstep) {
    const uint64_t p = (uint64_t)(row0 >> 1) + (uint64_t)i;
    const int64_t n0 = (int64_t)(2 * p - (uint64_t)row0);     // local row of global row 2p: -1 .. N - 1
    if (n0 >= N) return;
    const bool whole = n0 >= 0 && n0 + 1 < N;
    for (int j = j0; j < ncols; j += jstep) {
        double z0, z1;
        normal_pair(seed, draw, (uint32_t)col0 + (uint32_t)j, p, z0, z1);
        double* col = Zsoa + (int64_t)j * ldz;
        if (whole && (((uintptr_t)col + 8 * (uintptr_t)n0) & 15) == 0) {
            store_pair(col + n0, z0, z1);
        } else {
            if (n0 >= 0) col[n0] = z0;
            if (n0 + 1 < N) col[n0 + 1] = z1;
        }
    }
}

// one RK4 step of the Lorenz-63 system (example_06.py:28-46, 49-76; sigma 10, rho 28, beta 8/3), operand order as there
TTM_HD void lorenz63_rk4_step(double& x, double& y, double& z, double dt) {
    const double beta = 8.0 / 3.0, rho = 28.0, sigma = 10.0;
    auto f = [&](double a, double b, double c, double& da, double& db, double& dc) {
        da = -sigma * a + sigma * b;
        db = -a * c + rho * a - b;
        dc = a * b - beta * c;
    };
    double k1x, k1y, k1z, k2x, k2y, k2z, k3x, k3y, k3z, k4x, k4y, k4z;
    f(x, y, z, k1x, k1y, k1z);
    f(x + dt / 2 * k1x, y + dt / 2 * k1y, z + dt / 2 * k1z, k2x, k2y, k2z);
    f(x + dt / 2 * k2x, y + dt / 2 * k2y, z + dt / 2 * k2z, k3x, k3y, k3z);
    f(x + dt * k3x, y + dt * k3y, z + dt * k3z, k4x, k4y, k4z);
    x += dt / 6 * (k1x + 2 * k2x + 2 * k3x + k4x);
    y += dt / 6 * (k1y + 2 * k2y + 2 * k3y + k4y);
    z += dt / 6 * (k1z + 2 * k2z + 2 * k3z + k4z);
}

// argument check of ttm_normal_fill, shared by the library and the host definition below
TTM_HD bool normal_fill_args_ok(const double* Zsoa, int64_t ldz, int64_t N, int32_t ncols, int32_t col0, uint32_t draw, int64_t row0) {
    return Zsoa && N >= 1 && ncols >= 1 && col0 >= 0 && ldz >= N && row0 >= 0 && N <= INT64_MAX - row0 && draw < 0x80000000u;
}

// pairs of the window of global rows [row0, row0 + N)
TTM_HD int64_t normal_fill_pairs(int64_t N, int64_t row0) { return ((row0 + N - 1) >> 1) - (row0 >> 1) + 1; }

}  // namespace ttm

#if !defined(__HIPCC__)
// HOST BUILDS ONLY (as ttm_score in csrc/ttm_score.h): the entry point ttm_normal_fill of include/ttm.h for the host test
// double of the C ABI - the kernel's thread body, pair after pair.
extern "C" __attribute__((used, visibility("default"))) inline int ttm_normal_fill(double* Zsoa, int64_t ldz, int64_t N, int32_t ncols, int32_t col0,
                                                                                   uint64_t seed, uint32_t draw, int64_t row0, void*) {
    if (!ttm::normal_fill_args_ok(Zsoa, ldz, N, ncols, col0, draw, row0)) return TTM_E_ARG;
    const int64_t np = ttm::normal_fill_pairs(N, row0);
    for (int64_t i = 0; i < np; ++i) ttm::normal_fill_pair(Zsoa, ldz, N, ncols, col0, seed, draw, row0, i, 0, 1);
    return TTM_OK;
}
#endif
