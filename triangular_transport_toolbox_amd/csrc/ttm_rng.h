// ttm_rng.h - counter-based normal deviates for the observation-noise draws of the device-resident EnTF loop
// (example_06.py:286-288 draws them with np.random: synthetic input, any generator will do - this one is stateless, so a
// draw depends only on (seed, stream, row) and the filter is reproducible whatever the launch geometry) and for the
// reference draws of a fitted map (ttm_normal_fill: normal_pair, two deviates per block).
// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw 2011) + Box-Muller on two 53-bit uniforms.
// Beside them the quasi-Monte Carlo reference draws (ttm_sobol_normal_fill): Sobol' points from a table of direction numbers,
// pushed through the normal quantile function (normal_quantile: Wichura's AS 241).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/ttm.h"
#include "ttm_math.h"
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

// The normal quantile function: z with Phi(z) = u, for 2^-31 <= u <= 1 - 2^-31 (what a 30-bit point (q + 0.5) 2^-30 can be; outside
// that range the result is unspecified).  Algorithm AS 241, routine PPND16 (M. J. Wichura, "The percentage points of the normal
// distribution", Applied Statistics 37 (1988) 477-484; stated relative accuracy about 1e-16), restated: with q = u - 1/2,
//   |q| <= 0.425:  z = q A(r) / B(r),  r = 0.180625 - q^2
//   otherwise:     z = sign(q) C(r - 1.6) / D(r - 1.6),  r = sqrt(-log min(u, 1 - u))        (r <= 5)
// A .. D of degree 7.  The routine's third piece (r > 5: min(u, 1 - u) < exp(-25) = 1.4e-11) cannot be reached from u >= 2^-31,
// where r <= sqrt(31 log 2) = 4.64, and is left out.  Both pieces are evaluated for every argument and ONE quotient is formed of
// the selected numerator and denominator: in a wave of 64 Sobol' entries some lane is a tail entry nearly always (15 % of them
// are), so a branch would run both pieces anyway, with two divisions.  log and the quotient are ttm_math.h's (fast_log_normal, fast_div1:
// their arguments are normal numbers here); the N arguments of a call run as independent chains.
// The coefficients a0 .. a7, b0 (= 1) .. b7, c0 .. c7, d0 (= 1) .. d7, kept in constant memory as g_exp_coef is: scalar operands
// of the FMAs, no vector register and no move per step.  (As there: in a hipcc build the array exists on the device only - the host
// pass of a .hip file would read its uninitialised shadow, so normal_quantile has no host caller under __HIPCC__; host builds take
// the const array below.  One translation unit includes this header, so the definition in a header is not a duplicate.)
#if defined(__HIPCC__)
__device__ double g_ppnd16_coef[32] = {
#else
static const double g_ppnd16_coef[32] = {
#endif
    3.3871328727963666080e0,   1.3314166789178437745e+2,  1.9715909503065514427e+3,  1.3731693765509461125e+4,
    4.5921953931549871457e+4,  6.7265770927008700853e+4,  3.3430575583588128105e+4,  2.5090809287301226727e+3,
    1.0,                       4.2313330701600911252e+1,  6.8718700749205790830e+2,  5.3941960214247511077e+3,
    2.1213794301586595867e+4,  3.9307895800092710610e+4,  2.8729085735721942674e+4,  5.2264952788528545610e+3,
    1.42343711074968357734e0,  4.63033784615654529590e0,  5.76949722146069140550e0,  3.64784832476320460504e0,
    1.27045825245236838258e0,  2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4,
    1.0,                       2.05319162663775882187e0,  1.67638483018380384940e0,  6.89767334985100004550e-1,
    1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9};

// sqrt(y) for 0.5 <= y <= 32 (-log min(u, 1 - u) lies in [0.69, 21.5]): v_rsq_f64 (2^-23 or better), one coupled
// Newton step for sqrt and 1 / (2 sqrt) and the residual correction - 8 instructions, no range scaling and no special
// cases, within 1 ulp of the library's sqrt (13 instructions), which the host build calls.
TTM_HD double sqrt_midrange(double y) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double s = __builtin_amdgcn_rsq(y);
    double g = y * s, h = 0.5 * s;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g);
    h = fma(h, r, h);
    return fma(fma(-g, g, y), h, g);
#else
    return sqrt(y);
#endif
}

template <int N>
TTM_HD void normal_quantiles(const double* u, double* z) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) double* kc = (const __attribute__((address_space(4))) double*)g_ppnd16_coef;
#else
    const double* kc = g_ppnd16_coef;
#endif
    double q[N], rc[N], rt[N], a[N], b[N], c[N], d[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        q[i] = u[i] - 0.5;
        rc[i] = 0.180625 - q[i] * q[i];
        rt[i] = sqrt_midrange(-fast_log_normal(fmin(u[i], 1.0 - u[i]))) - 1.6;
        a[i] = kc[7]; b[i] = kc[15]; c[i] = kc[23]; d[i] = kc[31];
    }
#pragma unroll
    for (int k = 6; k >= 0; --k) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            a[i] = fma(a[i], rc[i], kc[k]);
            b[i] = fma(b[i], rc[i], kc[8 + k]);
            c[i] = fma(c[i], rt[i], kc[16 + k]);
            d[i] = fma(d[i], rt[i], kc[24 + k]);
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool central = fabs(q[i]) <= 0.425;
        z[i] = fast_div1(central ? q[i] * a[i] : copysign(c[i], q[i]), central ? b[i] : d[i]);
    }
}

TTM_HD double normal_quantile(double u) {
    double z;
    normal_quantiles<1>(&u, &z);
    return z;
}

// The Sobol' reference draws (ttm_sobol_normal_fill).  Global row i < 2^30 of a column with the direction numbers d[0 .. 29] and the
// digital shift s is the point q = s ^ XOR over the set bits b of the Gray code i ^ (i >> 1) of d[b]  (include/ttm.h).
// With i = 256 hi + t the Gray code splits: its bits 8 .. 29 are the Gray code of hi, its bits 0 .. 7 are t ^ (t >> 1) with bit 7
// flipped when hi is odd.  So q = sobol_high(d, s, hi) ^ sobol_low(d, t): the first is shared by the 256 rows of an aligned block
// (one per workgroup, column and block of rows), the second by the same t in every block (one per thread and column).
// A workgroup takes SOBOL_ROWS aligned blocks of 2^SOBOL_LOW rows (2^SOBOL_SPAN rows in all) of at most SOBOL_TILE columns.
enum { SOBOL_BITS = 30, SOBOL_LOW = 8, SOBOL_ROWS = 4, SOBOL_SPAN = 10, SOBOL_TILE = 16 };

TTM_HD uint32_t sobol_low(const uint32_t* d, uint32_t t) {
    const uint32_t g = t ^ (t >> 1);
    uint32_t q = 0;
    for (int b = 0; b < SOBOL_LOW; ++b) q ^= (0u - ((g >> b) & 1u)) & d[b];
    return q;
}

TTM_HD uint32_t sobol_high(const uint32_t* d, uint32_t s, uint32_t hi) {
    const uint32_t g = hi ^ (hi >> 1);
    uint32_t q = s ^ ((0u - (hi & 1u)) & d[SOBOL_LOW - 1]);
    for (int b = SOBOL_LOW; b < SOBOL_BITS; ++b) q ^= (0u - ((g >> (b - SOBOL_LOW)) & 1u)) & d[b];
    return q;
}

// What one thread of k_sobol_normal_fill does in one column `col` (its row 0 = global row row0): the global rows
// 256 (SOBOL_ROWS blk + r) + t, r < SOBOL_ROWS, that lie in the window [row0, row0 + N) - consecutive t are consecutive rows.
// low = sobol_low(d, t), high[r] = sobol_high(d, s, SOBOL_ROWS blk + r).  The quantiles are formed together, then stored.
TTM_HD void sobol_fill_rows(double* col, int64_t N, int64_t row0, int64_t blk, uint32_t t, uint32_t low, const uint32_t* high) {
    double u[SOBOL_ROWS], z[SOBOL_ROWS];
    for (int r = 0; r < SOBOL_ROWS; ++r) u[r] = ((double)(low ^ high[r]) + 0.5) * (1.0 / 1073741824.0);
    normal_quantiles<SOBOL_ROWS>(u, z);
    for (int r = 0; r < SOBOL_ROWS; ++r) {                       // (32-bit: global rows and N are at most 2^30; a row before the window wraps)
        const uint32_t n = ((((uint32_t)blk * SOBOL_ROWS + r) << SOBOL_LOW) | t) - (uint32_t)row0;
        if (n < (uint32_t)N) col[n] = z[r];
    }
}

// argument check of ttm_sobol_normal_fill, shared by the library and the host definition below; the blocks of
// SOBOL_ROWS 2^SOBOL_LOW aligned global rows that the window [row0, row0 + N) touches, from row0 >> SOBOL_SPAN on
TTM_HD bool sobol_fill_args_ok(const double* Zsoa, int64_t ldz, int64_t N, int32_t ncols, const uint32_t* dirs, int64_t row0) {
    return Zsoa && dirs && N >= 1 && ncols >= 1 && ldz >= N && row0 >= 0 && row0 <= ((int64_t)1 << SOBOL_BITS) && N <= ((int64_t)1 << SOBOL_BITS) - row0;
}

TTM_HD int64_t sobol_fill_blocks(int64_t N, int64_t row0) { return ((row0 + N - 1) >> SOBOL_SPAN) - (row0 >> SOBOL_SPAN) + 1; }

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

// likewise ttm_sobol_normal_fill: the kernel's thread body, block after block, column after column, thread after thread
extern "C" __attribute__((used, visibility("default"))) inline int ttm_sobol_normal_fill(double* Zsoa, int64_t ldz, int64_t N, int32_t ncols, const uint32_t* dirs,
                                                                                         const uint32_t* shift, int64_t row0, void*) {
    if (!ttm::sobol_fill_args_ok(Zsoa, ldz, N, ncols, dirs, row0)) return TTM_E_ARG;
    const int64_t blk0 = row0 >> ttm::SOBOL_SPAN, nblk = ttm::sobol_fill_blocks(N, row0);
    for (int64_t blk = blk0; blk < blk0 + nblk; ++blk)
        for (int32_t j = 0; j < ncols; ++j) {
            const uint32_t* d = dirs + (int64_t)j * ttm::SOBOL_BITS;
            uint32_t high[ttm::SOBOL_ROWS];
            for (int r = 0; r < ttm::SOBOL_ROWS; ++r) high[r] = ttm::sobol_high(d, shift ? shift[j] : 0u, (uint32_t)(blk * ttm::SOBOL_ROWS + r));
            for (uint32_t t = 0; t < (1u << ttm::SOBOL_LOW); ++t) ttm::sobol_fill_rows(Zsoa + (int64_t)j * ldz, N, row0, blk, t, ttm::sobol_low(d, t), high);
        }
    return TTM_OK;
}
#endif

// importance weights and resampling: the Philox blocks of the thresholds and the routines of ttm_weight_scan / ttm_resample
#include "ttm_resample.h"

// Metropolis-Hastings in the reference space of a fitted map: the accept uniforms and the routines of ttm_mh_step
#include "ttm_mcmc.h"

// sequential Monte Carlo with adaptive tempering: the routines of ttm_temper_scan (its step is ttm_mh_step_tempered of ttm_mcmc.h)
#include "ttm_smc.h"
