// ttm_smc.h - the temperature search of sequential Monte Carlo with adaptive tempering (ttm_temper_scan of include/ttm.h;
// DESIGN.md section 4): the per-row routines the kernels k_temper_sums / k_temper_finish of csrc/ttm_kernels.hip and the host
// definition of the entry point share.  Included at the end of csrc/ttm_rng.h, after ttm_resample.h (weight_q, weight_sq,
// weight_bits, halving_sum come from there) and ttm_mcmc.h (whose ttm_mh_step_tempered is the other device piece of an SMC run).
//
// The particles of a tempered run carry their UNTEMPERED log-weights l_i = log p - log q; moving the exponent from beta to
// beta + delta reweights them by exp(delta l_i).  Candidate c of a search is the vector v_i = fl(delta_c l_i) - ONE correctly
// rounded product - and its summary is, word for word, what ttm_weight_scan writes for that vector.  delta_c > 0 and rounding
// is monotone, so max_i fl(delta_c l_i) = fl(delta_c max_i l_i): the maximum of logw is found once for all candidates.
#pragma once

#include <math.h>
#include <stdint.h>

namespace ttm {

enum { TS_CMAX = 64 };                                  // candidates of one call

// the candidates as the kernels take them: by value, so a call reads the caller's host array once and a captured graph keeps them
struct TemperDeltas { double d[TS_CMAX]; };

// fl(delta * x), one rounding, and never the first half of an FMA: weight_q subtracts the tempered maximum from this product,
// and a compiler that contracts a * b - c (hipcc does by default) would form fma(delta, x, -m_c) - the difference of the EXACT
// product, not that of the rounded one ttm_weight_scan sees in a pre-multiplied vector.  The library and the host double are
// built with -ffp-contract=off; the pragma keeps the product whole under any other flags too.
TTM_HD double temper_mul(double delta, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return delta * x;
}

// q of row value x under candidate delta, whose tempered maximum is mc = temper_mul(delta, m)
TTM_HD uint64_t temper_q(double delta, double x, double mc, int K) { return weight_q(temper_mul(delta, x), mc, K); }

// argument check of ttm_temper_scan, shared by the library and the host definition below (delta is a host array)
inline bool temper_scan_args_ok(const double* logw, int64_t N, const double* delta, int32_t C, const ttm_weight_summary* summaries, const void* work) {
    if (!logw || !delta || !summaries || !work || N < 1 || N > ((int64_t)1 << RS_NMAX_LOG2) || C < 1 || C > TS_CMAX) return false;
    for (int c = 0; c < C; ++c) {
        if (!(delta[c] > 0.0) || delta[c] == INFINITY) return false;       // (NaN fails the comparison)
    }
    return true;
}

}  // namespace ttm

#if !defined(__HIPCC__)
#include <vector>
// HOST BUILDS ONLY (as ttm_weight_scan in csrc/ttm_resample.h): the entry point for the host test double of the C ABI.  The maximum
// and the bad count once, then every candidate row after row; S2 per tile of RS_TILE rows and over the tiles by halving, as the
// host ttm_weight_scan sums it.  The workspace is not used.
extern "C" __attribute__((used, visibility("default"))) inline int ttm_temper_scan(const double* logw, int64_t N, const double* delta, int32_t C,
                                                                                   ttm_weight_summary* summaries, void* work, void*) {
    if (!ttm::temper_scan_args_ok(logw, N, delta, C, summaries, work)) return TTM_E_ARG;
    const int K = ttm::weight_bits(N);
    double m = -INFINITY;
    uint64_t bad = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (ttm::weight_valid(logw[i])) m = logw[i] > m ? logw[i] : m; else ++bad;
    }
    const int64_t ntiles = (N + ttm::RS_TILE - 1) / ttm::RS_TILE;
    std::vector<double> tiles((size_t)ntiles), sq(ttm::RS_TILE);
    for (int c = 0; c < C; ++c) {
        const double mc = ttm::temper_mul(delta[c], m);
        uint64_t T = 0;
        for (int64_t b = 0; b < N; b += ttm::RS_TILE) {
            const int64_t n = N - b < ttm::RS_TILE ? N - b : ttm::RS_TILE;
            for (int64_t i = 0; i < n; ++i) {
                const uint64_t qi = ttm::temper_q(delta[c], logw[b + i], mc, K);
                T += qi;
                sq[(size_t)i] = ttm::weight_sq(qi, K);
            }
            tiles[(size_t)(b / ttm::RS_TILE)] = ttm::halving_sum(sq.data(), n);
        }
        summaries[c].m = mc;
        summaries[c].T = T;
        summaries[c].S2 = ttm::halving_sum(tiles.data(), ntiles);
        summaries[c].bad = bad;
    }
    return TTM_OK;
}
#endif
