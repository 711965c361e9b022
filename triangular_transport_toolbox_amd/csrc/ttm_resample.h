// ttm_resample.h - importance weights in fixed point and the resampling of an ensemble (ttm_weight_scan, ttm_resample of
// include/ttm.h): the per-row routines the kernels of csrc/ttm_kernels.hip and the host definitions of the
// two entry points share.  Included at the end of csrc/ttm_rng.h (philox4x32_10 and, through ttm_math.h, fast_exp come from there).
//
// All resampling arithmetic is on unsigned 64-bit integers, so the scan is associative: cum does not depend on the tile, the
// launch or a sharding of the rows.  For N log-weights, 1 <= N <= 2^30:
//   m     = the maximum of the entries that are neither NaN nor +inf (-inf if there is none)
//   K     = min(40, 62 - ceil(log2 N))
//   q_i   = min(2^K, floor(fast_exp(logw_i - m) 2^K)); 2^K exactly where logw_i = m; 0 for -inf, NaN and +inf (the last two `bad`)
//   cum_i = q_0 + ... + q_i,  T = cum_{N-1} <= N 2^K <= 2^62
// A weight below 2^-K of the largest is 0: the mass lost is at most N 2^-K of T (T >= 2^K), 9.1e-7 at N = 10^6, 2.4e-7 at N = 2^18.
#pragma once

#include <math.h>
#include <stdint.h>

namespace ttm {

// the scan tile (rows per workgroup of the three scan kernels: 256 threads x 4 rows) and the tiles one pass of the tile-sum scan holds
enum { RS_TILE = 1024, RS_THREADS = 256, RS_PASS = 256, RS_KMAX = 40, RS_NMAX_LOG2 = 30 };

TTM_HD int weight_bits(int64_t N) {
    int c = 0;
    while (((int64_t)1 << c) < N) ++c;                  // ceil(log2 N)
    return 62 - c < RS_KMAX ? 62 - c : RS_KMAX;
}

// an entry that takes part in the maximum: not NaN, not +inf
TTM_HD bool weight_valid(double logw) { return logw == logw && logw != INFINITY; }

// q of one row.  fast_exp (csrc/ttm_math.h) is within 1 ulp, so the product is within 2^(K - 52) <= 2^-12 of exp(.) 2^K:
// q is within one unit of the exact floor.  The scaling by 2^K is exact, the conversion truncates (= floor, the value is >= 0).
TTM_HD uint64_t weight_q(double logw, double m, int K) {
    const uint64_t one = (uint64_t)1 << K;
    if (!(logw > -INFINITY) || logw == INFINITY) return 0;       // -inf, NaN, +inf
    if (logw >= m) return one;                                    // the row(s) of the maximum
    const uint64_t q = (uint64_t)(fast_exp(logw - m) * (double)one);
    return q < one ? q : one;
}

// (q / 2^K)^2: the quotient is exact (q <= 2^40), the square rounds once
TTM_HD double weight_sq(uint64_t q, int K) {
    const double s = (double)q * (1.0 / (double)((uint64_t)1 << K));
    return s * s;
}

TTM_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The 64-bit random word of block j of a resampling (scheme, seed, draw): counter {lo32(j), hi32(j), 0xFFFFFFFF - scheme,
// 0x80000000 | draw}.  ttm_normal_fill has a column number below 2^31 as its third word and ttm_perturb 0x5EED as its fourth,
// so these blocks are disjoint from both.
TTM_HD uint64_t resample_word(uint64_t seed, uint32_t draw, int scheme, uint64_t j) {
    uint32_t r[4];
    philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), 0xFFFFFFFFu - (uint32_t)scheme, 0x80000000u | draw, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return ((uint64_t)r[0] << 32) | r[1];
}

// Threshold of offspring j < M <= 2^30 from its random word R (systematic: the word of block 0 for every j).  With T = a M + b:
// systematic / stratified t_j = j a + floor((j b + V) / M) = floor((j T + V) / M), V = mulhi64(R, T) < T; j b < 2^60 and
// V < 2^62, so nothing leaves 63 bits.  multinomial t_j = mulhi64(R, T).  0 <= t_j < T (t_j = 0 when T = 0).
TTM_HD uint64_t resample_threshold(uint64_t T, uint64_t M, int scheme, uint64_t j, uint64_t R) {
    const uint64_t V = mulhi64(R, T);
    if (scheme == TTM_RESAMPLE_MULTINOMIAL) return V;
    const uint64_t a = T / M, b = T - a * M;
    return j * a + (j * b + V) / M;
}

// min { i in [lo, hi) : cum[i] > t }, hi if there is none.  Reads cum[lo .. hi - 1] only and ends after at most 31 steps whatever cum holds.
TTM_HD int64_t cum_upper_bound(const uint64_t* cum, int64_t lo, int64_t hi, uint64_t t) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// argument checks of the two entry points, shared by the library and the host definitions below
TTM_HD bool weight_scan_args_ok(const double* logw, int64_t N, const uint64_t* cum, const ttm_weight_summary* summary, const void* work) {
    return logw && cum && summary && work && N >= 1 && N <= ((int64_t)1 << RS_NMAX_LOG2);
}

TTM_HD bool resample_args_ok(const uint64_t* cum, int64_t N, int64_t M, int32_t scheme, uint32_t draw, const double* Xsoa, int64_t ldx, int32_t ncols,
                             const double* Ysoa, int64_t ldy, const int32_t* idx) {
    if (!cum || N < 1 || N > ((int64_t)1 << RS_NMAX_LOG2) || M < 1 || M > ((int64_t)1 << RS_NMAX_LOG2)) return false;
    if (scheme < TTM_RESAMPLE_SYSTEMATIC || scheme > TTM_RESAMPLE_MULTINOMIAL || draw >= 0x80000000u || ncols < 0) return false;
    if (ncols == 0) return idx != nullptr;
    if (!Xsoa || !Ysoa || ldx < N || ldy < M) return false;
    const uintptr_t x0 = (uintptr_t)Xsoa, x1 = x0 + 8 * ((uintptr_t)(ncols - 1) * (uintptr_t)ldx + (uintptr_t)N);
    const uintptr_t y0 = (uintptr_t)Ysoa, y1 = y0 + 8 * ((uintptr_t)(ncols - 1) * (uintptr_t)ldy + (uintptr_t)M);
    return x1 <= y0 || y1 <= x0;                                   // source and destination must not overlap
}

// offspring j of a resampling: its ancestor (-1 when no row has cum > t, i.e. T = 0) from a search of cum[lo .. hi - 1], written to
// idx (if given), and the ncols entries of that row copied (NaN without an ancestor)
TTM_HD void resample_offspring(const uint64_t* cum, int64_t N, int64_t lo, int64_t hi, uint64_t t, int64_t j, const double* Xsoa, int64_t ldx, int ncols,
                               double* Ysoa, int64_t ldy, int32_t* idx) {
    int64_t i = cum_upper_bound(cum, lo, hi, t);
    if (i >= N) i = -1;
    if (idx) idx[j] = (int32_t)i;
    for (int c = 0; c < ncols; ++c) Ysoa[(int64_t)c * ldy + j] = i >= 0 ? Xsoa[(int64_t)c * ldx + i] : NAN;
}

// sum of v[0 .. n - 1] by halving (v is overwritten): a binary tree of depth ceil(log2 n)
inline double halving_sum(double* v, int64_t n) {
    while (n > 1) {
        const int64_t h = (n + 1) >> 1;
        for (int64_t i = 0; i + h < n; ++i) v[i] += v[i + h];
        n = h;
    }
    return n == 1 ? v[0] : 0.0;
}

}  // namespace ttm

#if !defined(__HIPCC__)
#include <vector>
// HOST BUILDS ONLY (as ttm_normal_fill in csrc/ttm_rng.h): the two entry points for the host test double of the C ABI, row after
// row with the routines above.  S2 is summed per tile of RS_TILE rows and then over the tiles by halving: a tree no deeper than the
// kernels' (include/ttm.h).  The workspace is not used.
extern "C" __attribute__((used, visibility("default"))) inline int ttm_weight_scan(const double* logw, int64_t N, uint64_t* cum, uint64_t* q,
                                                                                   ttm_weight_summary* summary, void* work, void*) {
    if (!ttm::weight_scan_args_ok(logw, N, cum, summary, work)) return TTM_E_ARG;
    const int K = ttm::weight_bits(N);
    double m = -INFINITY;
    uint64_t bad = 0, T = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (ttm::weight_valid(logw[i])) m = logw[i] > m ? logw[i] : m; else ++bad;
    }
    std::vector<double> tiles((size_t)((N + ttm::RS_TILE - 1) / ttm::RS_TILE)), sq(ttm::RS_TILE);
    for (int64_t b = 0; b < N; b += ttm::RS_TILE) {
        const int64_t n = N - b < ttm::RS_TILE ? N - b : ttm::RS_TILE;
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t qi = ttm::weight_q(logw[b + i], m, K);
            T += qi;
            cum[b + i] = T;
            if (q) q[b + i] = qi;
            sq[(size_t)i] = ttm::weight_sq(qi, K);
        }
        tiles[(size_t)(b / ttm::RS_TILE)] = ttm::halving_sum(sq.data(), n);
    }
    summary->m = m;
    summary->T = T;
    summary->S2 = ttm::halving_sum(tiles.data(), (int64_t)tiles.size());
    summary->bad = bad;
    return TTM_OK;
}

extern "C" __attribute__((used, visibility("default"))) inline int ttm_resample(const uint64_t* cum, int64_t N, int64_t M, int32_t scheme, uint64_t seed, uint32_t draw,
                                                                                const double* Xsoa, int64_t ldx, int32_t ncols, double* Ysoa, int64_t ldy,
                                                                                int32_t* idx, void*) {
    if (!ttm::resample_args_ok(cum, N, M, scheme, draw, Xsoa, ldx, ncols, Ysoa, ldy, idx)) return TTM_E_ARG;
    const uint64_t T = cum[N - 1];
    for (int64_t j = 0; j < M; ++j) {
        const uint64_t R = ttm::resample_word(seed, draw, scheme, scheme == TTM_RESAMPLE_SYSTEMATIC ? 0 : (uint64_t)j);
        ttm::resample_offspring(cum, N, 0, N, ttm::resample_threshold(T, (uint64_t)M, scheme, (uint64_t)j, R), j, Xsoa, ldx, ncols, Ysoa, ldy, idx);
    }
    return TTM_OK;
}
#endif
