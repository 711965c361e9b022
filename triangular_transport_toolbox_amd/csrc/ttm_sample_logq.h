// ttm_sample_logq.h - root searches of an integrated-rectifier map that also hand back the log-density term of the point
// they return: per component k of one sample
//
//     -1/2 S_k(x)^2 + log( dS_k/dx_k (x) g_k ),      dS_k/dx_k = r(g_k(x_k; x_<k)) + delta
//
// at x = the root search's result, so that a draw x = S^-1(z) leaves the kernel with log q(x) = sum_k of these terms (without
// the -1/2 log 2 pi per component) - include/ttm.h: ttm_inverse_logdensity.
//
// The searches themselves are sample_bisect / sample_newton of ttm_eval.h, called as they are: same trial points, same result,
// same `iters`.  What is added is ONE mon_eval<., true> at the point they returned.  That holds in every exit without a case
// distinction - converged, stopped at 100 trial points, Newton's return without a sign change, bisection under a cap (cap = 0:
// the last bracket end) - because nothing is carried out of the search but its result.  Price: one evaluation of S_k on top of
// the ~33 of a bisection and the ~6 of a Newton search (whose last trial evaluation is the same point: a variant of the loop
// that keeps its last m and dm would save it, as a second copy of the search).
//
// sample_root_logq / dense_sample_root_logq / xprog_sample_root_logq mirror sample_root (ttm_eval.h), dense_sample_root
// (ttm_dense.h) and xprog_sample_root (ttm_xprog.h): the same weight source, then the search.  The kernels (csrc/ttm_int.hip,
// csrc/ttm_kernels.hip: the LOGQ instantiations) and the host test double share them.
#pragma once

#include "ttm_eval.h"
#include "ttm_dense.h"
#include "ttm_xprog.h"

namespace ttm {

// the search through weight source w, then S_k = off + m and dS_k/dx_k at its result
template <int MONO, bool NEWTON, class W>
TTM_HD double sample_search_logq(const Comp& c, const Prog& p, double off, double zk, const W& w, int cap, int& it, double& S, double& dS) {
    const double r = NEWTON ? sample_newton<MONO>(c, p, off, zk, w, it) : sample_bisect<MONO>(c, p, off, zk, w, cap, it);
    double m, dm;
    mon_eval<MONO, true>(c, p, r, w, m, dm);
    S = off + m;                                             // (the grouping of the searches' own f = (off + m) - zk)
    dS = dm;
    return r;
}

// the component's term of the row's log-density; g: the factor of its own column (1 / sigma for raw coordinates) or 1
// (int_score_row's expression, csrc/ttm_logdensity.h)
TTM_HD double logq_term(double S, double dS, double g) { return -0.5 * (S * S) + fast_log(dS * g); }

template <int MONO, bool NEWTON, class XA, class Slots>
TTM_HD double sample_root_logq(const Comp& c, const Prog& p, VarCache<XA, double>& x, Slots& w, double off, double zk, int cap, int& it,
                               double& S, double& dS) {
    const int mono = (MONO >= 0) ? MONO : p.mono;
    if (mono == TTM_MONO_INTEGRATED && dense_B(c)) {
        dense_weights<double>(c, p, x, w);
        const DenseSet<Slots> dw{w};
        return sample_search_logq<MONO, NEWTON>(c, p, off, zk, dw, cap, it, S, dS);
    }
    if (c.n_mnt == 0 && c.n_xgrp == 0) {
        const UniformW uw{c.fold + c.off_wb};
        return sample_search_logq<MONO, NEWTON>(c, p, off, zk, uw, cap, it, S, dS);
    }
    mon_weights<double>(c, p, x, w);
    return sample_search_logq<MONO, NEWTON>(c, p, off, zk, w, cap, it, S, dS);
}

template <int PH, int PP, int RECT, bool NEWTON, class XA, class Slots>
TTM_HD double dense_sample_root_logq(const Comp& c, const Prog& p, double qw_sum, VarCache<XA, double>& x, Slots& w, double off, double zk,
                                     int cap, int& it, double& S, double& dS) {
    dense_weights<double>(c, p, x, w);
    DenseMonoSet<PH, PP, RECT> s;
    dense_monomials<PH, PP>(c, p, w, s.d);
    s.qw_sum = qw_sum;
    return sample_search_logq<TTM_MONO_INTEGRATED, NEWTON>(c, p, off, zk, s, cap, it, S, dS);
}

template <int PH, int PP, int RECT, bool NEWTON, class FP, class XA, class Row>
TTM_HD double xprog_sample_root_logq(const XProg& xp, const Prog& p, double qw_sum, FP fx, const XA& xa, Row& row, double zk, int cap, int& it,
                                     double& S, double& dS) {
    constexpr int PM = PH > PP ? PH : PP;
    xprog_values<PM>(xp, xa, row);
    DenseMonoSet<PH, PP, RECT> s;
    double off;
    xprog_mono<PH, PP>(xp, fx, row, s.d, off);
    s.qw_sum = qw_sum;
    Comp unused;
    return sample_search_logq<TTM_MONO_INTEGRATED, NEWTON>(unused, p, off, zk, s, cap, it, S, dS);
}

}  // namespace ttm

#if !defined(__HIPCC__)
// HOST BUILDS ONLY (the library's translation units are all compiled as HIP and never see this): the entry point
// ttm_inverse_logdensity of include/ttm.h around the routines above, row after row, with the library's argument checks - for the
// host test double of the C ABI (tests/hostemu), as ttm_logdensity in csrc/ttm_logdensity.h.  The family is the library's own plan:
// the monomial-form search (dense_sample_root_logq) when every component of the range has a dense B set, else the generic one
// (sample_root_logq) - what the double's ttm_inverse_bisect / ttm_inverse_newton run without options, so X and iters are theirs bit
// for bit.  (Options int_dense / int_xprog are the library's: they do not reach this routine, and the X-program search runs on the
// device alone.)
namespace ttm {
template <bool NEWTON>
inline void host_inverse_logdensity_rows(const ttm_program* p, const double* coef, const double* fold, int32_t k0, int32_t k1, const double* Z,
                                         int64_t ldz, double* X, int64_t ldx, int64_t N, int32_t* iters, const int32_t* cap, double* logq,
                                         const double* g_scale) {
    static const double erf_tab[TTM_ERF_TABLE_LEN] = { TTM_ERF_TABLE_VALUES };
    Prog g;
    g.qx = p->quad_x; g.qw = p->quad_w; g.erf_tab = erf_tab; g.Q = p->Q; g.family = p->family; g.mono = p->monotonicity;
    g.rect = p->rectifier; g.delta = p->delta;
    struct XRow {
        const double* X; int64_t ld, n;
        double operator()(int var) const { return X[(int64_t)var * ld + n]; }
    };
    struct Slots {
        double* base;
        double get(int i) const { return base[i]; }
        void set(int i, double v) { base[i] = v; }
    };
    DenseClass dcls{0, 0};
    const bool dense = p->family >= 0 && p->family <= 5 && dense_range_class(p->h_complex, k0, k1, dcls);
    const double qws = dense ? dense_qw_sum(g) : 0.0;
    int nb1 = 4096;                                          // (weight slots: nB + 1 of the largest component; the double's own searches keep 4096)
    for (int k = k0; k < k1; ++k) nb1 = p->h_nb1[k] > nb1 ? p->h_nb1[k] : nb1;
    double* scr = new double[(size_t)nb1];
    Slots w{scr};
    for (int64_t n = 0; n < N; ++n) {
        const XRow xa{X, ldx, n};
        double cbuf[8];
        VarCache<XRow, double> x(xa, CacheStore<double>{cbuf, 1});
        double lq = 0.0;
        for (int k = k0; k < k1; ++k) {
            const Comp c = make_comp(p->itab + p->h_comp_off[k], p->dpar + p->h_dpar_off[k], coef + p->h_coef_off[k], fold + p->h_fold_off[k]);
            const double zk = Z[(int64_t)(k - k0) * ldz + n];
            const int capk = cap ? cap[k - k0] : -1;
            const double off = nonmon_sum<double>(c, g, x);
            int it = 0;
            double r = 0.0, S = 0.0, dS = 0.0;
            if (dense) {
#define TTM_CALL(PH, PP, RECT) r = dense_sample_root_logq<PH, PP, RECT, NEWTON>(c, g, qws, x, w, off, zk, capk, it, S, dS)
                TTM_DENSE_DISPATCH(TTM_CALL, dcls, p->rectifier);
#undef TTM_CALL
            } else {
                r = sample_root_logq<-1, NEWTON>(c, g, x, w, off, zk, capk, it, S, dS);
            }
            lq += logq_term(S, dS, g_scale ? g_scale[k - k0] : 1.0);
            X[(int64_t)c.kc * ldx + n] = r;
            x.put(c.kc, r);
            if (it > iters[k - k0]) iters[k - k0] = it;
        }
        logq[n] = lq;
    }
    delete[] scr;
}
}  // namespace ttm

extern "C" __attribute__((used, visibility("default"))) inline int ttm_inverse_logdensity(const ttm_program* p, const double* coef, const double* fold, int32_t k0, int32_t k1,
                                                                                          const double* Zsoa, int64_t ldz, double* Xsoa, int64_t ldx, int64_t N, int32_t newton,
                                                                                          int32_t* iters, const int32_t* cap, double* logq, const double* g_scale, void*) {
    if (!p || !p->itab || !p->dpar || !p->h_comp_off || !p->h_dpar_off || !p->h_coef_off || !p->h_fold_off || !p->h_nb1 || !p->h_complex) return TTM_E_ARG;
    if (k0 < 0 || k1 > p->D || k0 >= k1) return TTM_E_ARG;
    if (!coef || !fold || !Zsoa || !Xsoa || !iters || !logq || N < 1 || ldx < N || ldz < N || (newton && cap)) return TTM_E_ARG;
    if (p->monotonicity != TTM_MONO_INTEGRATED) return TTM_E_UNSUPPORTED;
    if (p->Q < 1 || !p->quad_x || !p->quad_w) return TTM_E_ARG;
    if (newton) ttm::host_inverse_logdensity_rows<true>(p, coef, fold, k0, k1, Zsoa, ldz, Xsoa, ldx, N, iters, nullptr, logq, g_scale);
    else ttm::host_inverse_logdensity_rows<false>(p, coef, fold, k0, k1, Zsoa, ldz, Xsoa, ldx, N, iters, cap, logq, g_scale);
    return TTM_OK;
}
#endif
