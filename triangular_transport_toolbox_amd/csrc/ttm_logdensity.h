// ttm_logdensity.h - log-density of the pullback of an integrated-rectifier map and its score: per sample
//
//     log p(u) = sum_k [ -1/2 S_k(u)^2 + log( (r(g_k(u_ck; u_<k)) + delta) g_k ) ]            (without the -D/2 log 2 pi)
//
// and its gradient with respect to the own variables u_ck, conditioning columns (in front of the first component) held fixed.
// S_k is what the forward map evaluates: the nonmonotone sum plus the Q-node Gauss-Legendre sum of r(g) + delta over [0, u_ck]
// (integrate_rect's nodes and grouping); g = w_nB + sum_b w_b(u_<k) B_b(t) the argument of the rectifier, w the weights of
// mon_weights.  The log term is log(r + delta) for every rectifier (rect_all's `logr` drops delta for two of them: the objective's
// convention, not the density's).  g_k: a uniform factor per own column (1 / sigma of the column for raw coordinates, 1 without).
//
// The score differentiates the computed quantity - the quadrature SUM, not the integral it approximates:
//
//     d S_k / d u_ck = sum_q W_q / 2 [ (r(g(t_q)) + delta) + t_q r'(g(t_q)) g'(t_q) ],      t_q = u_ck (1 + xi_q) / 2
//     d S_k / d u_j  = d/du_j (nonmonotone sum) + sum_b I_b dw_b/du_j,      I_b = sum_q (u_ck W_q / 2) r'(g(t_q)) B_b(t_q)     (j != ck)
//     d log(r + delta) / d u_ck = rho g'(u_ck),     d log(r + delta) / d u_j = rho sum_b B_b(u_ck) dw_b/du_j,     rho = r'(g) / (r + delta) at u_ck
//
// so a nonmonotone term carries the adjoint -S_k c_i and a monotone term with B function b the adjoint lambda_b c_i,
// lambda_b = -S_k I_b + rho B_b(u_ck) (slot nB: the constant function 1).  S_k, I_b, B_b(u_ck) and rho are what
// sample_objective_int (ttm_eval.h) forms for the gradient with respect to the coefficients; here the same adjoints are taken
// against the variables: eval_A_d is the product rule over a term's factors, series_d the derivative of a folded series.
//
// int_score_row is the per-component routine, the sibling of sample_objective_int: k_logdensity_int (csrc/ttm_kernels.hip) runs
// it one row per thread over all components, the host test double runs it in a loop.  Written for clarity, not speed: the generic
// table walk only (mon_weights, for_each_B, nonmon_sum), no dense-B or X-program fast path, no division by a factor value.
#pragma once

#include "ttm_eval.h"

namespace ttm {

// r(g) and the TRUE derivative r'(g) of every rectifier (rect_all's `dr` is the factor of the reference's evaluate_dfdc: NaN for
// `squared` / ELU, and without the factor log 2 for softplus - parity with the reference's objective, not a derivative)
template <class R>
TTM_HD void rect_d(int mode, const R& g, R& r, R& dr) {
    switch (mode) {
        case TTM_RECT_EXPONENTIAL: r = fast_exp(g); dr = r; break;
        case TTM_RECT_SOFTPLUS:     // r = log(1 + 2^g): r' = log 2 / (1 + 2^-g)   (the exponent capped as in rect_all)
            r = rect_eval(mode, g); dr = kLn2 * fast_rcp(1.0 + fast_exp(vmin(-kLn2 * g, 700.0))); break;
        case TTM_RECT_SQUARED: r = g * g; dr = 2.0 * g; break;
        case TTM_RECT_EXPNEG: r = fast_exp(-g); dr = -r; break;
        default: { const R e = fast_exp(g); r = vselect_lt0(g, e, g + 1.0); dr = vselect_lt0(g, e, R(1.0)); } break;   // ELU
    }
}

// P_order(x) and its derivative, order >= 1
template <class R>
TTM_HD void poly_eval_d(int fam, int order, const R& x, R& p, R& dp) {
    R pm(1.0), dpm(0.0);
    poly_first(fam, x, p, dp);
    for (int n = 1; n < order; ++n) poly_next<true>(fam, n, x, pm, p, dpm, dp);
}

// one factor record F = {var, kind, order, parameter offset} at xv: its value v and d v / d x_var, both WITHOUT the exp(-x^2/4) of
// a Hermite-function factor (all 'HF' factors of a term share one exp(-sum x^2 / 4), eval_A) but with that exponential's
// derivative: an HF factor a P(x) e(x) contributes (a P' - x a P / 2) e
template <class R>
TTM_HD void factor_d(cint_p F, const Comp& c, const Prog& p, const R& xv, R& v, R& dv) {
    const int kind = TTM_UNI(F[1]), order = TTM_UNI(F[2]), p0 = TTM_UNI(F[3]);
    if (kind == TTM_KIND_POLY) {
        poly_eval_d(p.family, order, xv, v, dv);
    } else if (kind == TTM_KIND_HF) {
        R P, dP;
        poly_eval_d(p.family, order, xv, P, dP);
        v = c.dpar[p0] * P;
        dv = vfma(-0.5 * xv, v, c.dpar[p0] * dP);
    } else {
        st_eval<true, true>(p, kind, xv, c.dpar + p0, v, dv);
    }
}

// Derivatives of the A-part of a term (eval_A: the product of its factors on columns other than kc): f(var, dA/dx_var), one
// call per factor - the product rule, each factor's derivative times the values of the others (terms have two or three factors:
// the others are evaluated again per factor rather than divided out)
template <class XA, class F>
TTM_HD void eval_A_d(cint_p term, const Comp& c, const Prog& p, XA& x, F&& f) {
    const int f0 = TTM_UNI(term[0]);
    const int nf = TTM_UNI(term[1]);
    double ssq = 0.0;
    bool hf = false;
    for (int i = 0; i < nf; ++i) {
        cint_p Fi = c.facs + 4 * (f0 + i);
        if (TTM_UNI(Fi[1]) == TTM_KIND_HF) {
            const double xv = x(TTM_UNI(Fi[0]));
            ssq = fma(xv, xv, ssq);
            hf = true;
        }
    }
    const double e = hf ? fast_exp(-0.25 * ssq) : 1.0;
    for (int i = 0; i < nf; ++i) {
        cint_p Fi = c.facs + 4 * (f0 + i);
        const int var = TTM_UNI(Fi[0]);
        double v, d;
        factor_d(Fi, c, p, (double)x(var), v, d);
        for (int j = 0; j < nf; ++j) {
            if (j == i) continue;
            cint_p Fj = c.facs + 4 * (f0 + j);
            double vj, dj;
            factor_d(Fj, c, p, (double)x(TTM_UNI(Fj[0])), vj, dj);
            d = d * vj;
        }
        f(var, d * e);
    }
}

// d/dx_var of a folded series G = {var, P, fold offset, has_hf, ...} (a nonmonotone group or a cross group):
// sum_n al_n P_n(x) + e^{-x^2/4} sum_n be_n P_n(x), the normalisation constants of the Hermite functions folded into be
template <class XA>
TTM_HD double series_d(cint_p G, const Comp& c, const Prog& p, VarCache<XA, double>& x) {
    const int var = TTM_UNI(G[0]);
    const int P = TTM_UNI(G[1]);
    cdbl_p al = c.fold + TTM_UNI(G[2]);
    cdbl_p be = al + P;
    const int has_hf = TTM_UNI(G[3]);
    double xv, e = 0.0;
    if (has_hf) x.get_e(var, xv, e); else xv = x.get(var);
    double pm = 1.0, dpm = 0.0, pn, dp, dacc = 0.0, hacc = 0.0, dhacc = 0.0;
    poly_first(p.family, xv, pn, dp);
    for (int n = 1; n <= P; ++n) {
        dacc = fma(al[n - 1], dp, dacc);
        if (has_hf) {
            hacc = fma(be[n - 1], pn, hacc);
            dhacc = fma(be[n - 1], dp, dhacc);
        }
        if (n < P) poly_next<true>(p.family, n, xv, pm, pn, dpm, dp);
    }
    if (has_hf) dacc = fma(e, fma(-0.5 * xv, hacc, dhacc), dacc);          // d/dx [e B] = e (B' - x B / 2)
    return dacc;
}

// Component c of one row: logp += -1/2 S^2 + log((r + delta) g_k), and - with want_g - the component's contributions to the
// row's score: G.add(j, v) for own column j (the caller has set the row's columns to zero; columns in front of E get nothing).
// scratch slots: w (nB+1) | Bv (nB+1) | I (nB+1).  g_scale: D doubles or null.
template <class XA, class Slots, class GA>
TTM_HD void int_score_row(const Comp& c, const Prog& p, VarCache<XA, double>& x, Slots& w, Slots& Bv, Slots& I, int E, cdbl_p g_scale,
                          bool want_g, GA& G, double& logp) {
    mon_weights<double>(c, p, x, w);
    const double xk = x.get(c.kc);
    const double half = xk * 0.5;
    double mono = 0.0, dmono = 0.0;
    for (int b = 0; b <= c.nB; ++b) I.set(b, 0.0);
    for (int q = 0; q < p.Q; ++q) {
        const double t = half * p.qx[q] + half;
        double g = w.get(c.nB), dg = 0.0;
        for_each_B<true>(c, p, t, [&](int b, double v, double dv) {
            g = fma(w.get(b), v, g);
            dg = fma(w.get(b), dv, dg);
            Bv.set(b, v);
        });
        double r, dr;
        rect_d(p.rect, g, r, dr);
        const double term = half * (p.qw[q] * (r + p.delta));          // (integrate_rect's grouping: the forward map's bits)
        mono = (q == 0) ? term : mono + term;
        if (want_g) {
            dmono = fma(0.5 * p.qw[q], (r + p.delta) + t * (dr * dg), dmono);
            const double cq = (half * p.qw[q]) * dr;
            for (int b = 0; b < c.nB; ++b) I.set(b, fma(cq, Bv.get(b), I.get(b)));
            I.set(c.nB, I.get(c.nB) + cq);
        }
    }
    const double S = nonmon_sum<double>(c, p, x) + mono;
    // the rectifier's argument at x_k, its derivative, the values B_b(x_k)
    double g = w.get(c.nB), dg = 0.0;
    for_each_B<true>(c, p, xk, [&](int b, double v, double dv) {
        g = fma(w.get(b), v, g);
        dg = fma(w.get(b), dv, dg);
        Bv.set(b, v);
    });
    Bv.set(c.nB, 1.0);
    double r, dr;
    rect_d(p.rect, g, r, dr);
    const double rd = r + p.delta;
    const int k = c.kc - E;
    logp += -0.5 * (S * S) + fast_log(g_scale ? rd * g_scale[k] : rd);
    if (!want_g) return;
    const double rho = dr * fast_rcp(rd);
    auto add = [&](int var, double v) {
        const int j = var - E;
        if (j >= 0) G.add(j, g_scale ? g_scale[j] * v : v);          // (j < 0: a conditioning column, held fixed)
    };
    add(c.kc, fma(-S, dmono, rho * dg));
    // nonmonotone terms: adjoint -S c_i
    for (int gi = 0; gi < c.n_grp; ++gi) {
        cint_p Gr = c.grp + 4 * gi;
        if (TTM_UNI(Gr[0]) >= E) add(TTM_UNI(Gr[0]), -S * series_d(Gr, c, p, x));
    }
    for (int i = 0; i < c.n_gen; ++i) {
        cint_p T = c.nm_terms + 4 * TTM_UNI(c.gen[i]);
        const double a = -S * c.cnm[TTM_UNI(T[3])];
        eval_A_d(T, c, p, x, [&](int var, double dA) { add(var, a * dA); });
    }
    // monotone cross terms: adjoint lambda_b c_i
    for (int gi = 0; gi < c.n_xgrp; ++gi) {
        cint_p Gr = c.xgrp + 8 * gi;
        const int b = TTM_UNI(Gr[4]);
        if (TTM_UNI(Gr[0]) >= E) add(TTM_UNI(Gr[0]), fma(-S, I.get(b), rho * Bv.get(b)) * series_d(Gr, c, p, x));
    }
    for (int j = 0; j < c.n_mnt; ++j) {
        cint_p T = c.mon_terms + 4 * TTM_UNI(c.mnt[j]);
        int b = TTM_UNI(T[2]);
        if (b < 0) b = c.nB;
        const double a = fma(-S, I.get(b), rho * Bv.get(b)) * c.cmon[TTM_UNI(T[3])];
        eval_A_d(T, c, p, x, [&](int var, double dA) { add(var, a * dA); });
    }
}

}  // namespace ttm

#if !defined(__HIPCC__)
// HOST BUILDS ONLY (the library's translation units are all compiled as HIP and never see this): the entry point ttm_logdensity
// of include/ttm.h around int_score_row, row after row, with the library's argument checks - for the host test double of the
// C ABI (tests/hostemu), as ttm_score in csrc/ttm_score.h.
extern "C" __attribute__((used, visibility("default"))) inline int ttm_logdensity(const ttm_program* p, const double* coef, const double* fold, const double* Xsoa, int64_t ldx,
                                                                                  int64_t N, double* logp, double* Gsoa, int64_t ldg, const double* g_scale, void*) {
    if (!p || !p->itab || !p->dpar || !p->h_comp_off || !p->h_dpar_off || !p->h_coef_off || !p->h_fold_off || !p->h_nb1) return TTM_E_ARG;
    if (!coef || !fold || !Xsoa || (!logp && !Gsoa) || N < 1 || ldx < N || (Gsoa && ldg < N)) return TTM_E_ARG;
    if (p->monotonicity != TTM_MONO_INTEGRATED) return TTM_E_UNSUPPORTED;
    if (p->Q < 1 || !p->quad_x || !p->quad_w) return TTM_E_ARG;
    static const double erf_tab[TTM_ERF_TABLE_LEN] = { TTM_ERF_TABLE_VALUES };
    ttm::Prog g;
    g.qx = p->quad_x; g.qw = p->quad_w; g.erf_tab = erf_tab; g.Q = p->Q; g.family = p->family; g.mono = p->monotonicity;
    g.rect = p->rectifier; g.delta = p->delta;
    const int D = p->D, E = p->d_cols - p->D;
    int nb1 = 1;
    for (int k = 0; k < D; ++k) nb1 = p->h_nb1[k] > nb1 ? p->h_nb1[k] : nb1;
    struct XRow {
        const double* X; int64_t ld, n;
        double operator()(int var) const { return X[(int64_t)var * ld + n]; }
    };
    struct GRow {
        double* G; int64_t ld, n;
        void set(int k, double v) { G[(int64_t)k * ld + n] = v; }
        void add(int k, double v) { G[(int64_t)k * ld + n] += v; }
    };
    struct Slots {
        double* base;
        double get(int i) const { return base[i]; }
        void set(int i, double v) { base[i] = v; }
    };
    double* scr = new double[3 * (size_t)nb1];
    Slots w{scr}, Bv{scr + nb1}, I{scr + 2 * nb1};
    for (int64_t n = 0; n < N; ++n) {
        const XRow xa{Xsoa, ldx, n};
        GRow ga{Gsoa, ldg, n};
        double cbuf[8];
        ttm::VarCache<XRow, double> x(xa, ttm::CacheStore<double>{cbuf, 1});
        if (Gsoa) for (int k = 0; k < D; ++k) ga.set(k, 0.0);
        double lp = 0.0;
        for (int k = 0; k < D; ++k) {
            const ttm::Comp c = ttm::make_comp(p->itab + p->h_comp_off[k], p->dpar + p->h_dpar_off[k], coef + p->h_coef_off[k], fold + p->h_fold_off[k]);
            ttm::int_score_row(c, g, x, w, Bv, I, E, g_scale, Gsoa != nullptr, ga, lp);
        }
        if (logp) logp[n] = lp;
    }
    delete[] scr;
    return TTM_OK;
}
#endif
