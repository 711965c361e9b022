// ttm_score.h - score of the pullback density of a separable U-form map: the gradient, with respect to the own variables of
// one sample, of
//
//     log p(x) = -1/2 sum_k S_k(u)^2 + sum_k log m_k'(t_k) + const,     m_k = the monotone part of component k,
//
// where u is the (standardised) sample the map is evaluated on and t_k = a_k u_k + b_k the point the log-determinant term
// is taken at (the reference evaluates its derivative basis on the un-standardised sample, TM:2627 / 2695; without
// `ld_affine`: t = u).  With c the column of component k:
//
//     G_k = -g_k sum_{j >= k} S_j(u) dS_j/du_c (u)  +  m_k''(t_k) / m_k'(t_k)
//     dS_k/du_c = m_k'(u_c),     dS_j/du_c = f_jc'(u_c) = A'(u_c) + exp(-u_c^2/4) (B'(u_c) - u_c B(u_c) / 2)   (j > k)
//
// g_k: a uniform factor on the Gaussian part (1/sigma_c for a score in raw coordinates, 1 without `g_scale`).  Conditioning
// columns (columns in front of the first component) are held fixed: they get no output.
//
// u_score_row is the per-sample routine, next to u_component (csrc/ttm_uform.h) and built from its pieces: k_score_u
// (csrc/ttm_kernels.hip) runs it one row per thread, the host test double runs it in a loop, and the push-form kernel of
// banded maps (k_band_score, csrc/ttm_band.hip) is compared against it.  Written for clarity, not speed: the groups of a
// component are walked twice (S_k has to be complete before its products with the groups' derivatives are formed).
#pragma once

#include "ttm_uform.h"

namespace ttm {

// Horner pass of run-time degree P: value, first and second derivative
TTM_HD void u_horner2(int P, cdbl_p c, double x, double& v, double& dv, double& d2v) {
    double a = c[P], da = 0.0, dda = 0.0;
    for (int j = P - 1; j >= 0; --j) {
        dda = fma(dda, x, da);
        da = fma(da, x, a);
        a = fma(a, x, c[j]);
    }
    v = a; dv = da; d2v = 2.0 * dda;
}

// one nonmonotone group f(x) = A(x) + exp(-x^2/4) B(x) of the U section (rec: B[0..11] | A[0..11], fl: its flag word):
// value and derivative
TTM_HD void u_group_d(int fl, cdbl_p rec, double x, double& f, double& df) {
    double v, dv;
    f = 0.0; df = 0.0;
    if (fl & TTM_PLAN_HF) {
        const double e = exp_q_fast(x);
        u_poly<-1, true>(TTM_UG_DEGB(fl), rec, x, v, dv);
        f = e * v;
        df = e * fma(-0.5 * x, v, dv);                        // d/dx [e^{-x^2/4} B] = e^{-x^2/4} (B' - x B / 2)
    }
    if (fl & TTM_UGF_POLY) {
        u_poly<-1, true>(TTM_UG_DEGA(fl), rec + TTM_U_GHALF, x, v, dv);
        f += v;
        df += dv;
    }
}

// the special-term spline at t: first and second derivative with respect to t (u_spline's index arithmetic; three
// recurrences over the column's twelve coefficients).  The tail columns are exactly linear: d2g = 0 there.
TTM_HD void u_spline_d2(const double* tab, int nI, double sp_a, double sp_b, double sp_ds, double t, double& dg, double& d2g) {
    const double u = fma(t, sp_b, sp_a);
    const double fl = vfloor(vmin(vmax(u, -1.0), (double)(nI - 2)));
    const double s = fma(2.0, u - fl, -1.0);
    const double* cp = tab + ((int)fl + 1) * TTM_U_TSTRIDE;
    double a = cp[TTM_U_DEG], da = 0.0, dda = 0.0;
    for (int j = TTM_U_DEG - 1; j >= 0; --j) {
        dda = fma(dda, s, da);
        da = fma(da, s, a);
        a = fma(a, s, cp[j]);
    }
    dg = da * sp_ds;
    d2g = 2.0 * dda * (sp_ds * sp_ds);
}

// m_k'(t) and m_k''(t) of the monotone part of a component: polynomial / Hermite-function terms of its own variable (if any)
// plus the special-term spline (if any)
TTM_HD void u_monotone_d2(cint_p uc, cint_p ug_all, cdbl_p U, const double* tab, double t, double& dm, double& d2m) {
    dm = 0.0 * t; d2m = 0.0 * t;                              // (a NaN / infinite sample stays NaN whatever the terms)
    if (uc[TTM_UC_FLAGS] & TTM_UCF_OWN) {
        const int g = uc[TTM_UC_N_GRP];
        const int fl = (ug_all + TTM_UG_LEN * (uc[TTM_UC_GRP_OFF] + g))[TTM_UG_FLAGS];
        cdbl_p rec = U + uc[TTM_UC_DBL_OFF] + 4 + TTM_U_GSTRIDE * g;
        double v, dv, d2v;
        if (fl & TTM_PLAN_HF) {
            // d/dt [e B] = e (B' - t B / 2),   d2/dt2 [e B] = e (B'' - t B' + (t^2/4 - 1/2) B),   e = e^{-t^2/4}
            const double e = exp_q_fast(t);
            u_horner2(TTM_UG_DEGB(fl), rec, t, v, dv, d2v);
            dm = fma(e, fma(-0.5 * t, v, dv), dm);
            d2m = fma(e, fma(fma(0.25 * t, t, -0.5), v, fma(-t, dv, d2v)), d2m);
        }
        if (fl & TTM_UGF_POLY) {
            u_horner2(TTM_UG_DEGA(fl), rec + TTM_U_GHALF, t, v, dv, d2v);
            dm += dv;
            d2m += d2v;
        }
    }
    if (uc[TTM_UC_NI] > 0) {
        cdbl_p cd = U + uc[TTM_UC_DBL_OFF];
        double dg, d2g;
        u_spline_d2(tab, uc[TTM_UC_NI], cd[1], cd[2], cd[3], t, dg, d2g);
        dm += dg;
        d2m += d2g;
    }
}

// The score of one row.  U / Ug: the U section (uniform reads / the splines' per-row reads); xa(var): the row's value in column `var` of the sample matrix; E: columns in front of the first
// component (d_cols - D); g_scale (D doubles) / ld_affine (2 D doubles {a_k, b_k}): see above, nullable;
// G.set(k, v) / G.add(k, v): the row's score of own column k - accumulated in the output buffer itself.
template <class XA, class GA>
TTM_HD void u_score_row(cint_p ucomp, cint_p ugrp, cdbl_p U, const double* Ug, int D, int E, const XA& xa, cdbl_p g_scale, cdbl_p ld_affine, GA& G) {
    for (int k = 0; k < D; ++k) G.set(k, 0.0);
    for (int k = 0; k < D; ++k) {
        cint_p uc = ucomp + k * TTM_UC_LEN;
        cdbl_p cd = U + uc[TTM_UC_DBL_OFF];
        cint_p ug = ugrp + TTM_UG_LEN * uc[TTM_UC_GRP_OFF];
        const int n_grp = uc[TTM_UC_N_GRP], nI = uc[TTM_UC_NI];
        const double* tab = Ug + uc[TTM_UC_TAB_OFF];
        const double xk = xa(uc[TTM_UC_KC]);
        // S_k: constants, nonmonotone groups, monotone part (and the monotone part's derivative) - u_component's pieces
        double S = cd[0];
        for (int g = 0; g < n_grp; ++g) {
            double f, df;
            u_group_d(ug[TTM_UG_LEN * g + TTM_UG_FLAGS], cd + 4 + TTM_U_GSTRIDE * g, xa(ug[TTM_UG_LEN * g + TTM_UG_VAR]), f, df);
            S += f;
        }
        double m = 0.0, dm = 0.0 * xk;                        // (x 0: a NaN / infinite sample stays NaN whatever the terms)
        if (uc[TTM_UC_FLAGS] & TTM_UCF_OWN) {
            const bool own_hf = (ug[TTM_UG_LEN * n_grp + TTM_UG_FLAGS] & TTM_PLAN_HF) != 0;
            const double ek = own_hf ? exp_q_fast(xk) : 0.0;
            u_own<true>(uc, ugrp, U, xk, ek, m, dm);
        }
        if (nI > 0) {
            double g, dg;
            u_spline<true>(tab, nI, cd[1], cd[2], cd[3], xk, g, dg);
            m += g;
            dm += dg;
        }
        S += m;
        // Gaussian part: -g_c S_k dS_k/du_c for the own column and for every column a group of this component reads
        G.add(k, -(g_scale ? g_scale[k] : 1.0) * S * dm);
        for (int g = 0; g < n_grp; ++g) {
            const int j = ug[TTM_UG_LEN * g + TTM_UG_VAR] - E;
            if (j < 0) continue;                              // (a conditioning column: held fixed)
            double f, df;
            u_group_d(ug[TTM_UG_LEN * g + TTM_UG_FLAGS], cd + 4 + TTM_U_GSTRIDE * g, xa(j + E), f, df);
            G.add(j, -(g_scale ? g_scale[j] : 1.0) * S * df);
        }
        // log-determinant part: m_k''(t) / m_k'(t)
        const double t = ld_affine ? fma(ld_affine[2 * k], xk, ld_affine[2 * k + 1]) : xk;
        double dmt, d2mt;
        u_monotone_d2(uc, ugrp, U, tab, t, dmt, d2mt);
        G.add(k, fast_div(d2mt, dmt));
    }
}

}  // namespace ttm

#if !defined(__HIPCC__)
// HOST BUILDS ONLY (the library's translation units are all compiled as HIP and never see this): the entry point ttm_score of
// include/ttm.h around u_score_row, row after row, with the library's argument checks.  The host test double of the C ABI
// (tests/hostemu) includes the U-form headers and exports every entry point; it takes this one from here, next to the routine that
// is its whole body.  Inline and kept (`used`): a second host translation unit that includes this header shares the one definition.
// (Option no_uform is the library's: here a map with a U section always runs it.)
extern "C" __attribute__((used, visibility("default"))) inline int ttm_score(const ttm_program* p, const double* coef, const double* fold, const double* Xsoa, int64_t ldx, int64_t N, double* Gsoa,
                         int64_t ldg, const double* g_scale, const double* ld_affine, void*) {
    if (!p || !p->h_fold_off) return TTM_E_ARG;
    const int64_t need = (N + 1) & ~(int64_t)1;
    auto col_ok = [&](const void* ptr, int64_t ld) { return ptr && (uintptr_t)ptr % 16 == 0 && ld % 2 == 0 && ld >= need; };
    if (!coef || !fold || N < 1 || N >= ((int64_t)1 << 28) || !col_ok(Xsoa, ldx) || !col_ok(Gsoa, ldg) || (uintptr_t)fold % 16 != 0) return TTM_E_ARG;
    if (p->monotonicity != TTM_MONO_SEPARABLE || !p->u_enabled || !p->ucomp || !p->ugrp) return TTM_E_UNSUPPORTED;
    const double* U = fold + (((int64_t)p->h_fold_off[p->D] + 8 + 1) & ~(int64_t)1);      // (the U section: behind the folded coefficients)
    struct XRow {
        const double* X; int64_t ld, n;
        double operator()(int var) const { return X[(int64_t)var * ld + n]; }
    };
    struct GRow {
        double* G; int64_t ld, n;
        void set(int k, double v) { G[(int64_t)k * ld + n] = v; }
        void add(int k, double v) { G[(int64_t)k * ld + n] += v; }
    };
    for (int64_t n = 0; n < N; ++n) {
        const XRow xa{Xsoa, ldx, n};
        GRow ga{Gsoa, ldg, n};
        ttm::u_score_row(p->ucomp, p->ugrp, U, U, p->D, p->d_cols - p->D, xa, g_scale, ld_affine, ga);
    }
    return TTM_OK;
}
#endif

// (the log-density and score of integrated-rectifier maps: the other half of the score, with its own host-only entry point)
#include "ttm_logdensity.h"

#if !defined(__HIPCC__)
// (host builds: the root searches that carry the log-density of their draws out, with the host-only entry point
// ttm_inverse_logdensity - the host test double takes it from there, as the two above)
#include "ttm_sample_logq.h"
#endif

// (a gradient pulled through the map - the transposed-Jacobian solve from the same pieces, with its own host-only entry point)
#include "ttm_pull.h"
