// ttm_pull.h - a gradient pulled through a separable U-form map: the solve with the transposed Jacobian of the components
// [k0, k1) given the columns in front (ttm_pull_gradient of include/ttm.h).  With c(k) = E + k the column of
// component k, S_k(u) = const + sum_g f_kg(u_var(g)) + m_k(u_c(k)) is additive, so column c of J = dS/du depends on u_c alone:
// J_kk = m_k'(u_c(k)), J_jk = f_jg'(u_c(k)) summed over the groups g of component j > k that read column c(k).  J^T is upper
// triangular, and
//
//     W = J^-T (g_scale * G - [logdet] l),     l_k = m_k''(u_c(k)) / m_k'(u_c(k)),
//
// is a back substitution for i = k1 - 1 down to k0:  r_i = g_scale_i G_i - l_i - sum_{j > i} J_ji W_j,  W_i = r_i / m_i'.
// For a density p on x this is the gradient of the logarithm of its pullback p(T(z)) |det grad T(z)|, T = S^-1, with respect
// to z (G = grad_x log p, g_scale = sigma of the own columns when G is taken in raw coordinates).
//
// u_pull_row is the per-sample routine, next to u_score_row and built from its pieces (u_monotone_d2, u_group_d): ONE descending
// pass in push form - component i is complete when the pass reaches it (every component above has subtracted its share), takes
// m', m'' from one u_monotone_d2 at t = u, divides, and subtracts W_i f' from the open entries of the columns its groups read.
// k_pull_gradient_u (csrc/ttm_kernels.hip) runs it one row per thread, the host definition below in a loop.
#pragma once

namespace ttm {

// The pull of one row.  U / Ug, xa, E: as u_score_row; [k0, k1): the components; g_scale: k1 - k0 doubles, nullable; logdet:
// subtract l; ga(i): the row's entry of G for component k0 + i; W.get(i) / W.set(i, v): the row's entry of the output, which
// the sums are accumulated in (W may be G itself: entry i of G is read once, before entry i of W is first written).  Every
// product is an explicit fma or a single operation: the host build and the device build round alike.
template <class XA, class GA, class WA>
TTM_HD void u_pull_row(cint_p ucomp, cint_p ugrp, cdbl_p U, const double* Ug, int E, int k0, int k1, const XA& xa, const GA& ga, cdbl_p g_scale,
                       bool logdet, WA& W) {
    for (int i = 0; i < k1 - k0; ++i) W.set(i, g_scale ? g_scale[i] * ga(i) : ga(i));
    for (int k = k1 - 1; k >= k0; --k) {
        cint_p uc = ucomp + k * TTM_UC_LEN;
        cdbl_p cd = U + uc[TTM_UC_DBL_OFF];
        cint_p ug = ugrp + TTM_UG_LEN * uc[TTM_UC_GRP_OFF];
        const int n_grp = uc[TTM_UC_N_GRP];
        double dm, d2m;
        u_monotone_d2(uc, ugrp, U, Ug + uc[TTM_UC_TAB_OFF], xa(uc[TTM_UC_KC]), dm, d2m);
        double r = W.get(k - k0);
        if (logdet) r -= d2m / dm;
        const double w = r / dm;                              // (m' = 0: what IEEE division gives)
        W.set(k - k0, w);
        for (int g = 0; g < n_grp; ++g) {
            const int var = ug[TTM_UG_LEN * g + TTM_UG_VAR];
            const int j = var - E - k0;
            if (j < 0) continue;                              // (a conditioning column, or a component in front of k0: held fixed)
            double f, df;
            u_group_d(ug[TTM_UG_LEN * g + TTM_UG_FLAGS], cd + 4 + TTM_U_GSTRIDE * g, xa(var), f, df);
            W.set(j, fma(-w, df, W.get(j)));
        }
    }
}

// the argument check of ttm_pull_gradient behind the program's own (shared by the library and the host definition below)
TTM_HD bool pull_args_ok(const void* coef, const void* fold, const double* X, int64_t ldx, int64_t N, int ncols, int d_cols, const double* G, int64_t ldg,
                         const double* W, int64_t ldw) {
    const int64_t need = (N + 1) & ~(int64_t)1;
    auto col_ok = [&](const void* ptr, int64_t ld) { return ptr && (uintptr_t)ptr % 16 == 0 && ld % 2 == 0 && ld >= need; };
    if (!coef || !fold || N < 1 || N >= ((int64_t)1 << 28) || !col_ok(X, ldx) || !col_ok(G, ldg) || !col_ok(W, ldw) || (uintptr_t)fold % 16 != 0) return false;
    auto overlap = [](const double* a, int64_t na, const double* b, int64_t nb) {
        const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
        return a0 < b0 + 8 * (uintptr_t)nb && b0 < a0 + 8 * (uintptr_t)na;
    };
    const int64_t wlen = (int64_t)(ncols - 1) * ldw + N, glen = (int64_t)(ncols - 1) * ldg + N, xlen = (int64_t)(d_cols - 1) * ldx + N;
    if (!(W == G && ldw == ldg) && overlap(W, wlen, G, glen)) return false;      // (in place, or apart)
    return !overlap(W, wlen, X, xlen);
}

}  // namespace ttm

#if !defined(__HIPCC__)
// HOST BUILDS ONLY (as ttm_score in csrc/ttm_score.h): the entry point ttm_pull_gradient of include/ttm.h around u_pull_row, row
// after row, with the library's argument checks - for the host test double of the C ABI.
extern "C" __attribute__((used, visibility("default"))) inline int ttm_pull_gradient(const ttm_program* p, const double* coef, const double* fold, int32_t k0,
                                                                                     int32_t k1, const double* Xsoa, int64_t ldx, int64_t N, const double* Gsoa,
                                                                                     int64_t ldg, const double* g_scale, int32_t logdet, double* Wsoa,
                                                                                     int64_t ldw, void*) {
    if (!p || !p->h_fold_off || k0 < 0 || k1 > p->D || k0 >= k1) return TTM_E_ARG;
    if (!ttm::pull_args_ok(coef, fold, Xsoa, ldx, N, k1 - k0, p->d_cols, Gsoa, ldg, Wsoa, ldw)) return TTM_E_ARG;
    if (p->monotonicity != TTM_MONO_SEPARABLE || !p->u_enabled || !p->ucomp || !p->ugrp) return TTM_E_UNSUPPORTED;
    const double* U = fold + (((int64_t)p->h_fold_off[p->D] + 8 + 1) & ~(int64_t)1);      // (the U section: behind the folded coefficients)
    struct XRow {
        const double* X; int64_t ld, n;
        double operator()(int var) const { return X[(int64_t)var * ld + n]; }
    };
    struct WRow {
        double* W; int64_t ld, n;
        double get(int i) const { return W[(int64_t)i * ld + n]; }
        void set(int i, double v) { W[(int64_t)i * ld + n] = v; }
    };
    for (int64_t n = 0; n < N; ++n) {
        const XRow xa{Xsoa, ldx, n}, ga{Gsoa, ldg, n};
        WRow wa{Wsoa, ldw, n};
        ttm::u_pull_row(p->ucomp, p->ugrp, U, U, p->d_cols - p->D, k0, k1, xa, ga, g_scale, logdet != 0, wa);
    }
    return TTM_OK;
}
#endif
