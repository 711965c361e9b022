// ttm_mcmc.h - one step of Metropolis-Hastings in the reference space of a fitted map (ttm_mh_step and ttm_mh_step_tempered of
// include/ttm.h): the per-pair routines the kernel k_mh_step of csrc/ttm_kernels.hip and the host definition of the entry point
// share.  Included at the end of csrc/ttm_rng.h (philox4x32_10, normal_pair, load_pair / store_pair come from there).
//
// The chain of row n lives in reference space: z' = rho z + sqrt(1 - rho^2) xi is reversible with respect to N(0, I), the
// pulled-back target is w(x(z)) phi(z) with w = p / q, so the acceptance ratio is w(x') / w(x) for every rho in (-1, 1) - the
// independence sampler with the map as its proposal at rho = 0.  Between two launches the caller inverts the proposal and
// evaluates the target; one launch decides the step that was proposed by the launch before it and proposes the next one.
// The tempered target of sequential Monte Carlo, q^(1 - beta) p^beta = q w^beta, pulls back to w(x(z))^beta phi(z): the same
// proposal, the acceptance ratio (w(x') / w(x))^beta.  The log-weights a step reads and writes stay UNTEMPERED - beta enters the
// comparison alone -, and ttm_mh_step is the step at beta = 1 (1.0 * x is exact: the same decision, bit for bit).
#pragma once

#include <math.h>
#include <stdint.h>

namespace ttm {

// the arguments of ttm_mh_step / ttm_mh_step_tempered as the kernel takes them (s = sqrt((1 - rho)(1 + rho)), formed once on the
// host; beta = 1 for ttm_mh_step)
struct MhStep {
    double* Zcur; int64_t ldzc;
    double* Xcur; int64_t ldxc;
    const double* logw_cur; double* logw_out;
    const double* Zprop; int64_t ldzp;
    const double* Xprop; int64_t ldxp;
    const double* logw_prop;
    double* Znext; int64_t ldzn;
    double rho, s, beta;
    double* Xrec; int64_t ldxr;
    int32_t* n_acc; int32_t* n_bad;
    int64_t N; int32_t ncols, col0;
    uint64_t seed; uint32_t draw_accept, draw_propose;
    int64_t row0;
    // the Langevin drift (ttm_mh_step_langevin; all NULL / 0 for the two plain entry points)
    double* Wcur; int64_t ldwc;
    const double* Wprop; int64_t ldwp;
    const double* corr; double kappa;
};

// The accept uniforms of global rows 2p and 2p + 1 of draw `draw` (< 2^31) under `seed`: one Philox block of their own, counter
// {lo32(p), hi32(p), 0xFFFFFFFB, 0x80000000 | draw}, key {lo32(seed), hi32(seed)}; row 2p from r[0], r[1], row 2p + 1 from r[2],
// r[3], formed as in normal_pair (0 < u < 1).  The third word is 0xFFFFFFFF - 4: the reference draws have a column number
// below 2^31 there, resample_word 0xFFFFFFFF - scheme with scheme <= 2, and normal_deviate has 0x5EED as its fourth word.
TTM_HD void mh_uniform_pair(uint64_t seed, uint32_t draw, uint64_t p, double& u0, double& u1) {
    uint32_t r[4];
    philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), 0xFFFFFFFBu, 0x80000000u | draw, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    u0 = ((double)((((uint64_t)r[0] << 32) | r[1]) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    u1 = ((double)((((uint64_t)r[2] << 32) | r[3]) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

enum { MH_REJECT = 0, MH_ACCEPT = 1, MH_BAD = 2 };

// the decision of one row from the log-weight of its proposal lp, that of its current state lc and its uniform u: a proposal
// whose weight is NaN or +inf is `bad` and rejected; one of weight zero (-inf) is rejected; a chain whose own weight is zero
// takes the first admissible proposal.  beta: the exponent on the weight ratio (the difference is formed first and rounds once,
// then the product: nothing here is an a * b + c that could contract)
TTM_HD int mh_decide(double lp, double lc, double u, double beta) {
    if (lp != lp || lp == INFINITY) return MH_BAD;
    return (lp > -INFINITY && (lc == -INFINITY || log(u) < beta * (lp - lc))) ? MH_ACCEPT : MH_REJECT;
}

// The decision with the correction c of a proposal that is not reversible with respect to N(0, I) (the Langevin step): the log
// of the acceptance ratio is beta (lp - lc) + c - the product rounds, then the sum rounds (never an FMA, whatever the flags).  A
// NaN or +inf correction is `bad` as such a weight is; -inf rejects.
TTM_HD int mh_decide_corr(double lp, double lc, double u, double beta, double c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (lp != lp || lp == INFINITY || c != c || c == INFINITY) return MH_BAD;
    if (!(lp > -INFINITY && c > -INFINITY)) return MH_REJECT;
    const double t = beta * (lp - lc);
    return (lc == -INFINITY || log(u) < t + c) ? MH_ACCEPT : MH_REJECT;
}

// The rows n0 (if v0) and n0 + 1 (if v1) of a column: ONE 16-byte access when both are wanted and the address allows it,
// guarded 8-byte ones otherwise.  A row that is not wanted is neither read nor written (a load returns 0 for it).
TTM_HD bool mh_pair_aligned(const void* col, int64_t n0) { return (((uintptr_t)col + 8 * (uintptr_t)n0) & 15) == 0; }

TTM_HD void mh_load2(const double* col, int64_t n0, bool v0, bool v1, double& a, double& b) {
    if (v0 && v1 && mh_pair_aligned(col, n0)) {
        load_pair(col + n0, a, b);
    } else {
        a = v0 ? col[n0] : 0.0;
        b = v1 ? col[n0 + 1] : 0.0;
    }
}

TTM_HD void mh_store2(double* col, int64_t n0, bool v0, bool v1, double a, double b) {
    if (v0 && v1 && mh_pair_aligned(col, n0)) {
        store_pair(col + n0, a, b);
    } else {
        if (v0) col[n0] = a;
        if (v1) col[n0 + 1] = b;
    }
}

// What one thread of k_mh_step does: pair number i of the window of global rows [row0, row0 + N), as normal_fill_pair owns it,
// in the columns j0, j0 + jstep, ... < ncols.  Every column group forms the pair's decision for itself (one Philox block, two
// pairs of log-weights); the group with j0 = 0 alone writes logw_out, n_acc and n_bad.  An element of Zcur / Xcur is read and
// written by this thread only, so the state is updated in place.
// DRIFT (ttm_mh_step_langevin with its W matrices): the decision takes the correction corr[n] (if given), an accepted row takes
// its row of Wprop into Wcur with Z and X, and the proposal is fma(rho, z, fma(kappa, z + w, s xi)) from the state after the
// decision - Z is read at rho = 0 too.  A template parameter: the plain instantiation keeps the code it had.
template <bool DRIFT>
TTM_HD void mh_step_pair(const MhStep& a, int64_t i, int j0, int jstep) {
    const uint64_t p = (uint64_t)(a.row0 >> 1) + (uint64_t)i;
    const int64_t n0 = (int64_t)(2 * p - (uint64_t)a.row0);   // local row of global row 2p: -1 .. N - 1
    if (n0 >= a.N) return;
    const bool v0 = n0 >= 0, v1 = n0 + 1 < a.N;
    const bool accept_phase = a.logw_prop != nullptr;
    bool acc0 = false, acc1 = false;
    if (accept_phase) {
        double u0, u1, lp0, lp1, lc0, lc1;
        mh_uniform_pair(a.seed, a.draw_accept, p, u0, u1);
        mh_load2(a.logw_prop, n0, v0, v1, lp0, lp1);
        mh_load2(a.logw_cur, n0, v0, v1, lc0, lc1);
        int d0, d1;
        if (DRIFT && a.corr) {
            double c0, c1;
            mh_load2(a.corr, n0, v0, v1, c0, c1);
            d0 = v0 ? mh_decide_corr(lp0, lc0, u0, a.beta, c0) : MH_REJECT;
            d1 = v1 ? mh_decide_corr(lp1, lc1, u1, a.beta, c1) : MH_REJECT;
        } else {
            d0 = v0 ? mh_decide(lp0, lc0, u0, a.beta) : MH_REJECT;
            d1 = v1 ? mh_decide(lp1, lc1, u1, a.beta) : MH_REJECT;
        }
        acc0 = d0 == MH_ACCEPT;
        acc1 = d1 == MH_ACCEPT;
        if (j0 == 0) {
            mh_store2(a.logw_out, n0, v0, v1, acc0 ? lp0 : lc0, acc1 ? lp1 : lc1);
            if (a.n_acc) {
                if (acc0) a.n_acc[n0] += 1;
                if (acc1) a.n_acc[n0 + 1] += 1;
            }
            if (a.n_bad) {
                if (d0 == MH_BAD) a.n_bad[n0] += 1;
                if (d1 == MH_BAD) a.n_bad[n0 + 1] += 1;
            }
        }
    } else if (a.logw_out && j0 == 0) {
        double lc0, lc1;
        mh_load2(a.logw_cur, n0, v0, v1, lc0, lc1);
        mh_store2(a.logw_out, n0, v0, v1, lc0, lc1);
    }
    const bool propose = a.Znext != nullptr;
    const bool read_z = propose && (DRIFT || a.rho != 0.0);    // (rho = 0 without drift: the state does not enter the proposal and is not read)
    if (!propose && !a.Xrec && !(acc0 || acc1)) return;
    for (int j = j0; j < a.ncols; j += jstep) {
        // the loads take both rows of the pair whatever was decided - the lines are fetched whole anyway, and a wave then issues
        // one 16-byte load per matrix instead of three divergent forms; only the stores into the state are per accepted row
        double z0 = 0.0, z1 = 0.0, x0 = 0.0, x1 = 0.0, w0 = 0.0, w1 = 0.0;
        if (read_z) mh_load2(a.Zcur + (int64_t)j * a.ldzc, n0, v0, v1, z0, z1);
        if (a.Xrec) mh_load2(a.Xcur + (int64_t)j * a.ldxc, n0, v0, v1, x0, x1);
        if (DRIFT && propose) mh_load2(a.Wcur + (int64_t)j * a.ldwc, n0, v0, v1, w0, w1);
        if (accept_phase) {
            double zp0, zp1, xp0, xp1;
            mh_load2(a.Zprop + (int64_t)j * a.ldzp, n0, v0, v1, zp0, zp1);
            mh_load2(a.Xprop + (int64_t)j * a.ldxp, n0, v0, v1, xp0, xp1);
            if (acc0 || acc1) {
                mh_store2(a.Zcur + (int64_t)j * a.ldzc, n0, acc0, acc1, zp0, zp1);
                mh_store2(a.Xcur + (int64_t)j * a.ldxc, n0, acc0, acc1, xp0, xp1);
            }
            z0 = acc0 ? zp0 : z0; z1 = acc1 ? zp1 : z1;
            x0 = acc0 ? xp0 : x0; x1 = acc1 ? xp1 : x1;
            if (DRIFT) {
                double wp0, wp1;
                mh_load2(a.Wprop + (int64_t)j * a.ldwp, n0, v0, v1, wp0, wp1);
                if (acc0 || acc1) mh_store2(a.Wcur + (int64_t)j * a.ldwc, n0, acc0, acc1, wp0, wp1);
                w0 = acc0 ? wp0 : w0; w1 = acc1 ? wp1 : w1;
            }
        }
        if (a.Xrec) mh_store2(a.Xrec + (int64_t)j * a.ldxr, n0, v0, v1, x0, x1);
        if (propose) {
            double xi0, xi1;
            normal_pair(a.seed, a.draw_propose, (uint32_t)a.col0 + (uint32_t)j, p, xi0, xi1);
            if (DRIFT) {
                xi0 = fma(a.rho, z0, fma(a.kappa, z0 + w0, a.s * xi0));
                xi1 = fma(a.rho, z1, fma(a.kappa, z1 + w1, a.s * xi1));
            } else if (read_z) {
                xi0 = fma(a.rho, z0, a.s * xi0);
                xi1 = fma(a.rho, z1, a.s * xi1);
            }
            mh_store2(a.Znext + (int64_t)j * a.ldzn, n0, v0, v1, xi0, xi1);
        }
    }
}

TTM_HD bool mh_ranges_overlap(const double* x, const double* y, int64_t N) {
    const uintptr_t x0 = (uintptr_t)x, y0 = (uintptr_t)y, len = 8 * (uintptr_t)N;
    return x0 < y0 + len && y0 < x0 + len;
}

// argument check of ttm_mh_step / ttm_mh_step_tempered / ttm_mh_step_langevin, shared by the library and the host definition below
TTM_HD bool mh_step_args_ok(const MhStep& a) {
    if (!a.Zcur || !a.Xcur || !a.logw_cur || a.N < 1 || a.ncols < 1 || a.col0 < 0 || a.row0 < 0 || a.N > INT64_MAX - a.row0) return false;
    if (a.draw_accept >= 0x80000000u || a.draw_propose >= 0x80000000u) return false;
    if (!a.logw_prop && !a.Znext) return false;                                 // neither phase
    if (a.ldzc < a.N || a.ldxc < a.N || a.ldzp < a.N || a.ldxp < a.N || a.ldzn < a.N || a.ldxr < a.N) return false;   // (of matrices not in use too)
    if (a.logw_prop && (!a.Zprop || !a.Xprop || !a.logw_out)) return false;
    if (!(fabs(a.rho) < 1.0)) return false;                                      // (NaN fails the comparison)
    if (!(a.beta > 0.0 && a.beta <= 1.0)) return false;                          // (likewise)
    if ((a.Wcur != nullptr) != (a.Wprop != nullptr) || a.ldwc < a.N || a.ldwp < a.N) return false;   // (the W matrices: both or neither)
    if (a.corr && (!a.logw_prop || !a.Wcur)) return false;                       // (a correction: of a drifted proposal that is decided here)
    if (!(fabs(a.kappa) < INFINITY)) return false;
    if (a.logw_out && (mh_ranges_overlap(a.logw_out, a.logw_cur, a.N) || (a.logw_prop && mh_ranges_overlap(a.logw_out, a.logw_prop, a.N)))) return false;
    return true;
}

TTM_HD MhStep mh_step_pack(double* Zcur, int64_t ldzc, double* Xcur, int64_t ldxc, const double* logw_cur, double* logw_out, const double* Zprop,
                           int64_t ldzp, const double* Xprop, int64_t ldxp, const double* logw_prop, double* Znext, int64_t ldzn, double rho, double beta,
                           double* Xrec, int64_t ldxr, int32_t* n_acc, int32_t* n_bad, int64_t N, int32_t ncols, int32_t col0, uint64_t seed, uint32_t draw_accept,
                           uint32_t draw_propose, int64_t row0, double* Wcur = nullptr, int64_t ldwc = INT64_MAX, const double* Wprop = nullptr,
                           int64_t ldwp = INT64_MAX, const double* corr = nullptr, double kappa = 0.0) {
    MhStep a;
    a.Zcur = Zcur; a.ldzc = ldzc; a.Xcur = Xcur; a.ldxc = ldxc; a.logw_cur = logw_cur; a.logw_out = logw_out;
    a.Zprop = Zprop; a.ldzp = ldzp; a.Xprop = Xprop; a.ldxp = ldxp; a.logw_prop = logw_prop;
    a.Znext = Znext; a.ldzn = ldzn; a.rho = rho; a.s = sqrt((1.0 - rho) * (1.0 + rho)); a.beta = beta;
    a.Xrec = Xrec; a.ldxr = ldxr; a.n_acc = n_acc; a.n_bad = n_bad;
    a.N = N; a.ncols = ncols; a.col0 = col0; a.seed = seed; a.draw_accept = draw_accept; a.draw_propose = draw_propose; a.row0 = row0;
    a.Wcur = Wcur; a.ldwc = ldwc; a.Wprop = Wprop; a.ldwp = ldwp; a.corr = corr; a.kappa = kappa;
    return a;
}

// The correction of the Langevin step (ttm_langevin_corr).  With d = z + w the drift direction at the state, d' that at the
// proposal, mu(z) = rho z + kappa d(z) and s^2 = (1 - rho)(1 + rho),
//     c = log N(z; mu(z'), s^2) - log N(z'; mu(z), s^2) + log phi(z') - log phi(z)
//       = kappa [ sum_j (b_j d'_j - a_j d_j) + (kappa / 2) sum_j (d_j^2 - d'_j^2) ] / s^2,     a = z' - rho z,  b = z - rho z'
// (the phi terms and a^2 - b^2 cancel analytically: c is 0 at kappa = 0).  Two running sums per row over the columns in
// ascending order, every product an FMA, the division by s^2 last.
struct LangevinCorr {
    const double* Zcur; int64_t ldzc;
    const double* Wcur; int64_t ldwc;
    const double* Zprop; int64_t ldzp;
    const double* Wprop; int64_t ldwp;
    double rho, kappa, s2;
    int64_t N; int32_t ncols;
    double* corr;
};

TTM_HD void langevin_corr_term(double rho, double z, double w, double zp, double wp, double& s1, double& s2) {
    const double d = z + w, dp = zp + wp;
    const double a = fma(-rho, z, zp), b = fma(-rho, zp, z);
    s1 = fma(-a, d, fma(b, dp, s1));
    s2 = fma(-dp, dp, fma(d, d, s2));
}

// what one thread of k_langevin_corr does: the rows 2 i and 2 i + 1
TTM_HD void langevin_corr_pair(const LangevinCorr& a, int64_t i) {
    const int64_t n0 = 2 * i;
    if (n0 >= a.N) return;
    const bool v1 = n0 + 1 < a.N;
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0;
    for (int j = 0; j < a.ncols; ++j) {
        double z0, z1, w0, w1, zp0, zp1, wp0, wp1;
        mh_load2(a.Zcur + (int64_t)j * a.ldzc, n0, true, v1, z0, z1);
        mh_load2(a.Wcur + (int64_t)j * a.ldwc, n0, true, v1, w0, w1);
        mh_load2(a.Zprop + (int64_t)j * a.ldzp, n0, true, v1, zp0, zp1);
        mh_load2(a.Wprop + (int64_t)j * a.ldwp, n0, true, v1, wp0, wp1);
        langevin_corr_term(a.rho, z0, w0, zp0, wp0, s1a, s2a);
        langevin_corr_term(a.rho, z1, w1, zp1, wp1, s1b, s2b);
    }
    mh_store2(a.corr, n0, true, v1, a.kappa * fma(0.5 * a.kappa, s2a, s1a) / a.s2, a.kappa * fma(0.5 * a.kappa, s2b, s1b) / a.s2);
}

TTM_HD bool langevin_corr_args_ok(const LangevinCorr& a) {
    if (!a.Zcur || !a.Wcur || !a.Zprop || !a.Wprop || !a.corr || a.N < 1 || a.ncols < 1) return false;
    if (a.ldzc < a.N || a.ldwc < a.N || a.ldzp < a.N || a.ldwp < a.N) return false;
    return fabs(a.rho) < 1.0 && fabs(a.kappa) < INFINITY;                         // (NaN fails the comparisons)
}

TTM_HD LangevinCorr langevin_corr_pack(const double* Zcur, int64_t ldzc, const double* Wcur, int64_t ldwc, const double* Zprop, int64_t ldzp,
                                       const double* Wprop, int64_t ldwp, double rho, double kappa, int64_t N, int32_t ncols, double* corr) {
    LangevinCorr a;
    a.Zcur = Zcur; a.ldzc = ldzc; a.Wcur = Wcur; a.ldwc = ldwc; a.Zprop = Zprop; a.ldzp = ldzp; a.Wprop = Wprop; a.ldwp = ldwp;
    a.rho = rho; a.kappa = kappa; a.s2 = (1.0 - rho) * (1.0 + rho); a.N = N; a.ncols = ncols; a.corr = corr;
    return a;
}

}  // namespace ttm

#if !defined(__HIPCC__)
// HOST BUILDS ONLY (as ttm_normal_fill in csrc/ttm_rng.h): the entry points ttm_mh_step_langevin, ttm_mh_step_tempered (= no
// drift), ttm_mh_step (= beta 1) and ttm_langevin_corr of include/ttm.h for the host test double of the C ABI - the kernels'
// thread bodies, pair after pair.
extern "C" __attribute__((used, visibility("default"))) inline int ttm_mh_step_langevin(double* Zcur, int64_t ldzc, double* Xcur, int64_t ldxc,
                                                                                        const double* logw_cur, double* logw_out, const double* Zprop,
                                                                                        int64_t ldzp, const double* Xprop, int64_t ldxp, const double* logw_prop,
                                                                                        double* Znext, int64_t ldzn, double rho, double beta, double* Xrec,
                                                                                        int64_t ldxr, int32_t* n_acc, int32_t* n_bad, int64_t N, int32_t ncols,
                                                                                        int32_t col0, uint64_t seed, uint32_t draw_accept, uint32_t draw_propose,
                                                                                        int64_t row0, double* Wcur, int64_t ldwc, const double* Wprop,
                                                                                        int64_t ldwp, const double* corr, double kappa, void*) {
    const ttm::MhStep a = ttm::mh_step_pack(Zcur, ldzc, Xcur, ldxc, logw_cur, logw_out, Zprop, ldzp, Xprop, ldxp, logw_prop, Znext, ldzn, rho, beta, Xrec,
                                            ldxr, n_acc, n_bad, N, ncols, col0, seed, draw_accept, draw_propose, row0, Wcur, ldwc, Wprop, ldwp, corr, kappa);
    if (!ttm::mh_step_args_ok(a)) return TTM_E_ARG;
    const int64_t np = ttm::normal_fill_pairs(N, row0);
    if (Wcur)
        for (int64_t i = 0; i < np; ++i) ttm::mh_step_pair<true>(a, i, 0, 1);
    else
        for (int64_t i = 0; i < np; ++i) ttm::mh_step_pair<false>(a, i, 0, 1);
    return TTM_OK;
}

extern "C" __attribute__((used, visibility("default"))) inline int ttm_langevin_corr(const double* Zcur, int64_t ldzc, const double* Wcur, int64_t ldwc,
                                                                                     const double* Zprop, int64_t ldzp, const double* Wprop, int64_t ldwp,
                                                                                     double rho, double kappa, int64_t N, int32_t ncols, double* corr, void*) {
    const ttm::LangevinCorr a = ttm::langevin_corr_pack(Zcur, ldzc, Wcur, ldwc, Zprop, ldzp, Wprop, ldwp, rho, kappa, N, ncols, corr);
    if (!ttm::langevin_corr_args_ok(a)) return TTM_E_ARG;
    for (int64_t i = 0; i < (N + 1) / 2; ++i) ttm::langevin_corr_pair(a, i);
    return TTM_OK;
}

extern "C" __attribute__((used, visibility("default"))) inline int ttm_mh_step_tempered(double* Zcur, int64_t ldzc, double* Xcur, int64_t ldxc,
                                                                                        const double* logw_cur, double* logw_out, const double* Zprop,
                                                                                        int64_t ldzp, const double* Xprop, int64_t ldxp, const double* logw_prop,
                                                                                        double* Znext, int64_t ldzn, double rho, double beta, double* Xrec,
                                                                                        int64_t ldxr, int32_t* n_acc, int32_t* n_bad, int64_t N, int32_t ncols,
                                                                                        int32_t col0, uint64_t seed, uint32_t draw_accept, uint32_t draw_propose,
                                                                                        int64_t row0, void*) {
    return ttm_mh_step_langevin(Zcur, ldzc, Xcur, ldxc, logw_cur, logw_out, Zprop, ldzp, Xprop, ldxp, logw_prop, Znext, ldzn, rho, beta, Xrec, ldxr, n_acc,
                                n_bad, N, ncols, col0, seed, draw_accept, draw_propose, row0, nullptr, N, nullptr, N, nullptr, 0.0, nullptr);
}

extern "C" __attribute__((used, visibility("default"))) inline int ttm_mh_step(double* Zcur, int64_t ldzc, double* Xcur, int64_t ldxc, const double* logw_cur,
                                                                               double* logw_out, const double* Zprop, int64_t ldzp, const double* Xprop,
                                                                               int64_t ldxp, const double* logw_prop, double* Znext, int64_t ldzn, double rho,
                                                                               double* Xrec, int64_t ldxr, int32_t* n_acc, int32_t* n_bad, int64_t N,
                                                                               int32_t ncols, int32_t col0, uint64_t seed, uint32_t draw_accept,
                                                                               uint32_t draw_propose, int64_t row0, void*) {
    return ttm_mh_step_tempered(Zcur, ldzc, Xcur, ldxc, logw_cur, logw_out, Zprop, ldzp, Xprop, ldxp, logw_prop, Znext, ldzn, rho, 1.0, Xrec, ldxr, n_acc,
                                n_bad, N, ncols, col0, seed, draw_accept, draw_propose, row0, nullptr);
}
#endif
