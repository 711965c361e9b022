"""e_spl of tests/test_score.py: the error of the log-determinant quotient m''(t) / m'(t) taken from the degree-11 spline pieces
of the U section (their value and first derivative are verified when ttm_fold builds them; the second derivative is not).

Runs on the CPU, on the host test double.  Per case of tests/test_score.py and at its 200 test points (raw samples):
  q_u   = P''(s) sp_ds^2 / (P'(s) sp_ds + own1), evaluated HERE in NumPy from the numbers ttm_fold wrote into the U section (spline
          geometry, the column's twelve coefficients, the slope of a linear own term: include/ttm.h "U-form") - independent of the
          routine under test (u_score_row), whose log-determinant term is printed beside it for comparison;
  q_ref = m'' / m' of the oracle: m' = der_fun_mon . coeffs_mon, m'' by central differences of m' in the own column with steps
          h, h/2, h/4 (h = 1e-3 x the column's standard deviation), Richardson-extrapolated twice.
Prints e_spl = max |q_u - q_ref| / (1 + |q_ref|) and the differences' own error estimate per case.

    python tools/score_spline_error.py [case ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


UC_LEN, U_TSTRIDE, U_GSTRIDE, U_GHALF, UCF_OWN, PLAN_HF = 8, 14, 24, 12, 1, 1       # include/ttm.h


def u_section_quotient(tm, T):
    """m''(t) / m'(t) of every component at the raw samples T (rows x D), from the U section of the current coefficient vector."""
    cm = tm._cm
    coef = tm._pack_coeffs()
    fold = coef._ttm_fold.cpu().numpy()
    U = fold[int(tm._lib.ttm_uform_offset(tm._pp)):]
    uc = np.asarray(cm.ucomp[:cm.D * UC_LEN]).reshape(-1, UC_LEN)
    ug = np.asarray(cm.ugrp).reshape(-1, 8)
    q = np.zeros(T.shape)
    for k in range(cm.D):
        _, _, n_grp, grp_off, nI, tab_off, dbl_off, flags = (int(v) for v in uc[k])
        cd = U[dbl_off:]
        own1 = 0.0
        if flags & UCF_OWN:
            fl = int(ug[grp_off + n_grp, 1])
            assert not (fl & PLAN_HF) and ((fl >> 24) & 15) <= 1, 'own terms beyond a linear one: extend this tool'
            own1 = cd[4 + U_GSTRIDE * n_grp + U_GHALF + 1]
        t = T[:, k]
        d1, d2 = np.full(t.shape, own1), np.zeros(t.shape)
        if nI > 0:
            sp_a, sp_b, sp_ds = cd[1], cd[2], cd[3]
            u = t * sp_b + sp_a
            fl_ = np.floor(np.clip(u, -1.0, nI - 2.0))
            s_ = 2.0 * (u - fl_) - 1.0
            tab = U[tab_off:tab_off + nI * U_TSTRIDE].reshape(nI, U_TSTRIDE)[:, :12]
            for n in range(len(t)):
                P = np.polynomial.Polynomial(tab[int(fl_[n]) + 1])
                d1[n] += P.deriv(1)(s_[n]) * sp_ds
                d2[n] += P.deriv(2)(s_[n]) * sp_ds * sp_ds
        q[:, k] = d2 / d1
    return q


def main(names):
    from tests import test_score as ts
    from tests.hostemu import emu
    with emu.install():
        for name in names or ts.ALL_CASES:
            tm, om, X, E = ts.build(name)
            D = tm.D
            Xr = np.array(X[:ts.ROWS], dtype=float)
            std = np.asarray(tm.X_std, dtype=float)[E:E + D]
            mean = np.asarray(tm.X_mean, dtype=float)[E:E + D]
            q_u = u_section_quotient(tm, Xr[:, E:E + D])
            Xd = tm._import(Xr, True)
            G = tm.score_device(Xd, ts.ROWS, g_scale=tm._to_dev(np.zeros(D)), ld_affine=tm._to_dev(np.column_stack((std, mean))))
            q_code = tm._export(G, ts.ROWS, 0, D, False)
            with np.errstate(all='ignore'):
                d_code = np.abs(q_code - q_u) / (1.0 + np.abs(q_u))
            code_diff = float(np.nanmax(d_code))
            worst, fd_own = 0.0, 0.0
            for k in range(D):
                c = E + k

                def m1(col):
                    Xp = Xr.copy()
                    Xp[:, c] = col
                    return om.der_fun_mon(k, Xp) @ om.coeffs_mon[k]
                m2, d, fin = ts.richardson(m1, Xr[:, c], 1e-3 * float(om.X_std[c]))
                q_ref = m2 / m1(Xr[:, c])
                ok = fin & np.isfinite(q_ref) & np.isfinite(q_u[:, k])
                worst = max(worst, float(np.max(np.abs(q_u[ok, k] - q_ref[ok]) / (1.0 + np.abs(q_ref[ok])))))
                fd_own = max(fd_own, float(np.max(d[ok] / np.abs(m1(Xr[:, c])[ok]) / (1.0 + np.abs(q_ref[ok])))))
            print("    '%s': %.1e,   # (differences' own error %.1e; u_score_row's quotient against the NumPy one: %.1e)" % (name, worst, fd_own, code_diff), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
