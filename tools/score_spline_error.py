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


def u_section_quotient(tm, T):
    """m''(t) / m'(t) of every component at the raw samples T (rows x D), from the U section of the current coefficient vector
    (the section's layout lives in tests/uform_section.py, with the tests that hold it to mpmath)."""
    from tests import uform_section
    return uform_section.quotient(tm, T)


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
