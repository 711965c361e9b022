"""
The yardsticks of tests/test_pull_gradient.py - test infrastructure, from the oracle and the stored numbers of the U section alone
(nothing here calls the routine under test; tools/pull_spline_error.py prints the tables the test file records).

jacobian_truth: J_ref[n, j, i] = dS_j / dx_c(i) of the oracle's map at the first ROWS raw samples of a case of tests/test_score.py,
by central differences of OracleMap.map in every own column with the steps h, h/2, h/4, h = 1e-3 x the column's deviation,
Richardson-extrapolated twice (tests/test_score.py: richardson).  e_FD = max |r1 - r2| / (1 + |r2|); rows are kept when the
whole stencil is finite and e_FD <= 1e-9 in every entry.

logdet_truth: l_ref[n, i] = m_i''(u) / m_i'(u) / sigma_i at the STANDARDISED sample u - m' = der_fun_mon . coeffs_mon of the
oracle there, m'' by the same differences of m' in u (h = 1e-3: a standardised column has deviation 1); a row's own estimate is
|r1 - r2| / |m'| / (1 + |m'' / m'|), and rows are kept when it is finite and <= 1e-9 in every component.

slope_error / quotient_error: the resident splines against the oracle at the standardised samples, evaluated in NumPy from the
U section's numbers (tests/uform_section.py) - e_slope = max |m'_U - m'_ref| / sigma / (1 + |m'_ref| / sigma) (the metric an
entry of J_ref enters the backward error with), e_spl = max |q_U - q_ref| / (1 + |q_ref|), q = m'' / m' (the metric of E_SPL in
tests/test_score.py, there at the raw sample).
"""
import numpy as np

from tests import test_score as ts
from tests import uform_section

ROWS = ts.ROWS
STD = 'c5_shape_std'             # c5_shape refitted on standardised data (the map of ts.test_standardised_call_...): mean 0, deviation 1
CASES = ts.ALL_CASES + [STD]
_J, _L = {}, {}


def build(name):
    """(tm, om, X, E) of a case: those of tests/test_score.py, and STD."""
    if name != STD:
        return ts.build(name)
    from tests import test_band as band
    from triangular_transport_toolbox_amd.transport_map import transport_map
    from oracle.ttm_oracle import OracleMap
    tm0, _, X, E = ts.build('c5_shape', n=1201)
    Xs = (X - X.mean(axis=0)) / X.std(axis=0)
    mon, non = band.CASES['c5_shape']['spec']()
    tm = transport_map(X=Xs, monotone=mon, nonmonotone=non, verbose=False, monotonicity='separable monotonicity')
    om = OracleMap(X=Xs, monotone=mon, nonmonotone=non, monotonicity='separable monotonicity')
    for k in range(tm.D):
        tm.coeffs_mon[k], tm.coeffs_nonmon[k] = tm0.coeffs_mon[k].copy(), tm0.coeffs_nonmon[k].copy()
        om.coeffs_mon[k], om.coeffs_nonmon[k] = tm0.coeffs_mon[k].copy(), tm0.coeffs_nonmon[k].copy()
    return tm, om, Xs, E


def jacobian_truth(name, om, X, E):
    """(J_ref [ROWS x D x D], keep [ROWS], e_FD over the kept rows) - computed once per case and left unchanged."""
    if name not in _J:
        Xr = np.array(X[:ROWS], dtype=float)
        D = om.D
        J = np.zeros((ROWS, D, D))
        ok = np.ones(ROWS, dtype=bool)
        worst = np.zeros(ROWS)
        for i in range(D):
            c = E + i

            def S(col):
                Xp = Xr.copy()
                Xp[:, c] = col[:, 0]
                return om.map(Xp)
            r2, d, fin = ts.richardson(S, Xr[:, c:c + 1], 1e-3 * float(om.X_std[c]))
            with np.errstate(all='ignore'):
                err = d / (1.0 + np.abs(r2))
                ok &= np.all(fin & (err <= 1e-9), axis=1)
                worst = np.maximum(worst, np.max(np.where(np.isfinite(err), err, np.inf), axis=1))
            J[:, :, i] = r2
        J.setflags(write=False)
        ok.setflags(write=False)
        _J[name] = (J, ok, float(worst[ok].max()) if ok.any() else np.inf)
    return _J[name]


def _oracle_slopes(om, X, E):
    """(u [ROWS x d], m' [ROWS x D], m'' [ROWS x D], |r1 - r2| of m'', finite) at the standardised samples."""
    Xr = np.array(X[:ROWS], dtype=float)
    U = om._standardized(Xr)
    D = om.D
    m1, m2, dd, fin = (np.zeros((ROWS, D)) for _ in range(4))
    for k in range(D):
        c = E + k

        def slope(col):
            Up = U.copy()
            Up[:, c] = col
            return om.der_fun_mon(k, Up) @ om.coeffs_mon[k]
        m1[:, k] = slope(U[:, c])
        m2[:, k], dd[:, k], fin[:, k] = ts.richardson(slope, U[:, c], 1e-3)
    return U, m1, m2, dd, fin.astype(bool)


def logdet_truth(name, om, X, E):
    """(l_ref [ROWS x D] in raw coordinates, keep [ROWS], the largest own estimate over the kept rows)."""
    if name not in _L:
        _, m1, m2, dd, fin = _oracle_slopes(om, X, E)
        sigma = np.asarray(om.X_std, dtype=float)[E:E + om.D]
        with np.errstate(all='ignore'):
            q = m2 / m1
            own = dd / np.abs(m1) / (1.0 + np.abs(q))
            keep = np.all(fin & np.isfinite(q) & (own <= 1e-9), axis=1)
        l = q / sigma
        l.setflags(write=False)
        keep.setflags(write=False)
        _L[name] = (l, keep, float(own[keep].max()) if keep.any() else np.inf)
    return _L[name]


def u_section_slopes(tm, Ustd):
    """(m' [rows x D], m'' / m' [rows x D]) of every component at the standardised own samples Ustd (rows x D), in NumPy from the U
    section of the current coefficient vector (the arithmetic of uform_section.quotient, which keeps the quotient alone)."""
    comps = uform_section.read(tm)
    d1, q = np.zeros(Ustd.shape), np.zeros(Ustd.shape)
    for k, c in enumerate(comps):
        t = Ustd[:, k]
        a, b = np.full(t.shape, c.own_linear_slope), np.zeros(t.shape)
        if c.nI > 0:
            u = t * c.sp_b + c.sp_a
            fl_ = np.floor(np.clip(u, -1.0, c.nI - 2.0))
            s_ = 2.0 * (u - fl_) - 1.0
            for n in range(len(t)):
                P = np.polynomial.Polynomial(c.table[int(fl_[n]) + 1])
                a[n] += P.deriv(1)(s_[n]) * c.sp_ds
                b[n] += P.deriv(2)(s_[n]) * c.sp_ds * c.sp_ds
        d1[:, k] = a
        with np.errstate(all='ignore'):
            q[:, k] = b / a
    return d1, q


def spline_errors(tm, om, X, E):
    """(e_slope, e_spl at the standardised sample, rows that enter e_spl) of a case: see the module's docstring."""
    U, m1, m2, dd, fin = _oracle_slopes(om, X, E)
    D = om.D
    sigma = np.asarray(om.X_std, dtype=float)[E:E + D]
    d1, q_u = u_section_slopes(tm, U[:, E:E + D])
    e_slope = float(np.max(np.abs(d1 - m1) / sigma / (1.0 + np.abs(m1) / sigma)))
    with np.errstate(all='ignore'):
        q = m2 / m1
        ok = fin & np.isfinite(q) & np.isfinite(q_u) & (dd / np.abs(m1) / (1.0 + np.abs(q)) <= 1e-9)
    e_spl = float(np.max(np.abs(q_u[ok] - q[ok]) / (1.0 + np.abs(q[ok])))) if ok.any() else 0.0
    return e_slope, e_spl, int(np.all(ok, axis=1).sum())
