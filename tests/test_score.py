"""
Score of the pullback density (transport_map.evaluate_pullback_score / score_device, include/ttm.h: ttm_score) on the host test
double: the shared per-sample routine u_score_row (csrc/ttm_score.h) against finite differences of the oracle's density.

Truth (`fd_truth`): central differences of log OracleMap.evaluate_pullback_density in every own column with steps h, h/2,
h/4, h = 1e-3 x the column's standard deviation, Richardson-extrapolated twice: r1 = (4 D(h/2) - D(h)) / 3, r2 likewise from
h/2 and h/4.  r2 is the expected score; e_FD = |r1 - r2| / (1 + |r2|) is the reference's own error estimate.  Rows are kept
when the whole stencil is finite and e_FD <= 1e-9 in every column - a rule of the reference alone.  It drops nothing in any
case but class_55 (random coefficients make some of its components non-monotone), where at least 130 of 200 rows remain.

Tolerance in the metric |G - r2| / (1 + |r2|): 8 x (e_FD + e_spl), e_FD the largest over the kept rows (computed here, from
the oracle), e_spl the error of the second derivative of the degree-11 spline pieces in the log-determinant quotient (E_SPL
below).  The factor 8: both numbers are maxima over samples, not suprema over intervals, and the kernels sum in another order.

The training data of the cases is not standardised (means of ~0.3, deviations of 1.1 - 1.9): the 1 / sigma factor on the
Gaussian part and the raw-sample argument of the log-determinant part are pinned separately by the same comparison.
"""
import ctypes

import numpy as np
import pytest

from tests import test_band as band
from tests import test_band_linear as band_linear

ROWS = 200
BAND_CASES = sorted(band.CASES)
LONG_OWN = 'long_own'            # tests/test_band_linear.py: mixed_long (ten components: spline only / linear only / both)
DENSE = 'dense_5'                # specs.dense_separable_spec(5, 3): separable, U-form, not banded
ALL_CASES = BAND_CASES + [LONG_OWN, DENSE]

# e_spl per case: max over the 200 test points and the components of |q_u - q_ref| / (1 + |q_ref|), q = m''(t) / m'(t) at the
# raw sample.  q_u: from the U section the parent commit's ttm_fold writes on the host test double (P''(s) sp_ds^2 /
# (P'(s) sp_ds + own1), evaluated in NumPy from the section's numbers - not by the routine under test, whose own quotient agrees
# with it to 2e-14); q_ref: m' = der_fun_mon . coeffs_mon
# of the oracle, m'' by its central differences with the steps and the double Richardson extrapolation above.  Measured once on
# the CPU by tools/score_spline_error.py, before the push-form kernel was written; the differences' own error (|r1 - r2|, the same
# estimate as e_FD) is below 3e-12 in every case but class_55 (6e-10: derivatives near zero where its components are not monotone), so
# the figures are the splines', not the yardstick's.
E_SPL = {
    'c5_shape': 4.5e-10, 'class_55': 2.1e-09, 'class_77': 3.7e-10, 'lag_one': 4.8e-10,
    'few_c2b': 2.0e-10, 'few_c3': 2.3e-10, 'few_cond': 3.2e-10, 'few_cond2': 2.6e-10, 'few_entf': 3.2e-10,
    'few_ents': 0.0,             # (linear monotone parts, no spline anywhere: m'' = 0 exactly)
    'few_ex05': 1.1e-10, 'long_own': 5.8e-10, 'dense_5': 5.6e-10,
}


def build(name, n=5003):
    """(tm, om, X, E) of a case: the maps of tests/test_band.py, the long map with own terms, the dense non-banded map."""
    if name in band.CASES:
        tm, om, X, _ = band._build(name, n=n)
        return tm, om, X, band.CASES[name]['d'] - band.CASES[name]['D']
    if name == LONG_OWN:
        tm, om, X, _ = band_linear._build('mixed_long', n=n)
        return tm, om, X, 0
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    from oracle.ttm_oracle import OracleMap
    d = 5
    rng = np.random.default_rng(17 * d)
    X = rng.standard_normal((n, d)) @ (np.tril(rng.standard_normal((d, d)) * 0.4) + np.eye(d)).T + 0.3 * rng.standard_normal((n, d)) ** 2
    mon, non = specs.dense_separable_spec(5, 3)
    kw = dict(monotonicity='separable monotonicity')
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw)
    om = OracleMap(X=X, monotone=mon, nonmonotone=non, **kw)
    for k in range(d):
        cm_ = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
        cn_ = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        tm.coeffs_mon[k], om.coeffs_mon[k] = cm_.copy(), cm_.copy()
        tm.coeffs_nonmon[k], om.coeffs_nonmon[k] = cn_.copy(), cn_.copy()
    return tm, om, X, 0


def richardson(f, x0, h):
    """Central differences of f at x0 with steps h, h/2, h/4, extrapolated twice: (r2, |r1 - r2|, finite on the whole stencil)."""
    def cd(step):
        a, b = f(x0 + step), f(x0 - step)
        return (a - b) / (2.0 * step), np.isfinite(a) & np.isfinite(b)
    with np.errstate(all='ignore'):
        d1, f1 = cd(h)
        d2, f2 = cd(h / 2)
        d4, f4 = cd(h / 4)
        r1, r2 = (4.0 * d2 - d1) / 3.0, (4.0 * d4 - d2) / 3.0
        return r2, np.abs(r1 - r2), f1 & f2 & f4


_TRUTH = {}


def fd_truth(name, om, X, E):
    """(r2 [ROWS x D], keep [ROWS], e_FD) of a case - from the oracle alone; computed once per case and left unchanged."""
    if name not in _TRUTH:
        Xr = np.array(X[:ROWS], dtype=float)
        D = om.D
        r2 = np.zeros((ROWS, D))
        err = np.zeros((ROWS, D))
        fin = np.ones((ROWS, D), dtype=bool)
        for k in range(D):
            c = E + k

            def logp(col):
                Xp = Xr.copy()
                Xp[:, c] = col
                return np.log(om.evaluate_pullback_density(Xp[:, E:], X_star=Xp[:, :E] if E else None))
            r2[:, k], d, fin[:, k] = richardson(logp, Xr[:, c], 1e-3 * float(om.X_std[c]))
            with np.errstate(all='ignore'):
                err[:, k] = d / (1.0 + np.abs(r2[:, k]))
        with np.errstate(all='ignore'):
            keep = np.all(fin & (err <= 1e-9), axis=1)
        r2.setflags(write=False)
        keep.setflags(write=False)
        _TRUTH[name] = (r2, keep, float(err[keep].max()))
    return _TRUTH[name]


def metric(G, ref):
    return float(np.max(np.abs(G - ref) / (1.0 + np.abs(ref))))


def check_against_truth(name, G, om, X, E, label=''):
    """The row filter's two counts, then the product against r2 at 8 (e_FD + e_spl); every figure is printed before it is held."""
    r2, keep, e_fd = fd_truth(name, om, X, E)
    kept = int(keep.sum())
    tol = 8.0 * (e_fd + E_SPL[name])
    err = metric(G[:ROWS][keep], r2[keep])
    print('%s %s: kept %d / %d, e_FD %.3e, e_spl %.1e, tolerance %.3e, error %.3e' % (name, label, kept, ROWS, e_fd, E_SPL[name], tol, err))
    if name == 'class_55':
        assert 130 <= kept < ROWS
    else:
        assert kept == ROWS
    assert np.all(np.isfinite(G[:ROWS][keep]))
    assert err <= tol, (name, label, err, tol)


def own_and_star(X, E, rows=None):
    Xr = X if rows is None else X[:rows]
    return Xr[:, E:], (Xr[:, :E] if E else None)


@pytest.mark.parametrize('name', ALL_CASES)
def test_score_against_finite_differences_of_the_oracle(name):
    from tests.hostemu import emu
    with emu.install():
        tm, om, X, E = build(name)
        assert tm._cm.u_enabled
        # which routine a map takes: the dense map has no push records (the generic routine is all there is for it), the others are
        # banded - on the device they take k_band_score (tests/test_band_score.py holds the kernels' names); here every map runs
        # u_score_row, the body of the generic kernel
        assert (tm._cm.u_p_lag == 0) == (name == DENSE)
        own, star = own_and_star(X, E, ROWS)
        G = tm.evaluate_pullback_score(own, X_star=star)
        assert G.shape == (ROWS, tm.D)
        check_against_truth(name, G, om, X, E, 'host double')


@pytest.mark.parametrize('name', ['c5_shape', LONG_OWN])
def test_standardised_call_equals_the_raw_call_on_standardised_data(name):
    """score_device without g_scale / ld_affine against evaluate_pullback_score on data that is already standardised: there
    g_scale = 1 and ld_affine is the identity to rounding, and the two calls differ only in those arguments."""
    from tests.hostemu import emu
    from triangular_transport_toolbox_amd.transport_map import transport_map
    with emu.install():
        tm0, om, X, E = build(name, n=1201)
        Xs = (X - X.mean(axis=0)) / X.std(axis=0)
        mon, non = (band.CASES[name]['spec']() if name in band.CASES else band_linear.CASES['mixed_long']['spec']())
        tm = transport_map(X=Xs, monotone=mon, nonmonotone=non, verbose=False, monotonicity='separable monotonicity')
        for k in range(tm.D):
            tm.coeffs_mon[k], tm.coeffs_nonmon[k] = tm0.coeffs_mon[k].copy(), tm0.coeffs_nonmon[k].copy()
        assert np.max(np.abs(tm.X_mean)) < 1e-14 and np.max(np.abs(np.asarray(tm.X_std) - 1.0)) < 1e-14
        raw = tm.evaluate_pullback_score(Xs[:ROWS])
        Xd = tm._import(Xs[:ROWS], True)
        G = tm.score_device(Xd, ROWS)
        plain = tm._export(G, ROWS, 0, tm.D, False)
        assert np.all(np.isfinite(raw)) and metric(plain, raw) <= 1e-13


def test_conditioning_columns_given_separately_or_stacked_give_the_same_bits():
    from tests.hostemu import emu
    with emu.install():
        tm, om, X, E = build('few_cond', n=1201)
        assert E == 1
        a = tm.evaluate_pullback_score(X[:ROWS, E:], X_star=X[:ROWS, :E])
        b = tm.evaluate_pullback_score(X[:ROWS])
        assert a.shape == (ROWS, tm.D) and np.array_equal(a, b)


def test_maps_without_a_univariate_form_are_refused_with_the_reason(monkeypatch):
    from tests.hostemu import emu
    from tests.test_uform import _narrow_map
    from tests.util import load_case, case_X, ctor_kwargs, coeff_lists
    from triangular_transport_toolbox_amd import specs, termtable
    from triangular_transport_toolbox_amd.transport_map import transport_map
    with emu.install():
        rng = np.random.default_rng(3)
        X = rng.standard_normal((300, 3))
        mon, non = specs.banded_separable_spec(3, band=2)
        # an integrated-rectifier map
        mon_i, non_i = specs.banded_integrated_spec(3, 2, 2)
        tm = transport_map(X=X, monotone=mon_i, nonmonotone=non_i, verbose=False,
                           monotonicity='integrated rectifier')
        with pytest.raises(NotImplementedError, match='integrated'):
            tm.evaluate_pullback_score(X)
        # a separable map with a cross term
        tm = transport_map(X=X, monotone=mon, nonmonotone=[[[]], [[], [0]], [[], [0], [1], [0, 1]]], verbose=False,
                           monotonicity='separable monotonicity')
        with pytest.raises(NotImplementedError, match='cross'):
            tm.evaluate_pullback_score(X)
        # standardize_samples = False: the density takes its two parts on different samples - no function of X to differentiate
        mon_s, non_s = specs.banded_separable_spec(3, band=2)
        tm = transport_map(X=X, monotone=mon_s, nonmonotone=non_s, verbose=False, monotonicity='separable monotonicity',
                           standardize_samples=False)
        with pytest.raises(NotImplementedError, match='standardize_samples'):
            tm.evaluate_pullback_score(X)
        # special-term scales too fine for a spline (tests/test_uform.py)
        mon_n, non_n, kw = _narrow_map(0.02)
        tm = transport_map(X=X, monotone=mon_n, nonmonotone=non_n, **kw)
        with pytest.raises(NotImplementedError, match='too fine'):
            tm.evaluate_pullback_score(X)
        # a rejected spline fit (the case of tests/test_uform.py::test_rejected_fit_disables_uform)
        npz, desc = load_case('c3_sep')
        Xc = case_X('c3_sep', npz)[:500]
        tm = transport_map(X=Xc, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **ctor_kwargs(desc))
        tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
        assert np.all(np.isfinite(tm.evaluate_pullback_score(Xc[:50])))
        monkeypatch.setattr(termtable, 'U_TOL_VALUE', 0.0)          # nothing passes
        tm._refresh_uform()
        with pytest.raises(NotImplementedError, match='rejected'):
            tm.evaluate_pullback_score(Xc[:50])


def test_entry_point_refuses_bad_buffers():
    """ttm_score: TTM_E_ARG for an odd leading dimension, a misaligned pointer and N = 0; the same call with good arguments runs."""
    from tests.hostemu import emu
    with emu.install():
        tm, om, X, E = build('c5_shape', n=401)
        N, D = 400, tm.D
        coef = tm._pack_coeffs()
        Xd = tm._import(X[:N], True)
        G = tm._cols(D + 1, N)
        lib = tm._lib

        def call(g, ldg, n, x=None, ldx=None):
            return lib.ttm_score(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._ptr(Xd) if x is None else x,
                                 Xd.shape[1] if ldx is None else ldx, n, g, ldg, None, None, tm._stream())
        assert call(tm._ptr(G), G.shape[1], N) == 0
        assert call(tm._ptr(G), G.shape[1] - 1, N - 2) == -1        # odd ldg
        assert call(tm._ptr(G, 1), G.shape[1], N) == -1             # G 8 bytes off a 16-byte boundary
        assert call(tm._ptr(G), G.shape[1], N, x=tm._ptr(Xd, 1)) == -1
        assert call(tm._ptr(G), G.shape[1], N, ldx=Xd.shape[1] - 1) == -1
        assert call(tm._ptr(G), G.shape[1], 0) == -1                # N = 0
        assert call(tm._ptr(G), N - 2, N) == -1                     # ldg < N
        assert call(None, G.shape[1], N) == -1
