"""
Examples 02 (partial map) and 04 (Monod kinetics) of the reference against their fixtures (tests/golden/ex02_partial,
ex04_monod; make_golden.py ex02 ex04), on the host test double and on the GPU, and at 10^6 samples on the GPU against the
oracle.  Plus optimize() after the bounds of a separable component were edited (the batched native loops keep their
host vectors with their scratch between calls: the bounds must still be the ones the caller set).

  * Example 04: a separable map of the last two of 22 columns (skip_dimensions = 20: 20 observed rates to condition
    on, of which only the 19th is read); planned banded, a few components, lag 1 behind 20 conditioning columns ->
    k_band_few / k_band_few_inverse.
  * Example 02: the order-10 integrated second spiral component alone (skip_dimensions = 1, 55 monotone + 11
    nonmonotone terms, quadrature order 25), the shipped coefficients; conditional inverse at X_star = 0.6 on every
    row.  It has an X program: the forward map takes k_int_forward_x (reported as k_int_forward); the bisection takes
    k_int_root<bisect>, not k_int_root_x - the X-program root search is opt-in (tuning int_xprog = 2), off by default.
"""
import ctypes

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import check, coeff_lists, load_case, relerr


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


def ex02_X(N=10000):
    from triangular_transport_toolbox_amd import specs
    return specs.sample_spiral(N, seed=0)


def make(name, X=None, with_coeffs=True, prefix=''):
    from triangular_transport_toolbox_amd.transport_map import transport_map
    from tests.util import ctor_kwargs
    npz, desc = load_case(name)
    if X is None:
        X = npz['X'] if 'X' in npz else ex02_X()
    tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **ctor_kwargs(desc))
    if with_coeffs:
        tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D, prefix)
    return tm, npz, desc


def oracle(name, X, npz, desc):
    from oracle.ttm_oracle import OracleMap
    from tests.util import ctor_kwargs
    om = OracleMap(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], **ctor_kwargs(desc))
    om.coeffs_mon, om.coeffs_nonmon = coeff_lists(npz, om.D)
    return om


# ---------------------------------------------------------------------------------------------------------- Example 04

def test_example04_plan(backend):
    tm, _, _ = make('ex04_monod')
    assert tm.D == 2 and tm.skip_dimensions == 20 and tm.X.shape[1] == 22
    # banded, a few components; the conditioning columns in front of the first component keep the planned column cache
    # from covering every group, so the hot records only feed the push records (u_p_lag = 3)
    assert tm._cm.u_enabled and tm._cm.u_p_lag == 3 and tm._cm.u_h_cls == 2


def test_example04_map_objective_inverse(backend, ttm_opt):
    tm, npz, desc = make('ex04_monod')
    X = npz['X']
    if backend == 'hip':                               # (k_band_few at any N: the small-ensemble switch off)
        for name in ('u_loader', 'band_fwd', 'band_inv'):
            ttm_opt(name, 1)
    Z = tm.map(X)
    check('ex04/map', relerr(Z, npz['Z']), 1e-11, backend)
    if backend == 'hip':
        tm.forward_device(tm._Xs, tm._N)
        assert last_kernel(tm) == 'k_band_few'
    for k in range(2):
        A, solve_nonmon = tm.separable_setup(k)
        check('ex04/sep_A', relerr(A, npz['sep_A_%d' % k]), 1e-10, backend)
        for c, J, G in zip(npz['sep_c_%d' % k], npz['sep_J_%d' % k], npz['sep_G_%d' % k]):
            Jg, Gg = tm.separable_objective(c.copy(), A, k)
            check('ex04/sep_J', abs(Jg - J) / (1 + abs(J)), 1e-10, backend)
            check('ex04/sep_gradJ', relerr(Gg, G), 1e-10, backend)
        Jg, Gg = tm.separable_objective(npz['coeffs_mon_%d' % k].copy(), A, k)      # at the reference's optimum
        check('ex04/sep_J_at_optimum', abs(Jg - npz['sep_Jopt_%d' % k]) / (1 + abs(npz['sep_Jopt_%d' % k])), 1e-10, backend)
        check('ex04/sep_gradJ_at_optimum', relerr(Gg, npz['sep_Gopt_%d' % k]), 1e-10, backend)
        check('ex04/sep_c_nonmon', relerr(solve_nonmon(npz['coeffs_mon_%d' % k]), npz['coeffs_nonmon_%d' % k]), 1e-10, backend)
    # conditional inverse: 20-column X_star of varying rows, and the observations repeated on every row (the example)
    Xi = tm.inverse_map(npz['inv_Z'], X_star=npz['inv_Xstar'])
    check('ex04/inverse_varying_xstar', relerr(Xi, npz['inv_X']), 1e-11, backend)
    if backend == 'hip':
        tm.inverse_device(tm._cols(2, tm._N, zero=True), tm._N, X=tm._Xs.clone())
        assert last_kernel(tm) == 'k_band_few_inverse'
    Xo = tm.inverse_map(Z, X_star=np.repeat(npz['obs'][None, :], len(X), axis=0))
    check('ex04/inverse_observed_rates', relerr(Xo, npz['inv_obs_X']), 1e-11, backend)


def test_example04_optimize(backend):
    tm, npz, desc = make('ex04_monod', with_coeffs=False)
    tm.optimize()
    for k in range(2):
        check('ex04/optimize_coeffs_mon', float(np.max(np.abs(tm.coeffs_mon[k] - npz['coeffs_mon_%d' % k]))), 1e-8, backend)
        check('ex04/optimize_coeffs_nonmon', relerr(tm.coeffs_nonmon[k], npz['coeffs_nonmon_%d' % k]), 1e-8, backend)


# ---------------------------------------------------------------------------------------------------------- Example 02

def test_example02_map_objective_inverse(backend):
    X = ex02_X()
    tm, npz, desc = make('ex02_partial', X=X)
    assert tm.D == 1 and tm.skip_dimensions == 1
    assert [len(tm.coeffs_mon[0]), len(tm.coeffs_nonmon[0])] == [55, 11]
    assert int(tm._cm.complex[0]) & 16, 'Example 02 should have an X program'
    Z = tm.map(X)
    check('ex02/map', relerr(Z[:512], npz['Z']), 1e-11, backend)
    assert relerr(Z.mean(0), npz['Z_mean']) < 1e-12 and relerr(Z.std(0), npz['Z_std']) < 1e-12
    if backend == 'hip':
        Zs = tm.forward_device(tm._Xs, tm._N)
        assert last_kernel(tm) == 'k_int_forward'
        tm.inverse_device(Zs, tm._N, table=False)
        assert last_kernel(tm) == 'k_int_root<bisect>'          # (int_xprog = 1: X program for the map only)
    div = len(tm.coeffs_nonmon[0])
    J = tm.objective_function(None, 0, div)
    check('ex02/objective_J', abs(J - npz['J'][0]) / (1 + abs(npz['J'][0])), 1e-10, backend)
    check('ex02/objective_gradJ', relerr(tm.objective_function_jacobian(None, 0, div), npz['G_0']), 1e-10, backend)
    Xi = tm.inverse_map(npz['inv_Z'], X_star=npz['inv_Xstar'])
    check('ex02/inverse_constant_xstar', relerr(Xi, npz['inv_X']), 1e-6, backend)
    Xm = tm.inverse_map(Z[:256], X_star=npz['inv_Xstar'])
    check('ex02/inverse_of_map_constant_xstar', relerr(Xm, npz['inv_map_X']), 1e-6, backend)


def test_example02_optimize(backend):
    """optimize() from the shipped coefficients: the reference's BFGS takes no step there (the gradient is already below
    its gtol), and neither may the product's."""
    X = ex02_X()
    tm, npz, desc = make('ex02_partial', X=X)
    tm.optimize()
    check('ex02/optimize_coeffs_mon', float(np.max(np.abs(tm.coeffs_mon[0] - npz['opt_coeffs_mon_0']))), 1e-8, backend)
    check('ex02/optimize_coeffs_nonmon', float(np.max(np.abs(tm.coeffs_nonmon[0] - npz['opt_coeffs_nonmon_0']))), 1e-8, backend)


# -------------------------------------------------------------------------------------------- edited optimizer bounds

@pytest.mark.parametrize('which', ['lb', 'ub'])
def test_optimize_honours_edited_bounds(backend, which):
    """optimization_constraints_lb / _ub are public (the reference reads them in every optimize(), TM:3102): bounds
    edited between two calls hold in the second, whose batched native loops reuse the scratch of the first."""
    from scipy.optimize import minimize
    X = load_case('ex04_monod')[0]['X']
    tm, npz, desc = make('ex04_monod', X=X, with_coeffs=False)
    assert tm.native_optimizer and tm.optimizer_threads >= 2          # (two components: the batched native loops)
    tm.optimize()
    start_mon = [c.copy() for c in tm.coeffs_mon]
    start_non = [c.copy() for c in tm.coeffs_nonmon]
    m = len(tm.coeffs_mon[0])
    if which == 'lb':
        k, lb, ub = 0, np.full(m, 0.5), np.full(m, np.inf)
        assert np.min(start_mon[0]) < 0.5                       # (the bound cuts into the first optimum)
        tm.optimization_constraints_lb[0] = [0.5] * m
    else:
        k, lb, ub = 1, np.zeros(m), np.full(m, 0.6 * np.max(start_mon[1]))
        tm.optimization_constraints_ub[1] = ub.copy()
    tm.optimize()
    got = [c.copy() for c in tm.coeffs_mon]
    assert np.all(got[k] >= lb - 1e-12) and np.all(got[k] <= ub + 1e-12), (which, got[k])
    # a fresh map, the same bounds from the outset, the same starting point
    fresh, _, _ = make('ex04_monod', X=X, with_coeffs=False)
    fresh.coeffs_mon, fresh.coeffs_nonmon = [c.copy() for c in start_mon], [c.copy() for c in start_non]
    if which == 'lb':
        fresh.optimization_constraints_lb[0] = [0.5] * m
    else:
        fresh.optimization_constraints_ub[1] = ub.copy()
    fresh.optimize()
    for j in range(2):
        assert float(np.max(np.abs(got[j] - fresh.coeffs_mon[j]))) < 1e-10, (which, j, got[j], fresh.coeffs_mon[j])
        assert relerr(tm.coeffs_nonmon[j], fresh.coeffs_nonmon[j]) < 1e-10
    # the oracle: SciPy's L-BFGS-B on the same reduced problem, with the edited bounds
    om = oracle('ex04_monod', X, npz, desc)
    A, aux = om.separable_setup(k)
    opt = minimize(fun=lambda c: om.separable_objective(c, A, k), method='L-BFGS-B', x0=start_mon[k].copy(), jac=True,
                   bounds=[[a, b] for a, b in zip(lb, ub)])
    check('edited_bounds/%s_vs_scipy' % which, float(np.max(np.abs(got[k] - opt.x))), 1e-8, backend)


# ------------------------------------------------------------------------------------------------- full size (GPU)

def subset_with_tails(X, n_random=10000, n_tail=16, seed=3):
    rng = np.random.default_rng(seed)
    idx = set(rng.choice(len(X), size=n_random, replace=False).tolist())
    for j in range(X.shape[1]):
        order = np.argsort(X[:, j])
        idx.update(order[:n_tail].tolist())
        idx.update(order[-n_tail:].tolist())
    return np.array(sorted(idx))


@pytest.mark.gpu
def test_example04_full_size():
    """Example 04 at N = 10^6: rows resampled from the fixture's ensemble with jitter, 1 % pushed 8 sigma out; map,
    conditional inverse with a per-row X_star, and the round trip, against the oracle on >= 10^4 rows with the tails."""
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case('ex04_monod')
    X0 = npz['X']
    rng = np.random.default_rng(2024)
    N = 1000000
    sd = X0.std(0)
    X = X0[rng.integers(0, len(X0), N)] + 0.05 * sd * rng.standard_normal((N, X0.shape[1]))
    far = rng.choice(N, N // 100, replace=False)
    X[far] += 8.0 * sd * rng.choice([-1.0, 1.0], size=(len(far), X0.shape[1]))
    tm, _, _ = make('ex04_monod', X=X)
    om = oracle('ex04_monod', X, npz, desc)           # (the same standardisation as the map: the oracle sees the same X)
    idx = np.union1d(subset_with_tails(X, 10000), far[:500])
    Z = tm.map(X)
    tm.forward_device(tm._Xs, tm._N)
    assert last_kernel(tm) == 'k_band_few'
    err = relerr(Z[idx], om.map(X[idx]))
    check('ex04_full/map(k_band_few)_vs_oracle', err, 5e-11)     # (rows 8 sigma out under order-5 Hermite functions)
    Zin = Z.copy()
    star = X[:, :20]
    Xi = tm.inverse_map(Zin, X_star=star)
    tm.inverse_device(tm._cols(2, tm._N, zero=True), tm._N, X=tm._Xs.clone())
    assert last_kernel(tm) == 'k_band_few_inverse'
    err = relerr(Xi[idx], om.inverse_map(Zin[idx], X_star=star[idx]))
    check('ex04_full/conditional_inverse(k_band_few_inverse)_vs_oracle', err, 1e-9)
    # round trip: the table inverse of the map of X is X to the resolution of the reference's 1001-point table with linear
    # interpolation (TM:3987-4084) in the body of the ensemble
    body = np.setdiff1d(np.arange(N), far)
    check('ex04_full/round_trip', float(np.max(np.abs(Xi[body] - X[body, 20:]) / (1 + np.abs(X[body, 20:])))), 1e-3)


@pytest.mark.gpu
def test_example02_full_size():
    """Example 02 at N = 10^6: the map and the constant-X_star bisection inverse against the oracle on a subset."""
    X = ex02_X(1000000)
    tm, npz, desc = make('ex02_partial', X=X)
    om = oracle('ex02_partial', X, npz, desc)
    idx = subset_with_tails(X, 10000)
    Z = tm.map(X)
    Zs = tm.forward_device(tm._Xs, tm._N)
    assert last_kernel(tm) == 'k_int_forward'
    check('ex02_full/map(k_int_forward)_vs_oracle', relerr(Z[idx], om.map(X[idx])), 1e-11)
    tm.inverse_device(Zs, tm._N, table=False)
    assert last_kernel(tm) == 'k_int_root<bisect>'          # (int_xprog = 1: X program for the map only)
    Xi = tm.inverse_map(Z, X_star=np.full((len(X), 1), 0.6))     # 10^6 bisections at the example's constant X_star
    sub = idx[idx > 0][::5]
    Zq = np.vstack((Z[:1], Z[sub]))                   # (a row 0 of its own keeps the one-sample quirk off the subset)
    Xo = om.inverse_map(Zq, X_star=np.full((len(Zq), 1), 0.6))[1:]
    check('ex02_full/inverse_constant_xstar_vs_oracle', float(np.max(np.abs(Xi[sub] - Xo))), 1e-6)
