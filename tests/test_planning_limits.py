"""
Both sides of the planning limits that switch a component to another code path, against the oracle:

  * HOSTCOEF_MAX = 128 (transport_map.py): up to 128 coefficients of a component travel as kernel arguments (the host-driven
    objective, the native BFGS loop); 129 take the device-coefficient objective and SciPy's loop;
  * P_LAG_MAX = 5 with P_FEW_D = 4 (termtable.py): a map of at most four components is banded with groups up to five
    columns back (u_p_lag = 5), not six; at lag 3 with four components (u_p_lag = 3), not five;
  * X_NU_MAX = 40 and X_SUM_MAX = 192 (termtable.py): an integrated component has an X program (its forward map and its
    objective / gradient sums on the X-program kernels) with 40 distinct factors and 192 sums, not with 41 or 193.

Map, inverse and (integrated maps) the objective and its gradient on either side; the plan flag that names the path is
asserted, and on the GPU the kernel.
"""
import ctypes
import itertools

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import check, relerr


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


def samples(N, d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, d)) @ (np.tril(rng.standard_normal((d, d)) * 0.3) + np.eye(d)).T + \
        0.2 * rng.standard_normal((N, d)) ** 2


def pair(X, mon, non, seed, **kw):
    from oracle.ttm_oracle import OracleMap
    from triangular_transport_toolbox_amd.transport_map import transport_map
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw)
    om = OracleMap(X=X, monotone=mon, nonmonotone=non, **kw)
    rng = np.random.default_rng(seed)
    for k in range(tm.D):
        cm_ = (0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))) / np.sqrt(len(tm.coeffs_mon[k]))
        cn_ = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        tm.coeffs_mon[k], om.coeffs_mon[k] = cm_.copy(), cm_.copy()
        tm.coeffs_nonmon[k], om.coeffs_nonmon[k] = cn_.copy(), cn_.copy()
    return tm, om


# ------------------------------------------------------------------------------------------------ HOSTCOEF_MAX = 128

def integrated_spec(n_coef):
    """One integrated component of x_2 behind two conditioning columns with exactly n_coef coefficients: Hermite-function
    monomials of total order up to 8 that contain x_2 (monotone), a constant and Hermite functions of x_0, x_1 (nonmonotone)."""
    non = [[]] + [[j] * o + ['HF'] for j in (0, 1) for o in range(1, 5)]
    mon = []
    for order in range(1, 9):
        for entry in itertools.combinations_with_replacement(range(3), order):
            if 2 in entry:
                mon.append([int(e) for e in entry] + ['HF'])
    mon = mon[:n_coef - len(non)]
    assert len(mon) + len(non) == n_coef
    return [mon], [non]


@pytest.mark.parametrize('n_coef', [128, 129])
def test_coefficients_as_kernel_arguments(backend, n_coef):
    from triangular_transport_toolbox_amd import transport_map as tmod
    assert tmod.HOSTCOEF_MAX == 128
    mon, non = integrated_spec(n_coef)
    X = samples(400, 3, 7)
    kw = dict(monotonicity='integrated rectifier', quadrature_input={'order': 12})
    tm, om = pair(X, mon, non, 11, **kw)
    div = len(tm.coeffs_nonmon[0])
    c = np.concatenate((tm.coeffs_nonmon[0], tm.coeffs_mon[0]))
    assert len(c) == n_coef
    # the path: coefficients as kernel arguments (ttm_objective_host) at 128, through device memory (ttm_objective) at 129
    assert tm._coefficients_as_arguments(n_coef) == (n_coef <= tmod.HOSTCOEF_MAX)
    tm.coeffs_nonmon[0], tm.coeffs_mon[0] = c[:div].copy(), c[div:].copy()
    Z = tm.map(X)
    check('limits/hostcoef%d/map' % n_coef, relerr(Z, om.map(X)), 1e-11, backend)
    for v in (c, 0.5 * c + 0.01):
        J, Jo = tm.objective_function(v.copy(), 0, div), om.objective_function(v.copy(), 0, div)
        check('limits/hostcoef%d/J' % n_coef, abs(J - Jo) / (1 + abs(Jo)), 1e-10, backend)
        G, Go = tm.objective_function_jacobian(v.copy(), 0, div), om.objective_function_jacobian(v.copy(), 0, div)
        check('limits/hostcoef%d/gradJ' % n_coef, relerr(G, Go), 1e-9, backend)
    Zin = np.random.default_rng(3).standard_normal((200, 1))
    star = X[:200, :2]
    check('limits/hostcoef%d/inverse' % n_coef,
          float(np.max(np.abs(tm.inverse_map(Zin, X_star=star) - om.inverse_map(Zin, X_star=star)))), 1e-6, backend)


@pytest.mark.parametrize('n_coef', [128, 129])
def test_optimize_across_the_native_loop_gate(backend, n_coef):
    """optimize() at 128 coefficients (the library's BFGS loop) and 129 (SciPy's BFGS over the device objective): either
    ends on a stationary point of the oracle's objective (BFGS's gtol of 1e-5 on the gradient) below where it started."""
    mon, non = integrated_spec(n_coef)
    X = samples(200, 3, 8)
    kw = dict(monotonicity='integrated rectifier', quadrature_input={'order': 6})
    tm, om = pair(X, mon, non, 12, **kw)
    tm.coeffs_mon[0] = np.full(len(tm.coeffs_mon[0]), 0.05)
    tm.coeffs_nonmon[0] = np.zeros(len(tm.coeffs_nonmon[0]))
    div = len(om.coeffs_nonmon[0])
    c0 = np.concatenate((tm.coeffs_nonmon[0], tm.coeffs_mon[0]))
    tm.optimize()
    c = np.concatenate((tm.coeffs_nonmon[0], tm.coeffs_mon[0]))
    assert om.objective_function(c.copy(), 0, div) < om.objective_function(c0.copy(), 0, div)
    g = om.objective_function_jacobian(c.copy(), 0, div)
    check('limits/hostcoef%d/optimize_oracle_gradient_at_result' % n_coef, float(np.max(np.abs(g))), 2e-5, backend)


# ---------------------------------------------------------------------------------------- P_LAG_MAX = 5, P_FEW_D = 4

def banded_spec(D, skip, lag):
    """Separable map of D components behind `skip` conditioning columns; component k reads x_(k-1) and x_(k-lag) (when
    they exist) in a constant, linear and Hermite-function terms, and has LET / iRBF / RET terms of its own variable."""
    mon, non = [], []
    for k in range(D):
        kc = k + skip
        nm = [[]]
        for j in sorted({kc - 1, kc - lag}):
            if j >= 0:
                nm += [[j], [j] * 2 + ['HF'], [j] * 3 + ['HF']]
        non.append(nm)
        mon.append(['LET %d' % kc, 'iRBF %d' % kc, 'RET %d' % kc])
    return mon, non


@pytest.mark.parametrize('D,skip,lag,p_lag', [(2, 5, 5, 5), (2, 5, 6, 0), (4, 0, 3, 3), (5, 0, 3, 0)])
def test_band_lag_and_component_limits(backend, ttm_opt, D, skip, lag, p_lag):
    mon, non = banded_spec(D, skip, lag)
    d = D + skip
    X = samples(3000, d, 20 + 10 * D + lag)
    kw = dict(monotonicity='separable monotonicity')
    tm, om = pair(X, mon, non, 5, **kw)
    assert int(tm._cm.u_p_lag) == p_lag, (D, lag, int(tm._cm.u_p_lag))
    if backend == 'hip':
        for name in ('u_loader', 'band_fwd', 'band_inv'):
            ttm_opt(name, 1)
    Z = tm.map(X)
    check('limits/band_D%d_lag%d/map' % (D, lag), relerr(Z, om.map(X)), 1e-11, backend)
    if backend == 'hip':
        tm.forward_device(tm._Xs, tm._N)
        assert (last_kernel(tm) == 'k_band_few') == (p_lag > 0), last_kernel(tm)
    Zin = np.random.default_rng(4).standard_normal((500, D))
    star = X[:500, :skip] if skip else None
    Xi, Xo = tm.inverse_map(Zin, X_star=star), om.inverse_map(Zin, X_star=star)
    check('limits/band_D%d_lag%d/inverse' % (D, lag), relerr(Xi, Xo), 1e-9, backend)
    if backend == 'hip' and p_lag > 0:
        tm.inverse_device(tm._cols(D, tm._N, zero=True), tm._N, X=tm._Xs.clone())
        assert last_kernel(tm) == 'k_band_few_inverse'


# ------------------------------------------------------------------------------------ X_NU_MAX = 40, X_SUM_MAX = 192

def xprog_factors_spec(past):
    """Integrated component of x_4: Hermite functions of orders 1..10 of x_0 .. x_3 (nonmonotone) and of x_4 (monotone) -
    40 distinct factors; `past` adds the monotone term x_0 x_4 (a plain x_0: factor 41)."""
    non = [[]] + [[j] * o + ['HF'] for j in range(4) for o in range(1, 11)]
    mon = [[4] * o + ['HF'] for o in range(1, 11)] + ([[0, 4]] if past else [])
    return [mon], [non], 5


def xprog_sums_spec(past):
    """Integrated component of x_2 with 1 + 10 nonmonotone + 24 monotone products x 7 quadrature columns = 192 X-program
    sums; `past` adds the nonmonotone Hermite function of x_1 (sum 193)."""
    non = [[]] + [[0] * o + ['HF'] for o in range(1, 11)] + ([[1, 'HF']] if past else [])
    mon = [[2] * o + ['HF'] for o in range(1, 11)] + [[0] * p + [2, 'HF'] for p in range(1, 11)] + \
        [[1] * p + [2, 'HF'] for p in range(1, 5)]
    return [mon], [non], 3


@pytest.mark.parametrize('limit,past', [('X_NU_MAX', False), ('X_NU_MAX', True), ('X_SUM_MAX', False), ('X_SUM_MAX', True)])
def test_x_program_limits(backend, monkeypatch, limit, past):
    from triangular_transport_toolbox_amd import termtable
    from triangular_transport_toolbox_amd.transport_map import transport_map
    assert (termtable.X_NU_MAX, termtable.X_SUM_MAX) == (40, 192)
    mon, non, d = (xprog_factors_spec if limit == 'X_NU_MAX' else xprog_sums_spec)(past)
    X = samples(300, d, 50 + d + past)
    kw = dict(monotonicity='integrated rectifier', quadrature_input={'order': 8})
    tm, om = pair(X, mon, non, 17, **kw)
    assert bool(int(tm._cm.complex[0]) & 16) == (not past), 'X program at the limit, none past it'
    if backend == 'hostemu':
        # the limit is what decides: one lower and the case at the limit loses its X program, one higher and the case
        # past it gets one (planning only - the host test double runs no kernel of such a plan)
        with monkeypatch.context() as mp:
            mp.setattr(termtable, limit, getattr(termtable, limit) + (1 if past else -1))
            probe = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw)
            assert bool(int(probe._cm.complex[0]) & 16) == past
    tag = '%s_%s' % (limit.lower(), 'past' if past else 'at')
    div = len(tm.coeffs_nonmon[0])
    c = np.concatenate((tm.coeffs_nonmon[0], tm.coeffs_mon[0]))
    Z = tm.map(X)
    check('limits/%s/map' % tag, relerr(Z, om.map(X)), 1e-11, backend)
    if backend == 'hip':
        tm._device_sums(0, c)
        assert last_kernel(tm) == ('k_int_objective_walk' if past else 'k_int_objective')
        tm.forward_device(tm._Xs, tm._N)
        assert last_kernel(tm) == FORWARD_KERNEL[(limit, past)]
    for v in (c, 0.5 * c + 0.01):
        J, Jo = tm.objective_function(v.copy(), 0, div), om.objective_function(v.copy(), 0, div)
        check('limits/%s/J' % tag, abs(J - Jo) / (1 + abs(Jo)), 1e-10, backend)
        G, Go = tm.objective_function_jacobian(v.copy(), 0, div), om.objective_function_jacobian(v.copy(), 0, div)
        check('limits/%s/gradJ' % tag, relerr(G, Go), 1e-9, backend)
    Zin = np.random.default_rng(8).standard_normal((200, 1))
    star = X[:200, :d - 1]
    check('limits/%s/inverse' % tag,
          float(np.max(np.abs(tm.inverse_map(Zin, X_star=star) - om.inverse_map(Zin, X_star=star)))), 1e-6, backend)


# the forward map takes the X-program kernel only when its row block fits 64 KB of LDS (csrc/ttm_int.hip): 17 rows at the
# sum limit do, the 43 rows (3 + 40 factors) at the factor limit do not - there the X program serves the objective alone
FORWARD_KERNEL = {('X_NU_MAX', False): 'k_int_forward<walk>', ('X_NU_MAX', True): 'k_int_forward<walk>',
                  ('X_SUM_MAX', False): 'k_int_forward', ('X_SUM_MAX', True): 'k_int_forward<walk>'}
