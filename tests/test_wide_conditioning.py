"""
Banded separable maps of a few components at the widths and sizes test_random_few.py does not reach, through the forced
few-component kernels (k_band_few / k_band_few_inverse) against the oracle:

  * conditioning blocks wider than the band (skip = 3, 7, 20, 24): the first component reads only the last 1..3 of them;
  * 63..70 columns in all (k_import / k_export move 64-column tiles, blockIdx.y over the tiles), a few components at the end;
  * N = 1, 2, 63, 64, 65, 1023, 1024, 1025 around one band workgroup (BAND_CT = 1024 rows).

Each case checks the map, s, the conditional inverse, the pullback density (skip = 0), and the generic kernels (bands off)
to rounding.  Fixed seeds, a generator of its own.  Plus random integrated maps behind 3..6 conditioning columns (the
monomial-form kernels of csrc/ttm_int.hip against the generic ones, int_dense off).
"""
import ctypes

import numpy as np
import pytest

from tests.util import relerr

pytestmark = pytest.mark.gpu


def _lib():
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    lib.ttm_last_kernel.restype = ctypes.c_char_p
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    return lib


def wide_spec(rng, D, skip):
    """D components behind `skip` conditioning columns; component k reads up to three columns in front of it (lags 1..3,
    so the first component reads the last 1..3 conditioning columns), Hermite functions up to order 5 and plain terms."""
    mon, non = [], []
    for k in range(D):
        kc = k + skip
        nm = [[]]
        for lag in range(1, int(rng.integers(1, 4)) + 1):
            j = kc - lag
            if j < 0:
                continue
            nm.append([j])
            for o in range(2, 6):
                if rng.random() < 0.6:
                    nm.append([j] * o + ['HF'])
        non.append(nm)
        mon.append(['LET %d' % kc] + ['iRBF %d' % kc] * int(rng.integers(0, 4)) + ['RET %d' % kc])
    return mon, non


CASES = [(3, 2, 2049), (7, 3, 2049), (20, 2, 2049), (24, 4, 2049),              # conditioning wider than the band
         (61, 2, 1500), (61, 3, 1500), (62, 3, 1500), (67, 3, 1500),             # d = 63, 64, 65, 70 columns
         (2, 2, 1), (2, 2, 2), (2, 2, 63), (2, 2, 64), (2, 2, 65),               # N around one band workgroup
         (0, 3, 1023), (0, 3, 1024), (0, 3, 1025)]


@pytest.mark.parametrize('skip,D,N', CASES)
def test_wide_conditioning_and_small_n(skip, D, N):
    from oracle.ttm_oracle import OracleMap
    from triangular_transport_toolbox_amd.transport_map import transport_map
    lib = _lib()
    rng = np.random.default_rng(1000 + 97 * skip + 13 * D + N)
    mon, non = wide_spec(rng, D, skip)
    d = D + skip
    Xt = rng.standard_normal((max(N, 64), d)) @ (np.tril(rng.standard_normal((d, d)) * 0.2) + np.eye(d)).T
    Xt += 0.3 * rng.standard_normal(Xt.shape) ** 2
    kw = dict(monotonicity='separable monotonicity')
    # (the special terms are placed on the training ensemble; the maps are then evaluated on N rows)
    tm = transport_map(X=Xt, monotone=mon, nonmonotone=non, verbose=False, **kw)
    om = OracleMap(X=Xt, monotone=mon, nonmonotone=non, **kw)
    for k in range(D):
        cm_ = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
        cn_ = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        tm.coeffs_mon[k], om.coeffs_mon[k] = cm_.copy(), cm_.copy()
        tm.coeffs_nonmon[k], om.coeffs_nonmon[k] = cn_.copy(), cn_.copy()
    assert tm._cm.u_p_lag > 0, 'banded map expected'
    X = Xt[:N].copy()
    try:
        for name in (b'u_loader', b'band_fwd', b'band_inv'):
            lib.ttm_set_option(name, 1)
        Z, Zo = tm.map(X), om.map(X)
        assert relerr(Z, Zo) < 1e-11, ('map', relerr(Z, Zo))
        tm.forward_device(tm._Xs, tm._N)
        assert lib.ttm_last_kernel().decode() == 'k_band_few'
        Xs = (X - om.X_mean) / om.X_std
        for k in range(D):
            assert relerr(tm.s(Xs, k), om.s(Xs, k)) < 1e-11, ('s', k)
        Zin = rng.standard_normal((N, D))
        Zin[: max(1, N // 50)] *= 3.0
        star = X[:, :skip] if skip else None
        Xi, Xo = tm.inverse_map(Zin, X_star=star), om.inverse_map(Zin, X_star=star)
        assert relerr(Xi, Xo) < 1e-9, ('inverse', relerr(Xi, Xo))
        tm.inverse_device(tm._cols(D, tm._N, zero=True), tm._N, X=tm._Xs.clone())
        # (every monotone part here is LET / iRBF / RET with positive coefficients: increasing tables, never the sorted lookup)
        assert lib.ttm_last_kernel().decode() == 'k_band_few_inverse'
        if skip == 0:
            p, po = tm.evaluate_pullback_density(X), om.evaluate_pullback_density(X)
            ok = po > 1e-290
            assert relerr(np.log(p[ok]), np.log(po[ok])) < 1e-9
        lib.ttm_set_option(b'band_fwd', 0)
        lib.ttm_set_option(b'band_inv', 0)
        Zg, Xg = tm.map(X), tm.inverse_map(Zin, X_star=star)
        assert relerr(Z, Zg) < 1e-12 and relerr(Xi, Xg) < 1e-11, ('vs generic', relerr(Z, Zg), relerr(Xi, Xg))
    finally:
        lib.ttm_reset_options()


def integrated_spec(rng, D, skip):
    """D integrated components behind `skip` conditioning columns: Hermite functions of orders 1..4 of up to three columns
    in front (nonmonotone), Hermite functions of x_k and products with the column in front (monotone)."""
    mon, non = [], []
    for k in range(D):
        kc = k + skip
        nm = [[]]
        for lag in range(1, int(rng.integers(1, 4)) + 1):
            nm += [[kc - lag] * o + ['HF'] for o in range(1, 5) if rng.random() < 0.7]
        non.append(nm)
        mon.append([[kc] * o + ['HF'] for o in range(1, 4)] + [[kc - 1, kc, 'HF']])
    return mon, non


@pytest.mark.parametrize('skip,D,seed', [(3, 2, 0), (4, 1, 1), (5, 2, 2), (6, 3, 3)])
def test_random_integrated_map_behind_wide_conditioning(skip, D, seed):
    from oracle.ttm_oracle import OracleMap
    from triangular_transport_toolbox_amd.transport_map import transport_map
    lib = _lib()
    rng = np.random.default_rng(2000 + seed)
    mon, non = integrated_spec(rng, D, skip)
    d = D + skip
    N = 1500
    X = rng.standard_normal((N, d)) @ (np.tril(rng.standard_normal((d, d)) * 0.2) + np.eye(d)).T
    kw = dict(monotonicity='integrated rectifier', quadrature_input={'order': 12})
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw)
    om = OracleMap(X=X, monotone=mon, nonmonotone=non, **kw)
    for k in range(D):
        cm_ = 0.3 * rng.standard_normal(len(tm.coeffs_mon[k]))
        cn_ = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        tm.coeffs_mon[k], om.coeffs_mon[k] = cm_.copy(), cm_.copy()
        tm.coeffs_nonmon[k], om.coeffs_nonmon[k] = cn_.copy(), cn_.copy()
    try:
        Z, Zo = tm.map(X), om.map(X)
        assert relerr(Z, Zo) < 1e-11, ('map', relerr(Z, Zo))
        tm.forward_device(tm._Xs, tm._N)
        assert lib.ttm_last_kernel().decode().startswith('k_int_forward')
        Xs = (X - om.X_mean) / om.X_std
        for k in range(D):
            assert relerr(tm.s(Xs, k), om.s(Xs, k)) < 1e-11, ('s', k)
        Zin = rng.standard_normal((300, D))
        star = X[:300, :skip]
        Xi, Xo = tm.inverse_map(Zin, X_star=star), om.inverse_map(Zin, X_star=star)
        assert np.max(np.abs(Xi[1:] - Xo[1:])) < 1e-6, ('inverse', np.max(np.abs(Xi[1:] - Xo[1:])))
        lib.ttm_set_option(b'int_dense', 0)                     # the generic kernels: the same numbers to rounding
        Zg, Xg = tm.map(X), tm.inverse_map(Zin, X_star=star)
        assert relerr(Z, Zg) < 1e-12 and np.max(np.abs(Xi[1:] - Xg[1:])) < 1e-6, ('vs generic', relerr(Z, Zg))
    finally:
        lib.ttm_reset_options()
