"""
The whole table of the few-component band kernels (csrc/ttm_band.hip: k_band_few, k_band_few_inverse, k_band_few_roundtrip,
k_band_few_newton): every degree class (highest Hermite-function order 3, 5, 7, 10 -> classes 1..4) x every (groups per push
record, reach of the sweep) pair the kernels exist for x with / without plain polynomial nonmonotone terms x with / without the
density terms, for maps of D = 2 and D = 4 components at n = 5003 (two full tiles of 2048 rows, a partial one, an odd tail).
The host side picks one instantiation per launch from these run-time values; a dropped or swapped branch there shows here as a
wrong result or a wrong kernel name.

Builders and tolerances are those of tests/test_band.py (forward 1e-11, density terms 1e-10 / 1e-11, table inverse 1e-11, fused
round trip: the bits of the separate calls) and tests/test_band_newton.py (round trip of the ensemble 1e-7).
"""
import numpy as np
import pytest

from tests.test_band import _banded_with_conditioning
from tests.test_uform import _synthetic_separable
from tests.util import relerr

HF_ORDER = {1: 3, 2: 5, 3: 7, 4: 10}                # highest Hermite-function order of a degree class

# (groups per push record, reach) -> D -> (band width, conditioning columns in front).  Records of two groups: an all-hit map
# without conditioning columns; conditioning columns or a group three columns back make it records of three groups, a group
# further back records of five (termtable._compile_uform).
# (2, 2) - records of two groups, a sweep that reaches two columns back - is not planned for a map of two or four components:
# D = 2 without conditioning columns has one column to read (reach 1); D = 4 with band 2 misses the planned column cache and
# gets records of three groups, as any map with conditioning columns does (NOT_PLANNED, asserted below).  Sweeps of a few
# components inside a LONG band-2 map reach that branch: tests/test_band.py and tests/test_band_linear.py (tm.s, _forward_from).
REACH = {
    (2, 1): {2: (1, 0), 4: (1, 0)},
    (3, 1): {2: (1, 1), 4: (1, 1)},
    (3, 2): {2: (2, 1), 4: (2, 1)},
    (3, 3): {2: (3, 2), 4: (3, 0)},
    (5, 5): {2: (5, 4), 4: (5, 2)},
}
COMBOS = [(cls, lag, reach, D, plain) for cls in sorted(HF_ORDER) for (lag, reach) in sorted(REACH) for D in sorted(REACH[(lag, reach)])
          for plain in (False, True)]
NOT_PLANNED = {(2, 2): (4, 2, 0)}                   # D, band, conditioning columns: planned as (3, 2)
IDS = ['cls%d-lag%d-reach%d-D%d-%s' % (c, lg, r, D, 'plain' if pl else 'hf') for c, lg, r, D, pl in COMBOS]


def _spec(cls, lag, reach, D, plain):
    band, skip = REACH[(lag, reach)][D]
    if cls == 1 and plain and skip:
        return _banded_with_conditioning(D, skip, band=band), skip
    mon, non = _synthetic_separable(D + skip, band, HF_ORDER[cls], 1 if plain else 0, 2)
    return (mon[skip:], non[skip:]), skip           # (the components behind `skip` conditioning columns)


def _build(cls, lag, reach, D, plain, n=5003):
    """tests/test_band.py::_build for a map of the table: the same ensemble, the same coefficients."""
    from triangular_transport_toolbox_amd.transport_map import transport_map
    from oracle.ttm_oracle import OracleMap
    (mon, non), skip = _spec(cls, lag, reach, D, plain)
    d = D + skip
    rng = np.random.default_rng(17 * D)
    X = rng.standard_normal((n, d)) @ (np.tril(rng.standard_normal((d, d)) * 0.4) + np.eye(d)).T + 0.3 * rng.standard_normal((n, d)) ** 2
    kw = dict(monotonicity='separable monotonicity')
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw)
    om = OracleMap(X=X, monotone=mon, nonmonotone=non, **kw)
    for k in range(D):
        cm_ = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
        cn_ = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        tm.coeffs_mon[k], om.coeffs_mon[k] = cm_.copy(), cm_.copy()
        tm.coeffs_nonmon[k], om.coeffs_nonmon[k] = cn_.copy(), cn_.copy()
    return tm, om, X, rng, skip


def _reach_and_plain(cm):
    """What the host side of the band kernels derives from the program: how far back the groups reach, any plain terms."""
    from triangular_transport_toolbox_amd import termtable
    uc = np.asarray(cm.ucomp[:cm.D * termtable.UC_LEN]).reshape(-1, termtable.UC_LEN)
    ug = np.asarray(cm.ugrp).reshape(-1, termtable.UG_LEN)
    reach, plain = 1, False
    for k in range(cm.D):
        for g in range(int(uc[k, 2])):
            G = ug[int(uc[k, 3]) + g]
            reach = max(reach, int(uc[k, 0]) - int(G[0]))
            plain = plain or bool(int(G[1]) & termtable.UGF_POLY)
    return reach, plain


def _planned(tm, cls, lag, reach, plain):
    cm = tm._cm
    assert cm.u_enabled and cm.u_h_cls == cls and cm.u_p_lag == lag, (cm.u_enabled, cm.u_h_cls, cm.u_p_lag)
    assert _reach_and_plain(cm) == (reach, plain)


def test_the_table_is_whole_and_every_combination_is_planned_as_its_name_says():
    """Host side: 4 classes x the (record, reach) pairs x plain / not, both D; every listed map gets the degree class, the
    record shape, the reach and the plain-term flag of its name - and the pair left out is planned as (3, 2)."""
    from tests.hostemu import emu
    assert sorted(list(REACH) + list(NOT_PLANNED)) == [(2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (5, 5)]
    assert all(sorted(REACH[r]) == [2, 4] for r in REACH) and len(COMBOS) == 4 * 5 * 2 * 2
    with emu.install():
        for cls, lag, reach, D, plain in COMBOS:
            _planned(_build(cls, lag, reach, D, plain, n=300)[0], cls, lag, reach, plain)
        for (lag, reach), (D, band, skip) in NOT_PLANNED.items():
            REACH[(lag, reach)] = {D: (band, skip)}
            try:
                for cls in HF_ORDER:
                    for plain in (False, True):
                        _planned(_build(cls, lag, reach, D, plain, n=300)[0], cls, 3, reach, plain)
            finally:
                del REACH[(lag, reach)]


@pytest.mark.gpu
@pytest.mark.parametrize('cls,lag,reach,D,plain', COMBOS, ids=IDS)
def test_few_component_kernels_over_the_whole_table(cls, lag, reach, D, plain, ttm_opt):
    import torch
    from tests.test_band_newton import _newton
    from tests.test_full_size import _last_kernel
    tm, om, X, rng, E = _build(cls, lag, reach, D, plain)
    _planned(tm, cls, lag, reach, plain)
    d, N, Xs = D + E, tm._N, tm._Xs
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1); ttm_opt('band_inv', 1)
    # ---- forward ----
    Zo = om.map(X)
    Z = tm.forward_device(Xs, N)
    assert _last_kernel(tm) == 'k_band_few'
    err = relerr(Z[:, :N].T.cpu().numpy(), Zo)
    print('forward', err)
    assert err < 1e-11
    assert relerr(tm.map(X), Zo) < 1e-11
    # ---- forward + log-determinant + sum of squares ----
    sigma = tm._to_dev(np.asarray(tm.X_std[E:E + D], dtype=float))
    ld, ss = tm._zeros(N), tm._zeros(N)
    Zd = tm.forward_device(Xs, N, logdet=ld, sigma=sigma, sumsq=ss)
    assert _last_kernel(tm) == 'k_band_few<density>'
    assert torch.equal(Zd[:, :N], Z[:, :N])
    with np.errstate(all='ignore'):
        ldo = om._log_determinant((X - om.X_mean) / om.X_std, skip_in_std=True)
    ok = np.isfinite(ldo)
    ldg, ssg = ld.cpu().numpy(), ss.cpu().numpy()
    print('logdet', relerr(ldg[ok], ldo[ok]), 'sumsq', relerr(ssg, np.sum(Zo ** 2, axis=1)), 'finite', ok.mean())
    assert ok.mean() > 0.9 and np.array_equal(np.isfinite(ldg), ok)
    assert relerr(ldg[ok], ldo[ok]) < 1e-10 and relerr(ssg, np.sum(Zo ** 2, axis=1)) < 1e-11
    # ---- Newton: the round trip of the ensemble (first: on a coefficient vector that has no tables yet) ----
    Xn, iters, name = _newton(tm, Z, N, Xs[:E] if E else None)
    assert name == 'k_band_few_newton'
    rt = float((Xn[:, :N] - Xs[:, :N]).abs().max().item())
    print('newton round trip', rt, 'trial points', iters.tolist())
    assert rt < 1e-7
    # ---- table inverse ----
    Zin = rng.standard_normal((N, D))
    Zin[:40] *= 3.5                                         # (targets beyond the resident window and beyond the tables)
    Xstar = X[:, :E] if E else None
    Xo = om.inverse_map(Zin, X_star=Xstar)
    Xi = tm.inverse_map(Zin, X_star=Xstar)
    print('table inverse', relerr(Xi, Xo))
    assert relerr(Xi, Xo) < 1e-11
    tm.inverse_device(tm._cols(D, N, zero=True), N)
    assert _last_kernel(tm) == 'k_band_few_inverse'
    # ---- forward + table inverse in one launch: the bits of the separate calls ----
    ttm_opt('roundtrip_fused', 1)                           # (every shape through the fused kernel)

    def same(a, b):
        return np.array_equal(a[:, :N].cpu().numpy(), b[:, :N].cpu().numpy(), equal_nan=True)
    for dens in (False, True):
        l1, s1 = (tm._zeros(N), tm._zeros(N)) if dens else (None, None)
        Z1 = tm.forward_device(Xs, N, logdet=l1, sigma=sigma if dens else None, sumsq=s1)
        X1 = tm._cols(d, N, zero=True)
        if E:
            X1[:E, :N].copy_(Xs[:E, :N])
        tm.inverse_device(Z1, N, X=X1)
        assert _last_kernel(tm) == 'k_band_few_inverse'
        l2, s2 = (tm._zeros(N), tm._zeros(N)) if dens else (None, None)
        Z2, X2 = tm.roundtrip_device(Xs, N, logdet=l2, sigma=sigma if dens else None, sumsq=s2)
        assert _last_kernel(tm) == ('k_band_few_roundtrip<density>' if dens else 'k_band_few_roundtrip')
        assert same(Z1, Z2) and same(X1, X2), dens
        if dens:
            assert np.array_equal(l1.cpu().numpy(), l2.cpu().numpy(), equal_nan=True)
            assert np.array_equal(s1.cpu().numpy(), s2.cpu().numpy(), equal_nan=True)
