"""
Score of the pullback density on the device: the push-form kernel of banded maps (k_band_score, csrc/ttm_band.hip) and the
generic kernel (k_score_u, csrc/ttm_kernels.hip) against the finite-difference truth of tests/test_score.py, against each other,
and for the properties every sample kernel here is held to - the same bits whatever the chunking, the ensemble size and the
padding; a row's result owned by that row alone.  N = 5003 (odd, several workgroups under the tests' settings) unless said.
"""
import ctypes

import numpy as np
import pytest

from tests import test_score as ts
from tests.util import relerr

N = 5003
SETTINGS = ((-1, -1), (1, -1), (3, 2), (2, 1))      # (band_cus, rt_block) of tests/test_band.py: one tile per chunk | several tiles | several blocks

pytestmark = pytest.mark.gpu


def _last(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


def _raw_args(tm, E):
    """g_scale and ld_affine of evaluate_pullback_score, on the device."""
    D = tm.D
    std = np.asarray(tm.X_std, dtype=float)[E:E + D]
    mean = np.asarray(tm.X_mean, dtype=float)[E:E + D]
    return tm._to_dev(np.ascontiguousarray(1.0 / std)), tm._to_dev(np.ascontiguousarray(np.column_stack((std, mean))))


def _score(tm, Xd, n, gs, af, G=None):
    """ttm_score on a standardised device matrix -> (n x D host array, name of the kernel that ran)."""
    G = tm.score_device(Xd, n, g_scale=gs, ld_affine=af, G=G)
    name = _last(tm)
    return G[:, :n].cpu().numpy().T.copy(), name


@pytest.mark.parametrize('name', ts.ALL_CASES)
def test_score_kernels_against_finite_differences_and_against_each_other(name, ttm_opt):
    tm, om, X, E = ts.build(name, n=N)
    banded = name != ts.DENSE
    assert (tm._cm.u_p_lag > 0) == banded
    own, star = ts.own_and_star(X, E)
    gs, af = _raw_args(tm, E)
    Xd = tm._import(X, True)
    # the generic kernel: what the push-form kernel replaces for banded maps, all there is for the others
    ttm_opt('band_score', 0)
    Gu, kern = _score(tm, Xd, N, gs, af)
    assert kern == 'k_score_u'
    ts.check_against_truth(name, tm.evaluate_pullback_score(own, X_star=star), om, X, E, 'k_score_u')
    first = None
    for cus, block in SETTINGS:
        ttm_opt('band_score', -1); ttm_opt('band_cus', cus); ttm_opt('rt_block', block)
        Gb, kern = _score(tm, Xd, N, gs, af)
        assert kern == ('k_band_score' if banded else 'k_score_u'), (cus, block)
        G = tm.evaluate_pullback_score(own, X_star=star)
        assert np.array_equal(G, Gb)                          # (the method is the one launch, exported)
        ts.check_against_truth(name, G, om, X, E, 'cus %d block %d' % (cus, block))
        # same polynomials, another order: the bound k_band_forward is held to against the kernels it replaces, on all rows
        err = relerr(Gb, Gu)
        print('%s cus %d block %d: push form against generic %.3e' % (name, cus, block, err))
        assert err < 1e-11, (cus, block, err)
        # the bits do not depend on how the rows are cut into chunks and tiles or the components into blocks
        first = Gb if first is None else first
        assert np.array_equal(Gb, first), (cus, block)
    # the plain score in standardised coordinates takes the same kernels
    ttm_opt('band_cus', -1); ttm_opt('rt_block', -1)
    Gp, kern = _score(tm, Xd, N, None, None)
    assert kern == ('k_band_score' if banded else 'k_score_u')
    ttm_opt('band_score', 0)
    Gpu, kern = _score(tm, Xd, N, None, None)
    assert kern == 'k_score_u'
    # (class_55 is left to the raw-coordinate comparison above: its random coefficients make some components non-monotone, m'
    # changes sign and m'' / m' has poles - next to one, two summation orders differ by any amount, and among 5003 rows of
    # this second set of evaluation points some lie next to one)
    if name != 'class_55':
        assert relerr(Gp, Gpu) < 1e-11


@pytest.mark.parametrize('name', ['c5_shape', 'few_ents'])
def test_small_ensembles_repeats_and_padding_give_the_same_bits(name, ttm_opt):
    import torch
    tm, om, X, E = ts.build(name, n=N)
    gs, af = _raw_args(tm, E)
    d, D = tm._cm.d_cols, tm.D
    Xd = tm._import(X, True)
    G0, kern = _score(tm, Xd, N, gs, af)
    assert kern == 'k_band_score' and np.all(np.isfinite(G0))
    # the same call again
    assert np.array_equal(_score(tm, Xd, N, gs, af)[0], G0)
    # the first n rows as an ensemble of their own
    for n in (1, 2, 63, 513):
        Xn = tm._cols(d, n, zero=True)
        Xn[:, :n] = Xd[:, :n]
        Gn, kern = _score(tm, Xn, n, gs, af)
        assert kern == 'k_band_score' and np.array_equal(Gn, G0[:n]), n
    # padded leading dimensions (even: the matrices are read and written two rows at a time), padding rows of X poisoned, of G
    # pre-filled: rows [0, N) as before, the padding of G beyond N rounded up to even untouched
    ld = N + 1 + 6
    Xp = torch.full((d, ld), float('nan'), dtype=torch.float64, device=Xd.device)
    Xp[:, :N] = Xd[:, :N]
    Gp = torch.full((D, ld), -7.25, dtype=torch.float64, device=Xd.device)
    for band_score in (-1, 0):                                # each kernel against its own unpadded call, bit for bit
        ttm_opt('band_score', band_score)
        want, kern = _score(tm, Xd, N, gs, af)
        assert kern == ('k_score_u' if band_score == 0 else 'k_band_score')
        Gp.fill_(-7.25)
        got, kern = _score(tm, Xp, N, gs, af, G=Gp)
        assert kern == ('k_score_u' if band_score == 0 else 'k_band_score')
        assert np.all(Gp[:, N + 1:].cpu().numpy() == -7.25)
        assert np.array_equal(got, want)


def _tail_truth(om, x_row, E):
    """Score of one sample far in a tail, by the differences of tests/test_score.py (same steps, same double extrapolation) taken
    of the oracle's own pieces instead of the logarithm of their product: the density underflows there, and log p itself is
    ~1e12, so its differences with steps of 1e-3 keep two digits.  With dS_k/dx_j and d(log det)/dx_j from the differences,
    d log p / dx_j = -sum_k S_k dS_k/dx_j + d(log det)/dx_j: a component that does not read column j contributes an exact zero,
    the others lose the digits of S_k ~ 1e6 only (1e-7).  -> (r2 [D], e_FD of the row: the differences' own error, carried through
    the same formula)"""
    D = om.D
    S0 = om.map(x_row[None, :])[0]
    r2, err = np.zeros(D), np.zeros(D)
    for k in range(D):
        c = E + k

        def at(col):
            Xp = np.repeat(x_row[None, :], len(col), axis=0)
            Xp[:, c] = col
            return Xp
        h = 1e-3 * float(om.X_std[c])
        x0 = np.array([x_row[c]])
        v, dlt = np.zeros(D + 1), np.zeros(D + 1)
        for i in range(D):
            a, b, fin = ts.richardson(lambda col, i=i: om.map(at(col))[:, i], x0, h)
            assert fin[0]
            v[i], dlt[i] = a[0], b[0]
        a, b, fin = ts.richardson(lambda col: om._log_determinant(at(col), skip_in_std=False), x0, h)
        assert fin[0]
        v[D], dlt[D] = a[0], b[0]
        r2[k] = -np.dot(S0, v[:D]) + v[D]
        err[k] = (np.dot(np.abs(S0), dlt[:D]) + dlt[D]) / (1.0 + abs(r2[k]))
    return r2, float(err.max())


@pytest.mark.parametrize('name', ['c5_shape', ts.LONG_OWN])
def test_a_row_is_owned_by_its_sample_alone(name, ttm_opt):
    """NaN, +inf and a value far beyond every spline's support (the tail column is exactly linear: m'' = 0) in one own column of
    three rows: no other row changes; the score of the column itself is NaN for the first two (so is every score that depends on
    the sample); the third row equals the finite-difference truth of the tail, held at 8 (e_FD + e_spl) with the row's own e_FD.
    (The truth of that row: _tail_truth - the same differences, of the oracle's map and log-determinant; its e_FD is ~1e-7.)"""
    tm, om, X, E = ts.build(name, n=N)
    gs, af = _raw_args(tm, E)
    c = 1
    rows = (7, 2049, 4100)                                   # (first tile, a chunk boundary of the tests' settings, the last chunk)
    Xb = X.copy()
    Xb[rows[0], E + c] = np.nan
    Xb[rows[1], E + c] = np.inf
    Xb[rows[2], E + c] = 1e6
    truth, e_fd = _tail_truth(om, Xb[rows[2]], E)
    tol = 8.0 * (e_fd + ts.E_SPL[name])
    Xd, Xbd = tm._import(X, True), tm._import(Xb, True)
    others = np.ones(N, dtype=bool)
    others[list(rows)] = False
    for band_score, cus, block in ((0, -1, -1), (-1, -1, -1), (-1, 3, 2)):
        ttm_opt('band_score', band_score); ttm_opt('band_cus', cus); ttm_opt('rt_block', block)
        G0, kern = _score(tm, Xd, N, gs, af)
        Gb, _ = _score(tm, Xbd, N, gs, af)
        assert kern == ('k_score_u' if band_score == 0 else 'k_band_score')
        assert np.array_equal(Gb[others], G0[others])
        assert np.isnan(Gb[rows[0], c]) and np.isnan(Gb[rows[1], c])
        assert np.all(np.isfinite(Gb[rows[2]]))
        err = ts.metric(Gb[rows[2]], truth)
        print('%s %s: tail row error %.3e, e_FD %.3e, tolerance %.3e' % (name, kern, err, e_fd, tol))
        assert err <= tol
