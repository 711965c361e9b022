"""
A gradient pulled through the map: ttm_pull_gradient / k_pull_gradient_u / u_pull_row (include/ttm.h, csrc/ttm_pull.h) and
transport_map.pull_gradient_device / pull_gradient, on the host test double and on the GPU.

Truth (tests/pull_truth.py, from the oracle alone).  J_ref[j, i] = dS_j / dx_c(i): central differences of OracleMap.map in every
own column with the steps h, h/2, h/4, h = 1e-3 x the column's deviation, extrapolated twice; e_FD = max |r1 - r2| / (1 + |r2|);
rows are kept when the stencil is finite and e_FD <= 1e-9.  All 200 rows are kept in all cases (e_FD 8e-13 .. 3.9e-12), so the
condition is kept == 200 everywhere (class_55 has negative diagonal entries; the metric does not mind).

Metric.  A BACKWARD error, so the conditioning of J does not enter.  With seeded standard-normal raw gradients G, g_scale = sigma
and logdet = 0 the call returns W with J_x^T W = G, J_x the Jacobian in raw coordinates, and
    eta = max_i |sum_j Jref_ji W_j - G_i| / ( |G_i| + sum_j (1 + |Jref_ji|) |W_j| ).
An error dJ of an entry of the Jacobian moves the numerator by |dJ| |W_j| and is measured as |dJ| / (1 + |Jref|) by the
denominator: that is the metric of e_FD (the yardstick's entries) and of e_slope (the resident splines' first derivative against
the oracle's derivative basis, the only part of J the U section approximates; E_SLOPE below).  Tolerance 8 x (e_FD + e_slope);
the factor 8 is that of tests/test_score.py (maxima over samples, not suprema; another order of summation).
With logdet = 1 the right-hand side is G - l_ref, l_ref = m'' / m' / sigma at the STANDARDISED sample (m' from the oracle's
derivative basis, m'' by its Richardson differences; a row is kept when its own estimate is <= 1e-9, which keeps all 200 rows
in every case, class_55 included - its cap stays at 130 as in tests/test_score.py); the denominator gains 1 + |l_ref_i|, the
metric of e_spl (the splines' quotient m'' / m', E_SPL_STD below: measured as E_SPL of tests/test_score.py was, at the
standardised sample) and of the differences' own estimate e_l, and the tolerance is 8 x (e_FD + e_slope + e_spl + e_l).

E_SLOPE / E_SPL_STD: measured once on the CPU by tools/pull_spline_error.py from the numbers of the U section, evaluated in NumPy
(tests/pull_truth.py: u_section_slopes), never by the routine under test.

Comparisons between two calls of one backend are bitwise.  Every figure is printed before it is held.
"""
import ctypes

import numpy as np
import pytest

from tests import pull_truth as pt
from tests import test_score as ts
from tests.test_mcmc import backend, same_bits                     # noqa: F401  (the backend fixture: hostemu, and hip marked gpu)

ROWS = pt.ROWS
SENTINEL = -7.25e300
E_ARG, E_UNSUPPORTED = -1, -4

# (e_slope, e_spl at the standardised sample) per case - tools/pull_spline_error.py
E_SLOPE = {
    'c5_shape': (8.9e-13, 3.4e-10), 'class_55': (6.8e-12, 5.6e-09), 'class_77': (5.2e-13, 4.3e-10), 'few_c2b': (3.4e-13, 2.3e-10),
    'few_c3': (4.9e-13, 2.0e-10), 'few_cond': (8.2e-13, 4.2e-10), 'few_cond2': (6.5e-13, 3.6e-10), 'few_entf': (8.2e-13, 3.6e-10),
    'few_ents': (0.0, 0.0),      # (linear monotone parts, no spline anywhere)
    'few_ex05': (6.7e-13, 2.2e-10), 'lag_one': (7.2e-13, 3.5e-10), 'long_own': (1.1e-12, 6.4e-10), 'dense_5': (4.4e-13, 4.1e-10),
    pt.STD: (5.8e-13, 2.4e-10),
}

_MAPS = {}


def case(name, backend):
    """(tm, om, X, E) of a case, built once per backend."""
    key = (name, backend)
    if key not in _MAPS:
        _MAPS[key] = pt.build(name)
    return _MAPS[key]


def gradients(name, D):
    return np.random.default_rng(sum(map(ord, name))).standard_normal((ROWS, D))


def sigma_of(tm, E, k0=0):
    return np.asarray(tm.X_std, dtype=float)[E + k0:E + tm.D]


def eta(J, W, rhs, G, extra=None):
    """The backward error of the rows: J [n, j, i], W, rhs, G [n, i]; extra: what the denominator gains."""
    res = np.abs(np.einsum('nji,nj->ni', J, W) - rhs)
    den = np.abs(G) + np.einsum('nji,nj->ni', 1.0 + np.abs(J), np.abs(W))
    if extra is not None:
        den = den + extra
    return float(np.max(res / den))


def pull_host(tm, X, G, E, k0=0, logdet=False, g_scale=True):
    """pull_gradient_device on host arrays: X the raw rows (all columns), G rows x (D - k0) -> W rows x (D - k0)."""
    N = X.shape[0]
    Xd = tm._import(X, True)
    Gd = tm._import(G, False)
    gs = tm._to_dev(sigma_of(tm, E, k0)) if g_scale else None
    W = tm.pull_gradient_device(Xd, N, Gd, k0=k0, g_scale=gs, logdet=logdet)
    assert tuple(W.shape) == (tm.D - k0, N + (N & 1))
    if tm._dev.type == 'cuda':
        assert last_kernel(tm) == 'k_pull_gradient_u'
    return tm._export(W, N, 0, tm.D - k0, False)


def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


# ------------------------------------------------------------------------------------------ against the oracle

@pytest.mark.parametrize('name', ts.ALL_CASES)
def test_pull_against_the_oracles_jacobian(backend, name):
    tm, om, X, E = case(name, backend)
    D = tm.D
    J, keep, e_fd = pt.jacobian_truth(name, om, X, E)
    e_slope, e_spl = E_SLOPE[name]
    G = gradients(name, D)
    W = pull_host(tm, X[:ROWS], G, E)
    kept = int(keep.sum())
    tol = 8.0 * (e_fd + e_slope)
    err = eta(J[keep], W[keep], G[keep], G[keep])
    print('%s %s logdet 0: kept %d / %d, e_FD %.3e, e_slope %.1e, tolerance %.3e, eta %.3e' % (backend, name, kept, ROWS, e_fd, e_slope, tol, err))
    assert kept == ROWS
    assert np.all(np.isfinite(W))
    assert err <= tol, (name, err, tol)
    # logdet = 1: the right-hand side G - l_ref
    l_ref, keep_l, e_l = pt.logdet_truth(name, om, X, E)
    both = keep & keep_l
    kept = int(both.sum())
    W1 = pull_host(tm, X[:ROWS], G, E, logdet=True)
    tol = 8.0 * (e_fd + e_slope + e_spl + e_l)
    err = eta(J[both], W1[both], (G - l_ref)[both], G[both], extra=1.0 + np.abs(l_ref[both]))
    print('%s %s logdet 1: kept %d / %d, own estimate of l_ref %.3e, e_spl %.1e, tolerance %.3e, eta %.3e' % (backend, name, kept, ROWS, e_l, e_spl, tol, err))
    assert kept >= 130 if name == 'class_55' else kept == ROWS
    assert np.all(np.isfinite(W1[both]))
    assert err <= tol, (name, err, tol)


def test_the_pulled_score_of_the_maps_own_density_is_minus_z(backend):
    """Known answer through the public surface: the pullback density of the map pulls back to the reference density phi, whose
    gradient is -z - so pull_gradient(X, evaluate_pullback_score(X)) = -map(X).  On a standardised map (mean 0, deviation 1 to
    1e-14: the score's log-determinant term, taken at the raw sample, is then the pull's).  As a backward error:
    |sum_j Jref_ji (W_j + Z_j)| against the denominator and the tolerance of the logdet = 1 comparison above."""
    tm, om, X, E = case(pt.STD, backend)
    assert np.max(np.abs(tm.X_mean)) < 1e-14 and np.max(np.abs(np.asarray(tm.X_std) - 1.0)) < 1e-14
    J, keep, e_fd = pt.jacobian_truth(pt.STD, om, X, E)
    l_ref, keep_l, e_l = pt.logdet_truth(pt.STD, om, X, E)
    e_slope, e_spl = E_SLOPE[pt.STD]
    Xr = X[:ROWS]
    G = tm.evaluate_pullback_score(Xr)
    W = tm.pull_gradient(Xr, G)
    Z = tm.map(Xr)
    assert W.shape == (ROWS, tm.D)
    both = keep & keep_l
    tol = 8.0 * (e_fd + e_slope + e_spl + e_l)
    res = np.abs(np.einsum('nji,nj->ni', J, W + Z))
    den = np.abs(G) + np.einsum('nji,nj->ni', 1.0 + np.abs(J), np.abs(W)) + 1.0 + np.abs(l_ref)
    err = float(np.max((res / den)[both]))
    direct = float(np.max(np.abs(W + Z) / (1.0 + np.abs(Z))))
    print('%s: kept %d / %d, tolerance %.3e, backward error of W + Z %.3e (max |W + Z| / (1 + |Z|) = %.3e)' % (backend, int(both.sum()), ROWS, tol, err, direct))
    assert int(both.sum()) == ROWS and err <= tol
    # without the log-determinant term the same call is J^-T sigma G: another answer
    assert not np.allclose(tm.pull_gradient(Xr, G, logdet=False), W)


# ------------------------------------------------------------------------------------------ the entry point on padded buffers

def raw_call(tm, Xd, N, G, W, k0=0, k1=None, g_scale=None, logdet=1, ldx=None, ldg=None, ldw=None, x=None, coef=None):
    """ttm_pull_gradient itself: Xd a (d, ld) device tensor, G / W device tensors or raw pointers."""
    import torch
    coef = tm._pack_coeffs() if coef is None else coef
    p = lambda t: tm._ptr(t) if isinstance(t, torch.Tensor) else t
    rc = tm._lib.ttm_pull_gradient(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), k0, tm.D if k1 is None else k1, p(Xd) if x is None else x,
                                   Xd.shape[1] if ldx is None else ldx, N, p(G), G.shape[1] if ldg is None else ldg, p(g_scale), logdet, p(W),
                                   W.shape[1] if ldw is None else ldw, tm._stream())
    if tm._dev.type == 'cuda':
        torch.cuda.synchronize()
    return rc


def padded(tm, host, ld):
    """A (columns + 1, ld) sentinel-filled device matrix with `host` (columns x N) in its corner."""
    import torch
    cols, N = host.shape
    h = np.full((cols + 1, ld), SENTINEL)
    h[:cols, :N] = host
    return torch.from_numpy(h).to(tm._dev)


@pytest.mark.parametrize('name', ['c5_shape', 'few_cond', 'few_cond2', 'few_ents', 'dense_5'])
def test_ownership_in_place_windows_and_trailing_blocks(backend, name):
    """Per N in {1, 2, 3, 255, 257, 513}: nothing but rows [0, N) of W's columns is written (sentinel fill; X and G keep their
    bits); in place = out of place; a window of rows = those rows of the whole call; a call with k0 > 0 (and one with k1 < D)
    writes its own block alone and solves that block - held against J_ref's block by the backward error above (a NumPy solve of
    the block gives the same figure by construction, so the residual is formed directly)."""
    import torch
    tm, om, X, E = case(name, backend)
    D, d = tm.D, tm._cm.d_cols
    rng = np.random.default_rng(11)
    sig = tm._to_dev(sigma_of(tm, E))
    for N in (1, 2, 3, 255, 257, 513):
        ld = N + (N & 1) + 2
        Xh = np.ascontiguousarray(tm._import(X[:N], True)[:, :N].cpu().numpy())
        Gh = rng.standard_normal((D, N))
        Xd, Gd, Wd = padded(tm, Xh, ld), padded(tm, Gh, ld), padded(tm, np.full((D, N), SENTINEL), ld)
        assert raw_call(tm, Xd, N, Gd, Wd, g_scale=sig) == 0
        W = Wd.cpu().numpy()
        assert np.all(W[:D, N:] == SENTINEL) and np.all(W[D] == SENTINEL) and np.all(np.isfinite(W[:D, :N]))
        assert same_bits(Gd.cpu().numpy()[:D, :N], Gh) and same_bits(Xd.cpu().numpy()[:d, :N], Xh)
        # in place
        Gi = padded(tm, Gh, ld)
        assert raw_call(tm, Xd, N, Gi, Gi, g_scale=sig) == 0
        assert same_bits(Gi.cpu().numpy(), W), (name, N)
        # windows of rows (even starts: the columns stay 16-byte aligned)
        for a, b in ((0, N // 2), (2 * (N // 4), N), (N - 1 - ((N - 1) & 1), N)):
            if b <= a:
                continue
            Ww = padded(tm, np.full((D, N), SENTINEL), ld)
            assert raw_call(tm, Xd, b - a, tm._ptr(Gd, a), tm._ptr(Ww, a), g_scale=sig, x=tm._ptr(Xd, a), ldg=ld, ldw=ld) == 0
            w = Ww.cpu().numpy()
            assert same_bits(w[:D, a:b], W[:D, a:b]), (name, N, a, b)
            w[:D, a:b] = SENTINEL
            assert np.all(w == SENTINEL)
    # blocks: [k0, D) and [0, k1), 200 rows against J_ref's block; the other components' rows of a D-column buffer stay sentinels
    J, keep, e_fd = pt.jacobian_truth(name, om, X, E)
    tol = 8.0 * (e_fd + E_SLOPE[name][0])
    N, ld = ROWS, ROWS + 2
    Xd = padded(tm, tm._import(X[:N], True)[:, :N].cpu().numpy(), ld)
    Gh = gradients(name, D).T.copy()
    sigma = sigma_of(tm, E)
    for k0, k1 in ((1, D), (D - 1, D), (0, D - 1), (1, 2)):
        if not 0 <= k0 < k1 <= D:
            continue
        Gd, Wd = padded(tm, Gh, ld), padded(tm, np.full((D, N), SENTINEL), ld)
        rc = raw_call(tm, Xd, N, tm._ptr(Gd, k0 * ld), tm._ptr(Wd, k0 * ld), k0=k0, k1=k1, g_scale=tm._to_dev(sigma[k0:k1]), logdet=0, ldg=ld, ldw=ld)
        assert rc == 0
        w = Wd.cpu().numpy()
        blk = w[k0:k1, :N].T.copy()
        w[k0:k1, :N] = SENTINEL
        assert np.all(w == SENTINEL), (name, k0, k1)
        g = Gh[k0:k1].T
        err = eta(J[:, k0:k1, k0:k1], blk, g, g)
        print('%s %s block [%d, %d): tolerance %.3e, eta %.3e' % (backend, name, k0, k1, tol, err))
        assert err <= tol, (name, k0, k1)
        # the NumPy solve of the block: W - W_ref = J^-T (J^T W - g), so |W - W_ref| <= |J^-T| (tol x the denominator of eta)
        Jb = J[:, k0:k1, k0:k1]
        Jt = np.transpose(Jb, (0, 2, 1))
        ref = np.linalg.solve(Jt, g[:, :, None])[:, :, 0]
        den = np.abs(g) + np.einsum('nji,nj->ni', 1.0 + np.abs(Jb), np.abs(blk))
        cap = np.einsum('nij,nj->ni', np.abs(np.linalg.inv(Jt)), tol * den)
        worst = float(np.max(np.abs(blk - ref) / cap))
        print('%s %s block [%d, %d): largest |W - solve| / bound = %.3f' % (backend, name, k0, k1, worst))
        assert worst <= 1.0, (name, k0, k1)
        # without g_scale the same block solves J^T W = G / sigma: the values of a call with g_scale = NULL
        Wn = padded(tm, np.full((D, N), SENTINEL), ld)
        assert raw_call(tm, Xd, N, tm._ptr(Gd, k0 * ld), tm._ptr(Wn, k0 * ld), k0=k0, k1=k1, g_scale=None, logdet=0, ldg=ld, ldw=ld) == 0
        blk_n = Wn.cpu().numpy()[k0:k1, :N].T.copy()
        gn = g / sigma[k0:k1]
        err = eta(Jb, blk_n, gn, gn)
        print('%s %s block [%d, %d) without g_scale: eta %.3e' % (backend, name, k0, k1, err))
        assert err <= tol, (name, k0, k1)
        if k0 > 0 and k1 == D:                                  # the device method's k0 is this call
            assert same_bits(pull_host(tm, X[:N], g, E, k0=k0), blk)


def test_a_non_finite_row_stays_in_its_row(backend):
    """NaN / inf in a sample or a gradient: the entries of that row that depend on it are not finite, every other row keeps its bits."""
    tm, om, X, E = case('c5_shape', backend)
    D, N = tm.D, 64
    G = gradients('c5_shape', D)[:N].copy()
    Xr = np.array(X[:N], dtype=float)
    clean = pull_host(tm, Xr, G, E, logdet=True)
    Xb, Gb = Xr.copy(), G.copy()
    Xb[5, E + 2] = np.nan
    Xb[6, E + D - 1] = np.inf
    Gb[9, 0] = np.inf
    Gb[10, D - 1] = np.nan
    got = pull_host(tm, Xb, Gb, E, logdet=True)
    rows = np.array([5, 6, 9, 10])
    others = np.setdiff1d(np.arange(N), rows)
    assert same_bits(got[others], clean[others])
    assert not np.isfinite(got[5, 2]) and not np.isfinite(got[6, D - 1]) and not np.isfinite(got[9, 0]) and not np.all(np.isfinite(got[10]))
    # a gradient entry of component 0 reaches W_0 alone (J^T is upper triangular: nothing above depends on it)
    assert same_bits(got[9, 1:], clean[9, 1:])


def test_entry_point_refuses_bad_arguments(backend):
    tm, om, X, E = case('c5_shape', backend)
    N, D = 400, tm.D
    Xd = tm._import(X[:N], True)
    G, W = tm._cols(D + 1, N, zero=True), tm._cols(D + 1, N, zero=True)
    ld = G.shape[1]
    assert raw_call(tm, Xd, N, G, W) == 0
    assert raw_call(tm, Xd, N, G, G) == 0                                         # in place
    bad = [dict(ldw=ld - 1), dict(ldg=ld - 1), dict(ldx=ld - 1), dict(W=tm._ptr(W, 1)), dict(G=tm._ptr(G, 1)), dict(x=tm._ptr(Xd, 1)),
           dict(N=0), dict(ldw=N - 2), dict(W=None), dict(G=None), dict(x=ctypes.c_void_p(0)),
           dict(k0=-1), dict(k0=D), dict(k1=D + 1), dict(k0=2, k1=2), dict(k0=3, k1=2),
           dict(W=tm._ptr(G, 2)), dict(W=tm._ptr(G, ld)), dict(W=tm._ptr(G, ld + 2)),   # partial overlaps of W and G
           dict(W=Xd), dict(W=tm._ptr(Xd, (tm._cm.d_cols - 1) * ld)), dict(W=tm._ptr(Xd, 2))]          # W over X
    for kw in bad:
        args = dict(dict(Xd=Xd, N=N, G=G, W=W, ldg=ld, ldw=ld), **kw)
        rc = raw_call(tm, **args)
        print('%s %s: %d' % (backend, sorted(kw), rc))
        assert rc == E_ARG, kw


def test_maps_without_a_univariate_form_are_refused(backend):
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 3))
    G = rng.standard_normal((300, 3))
    mon, non = specs.banded_separable_spec(3, band=2)
    mon_i, non_i = specs.banded_integrated_spec(3, 2, 2)
    tm_i = transport_map(X=X, monotone=mon_i, nonmonotone=non_i, verbose=False, monotonicity='integrated rectifier')
    tm_c = transport_map(X=X, monotone=mon, nonmonotone=[[[]], [[], [0]], [[], [0], [1], [0, 1]]], verbose=False, monotonicity='separable monotonicity')
    mon_d, non_d = specs.dense_separable_spec(3, 3)
    non_d[2] = list(non_d[2]) + [[0, 1]]                                          # a dense map with a cross term
    tm_d = transport_map(X=X, monotone=mon_d, nonmonotone=non_d, verbose=False, monotonicity='separable monotonicity')
    for tm, why in ((tm_i, 'integrated'), (tm_c, 'cross'), (tm_d, 'cross')):
        with pytest.raises(NotImplementedError, match=why):
            tm.pull_gradient(X, G)
        Xd, Gd = tm._import(X, True), tm._import(G, False)
        with pytest.raises(NotImplementedError, match=why):
            tm.pull_gradient_device(Xd, 300, Gd)
        rc = raw_call(tm, Xd, 300, Gd, tm._cols(3, 300))
        print('%s %s: %d' % (backend, why, rc))
        assert rc == E_UNSUPPORTED
    tm_s = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, monotonicity='separable monotonicity')
    for k in range(3):                                                          # (an unfitted map has m' = 0: give it slopes)
        tm_s.coeffs_mon[k] = 0.2 + 0.5 * rng.random(len(tm_s.coeffs_mon[k]))
        tm_s.coeffs_nonmon[k] = 0.3 * rng.standard_normal(len(tm_s.coeffs_nonmon[k]))
    assert np.all(np.isfinite(tm_s.pull_gradient(X, G)))
    with pytest.raises(ValueError, match='G must'):
        tm_s.pull_gradient(X, G[:299])
    with pytest.raises(ValueError, match='G must'):
        tm_s.pull_gradient(X, np.zeros((300, 4)))
    # fewer columns of G: the trailing components, the columns in front as X_star
    W2 = tm_s.pull_gradient(X[:, 1:], G[:, 1:], X_star=X[:, :1])
    Xd = tm_s._import(X, True)
    ref = tm_s._export(tm_s.pull_gradient_device(Xd, 300, tm_s._import(G[:, 1:], False), k0=1, g_scale=tm_s._to_dev(np.asarray(tm_s.X_std, dtype=float)[1:])),
                       300, 0, 2, False)
    assert W2.shape == (300, 2) and same_bits(W2, ref)
