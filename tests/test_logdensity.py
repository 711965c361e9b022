"""
Log-density and score of integrated-rectifier maps (transport_map.evaluate_pullback_logdensity / logdensity_device,
include/ttm.h: ttm_logdensity; the per-sample routine int_score_row of csrc/ttm_logdensity.h) on the host test double and on
the device, against the oracle alone.

Truth.  log p(x) = -D/2 log 2 pi + sum_k [ -1/2 S_k(u)^2 + log((r(g_k(u)) + delta) / sigma_ck) ] is put together from
OracleMap.s, fun_mon . coeffs_mon, rect.evaluate(...) + delta and X_std.  The score is the central differences of that log p in
every own column with steps h, h/2, h/4, h = 1e-3 sigma_c, Richardson-extrapolated twice (tests/test_score.py: richardson); r2 is
the expected score, e_FD = |r1 - r2| / (1 + |r2|) the reference's own error estimate.  200 rows; a row is kept when the whole
stencil is finite and e_FD <= 1e-9 in every column - a rule of the oracle alone.

Metric |a - b| / (1 + |b|).  Tolerances: 8 e_FD + 1e-11 for the score (e_FD the largest over the kept rows, computed here), 1e-11
for log p - the bound tests/test_int_dense.py holds the integrated kernels to against the oracle.  Every figure is printed before
it is held.

The data is neither centred nor of unit deviation (scaled by 1.1 + 0.2 j per column, shifted by 0.3): the 1 / sigma factors
are pinned by the same comparison.
"""
import ctypes

import numpy as np
import pytest

from tests.hostemu import emu
from tests.test_score import richardson

ROWS = 200
N_TRAIN = 1201
KIND = 'integrated rectifier'
RECTS = ['softplus', 'exponential', 'expneg', 'explinearunit', 'squared']
MIN_KEPT = {'softplus': ROWS, 'exponential': ROWS, 'expneg': ROWS, 'explinearunit': 195, 'squared': 150}


def _spec(name):
    from triangular_transport_toolbox_amd import specs
    if name == 'spiral3':
        return specs.spiral_spec(3, 2), 2, 5
    if name == 'spiral10':
        return specs.spiral_spec(10, 2), 2, 5
    if name == 'band5':
        return specs.banded_integrated_spec(5, 2, 2), 5, 7
    assert name == 'special_cond'
    mon = [[[1]], [[2], 'iRBF 2', 'iRBF 2', [1, 2]], [[3], 'LET 3', 'RET 3', [2, 3, 'HF']]]
    non = [[[], [0]], [[], [0], [1], [0, 1]], [[], [1], [2], [1, 2, 'HF'], 'RBF 2']]
    return (mon, non), 4, 11


def data(d, seed, n=N_TRAIN):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)) @ (np.tril(rng.standard_normal((d, d)) * 0.4) + np.eye(d)).T + 0.3 * rng.standard_normal((n, d)) ** 2
    return X * (1.1 + 0.2 * np.arange(d)) + 0.3, rng


def build(name, rect='softplus', Q=12, n=N_TRAIN, oracle=True, X=None, **extra):
    """(tm, om, X, E) of a case; the map is made for whichever backend is installed."""
    from triangular_transport_toolbox_amd.transport_map import transport_map
    from oracle.ttm_oracle import OracleMap
    (mon, non), d, seed = _spec(name)
    Xd, rng = data(d, seed, n)
    X = Xd if X is None else X
    kw = dict(monotonicity=KIND, rectifier_type=rect, quadrature_input={'order': Q})
    kw.update(extra)
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw)
    om = OracleMap(X=X, monotone=mon, nonmonotone=non, **kw) if oracle else None
    for k in range(tm.D):
        m, q = len(tm.coeffs_mon[k]), len(tm.coeffs_nonmon[k])
        cm_ = 0.4 * rng.standard_normal(m) / (1 + 0.5 * np.arange(m))
        cm_[0] += 0.5
        cn_ = 0.3 * rng.standard_normal(q) / (1 + np.arange(q))
        tm.coeffs_mon[k], tm.coeffs_nonmon[k] = cm_.copy(), cn_.copy()
        if om is not None:
            om.coeffs_mon[k], om.coeffs_nonmon[k] = cm_.copy(), cn_.copy()
    return tm, om, X, d - tm.D


def oracle_logp(om, X):
    """log p of the raw rows X (all d columns) from the oracle's pieces."""
    E, D = om.skip_dimensions, om.D
    with np.errstate(all='ignore'):
        U = (X - om.X_mean) / om.X_std
        lp = np.full(X.shape[0], -0.5 * D * np.log(2 * np.pi))
        for k in range(D):
            S = om.s(U.copy(), k)
            g = np.dot(om.fun_mon(k, U.copy()), om.coeffs_mon[k][:, None])[..., 0]
            r = om.rect.evaluate(g) + om.delta
            lp += -0.5 * S ** 2 + np.log(r / om.X_std[E + k])
    return lp


_TRUTH = {}


def truth(key, om, X, E):
    """(log p [ROWS], r2 [ROWS x D], keep [ROWS], e_FD) of a case - from the oracle alone, computed once and left unchanged."""
    if key not in _TRUTH:
        Xr = np.array(X[:ROWS], dtype=float)
        D = om.D
        lp = oracle_logp(om, Xr)
        r2, err, fin = np.zeros((ROWS, D)), np.zeros((ROWS, D)), np.ones((ROWS, D), dtype=bool)
        for k in range(D):
            c = E + k

            def logp(col):
                Xp = Xr.copy()
                Xp[:, c] = col
                return oracle_logp(om, Xp)
            r2[:, k], dlt, fin[:, k] = richardson(logp, Xr[:, c], 1e-3 * float(om.X_std[c]))
            with np.errstate(all='ignore'):
                err[:, k] = dlt / (1.0 + np.abs(r2[:, k]))
        with np.errstate(all='ignore'):
            keep = np.all(fin & (err <= 1e-9), axis=1) & np.isfinite(lp)
        for a in (lp, r2, keep):
            a.setflags(write=False)
        _TRUTH[key] = (lp, r2, keep, float(err[keep].max()))
    return _TRUTH[key]


def metric(a, b):
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if np.size(a) else 0.0


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


def check_against_truth(key, tm, om, X, E, rect, backend):
    lp_ref, r2, keep, e_fd = truth(key, om, X, E)
    own, star = X[:ROWS, E:], (X[:ROWS, :E] if E else None)
    logp, G = tm.evaluate_pullback_logdensity(own, X_star=star, score=True)
    assert logp.shape == (ROWS,) and G.shape == (ROWS, tm.D)
    kept = int(keep.sum())
    tol = 8.0 * e_fd + 1e-11
    e_lp, e_g = metric(logp[keep], lp_ref[keep]), metric(G[keep], r2[keep])
    print('%s %s: kept %d / %d, e_FD %.3e, log p error %.3e (1e-11), score error %.3e (%.3e)' % (key, backend, kept, ROWS, e_fd, e_lp, e_g, tol))
    assert kept >= MIN_KEPT[rect]
    assert np.all(np.isfinite(logp[keep])) and np.all(np.isfinite(G[keep]))
    assert e_lp <= 1e-11, (key, e_lp)
    assert e_g <= tol, (key, e_g, tol)
    return logp, G


@pytest.mark.parametrize('rect', RECTS)
def test_spiral3_every_rectifier(backend, rect):
    """Cross terms in the monotone part (the weights' walk: mnt / xgrp), each of the five rectifiers - r' of `squared` and the
    ELU included, which the objective's rectifier routine does not have."""
    tm, om, X, E = build('spiral3', rect)
    check_against_truth(('spiral3', rect, 12), tm, om, X, E, rect, backend)


@pytest.mark.parametrize('Q', [12, 100])
@pytest.mark.parametrize('rect', ['softplus', 'exponential'])
def test_band5_derivative_of_the_quadrature_sum(backend, rect, Q):
    """Five components, band 2.  At Q = 12 with the exponential rectifier the derivative of the quadrature sum and r(g(x_k)) + delta
    differ by 1.5e-4 on this map: only the former passes."""
    tm, om, X, E = build('band5', rect, Q)
    check_against_truth(('band5', rect, Q), tm, om, X, E, rect, backend)


@pytest.mark.parametrize('rect', ['softplus', 'exponential'])
def test_special_terms_and_a_conditioning_column(backend, rect):
    """Special terms of x_k, a special-term factor on another column, cross terms and one conditioning column; the conditioning
    column given separately or stacked: the same bits."""
    tm, om, X, E = build('special_cond', rect)
    assert E == 1
    logp, G = check_against_truth(('special_cond', rect, 12), tm, om, X, E, rect, backend)
    logp2, G2 = tm.evaluate_pullback_logdensity(X[:ROWS], score=True)
    assert np.array_equal(logp, logp2) and np.array_equal(G, G2)


def test_spiral10_smaller_block(backend):
    """Example 01's shipped order: nB + 1 = 11, three slot sets of 11 no longer fit 256 threads."""
    tm, om, X, E = build('spiral10', 'softplus')
    assert max(int(v) for v in tm._cm.nb1) == 11
    check_against_truth(('spiral10', 'softplus', 12), tm, om, X, E, 'softplus', backend)


@pytest.mark.parametrize('name', ['band5', 'special_cond'])
def test_device_call_on_standardised_data_equals_the_raw_call(backend, name):
    """logdensity_device without g_scale against evaluate_pullback_logdensity on data that is already standardised: there
    g_scale = 1 to rounding and the two calls differ only in that argument and the constant."""
    _, d, seed = _spec(name)
    X, _ = data(d, seed)
    Xs = (X - X.mean(axis=0)) / X.std(axis=0)
    tm, _, _, E = build(name, 'softplus', oracle=False, X=Xs)
    assert np.max(np.abs(tm.X_mean)) < 1e-14 and np.max(np.abs(np.asarray(tm.X_std) - 1.0)) < 1e-14
    logp_raw, G_raw = tm.evaluate_pullback_logdensity(Xs[:ROWS], score=True)
    Xd = tm._import(Xs[:ROWS], True)
    logp, G = tm.logdensity_device(Xd, ROWS)
    logp = logp[:ROWS].cpu().numpy() - 0.5 * tm.D * np.log(2 * np.pi)
    G = tm._export(G, ROWS, 0, tm.D, False)
    assert np.all(np.isfinite(logp_raw)) and np.all(np.isfinite(G_raw))
    assert metric(logp, logp_raw) <= 1e-13 and metric(G, G_raw) <= 1e-13


def test_log_density_alone_has_the_same_bits(backend):
    tm, _, X, E = build('special_cond', 'exponential', oracle=False)
    logp, G = tm.evaluate_pullback_logdensity(X[:ROWS], score=True)
    alone = tm.evaluate_pullback_logdensity(X[:ROWS])
    assert isinstance(alone, np.ndarray) and alone.shape == (ROWS,) and np.array_equal(alone, logp)
    # the score alone (no log p buffer) on the device entry point: the same bits again
    Xd = tm._import(X[:ROWS], True)
    gs = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float)[E:])
    _, G2 = tm.logdensity_device(Xd, ROWS, G=tm._cols(tm.D, ROWS), g_scale=gs)
    assert np.array_equal(tm._export(G2, ROWS, 0, tm.D, False), G)


@pytest.mark.parametrize('name,rect', [('band5', 'softplus'), ('special_cond', 'exponential'), ('spiral3', 'squared')])
def test_log_density_is_the_forward_maps(backend, name, rect):
    """-1/2 sumsq + logdet(sigma) of ttm_forward on the same buffers: the same S_k and the same r + delta."""
    tm, _, X, E = build(name, rect, oracle=False)
    Xd = tm._import(X[:ROWS], True)
    sigma = tm._to_dev(np.asarray(tm.X_std, dtype=float)[E:])
    gs = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float)[E:])
    ld, ss = tm._empty(ROWS), tm._empty(ROWS)
    tm.forward_device(Xd, ROWS, logdet=ld, sigma=sigma, sumsq=ss)
    logp, _ = tm.logdensity_device(Xd, ROWS, logp=tm._empty(ROWS), g_scale=gs)
    ref = (-0.5 * ss + ld).cpu().numpy()
    got = logp.cpu().numpy()
    pub = tm.evaluate_pullback_logdensity(X[:ROWS]) + 0.5 * tm.D * np.log(2 * np.pi)
    fin = np.isfinite(ref)
    print('%s %s %s: finite %d / %d, error %.3e, public %.3e' % (name, rect, backend, fin.sum(), ROWS, metric(got[fin], ref[fin]), metric(pub[fin], ref[fin])))
    assert fin.sum() >= 150 and np.array_equal(np.isfinite(got), fin)
    assert metric(got[fin], ref[fin]) <= 1e-11 and metric(pub[fin], ref[fin]) <= 1e-11


def test_without_standardisation_the_given_samples_are_used_as_they_are(backend):
    """standardize_samples = False: X is taken as u, sigma = 1 - the standardised-coordinates density of the device call."""
    _, d, seed = _spec('band5')
    X, _ = data(d, seed)
    Xs = (X - X.mean(axis=0)) / X.std(axis=0)
    tm, _, _, E = build('band5', 'softplus', oracle=False, X=Xs, standardize_samples=False)
    logp, G = tm.evaluate_pullback_logdensity(0.5 * Xs[:ROWS] + 0.1, score=True)
    Xd = tm._import(0.5 * Xs[:ROWS] + 0.1, False)
    lp2, G2 = tm.logdensity_device(Xd, ROWS)
    assert np.array_equal(logp, lp2[:ROWS].cpu().numpy() - 0.5 * tm.D * np.log(2 * np.pi))
    assert np.array_equal(G, tm._export(G2, ROWS, 0, tm.D, False))


def test_separable_maps_are_sent_to_their_own_functions(backend):
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    X, _ = data(3, 3, 300)
    mon, non = specs.banded_separable_spec(3, band=2)
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, monotonicity='separable monotonicity')
    with pytest.raises(NotImplementedError, match='evaluate_pullback_density / evaluate_pullback_score'):
        tm.evaluate_pullback_logdensity(X)
    with pytest.raises(NotImplementedError):
        tm.logdensity_device(tm._Xs, tm._N)
    # the entry point itself
    coef = tm._pack_coeffs()
    out = tm._empty(tm._N)
    rc = tm._lib.ttm_logdensity(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._ptr(tm._Xs), tm._Xs.shape[1], tm._N, tm._ptr(out),
                                None, tm._N, None, tm._stream())
    from triangular_transport_toolbox_amd import _capi
    assert rc == _capi.TTM_E_UNSUPPORTED


def test_entry_point_refuses_bad_arguments(backend):
    """ttm_logdensity: TTM_E_ARG for null coef / fold / Xsoa, both outputs null, N < 1, ldx < N and ldg < N; the same call with good
    arguments runs."""
    tm, _, X, E = build('band5', 'softplus', oracle=False)
    N, D = 100, tm.D
    coef = tm._pack_coeffs()
    Xd = tm._import(X[:N], True)
    G, lp = tm._cols(D, N), tm._empty(N)
    good = dict(coef=tm._ptr(coef), fold=tm._ptr(coef._ttm_fold), x=tm._ptr(Xd), ldx=Xd.shape[1], n=N, lp=tm._ptr(lp), g=tm._ptr(G), ldg=G.shape[1])

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return tm._lib.ttm_logdensity(tm._pp, a['coef'], a['fold'], a['x'], a['ldx'], a['n'], a['lp'], a['g'], a['ldg'], None, tm._stream())
    assert call() == 0
    assert call(lp=None) == 0 and call(g=None) == 0
    assert call(g=None, ldg=0) == 0                                 # (ldg is not looked at without G)
    for bad in (dict(coef=None), dict(fold=None), dict(x=None), dict(lp=None, g=None), dict(n=0), dict(n=-3), dict(ldx=N - 1), dict(ldg=N - 1)):
        assert call(**bad) == -1, bad                               # TTM_E_ARG


# ---------------------------------------------------------------------------------------------------------------------
# device only: every row against the host double, tails and seams, padded leading dimensions, the kernel's name
# ---------------------------------------------------------------------------------------------------------------------

def _raw_call(tm, Xcols, ldx, N, E, ldg=None, fill=None):
    """ttm_logdensity on a d x ldx device matrix with g_scale = 1 / sigma -> (logp tensor [ldg], G tensor [D x ldg])."""
    import torch
    ldg = N if ldg is None else ldg
    coef = tm._pack_coeffs()
    gs = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float)[E:])
    lp = torch.full((ldg,), fill if fill is not None else 0.0, dtype=torch.float64, device=Xcols.device)
    G = torch.full((tm.D, ldg), fill if fill is not None else 0.0, dtype=torch.float64, device=Xcols.device)
    rc = tm._lib.ttm_logdensity(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._ptr(Xcols), ldx, N, tm._ptr(lp), tm._ptr(G), ldg,
                                tm._ptr(gs), tm._stream())
    assert rc == 0
    return lp, G


@pytest.mark.gpu
@pytest.mark.parametrize('name,rect', [('band5', 'softplus'), ('special_cond', 'exponential')])
def test_every_row_against_the_host_double(name, rect):
    """N = 5003 (several workgroups, a ragged tail), 257 (one row into the second workgroup) and 1: every row of log p and of the
    score within 1e-11 of the host double's, which the 200-row truth does not reach."""
    import torch
    n = 5003
    with emu.install():
        tm_h, _, X, E = build(name, rect, n=n, oracle=False)
        lp_h, G_h = tm_h.evaluate_pullback_logdensity(X, score=True)
    tm, _, X2, _ = build(name, rect, n=n, oracle=False)
    assert np.array_equal(X, X2)
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    tm.logdensity_device(tm._Xs, tm._N)
    assert tm._lib.ttm_last_kernel().decode() == 'k_logdensity_int'
    lp, G = tm.evaluate_pullback_logdensity(X, score=True)
    fin = np.isfinite(lp_h) & np.all(np.isfinite(G_h), axis=1)
    print('%s %s: N %d, finite rows %d, log p error %.3e, score error %.3e' % (name, rect, n, fin.sum(), metric(lp[fin], lp_h[fin]), metric(G[fin], G_h[fin])))
    assert fin.sum() >= n - 50
    assert np.array_equal(np.isfinite(lp), np.isfinite(lp_h))
    assert metric(lp[fin], lp_h[fin]) <= 1e-11 and metric(G[fin], G_h[fin]) <= 1e-11
    for m in (257, 1):
        lpm, Gm = tm.evaluate_pullback_logdensity(X[:m], score=True)
        f = fin[:m]
        assert lpm.shape == (m,) and Gm.shape == (m, tm.D)
        assert metric(lpm[f], lp_h[:m][f]) <= 1e-11 and metric(Gm[f], G_h[:m][f]) <= 1e-11
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_padded_leading_dimensions_are_left_alone():
    """ldx = ldg = N + 7: rows [N, ld) of X are NaN, the output pads hold a sentinel - unchanged afterwards, and the results are
    those of the tight call bit for bit."""
    import torch
    tm, _, X, E = build('special_cond', 'softplus', oracle=False)
    N, d, D = 1000, 4, tm.D
    ld = N + 7
    Xt = tm._import(X[:N], True)[:, :N].contiguous()
    lp0, G0 = _raw_call(tm, Xt, N, N, E)
    Xp = torch.full((d, ld), float('nan'), dtype=torch.float64, device=Xt.device)
    Xp[:, :N] = Xt
    sentinel = -7.25
    lp1, G1 = _raw_call(tm, Xp, ld, N, E, ldg=ld, fill=sentinel)
    torch.cuda.synchronize()
    assert torch.all(lp1[N:] == sentinel) and torch.all(G1[:, N:] == sentinel)
    assert torch.equal(lp1[:N], lp0) and torch.equal(G1[:, :N], G0)
    assert bool(torch.isfinite(lp0).all()) and bool(torch.isfinite(G0).all())
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    assert tm._lib.ttm_last_kernel().decode() == 'k_logdensity_int'
