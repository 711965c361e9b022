"""
Draws with their log-density: transport_map.sample(logdensity=True) / sample_device(logq=) / inverse_device(logq=) and the entry
point ttm_inverse_logdensity (include/ttm.h; per-sample routines of csrc/ttm_sample_logq.h), on the host test double and on the
device.

Truth is the oracle alone: log q of the inverted components k0 .. D - 1 at the RETURNED rows, put together from OracleMap.s,
fun_mon . coeffs_mon, rect.evaluate(...) + delta and X_std (tests/test_logdensity.py: oracle_logp, here restricted to the inverted
components), conditioning columns stacked in front.  Metric |a - b| / (1 + |b|), tolerance 1e-11 - the bound tests/test_logdensity.py
and tests/test_int_dense.py hold these kernels to.  A row is compared when every own column of the returned sample has |u| <= 10 in
standardised coordinates (searches that run away to |x| ~ 1e15 cancel in any evaluation).  Every figure is printed before it is
held.

Maps: tests/test_logdensity.build(name, rect, alternate_root_finding=False, root_finder=...); draws: seed 3, draw 0; N = 257 (one
full block of 256 threads plus one row, plus the replay of sample 0 under a cap for bisection).
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.hostemu import emu
from tests.test_logdensity import RECTS, build, metric
from tests.util import options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 257
SEED, DRAW = 3, 0
METHODS = ['newton', 'reference']
CASES = [('spiral3', r) for r in RECTS if r != 'squared'] + [('spiral10', 'softplus'), ('band5', 'softplus')] + \
        [('special_cond', r) for r in RECTS]
SENTINEL = -7.25e300
E_ARG, E_UNSUPPORTED = -1, -4


def floor_of(name, rect):
    if name != 'special_cond':
        return N
    return 120 if rect == 'squared' else 200


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


_MAPS = {}


def case(backend, name, rect, method):
    """(tm, om, X, E) of a case, made once per backend (the oracle is shared and left unchanged)."""
    key = (backend, name, rect)
    if key not in _MAPS:
        _MAPS[key] = build(name, rect, alternate_root_finding=False, root_finder=method)
    tm = _MAPS[key][0]
    tm.root_finder = method
    return _MAPS[key]


def oracle_terms(om, Xfull, k0):
    """(S [N x (D - k0)], dS/du the same shape) of the components k0 .. D - 1 at the raw rows Xfull (all d columns)."""
    D = om.D
    with np.errstate(all='ignore'):
        U = (Xfull - om.X_mean) / om.X_std
        S, dS = np.zeros((Xfull.shape[0], D - k0)), np.zeros((Xfull.shape[0], D - k0))
        for k in range(k0, D):
            S[:, k - k0] = om.s(U.copy(), k)
            g = np.dot(om.fun_mon(k, U.copy()), om.coeffs_mon[k][:, None])[..., 0]
            dS[:, k - k0] = om.rect.evaluate(g) + om.delta
    return S, dS


def oracle_logq(om, Xfull, k0):
    """log q of the components k0 .. D - 1 given the columns in front, at the raw rows Xfull."""
    E, D = om.skip_dimensions, om.D
    S, dS = oracle_terms(om, Xfull, k0)
    with np.errstate(all='ignore'):
        sig = om.X_std[E + k0:E + D]
        return -0.5 * (D - k0) * np.log(2 * np.pi) + np.sum(-0.5 * S ** 2 + np.log(dS / sig), axis=1)


def kept_rows(om, Xfull, k0):
    E = om.skip_dimensions
    with np.errstate(all='ignore'):
        U = (Xfull - om.X_mean) / om.X_std
        return np.all(np.abs(U[:, E + k0:]) <= 10.0, axis=1)


def stacked(X_star, X, n):
    if X_star is None:
        return X
    return np.column_stack((np.broadcast_to(np.asarray(X_star, dtype=float).reshape(-1, np.shape(X_star)[-1]), (n, np.shape(X_star)[-1])), X))


def check_against_oracle(label, tm, om, star, floor, backend, k0=0, n=N, **kw):
    X, logq = tm.sample(n, X_star=star, seed=SEED, draw=DRAW, logdensity=True, **kw)
    # (as inverse_map: without skip_dimensions the conditioning columns come back in front of the drawn ones)
    assert X.shape == (n, tm.D) and logq.shape == (n,) and logq.dtype == np.float64
    Xfull = stacked(star, X, n) if tm.skip_dimensions else X
    keep = kept_rows(om, Xfull, k0)
    ref = oracle_logq(om, Xfull, k0)
    err = metric(logq[keep], ref[keep])
    print('%s %s: kept %d / %d (floor %d), log q error %.3e (1e-11)' % (label, backend, int(keep.sum()), n, floor, err))
    assert int(keep.sum()) >= floor
    assert np.all(np.isfinite(logq[keep]))
    assert err <= 1e-11, (label, err)
    return X, logq


# ------------------------------------------------------------------------------------------ 1: against the oracle alone

@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name,rect', CASES)
def test_logq_of_the_draws_against_the_oracle(backend, name, rect, method):
    tm, om, X, E = case(backend, name, rect, method)
    star = X[:N, :E] if E else None
    check_against_oracle('%s/%s/%s' % (name, rect, method), tm, om, star, floor_of(name, rect), backend)


# ------------------------------------------------------------------------------------------ the entry point, driven directly

def device_of(backend):
    return 'cpu' if backend == 'hostemu' else 'cuda'


def entry(tm, backend, Zs, Xs, n, newton, cap=None, logq=None, row0=0, plain=False):
    """ttm_inverse_logdensity (plain: ttm_inverse_bisect / ttm_inverse_newton) on rows [row0, row0 + n) of the device matrices.
    Returns (rc, iters)."""
    import torch
    coef = tm._pack_coeffs()
    iters = torch.zeros(tm.D, dtype=torch.int32, device=device_of(backend))
    head = (tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, tm.D, tm._ptr(Zs, row0), Zs.shape[1], tm._ptr(Xs, row0), Xs.shape[1], n)
    itp = ctypes.c_void_p(iters.data_ptr())
    capp = None if cap is None else ctypes.c_void_p(cap.data_ptr())
    if plain and newton:
        rc = tm._lib.ttm_inverse_newton(*head, itp, tm._stream())
    elif plain:
        rc = tm._lib.ttm_inverse_bisect(*head, itp, capp, tm._stream())
    else:
        rc = tm._lib.ttm_inverse_logdensity(*head, int(newton), itp, capp, tm._ptr(logq, row0), None, tm._stream())
    return rc, iters.cpu().numpy()


def buffers(tm, star, E, n):
    """(Zs, Xs) of a draw: the reference deviates of all components and the matrix the inverse writes into."""
    Xs = tm._conditioned_cols(star, E, n)
    Zs = tm.reference_device(n, seed=SEED, draw=DRAW)
    return Zs, Xs


# ------------------------------------------------------------------------------------------ 2: the value is the root's

@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name,rect', [('spiral3', 'softplus'), ('spiral3', 'exponential'), ('band5', 'softplus'), ('special_cond', 'softplus'),
                                       ('special_cond', 'explinearunit')])
def test_logq_is_the_density_at_the_root(backend, name, rect, method):
    """On kept rows whose search converged (iters < 100; a row's own count comes from the call on that row alone, which also has
    to reproduce the row of the whole call bit for bit): |logq - (sum log dS - 1/2 sum z^2)| <= sum_k 1e-9 (|z_k| + 1), z the
    reference draws and dS the oracle's - the stopping rule |S - z| <= 1e-9 gives 1/2 |S^2 - z^2| <= 1e-9 (|z| + 1) to first order."""
    import torch
    tm, om, X, E = case(backend, name, rect, method)
    newton = method == 'newton'
    star = X[:N, :E] if E else None
    Zs, Xs = buffers(tm, star, E, N)
    logq = torch.full((N,), SENTINEL, dtype=torch.float64, device=device_of(backend))
    rc, _ = entry(tm, backend, Zs, Xs, N, newton, logq=logq)
    assert rc == 0
    U, lq, z = Xs[:, :N].cpu().numpy().T.copy(), logq.cpu().numpy(), Zs[:, :N].cpu().numpy().T.copy()
    # rows one by one: the row's own trial-point count, and the same bits
    Xr = tm._conditioned_cols(star, E, N)
    lr = torch.full((N,), SENTINEL, dtype=torch.float64, device=device_of(backend))
    its = np.zeros(N, dtype=np.int64)
    for n in range(N):
        rc, it = entry(tm, backend, Zs, Xr, 1, newton, logq=lr, row0=n)
        assert rc == 0
        its[n] = it.max()
    assert np.array_equal(Xr[:, :N].cpu().numpy().T, U, equal_nan=True) and np.array_equal(lr.cpu().numpy(), lq, equal_nan=True)
    Xfull = U * om.X_std + om.X_mean
    keep = kept_rows(om, Xfull, 0) & (its < 100)
    _, dS = oracle_terms(om, Xfull, 0)
    with np.errstate(all='ignore'):
        expect = np.sum(np.log(dS) - 0.5 * z ** 2, axis=1)
        bound = np.sum(1e-9 * (np.abs(z) + 1.0), axis=1)
        diff = np.abs(lq - expect)
    worst = float(np.max((diff / bound)[keep]))
    print('%s/%s/%s %s: %d rows kept and converged of %d, largest |logq - root value| / bound = %.3e (1)' % (name, rect, method, backend, int(keep.sum()), N, worst))
    assert int(keep.sum()) >= floor_of(name, rect)
    assert np.all(diff[keep] <= bound[keep])


# ------------------------------------------------------------------------------------------ 3: same draws

@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name,rect', [('spiral3', 'softplus'), ('spiral3', 'expneg'), ('spiral10', 'softplus'), ('band5', 'softplus'),
                                       ('special_cond', 'softplus'), ('special_cond', 'squared')])
def test_the_draws_are_those_of_the_plain_search(backend, name, rect, method):
    import torch
    tm, om, X, E = case(backend, name, rect, method)
    newton = method == 'newton'
    star = X[:N, :E] if E else None
    Xa, _ = tm.sample(N, X_star=star, seed=SEED, draw=DRAW, logdensity=True)
    Xb = tm.sample(N, X_star=star, seed=SEED, draw=DRAW)
    assert Xa.shape == Xb.shape and np.array_equal(Xa, Xb, equal_nan=True)
    # the entry point against the plain one: all rows, then (bisection) row 0 again under the cap the rows behind it give
    dev = device_of(backend)
    Zs, Xp = buffers(tm, star, E, N)
    _, Xf = buffers(tm, star, E, N)
    logq = torch.zeros(N, dtype=torch.float64, device=dev)
    rc_p, it_p = entry(tm, backend, Zs, Xp, N, newton, plain=True)
    rc_f, it_f = entry(tm, backend, Zs, Xf, N, newton, logq=logq)
    assert rc_p == 0 and rc_f == 0
    print('%s/%s/%s %s: iters plain %s fused %s' % (name, rect, method, backend, it_p, it_f))
    assert np.array_equal(it_p, it_f) and torch.equal(Xp.view(torch.int64), Xf.view(torch.int64))
    if not newton:
        for capv in (it_p, np.zeros_like(it_p), np.minimum(it_p, 3)):
            cap = torch.from_numpy(np.ascontiguousarray(capv, dtype=np.int32)).to(dev)
            rc_p, ic_p = entry(tm, backend, Zs, Xp, 1, False, cap=cap, plain=True)
            rc_f, ic_f = entry(tm, backend, Zs, Xf, 1, False, cap=cap, logq=logq)
            assert rc_p == 0 and rc_f == 0
            assert np.array_equal(ic_p, ic_f) and torch.equal(Xp.view(torch.int64), Xf.view(torch.int64))
            assert np.all(ic_f <= capv)


# ------------------------------------------------------------------------------------------ 4: every kernel family

def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


@pytest.mark.parametrize('method', METHODS)
def test_every_kernel_family_carries_the_density(backend, method):
    """The three kernel families of the device library by option, each named.  (The host double's entry point follows the library's
    default plan whatever the options - csrc/ttm_sample_logq.h - so there the runs repeat the monomial-form search; its generic search
    is what the `special_cond` cases of the other tests run.)"""
    tm, om, X, E = case(backend, 'spiral3', 'softplus', method)
    tag = 'newton' if method == 'newton' else 'bisect'
    # (the library's own plan keeps the root searches off the X programs - option int_xprog = 2 sends them there, csrc/ttm_options.h -
    # so the default and int_xprog = 0 both take k_int_root)
    expected = [({'int_xprog': 2}, 'k_int_root_x<%s,logq>' % tag), ({}, 'k_int_root<%s,logq>' % tag), ({'int_xprog': 0}, 'k_int_root<%s,logq>' % tag),
                ({'int_dense': 0}, 'k_inverse_%s<logq>' % tag)]
    seen = []
    for opts, kernel in expected:
        with options(tm._lib, **opts):
            check_against_oracle('spiral3/softplus/%s %s' % (method, opts or 'default'), tm, om, None, N, backend)
            if backend == 'hip':                  # (sample() ends on the layout change: the name on the device-resident call)
                tm.sample_device(N, seed=SEED, draw=DRAW, logq=True)
                seen.append(last_kernel(tm))
    if backend == 'hip':
        print('kernels: %s' % seen)
        assert seen == [k for _, k in expected]


# ------------------------------------------------------------------------------------------ 5: ownership and padding

@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('name', ['spiral3', 'special_cond'])
def test_only_the_rows_of_the_call_are_written_and_padding_is_not_read(backend, name, method):
    import torch
    tm, om, X, E = case(backend, name, 'softplus', method)
    newton = method == 'newton'
    dev = device_of(backend)
    d, D = tm._cm.d_cols, tm.D
    for n in (1, 2, 255, 256, 257):
        for ld in (n + 3, n + (n & 1)):
            Zfull = tm.reference_device(n, seed=SEED, draw=DRAW)[:, :n]
            cond = torch.from_numpy(np.ascontiguousarray(((X[:n, :E] - tm.X_mean[:E]) / tm.X_std[:E]).T)).to(dev) if E else None
            results = []
            for poison in (SENTINEL, float('nan'), 3.0):
                Zs = torch.full((D, ld), poison, dtype=torch.float64, device=dev)
                Zs[:, :n] = Zfull
                Xs = torch.full((d + 1, ld), SENTINEL, dtype=torch.float64, device=dev)      # (one column of slack behind)
                Xs[E:d, n:] = poison
                if E:
                    Xs[:E, :] = poison
                    Xs[:E, :n] = cond
                before = Xs.clone()
                logq = torch.full((ld + 2,), SENTINEL, dtype=torch.float64, device=dev)
                rc, it = entry(tm, backend, Zs, Xs, n, newton, logq=logq)
                assert rc == 0
                # nothing outside rows [0, n) of the inverted columns and of logq
                assert torch.equal(Xs[:E].view(torch.int64), before[:E].view(torch.int64))
                assert torch.equal(Xs[E:, n:].view(torch.int64), before[E:, n:].view(torch.int64))
                assert torch.equal(Xs[d].view(torch.int64), before[d].view(torch.int64))
                assert bool(torch.all(logq[n:] == SENTINEL))
                assert not bool(torch.any(logq[:n] == SENTINEL)) and not bool(torch.any(Xs[E:d, :n] == SENTINEL))
                results.append((Xs[E:d, :n].cpu().numpy().copy(), logq[:n].cpu().numpy().copy(), it))
            for Xo, lo, io in results[1:]:
                assert np.array_equal(Xo, results[0][0], equal_nan=True) and np.array_equal(lo, results[0][1], equal_nan=True)
                assert np.array_equal(io, results[0][2])
    print('%s/%s %s: rows and padding hold for N in 1, 2, 255, 256, 257 and ld = N + 3, N + (N & 1)' % (name, method, backend))


# ------------------------------------------------------------------------------------------ 6: conditioning and windows

@pytest.mark.parametrize('method', METHODS)
def test_conditional_density_for_every_conditioning_shape(backend, method):
    # skip_dimensions = 0: X_star holds the first E components
    tm, om, X, _ = case(backend, 'spiral3', 'softplus', method)
    Xc, _ = check_against_oracle('spiral3 | x_0 as (N, 1)/%s' % method, tm, om, X[:N, :1], N, backend, k0=1)
    assert np.max(np.abs(Xc[:, 0] - X[:N, 0])) <= 1e-14 * (1.0 + np.max(np.abs(X[:N, 0])))     # (standardised and back)
    check_against_oracle('spiral3 | x_0, one point/%s' % method, tm, om, X[5, :1], N, backend, k0=1)
    tb, ob, Xb, _ = case(backend, 'band5', 'softplus', method)
    check_against_oracle('band5 | x_0 .. x_2 as (N, 3)/%s' % method, tb, ob, Xb[:N, :3], N, backend, k0=3)
    # skip_dimensions = 1: the conditioning column of the map
    tm, om, X, E = case(backend, 'special_cond', 'softplus', method)
    assert E == 1 and tm.skip_dimensions == 1
    check_against_oracle('special_cond (N, 1)/%s' % method, tm, om, X[:N, :1], 200, backend)
    Xp, lp = check_against_oracle('special_cond one point (1,)/%s' % method, tm, om, X[7, :1], 200, backend)
    Xq, lq = tm.sample(N, X_star=X[7:8, :1], seed=SEED, draw=DRAW, logdensity=True)
    assert np.array_equal(Xp, Xq, equal_nan=True) and np.array_equal(lp, lq, equal_nan=True)


def test_a_window_of_rows_equals_those_rows_of_the_whole(backend):
    """Newton: rows are independent, and so are their densities."""
    tm, om, X, E = case(backend, 'special_cond', 'softplus', 'newton')
    r, n1 = 131, 126
    Xw, lw = tm.sample(r + n1, X_star=X[:r + n1, :E], seed=SEED, draw=DRAW, logdensity=True)
    Xr, lr = tm.sample(n1, X_star=X[r:r + n1, :E], seed=SEED, draw=DRAW, row0=r, logdensity=True)
    assert np.array_equal(Xr, Xw[r:], equal_nan=True) and np.array_equal(lr, lw[r:], equal_nan=True)
    tm, om, X, E = case(backend, 'spiral3', 'softplus', 'newton')
    Xw, lw = tm.sample(r + n1, seed=SEED, draw=DRAW, logdensity=True)
    Xr, lr = tm.sample(n1, seed=SEED, draw=DRAW, row0=r, logdensity=True)
    assert np.array_equal(Xr, Xw[r:]) and np.array_equal(lr, lw[r:])


@pytest.mark.parametrize('method', METHODS)
def test_g_scale_is_the_change_to_raw_coordinates(backend, method):
    """raw log q - standardised log q = -sum log sigma.  Bound: each of the D terms is log(dS / sigma) against log(dS) - log(sigma):
    the division and each logarithm within an ulp or two of values no larger than the row's largest term - 4 ulp of
    (1 + |log q|) per component."""
    tm, om, X, E = case(backend, 'spiral3', 'softplus', method)
    Xraw, raw = tm.sample(N, seed=SEED, draw=DRAW, logdensity=True)
    Xs, lq = tm.sample_device(N, seed=SEED, draw=DRAW, logq=True)
    std = lq[:N].cpu().numpy() - 0.5 * tm.D * np.log(2 * np.pi)
    assert np.array_equal(tm._export(Xs, N, 0, tm._cm.d_cols, True), Xraw)
    shift = -float(np.sum(np.log(np.asarray(tm.X_std, dtype=float))))
    err = np.abs((raw - std) - shift)
    tol = 4.0 * 2.0 ** -52 * tm.D * (1.0 + np.maximum(np.abs(raw), np.abs(std)))
    print('g_scale/%s %s: largest |raw - standardised + sum log sigma| = %.3e, in units of the bound %.3f' % (method, backend, float(err.max()), float((err / tol).max())))
    assert np.all(err <= tol)
    # a buffer instead of True is filled and handed back
    import torch
    buf = torch.zeros(N, dtype=torch.float64, device=device_of(backend))
    _, got = tm.sample_device(N, seed=SEED, draw=DRAW, logq=buf)
    assert got is buf and torch.equal(buf, lq[:N])


# ------------------------------------------------------------------------------------------ 7: separable maps

_SEP = {}


def separable(backend, name):
    from tests.test_band import _build
    if (backend, name) not in _SEP:
        _SEP[(backend, name)] = _build(name, n=1001)
    return _SEP[(backend, name)]


@pytest.mark.parametrize('inverse', ['table', 'reference', 'newton'])
@pytest.mark.parametrize('name', ['few_c2b', 'few_cond', 'c5_shape'])
def test_separable_maps_compose_the_inverse_and_the_density_pass(backend, name, inverse):
    import torch
    tm, om, X, _ = separable(backend, name)
    tm.alternate_root_finding = inverse == 'table'
    tm.root_finder = 'newton' if inverse == 'newton' else 'reference'
    E, D, d = tm.skip_dimensions, tm.D, tm._cm.d_cols
    star = X[:N, :E] if E else None
    Xa, logq = tm.sample(N, X_star=star, seed=SEED, draw=DRAW, logdensity=True)
    Xb = tm.sample(N, X_star=star, seed=SEED, draw=DRAW)
    assert np.array_equal(Xa, Xb, equal_nan=True)
    # the test's own composition on the device matrix of the plain inverse
    coef = tm._pack_coeffs()
    Zs, Xs = buffers(tm, star, E, N)
    if inverse == 'table':
        tm._inverse_table(coef, 0, D, Zs, Xs, N)
    else:
        tm._inverse_bisect(coef, 0, D, Zs, Xs, N)
    dev = device_of(backend)
    logdet, sumsq = torch.zeros(N, dtype=torch.float64, device=dev), torch.zeros(N, dtype=torch.float64, device=dev)
    sigma = torch.reciprocal(torch.from_numpy(np.ascontiguousarray(1.0 / np.asarray(tm.X_std, dtype=float)[E:E + D])).to(dev))
    rc = tm._lib.ttm_forward(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._ptr(Xs), Xs.shape[1], N, 0, D, None, N, tm._ptr(logdet),
                             tm._ptr(sigma), tm._ptr(sumsq), tm._stream())
    assert rc == 0
    own = (logdet - 0.5 * sumsq).cpu().numpy() - 0.5 * D * np.log(2 * np.pi)
    fin = np.isfinite(own)
    print('%s/%s %s: %d finite rows of %d, log q in [%.3f, %.3f]' % (name, inverse, backend, int(fin.sum()), N, float(own[fin].min()), float(own[fin].max())))
    assert int(fin.sum()) >= N // 2
    assert np.array_equal(logq, own, equal_nan=True)
    # the fused entry point is for integrated-rectifier maps
    lq = torch.full((N,), SENTINEL, dtype=torch.float64, device=dev)
    for newton in (0, 1):
        rc, _ = entry(tm, backend, Zs, Xs, N, newton, logq=lq)
        assert rc == E_UNSUPPORTED
    assert bool(torch.all(lq == SENTINEL))


# ------------------------------------------------------------------------------------------ 8: refusals

def test_bad_arguments_are_refused(backend):
    import torch
    tm, om, X, E = case(backend, 'spiral3', 'softplus', 'newton')
    dev = device_of(backend)
    Zs, Xs = buffers(tm, None, 0, N)
    coef = tm._pack_coeffs()
    logq = torch.full((N,), SENTINEL, dtype=torch.float64, device=dev)
    iters = torch.zeros(tm.D, dtype=torch.int32, device=dev)
    cap = torch.full((tm.D,), 5, dtype=torch.int32, device=dev)
    ld = Zs.shape[1]
    assert Xs.shape[1] == ld and ld >= N
    good = dict(coef=tm._ptr(coef), fold=tm._ptr(coef._ttm_fold), Z=tm._ptr(Zs), ldz=ld, X=tm._ptr(Xs), ldx=ld, N=N, newton=0,
                iters=ctypes.c_void_p(iters.data_ptr()), cap=None, logq=tm._ptr(logq))

    def call(**over):
        a = dict(good, **over)
        return tm._lib.ttm_inverse_logdensity(tm._pp, a['coef'], a['fold'], 0, tm.D, a['Z'], a['ldz'], a['X'], a['ldx'], a['N'], a['newton'],
                                              a['iters'], a['cap'], a['logq'], None, tm._stream())

    bad = {'null logq': dict(logq=None), 'null coef': dict(coef=None), 'null fold': dict(fold=None), 'null Z': dict(Z=None),
           'null X': dict(X=None), 'null iters': dict(iters=None), 'N = 0': dict(N=0), 'N < 0': dict(N=-3), 'ldx < N': dict(ldx=N - 1),
           'ldz < N': dict(ldz=N - 1), 'cap with newton': dict(newton=1, cap=ctypes.c_void_p(cap.data_ptr()))}
    for what, over in bad.items():
        rc = call(**over)
        print('%s %s: rc %d' % (backend, what, rc))
        assert rc == E_ARG, what
    assert bool(torch.all(logq == SENTINEL)) and int(iters.abs().sum().item()) == 0
    assert call() == 0 and call(cap=ctypes.c_void_p(cap.data_ptr())) == 0 and call(newton=1) == 0
    assert not bool(torch.any(logq == SENTINEL))


# ------------------------------------------------------------------------------------------ 9: the timing tool

@pytest.mark.gpu
def test_timing_tool_runs(tmp_path):
    """tools/sample_logdensity_bench.py in a fresh child process on a small ensemble (as tests/test_bench_tools.py runs its tools;
    the time limit ends a hang and gates no speed)."""
    out = tmp_path / 'result.json'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'sample_logdensity_bench.py'), '--workloads', 'C2a', '--rows', '65536',
                          '--launches', '4', '--rounds', '2', '--label', 'small', '--out', str(out)],
                         capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    js = json.loads(res.stdout.splitlines()[-1])
    assert js['label'] == 'small' and js['rounds'] == 2 and json.loads(out.read_text()) == js
    wl = js['workloads']['C2a']
    assert wl['N'] == 65536 and sorted(wl['methods']) == ['newton', 'reference']
    for method, m in wl['methods'].items():
        v = m['versions']
        assert sorted(v) == ['fused', 'plain', 'two_pass']
        assert all(len(x['ms_rounds']) == 2 and x['ms'] > 0 for x in v.values())
        assert v['fused']['kernel'].endswith(',logq>') and 'logq' not in v['plain']['kernel'] and v['two_pass']['kernel'] == 'k_logdensity_int'
        assert v['two_pass']['fused_x_equals_plain_x'] is True
        print('%s: fused %.4f ms, plain %.4f ms, two_pass %.4f ms, logq against two_pass %.3e on %d rows' % (
            method, v['fused']['ms'], v['plain']['ms'], v['two_pass']['ms'], v['two_pass']['max_rel_diff_of_logq_to_two_pass'], v['two_pass']['rows_compared']))
        assert v['two_pass']['max_rel_diff_of_logq_to_two_pass'] <= 1e-11
