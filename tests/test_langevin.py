"""
Langevin moves in the reference space of a fitted map: ttm_langevin_corr / k_langevin_corr, ttm_mh_step_langevin / k_mh_step<drift>
(include/ttm.h, csrc/ttm_mcmc.h) and transport_map.mcmc_device / sample_mcmc with grad_log_target_pdf, on the host test double and
on the GPU.

Expected values.  The correction is held to its DEFINITION - four Gaussian log-densities in mpmath at 50 digits, not the
simplified sum the kernel forms - within (ncols + 16) 2^-52 T, T = kappa / s^2 sum_j (|b_j d'_j| + |a_j d_j| + (kappa / 2)
(d_j^2 + d'_j^2)) the sum of the absolute values of the terms (from mpmath): each of the two running sums takes 2 ncols FMAs whose
inputs a, b, d, d' carry one rounding each, the combination three more.  The step is held to a NumPy restatement: the accept
uniforms of tests/test_mcmc.py (accept_uniform), the rule log u < beta (lp - lc) + c with the product and the sum rounded
separately, the proposal as two exact FMAs (exact_fma) of the deviates ttm_normal_fill writes on the same backend - so every
output is compared BITWISE.  A decision is compared only where |log u - (beta (lp - lc) + c)| > 64 * 2^-52 (1 + |beta (lp - lc)|
+ |c|); the seeds are chosen so that the restatement reports no such row (restatement_has_no_knife_edge_rows, which the step
test runs first), and the composition test counts its own.

The caps of the stationarity tests are conditions on a deterministic generator; the docstrings record the host double's figures.
"""
import ctypes
import json
import os
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

from tests.test_mcmc import (E_ARG, ISENT, KNIFE, ROOT, SENTINEL, accept_uniform, backend, exact_fma, gauss_host, last_kernel, make,   # noqa: F401
                             make_inputs, same_bits)

MATS = ('Zcur', 'Xcur', 'Zprop', 'Xprop', 'Znext', 'Xrec', 'Wcur', 'Wprop')
VECS = ('logw_cur', 'logw_out', 'logw_prop', 'corr')
CNTS = ('n_acc', 'n_bad')
ORDER = ('Zcur', 'ldzc', 'Xcur', 'ldxc', 'logw_cur', 'logw_out', 'Zprop', 'ldzp', 'Xprop', 'ldxp', 'logw_prop', 'Znext', 'ldzn', 'rho', 'beta', 'Xrec', 'ldxr',
         'n_acc', 'n_bad', 'N', 'ncols', 'col0', 'seed', 'draw_accept', 'draw_propose', 'row0')
DRIFT = ('Wcur', 'ldwc', 'Wprop', 'ldwp', 'corr', 'kappa')
LD_OF = {'Zcur': 'ldzc', 'Xcur': 'ldxc', 'Zprop': 'ldzp', 'Xprop': 'ldxp', 'Znext': 'ldzn', 'Xrec': 'ldxr', 'Wcur': 'ldwc', 'Wprop': 'ldwp'}


def dev_of(backend):
    return 'cpu' if backend == 'hostemu' else 'cuda'


def sync(backend):
    if backend == 'hip':
        import torch
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ ttm_langevin_corr

def corr_definition(z, w, zp, wp, rho, kappa):
    """(c, T) of one row in mpmath: c = log N(z; mu(z'), s^2) - log N(z'; mu(z), s^2) + log phi(z') - log phi(z) with
    mu(z) = rho z + kappa (z + w), and the sum T of the absolute values of the simplified form's terms."""
    with mp.workdps(50):
        rho, kappa = mp.mpf(float(rho)), mp.mpf(float(kappa))
        s2 = 1 - rho * rho
        z, w, zp, wp = ([mp.mpf(float(v)) for v in a] for a in (z, w, zp, wp))
        n = len(z)

        def log_normal(x, m, var):
            return -sum((xi - mi) ** 2 for xi, mi in zip(x, m)) / (2 * var) - mp.mpf(n) / 2 * mp.log(2 * mp.pi * var)
        d = [a + b for a, b in zip(z, w)]
        dp = [a + b for a, b in zip(zp, wp)]
        mu = [rho * a + kappa * b for a, b in zip(z, d)]
        mup = [rho * a + kappa * b for a, b in zip(zp, dp)]
        zero = [mp.mpf(0)] * n
        c = log_normal(z, mup, s2) - log_normal(zp, mu, s2) + log_normal(zp, zero, mp.mpf(1)) - log_normal(z, zero, mp.mpf(1))
        T = mp.mpf(0)
        for j in range(n):
            a, b = zp[j] - rho * z[j], z[j] - rho * zp[j]
            T += abs(b * dp[j]) + abs(a * d[j]) + abs(kappa) / 2 * (d[j] ** 2 + dp[j] ** 2)
        return c, abs(kappa) / s2 * T


def call_corr(backend, mats, N, ncols, rho, kappa, lds, offset=0, null=(), override=None):
    """ttm_langevin_corr on sentinel-padded buffers: matrix m has `offset` doubles of slack in front, ncols + 1 columns of lds[m]
    doubles.  Returns (rc, corr buffer with its padding)."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    bufs, args = {}, []
    for name in ('Zcur', 'Wcur', 'Zprop', 'Wprop'):
        ld = lds[name]
        h = np.full(offset + (ncols + 1) * ld, SENTINEL)
        h[offset:].reshape(ncols + 1, ld)[:ncols, :N] = mats[name]
        bufs[name] = torch.from_numpy(h).to(dev_of(backend))
        args += [None if name in null else ctypes.c_void_p(bufs[name].data_ptr() + 8 * offset), ld]
    out = torch.full((offset + N + 3,), SENTINEL, dtype=torch.float64, device=dev_of(backend))
    vals = dict(rho=rho, kappa=kappa, N=N, ncols=ncols, corr=None if 'corr' in null else ctypes.c_void_p(out.data_ptr() + 8 * offset))
    vals.update(override or {})
    for name, ld in (override or {}).items():
        if name in LD_OF.values():
            args[2 * ('ldzc', 'ldwc', 'ldzp', 'ldwp').index(name) + 1] = ld
    rc = lib.ttm_langevin_corr(*args, vals['rho'], vals['kappa'], vals['N'], vals['ncols'], vals['corr'], None)
    sync(backend)
    return rc, out.cpu().numpy()


def corr_inputs(N, ncols, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal((ncols, N)) * s for k, s in (('Zcur', 1.0), ('Wcur', 1.3), ('Zprop', 1.0), ('Wprop', 1.3))}


@pytest.mark.parametrize('ncols', [1, 2, 5, 40])
def test_correction_against_its_definition(backend, ncols):
    worst = 0.0
    for N in (1, 2, 257):
        for offset, (rho, kappa) in ((0, (0.7, 0.3)), (1, (-0.4, 1.4)), (0, (0.0, 1.0)), (1, (0.9, 0.05))):
            mats = corr_inputs(N, ncols, 100 * ncols + N)
            lds = dict(Zcur=N + 1, Wcur=N + 2, Zprop=N + 3, Wprop=N + 4)
            rc, out = call_corr(backend, mats, N, ncols, rho, kappa, lds, offset=offset)
            assert rc == 0
            assert np.all(out[:offset] == SENTINEL) and np.all(out[offset + N:] == SENTINEL)
            got = out[offset:offset + N]
            for n in range(N):
                ref, T = corr_definition(*(mats[k][:, n] for k in ('Zcur', 'Wcur', 'Zprop', 'Wprop')), rho, kappa)
                bound = (ncols + 16) * 2.0 ** -52 * T
                err = abs(mp.mpf(float(got[n])) - ref)
                worst = max(worst, float(err / bound))
                assert err <= bound, (N, n, rho, kappa, float(err), float(bound))
            # kappa = 0: exactly 0
            rc, out = call_corr(backend, mats, N, ncols, rho, 0.0, lds, offset=offset)
            assert rc == 0 and np.all(out[offset:offset + N] == 0.0)
    if backend == 'hip':
        from triangular_transport_toolbox_amd import _capi
        lib = _capi.load()
        lib.ttm_last_kernel.restype = ctypes.c_char_p
        assert lib.ttm_last_kernel().decode() == 'k_langevin_corr'
    print('%s ncols %d: largest |c - definition| / bound = %.3f' % (backend, ncols, worst))


def test_correction_argument_errors(backend):
    N, ncols = 10, 3
    mats = corr_inputs(N, ncols, 1)
    lds = dict(Zcur=N, Wcur=N, Zprop=N, Wprop=N)
    assert call_corr(backend, mats, N, ncols, 0.5, 0.5, lds)[0] == 0
    nan, inf = float('nan'), float('inf')
    for kw in ([dict(null=(k,)) for k in ('Zcur', 'Wcur', 'Zprop', 'Wprop', 'corr')] +
               [dict(override={k: N - 1}) for k in ('ldzc', 'ldwc', 'ldzp', 'ldwp')] +
               [dict(override=o) for o in (dict(N=0), dict(ncols=0), dict(rho=1.0), dict(rho=-1.0), dict(rho=nan), dict(kappa=nan), dict(kappa=inf))]):
        rc, out = call_corr(backend, mats, N, ncols, 0.5, 0.5, lds, **kw)
        print('%s %s: %d' % (backend, kw, rc))
        assert rc == E_ARG and np.all(out == SENTINEL), kw


# ------------------------------------------------------------------------------------------ ttm_mh_step_langevin on padded buffers

def drift_inputs(N, ncols, seed, planted=True):
    """make_inputs of tests/test_mcmc.py (its planted log-weights in rows 3 .. 8) with W matrices and a correction; N >= 16: the
    planted corrections NaN, +inf, -inf in rows 9, 10, 11."""
    inp = make_inputs(N, ncols, seed, planted=planted)
    rng = np.random.default_rng(seed + 12345)
    inp['Wcur'] = -inp['Zcur'] + 0.5 * rng.standard_normal((ncols, N))
    inp['Wprop'] = -inp['Zprop'] + 0.5 * rng.standard_normal((ncols, N))
    inp['corr'] = 0.7 * rng.standard_normal(N)
    if planted and N >= 16:
        inp['corr'][9], inp['corr'][10], inp['corr'][11] = np.nan, np.inf, -np.inf
    return inp


def step(backend, entry, inp, N, ncols, accept=True, propose=True, rho=0.0, beta=1.0, kappa=0.0, drift=True, corr=True, col0=0, row0=0, seed=0, da=1,
         dp=2, offset=0, pad=3, null=(), override=None):
    """ttm_mh_step_langevin (entry 'langevin') or ttm_mh_step_tempered ('tempered') on the sentinel-padded buffers of
    tests/test_mcmc.py: step.  drift False: Wcur, Wprop and corr are NULL.  Returns (rc, {name: whole host buffer}, {name: view})."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    ld = max(N, 1) + pad
    bufs, ptrs = {}, {}
    for name in MATS + VECS + CNTS:
        cols = ncols if name in MATS else 1
        fp = name not in CNTS
        h = np.full(offset + (cols + 1) * ld + 2, SENTINEL if fp else ISENT, dtype=np.float64 if fp else np.int32)
        if name in inp:
            h[offset:offset + (cols + 1) * ld].reshape(cols + 1, ld)[:cols, :N] = inp[name]
        t = torch.from_numpy(h).to(dev_of(backend))
        bufs[name] = t
        ptrs[name] = t.data_ptr() + (8 if fp else 4) * offset
    args = {name: ctypes.c_void_p(ptrs[name]) for name in MATS + VECS + CNTS}
    args.update({v: ld for v in LD_OF.values()})
    args.update(N=N, ncols=ncols, col0=col0, row0=row0, seed=seed, draw_accept=da, draw_propose=dp, rho=rho, beta=beta, kappa=kappa)
    if not accept:
        args.update(Zprop=None, Xprop=None, logw_prop=None, corr=None)
    if not propose:
        args.update(Znext=None)
    if not drift:
        args.update(Wcur=None, Wprop=None, corr=None)
    if not corr:
        args.update(corr=None)
    for name in null:
        args[name] = None
    args.update(override or {})
    if entry == 'tempered':
        rc = lib.ttm_mh_step_tempered(*[args[k] for k in ORDER], None)
    else:
        rc = lib.ttm_mh_step_langevin(*[args[k] for k in ORDER + DRIFT], None)
    sync(backend)
    lib.ttm_last_kernel.restype = ctypes.c_char_p
    step.kernel = lib.ttm_last_kernel().decode()                 # (of this call, when it launched)
    host, view = {}, {}
    for name, t in bufs.items():
        cols = ncols if name in MATS else 1
        host[name] = t.cpu().numpy().copy()
        view[name] = host[name][offset:offset + (cols + 1) * ld].reshape(cols + 1, ld)
    return rc, host, view


def decide(lp, lc, u, beta, c):
    """(accept, bad, knife, margin) of the rule with a correction: the product rounds, then the sum."""
    lp, lc, c = (np.asarray(a, dtype=float) for a in (lp, lc, c))
    with np.errstate(invalid='ignore'):
        bad = np.isnan(lp) | (lp == np.inf) | np.isnan(c) | (c == np.inf)
        ok = ~bad & (lp > -np.inf) & (c > -np.inf)
        t = beta * (lp - lc)
        v = t + c
        logu = np.log(u)
        accept = ok & ((lc == -np.inf) | (logu < v))
        compared = ok & (lc != -np.inf) & np.isfinite(v)
        margin = np.where(compared, np.abs(logu - v), np.inf)
        knife = margin <= KNIFE * (1.0 + np.where(compared, np.abs(t) + np.abs(c), 0.0))
    return accept, bad, knife, margin


STEP_SHAPES = [(N, row0, offset) for N in (1, 2, 3, 4099) for row0 in (0, 7) for offset in (0, 1)]
DRIFT_SHAPES = [(N, row0, offset) for N in (1, 2, 3, 1027) for row0 in (0, 7) for offset in (0, 1)]      # (the restatement's FMAs are exact rationals: kept small)
PHASES = [(True, True), (True, False), (False, True)]
SEEDS = (11, 2 ** 40 + 7)
BETAS = (1.0, 0.37)


def restatement_has_no_knife_edge_rows():
    """The inputs of the step tests: no row's comparison lies within the knife-edge margin (a condition on the seeds; no library)."""
    smallest, total = np.inf, 0
    for N, row0, offset in STEP_SHAPES + DRIFT_SHAPES:
        for seed in SEEDS:
            for beta in BETAS:
                inp = drift_inputs(N, 3, seed)
                rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
                _, _, knife, margin = decide(inp['logw_prop'], inp['logw_cur'], accept_uniform(seed, 3, rows), beta, inp['corr'])
                smallest, total = min(smallest, float(margin.min())), total + int(knife.sum())
    print('restatement: %d knife-edge rows, smallest margin %.3e' % (total, smallest))
    assert total == 0


def test_without_drift_it_is_the_tempered_step(backend):
    """W and corr NULL: every buffer - outputs, state, counts and the padding around them - holds the bits ttm_mh_step_tempered
    leaves, on the shapes check_step of tests/test_mcmc.py walks (odd row0, N = 1, col0 > 0, accept-only, propose-only); and
    that call reports the plain kernel."""
    for N, row0, offset in STEP_SHAPES:
        for rho in (0.0, 0.5):
            for accept, propose in PHASES:
                for beta in BETAS:
                    inp = drift_inputs(N, 3, 11)
                    kw = dict(accept=accept, propose=propose, rho=rho, beta=beta, col0=1, row0=row0, seed=11, da=3, dp=4, offset=offset, drift=False)
                    rc_t, host_t, _ = step(backend, 'tempered', inp, N, 3, **kw)
                    rc_l, host_l, _ = step(backend, 'langevin', inp, N, 3, kappa=0.25, **kw)
                    assert rc_t == 0 and rc_l == 0
                    for name in host_t:
                        a, b = host_t[name], host_l[name]
                        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), (name, N, row0)
                    if backend == 'hip':
                        assert step.kernel == 'k_mh_step'


def library_deviates(backend, N, ncols, col0, seed, draw, row0):
    import torch
    from triangular_transport_toolbox_amd import _capi
    Z = torch.full((ncols * N,), SENTINEL, dtype=torch.float64, device=dev_of(backend))
    assert _capi.load().ttm_normal_fill(ctypes.c_void_p(Z.data_ptr()), N, N, ncols, col0, seed, draw, row0, None) == 0
    return Z.cpu().numpy().reshape(ncols, N)


def test_step_with_drift_against_the_restatement(backend):
    restatement_has_no_knife_edge_rows()
    accepted = rows_seen = bad_seen = 0
    for N, row0, offset in DRIFT_SHAPES:
        for rho in (0.0, 0.5, -0.3):
            for accept, propose in PHASES:
                for seed, beta in zip(SEEDS, BETAS):
                    ncols, col0, da, dp = 3, 1, 3, 4
                    kappa = (1.0 - rho) * beta
                    inp = drift_inputs(N, ncols, seed)
                    rc, host, view = step(backend, 'langevin', inp, N, ncols, accept=accept, propose=propose, rho=rho, beta=beta, kappa=kappa, col0=col0,
                                          row0=row0, seed=seed, da=da, dp=dp, offset=offset)
                    assert rc == 0
                    if backend == 'hip':
                        assert step.kernel == 'k_mh_step<drift>'
                    rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
                    if accept:
                        acc, bad, knife, _ = decide(inp['logw_prop'], inp['logw_cur'], accept_uniform(seed, da, rows), beta, inp['corr'])
                    else:
                        acc, bad, knife = (np.zeros(N, bool) for _ in range(3))
                    assert int(knife.sum()) == 0
                    post = {k: np.where(acc, inp[k.replace('cur', 'prop')], inp[k]) for k in ('Zcur', 'Xcur', 'Wcur')}
                    assert np.array_equal(view['n_acc'][0, :N] - inp['n_acc'], acc.astype(np.int32)), 'decisions'
                    assert np.array_equal(view['n_bad'][0, :N] - inp['n_bad'], bad.astype(np.int32))
                    for k in post:
                        assert same_bits(view[k][:ncols, :N], post[k]), k
                    assert same_bits(view['logw_out'][0, :N], np.where(acc, inp['logw_prop'], inp['logw_cur']))
                    assert same_bits(view['Xrec'][:ncols, :N], post['Xcur'])
                    for name in ('Zprop', 'Xprop', 'Wprop', 'logw_cur', 'logw_prop', 'corr'):
                        cols = ncols if name in MATS else 1
                        assert same_bits(view[name][:cols, :N], np.reshape(inp[name], (cols, N))), name
                    if propose:
                        xi = library_deviates(backend, N, ncols, col0, seed, dp, row0)
                        s = np.sqrt((1.0 - rho) * (1.0 + rho))
                        ref = exact_fma(rho, post['Zcur'], exact_fma(kappa, post['Zcur'] + post['Wcur'], s * xi))
                        assert same_bits(view['Znext'][:ncols, :N], ref), (N, row0, rho)
                    else:
                        assert np.all(view['Znext'] == SENTINEL)
                    for name in host:                                                   # nothing outside rows [0, N) of the columns in use
                        cols = ncols if name in MATS else 1
                        sent = ISENT if name in CNTS else SENTINEL
                        assert np.all(host[name][:offset] == sent) and np.all(host[name][-2:] == sent) and np.all(view[name][:cols, N:] == sent) \
                            and np.all(view[name][cols] == sent), name
                    if accept and N == 1027:
                        accepted, rows_seen, bad_seen = accepted + int(acc.sum()), rows_seen + N, bad_seen + int(bad.sum())
    print('%s: %d of %d rows accepted (%.3f), %d bad' % (backend, accepted, rows_seen, accepted / rows_seen, bad_seen))
    assert 0.2 < accepted / rows_seen < 0.8
    assert bad_seen == 4 * (rows_seen // 1027)                  # (lp NaN, lp +inf, c NaN, c +inf per call)


def test_step_argument_errors(backend):
    N, ncols = 10, 2
    inp = drift_inputs(N, ncols, 1, planted=False)
    assert step(backend, 'langevin', inp, N, ncols, rho=0.5, kappa=0.5)[0] == 0
    assert step(backend, 'langevin', inp, N, ncols, rho=0.5, kappa=0.5, corr=False)[0] == 0          # (no correction: the plain rule)
    nan, inf = float('nan'), float('inf')
    cases = [dict(null=('Wcur',)), dict(null=('Wprop',)), dict(null=('Wcur', 'Wprop')),               # (the last: corr without W)
             dict(override={'ldwc': N - 1}), dict(override={'ldwp': N - 1}), dict(accept=False, override={'corr': ctypes.c_void_p(8)}),
             dict(kappa=nan), dict(kappa=inf), dict(kappa=-inf), dict(beta=0.0), dict(rho=1.0), dict(null=('Zcur',))]
    for kw in cases:
        rc, host, view = step(backend, 'langevin', inp, N, ncols, **dict(dict(rho=0.5, kappa=0.5), **kw))
        print('%s %s: %d' % (backend, kw, rc))
        assert rc == E_ARG, kw
        for name in ('Zcur', 'Xcur', 'Wcur', 'n_acc', 'n_bad'):
            cols = ncols if name in MATS else 1
            assert np.array_equal(view[name][:cols, :N], np.reshape(inp[name], (cols, N))), (kw, name)
        for name in ('logw_out', 'Znext', 'Xrec'):
            assert np.all(host[name] == SENTINEL), (kw, name)


# ------------------------------------------------------------------------------------------ the class

def gauss_device(tm, k0=0):
    """(target, gradient) of N(X_mean, diag(X_std^2)) in the device convention."""
    mu = tm._to_dev(np.asarray(tm.X_mean, dtype=float))[k0:, None]
    sd = tm._to_dev(np.asarray(tm.X_std, dtype=float))[k0:, None]
    return (lambda raw: -0.5 * (((raw - mu) / sd) ** 2).sum(dim=0)), (lambda raw: -(raw - mu) / (sd * sd))


def gauss_grad_host(mu, sd):
    return lambda X: -(X - mu) / (sd * sd)


def test_composition(backend):
    """mcmc_device with a gradient against the same chain put together from reference_device, inverse_device(logq=True),
    pull_gradient_device, ttm_langevin_corr and the decision in NumPy: bit for bit on the trace, Z, X and W; the log-weights to
    1e-12 (the bound of tests/test_mcmc.py: test_composition)."""
    import torch
    tm, _ = make('c3_sep')
    N, steps, rho, seed, draw0 = 513, 6, 0.6, 77, 40
    D, ld = tm.D, 514
    target, grad = gauss_device(tm)
    trace, state = tm.mcmc_device(target, N, steps, rho=rho, seed=seed, draw=draw0, grad_log_target_pdf=grad)
    assert last_kernel(tm) == ('hostemu' if backend == 'hostemu' else 'k_mh_step<drift>')
    assert tuple(trace.shape) == (steps, D, ld) and tuple(state['W'].shape) == (D, ld)
    g_scale = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float))
    sigma = tm._to_dev(np.asarray(tm.X_std, dtype=float))
    const = 0.5 * D * np.log(2 * np.pi)
    kappa = 1.0 - rho
    s = float(np.sqrt((1.0 - rho) * (1.0 + rho)))
    rows = np.arange(N, dtype=np.uint64)

    def invert(Zdev):
        Xd, logq = tm.inverse_device(Zdev, N, logq=True, g_scale=g_scale)
        raw = Xd[:D, :N] * tm._std_d[:D, None] + tm._mean_d[:D, None]
        logw = target(raw).reshape(N).to(torch.float64) - (logq[:N] - const)
        G = tm._cols(D, N, zero=True)
        G[:, :N].copy_(grad(raw))
        W = tm.pull_gradient_device(Xd, N, G, g_scale=sigma, logdet=True)
        return Xd[:, :N].cpu().numpy().copy(), logw.cpu().numpy().copy(), W

    def to_dev(a):
        t = tm._cols(D, N, zero=True)
        t[:, :N].copy_(torch.from_numpy(np.ascontiguousarray(a)))
        return t
    Zdev = tm.reference_device(N, seed=seed, draw=draw0)
    Z = Zdev[:, :N].cpu().numpy().copy()
    X, logw, Wdev = invert(Zdev)
    W = Wdev[:, :N].cpu().numpy().copy()
    n_acc = np.zeros(N, dtype=np.int64)
    excluded, smallest = 0, np.inf
    for t in range(1, steps + 1):
        xi = tm.reference_device(N, seed=seed, draw=draw0 + t)[:, :N].cpu().numpy()
        Zp = exact_fma(rho, Z, exact_fma(kappa, Z + W, s * xi))
        Zp_dev = to_dev(Zp)
        Xp, logwp, Wp_dev = invert(Zp_dev)
        Wp = Wp_dev[:, :N].cpu().numpy().copy()
        c = tm._empty(N)
        Zc_dev, Wc_dev = to_dev(Z), to_dev(W)
        assert tm._lib.ttm_langevin_corr(tm._ptr(Zc_dev), ld, tm._ptr(Wc_dev), ld, tm._ptr(Zp_dev), ld, tm._ptr(Wp_dev), ld, rho, kappa, N, D, tm._ptr(c),
                                         tm._stream()) == 0
        acc, bad, knife, margin = decide(logwp, logw, accept_uniform(seed, draw0 + t, rows), 1.0, c.cpu().numpy())
        excluded, smallest = excluded + int(knife.sum()), min(smallest, float(margin.min()))
        assert not bad.any()
        Z, X, W, logw = np.where(acc, Zp, Z), np.where(acc, Xp, X), np.where(acc, Wp, W), np.where(acc, logwp, logw)
        n_acc += acc
        assert same_bits(trace[t - 1][:, :N].cpu().numpy(), X), t
    print('%s: %d rows excluded, smallest margin %.3e, acceptance rate %.3f' % (backend, excluded, smallest, n_acc.mean() / steps))
    assert excluded == 0
    assert np.array_equal(state['n_acc'].cpu().numpy(), n_acc)
    for key, ref in (('Z', Z), ('X', X), ('W', W)):
        assert same_bits(state[key][:, :N].cpu().numpy(), ref), key
    err = float(np.max(np.abs(state['logw'].cpu().numpy() - logw)))
    print('%s: final log-weights, max |a - b| = %.3e' % (backend, err))
    assert err <= 1e-12
    assert 0.05 < n_acc.mean() / steps < 0.999


def test_continuation(backend):
    """3 + 3 steps = 6 steps, bit for bit (trace, Z, X, W, log-weights, counts); a state without W continued with a gradient
    computes it once and then runs the Langevin chain from that state; a state with W continued without a gradient ignores it."""
    tm, _ = make('c3_sep')
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    target, grad = gauss_host(mu, sd), gauss_grad_host(mu, sd)
    N, seed = 257, 3
    kw = dict(rho=0.6, seed=seed, grad_log_target_pdf=grad)
    X, info = tm.sample_mcmc(target, N, 6, draw=5, **kw)
    Xa, infoa = tm.sample_mcmc(target, N, 3, draw=5, **kw)
    assert 'W' in infoa['state']
    Xb, infob = tm.sample_mcmc(target, N, 3, init=infoa['state'], **dict(kw, seed=0))
    assert infob['draws'] == (8, 11)
    assert same_bits(np.concatenate((Xa, Xb)), X) and same_bits(infob['logw'], info['logw'])
    for key in ('Z', 'X', 'W'):
        assert same_bits(infob['state'][key][:, :N].cpu().numpy(), info['state'][key][:, :N].cpu().numpy()), key
    assert np.array_equal(infob['accept_rate'], info['accept_rate']) and np.array_equal(infob['n_bad'], info['n_bad'])
    rate = float(info['accept_rate'].mean())
    print('%s: acceptance rate %.3f' % (backend, rate))
    assert 0.05 < rate < 0.999
    # a plain run's state, continued with a gradient: the W of its rows, computed once - the state that run's Langevin
    # continuation from (Z, X, logw, W) takes
    Xp, infop = tm.sample_mcmc(target, N, 3, rho=0.6, seed=seed, draw=5)
    assert 'W' not in infop['state']
    Xc, infoc = tm.sample_mcmc(target, N, 2, init=infop['state'], rho=0.6, grad_log_target_pdf=grad)
    Xs = tm._import(Xp[-1], True)
    G = tm._import(grad(Xp[-1]), False)
    W0 = tm.pull_gradient_device(Xs, N, G, g_scale=tm._to_dev(sd), logdet=True)
    Xd, infod = tm.sample_mcmc(target, N, 2, init=dict(infop['state'], W=W0), rho=0.6, grad_log_target_pdf=grad)
    werr = float(np.max(np.abs(infoc['state']['W'][:, :N].cpu().numpy() - infod['state']['W'][:, :N].cpu().numpy())))
    print('%s: W computed from the state against W from the exported rows, after two steps: max difference %.3e' % (backend, werr))
    assert Xc.shape == (2, N, tm.D) and 'W' in infoc['state'] and np.all(np.isfinite(Xc))
    # a Langevin state continued without a gradient: the plain chain from (Z, X, logw)
    plain = {k: v for k, v in infoa['state'].items() if k != 'W'}
    Xe, infoe = tm.sample_mcmc(target, N, 2, init=infoa['state'], rho=0.6)
    Xf, infof = tm.sample_mcmc(target, N, 2, init=plain, rho=0.6)
    assert same_bits(Xe, Xf) and 'W' not in infoe['state']


def stationarity(tm, backend, run):
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    n, steps = 8192, 30
    x0 = mu + sd * np.random.default_rng(2024).standard_normal((n, tm.D))
    X, info = run(n, steps, x0)
    assert X.shape == (1, n, tm.D)
    y = (X[0] - mu) / sd
    e1 = np.sqrt(n) * y.mean(axis=0)
    e2 = np.sqrt(n / 2.0) * ((y ** 2).mean(axis=0) - 1.0)
    rate = float(info['accept_rate'].mean())
    moved = float(np.mean(np.any(X[0] != x0, axis=1)))
    print('%s: standardised errors of the means %s, of the second moments %s; acceptance rate %.4f; chains that moved %.4f'
          % (backend, ' '.join('%.2f' % v for v in e1), ' '.join('%.2f' % v for v in e2), rate, moved))
    assert np.all(info['n_bad'] == 0)
    assert np.max(np.abs(e1)) <= 4.5 and np.max(np.abs(e2)) <= 4.5
    assert 0.05 < rate < 0.999


def test_stationarity(backend):
    """The design of tests/test_mcmc.py: test_stationarity with Langevin moves - c3_sep with the Newton inverse, target
    N(X_mean, diag(X_std^2)), 8192 chains started IN the target (np.random.default_rng(2024)), 30 steps at rho = 0.7, seed 1,
    draws 0 .. 30; caps as there: every standardised error <= 4.5, acceptance strictly between 0.05 and 0.999, n_bad == 0.  (A
    wrong correction shows: without c the moments of a Gaussian toy are 60 to 350 sigma off after 30 steps.)
    The host double gives 1.60 1.24 0.55 0.59 for the means and 0.83 -1.56 -0.93 0.10 for the second moments at an acceptance rate
    of 0.634 (0.385 without the gradient; 99 % of the chains have moved)."""
    tm, _ = make('c3_sep', alternate_root_finding=False, root_finder='newton')
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    stationarity(tm, backend, lambda n, steps, x0: tm.sample_mcmc(gauss_host(mu, sd), n, steps, rho=0.7, seed=1, draw=0, init=x0, burn=steps - 1,
                                                                  grad_log_target_pdf=gauss_grad_host(mu, sd)))


def test_stationarity_with_autograd(backend):
    """The same run with the device convention and grad_log_target_pdf = 'autograd' (torch differentiates the target on either
    backend's tensors).
    The host double gives the figures of test_stationarity digit for digit."""
    tm, _ = make('c3_sep', alternate_root_finding=False, root_finder='newton')
    target, _ = gauss_device(tm)
    stationarity(tm, backend, lambda n, steps, x0: tm.sample_mcmc(target, n, steps, rho=0.7, seed=1, draw=0, init=x0, burn=steps - 1, target_on_device=True,
                                                                  grad_log_target_pdf='autograd'))


def test_python_argument_errors(backend):
    import torch
    tm, Xtrain = make('c3_sep')
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    target, grad = gauss_host(mu, sd), gauss_grad_host(mu, sd)
    X, info = tm.sample_mcmc(target, 16, 4, seed=1, draw=0, grad_log_target_pdf=grad)
    assert X.shape == (4, 16, tm.D) and tuple(info['state']['W'].shape) == (tm.D, 16)
    with pytest.raises(ValueError, match='autograd'):
        tm.sample_mcmc(target, 16, 4, draw=0, grad_log_target_pdf='autograd')
    with pytest.raises(ValueError, match='grad_log_target_pdf'):
        tm.sample_mcmc(target, 16, 4, draw=0, grad_log_target_pdf=lambda X: grad(X)[:, :-1])
    with pytest.raises(ValueError, match='grad_log_target_pdf'):
        tm.sample_mcmc(target, 16, 4, draw=0, grad_log_target_pdf=lambda X: grad(X)[:15])
    dtarget, dgrad = gauss_device(tm)
    with pytest.raises(ValueError, match='grad_log_target_pdf'):
        tm.sample_mcmc(dtarget, 16, 4, draw=0, target_on_device=True, grad_log_target_pdf=lambda raw: dgrad(raw)[:, :15])
    with pytest.raises(ValueError, match='grad_log_target_pdf'):
        tm.mcmc_device(dtarget, 16, 4, draw=0, grad_log_target_pdf='finite differences')
    # a non-finite initial W
    with pytest.raises(ValueError, match='initial'):
        tm.sample_mcmc(target, 16, 4, draw=0, grad_log_target_pdf=lambda X: np.where(np.arange(16)[:, None] == 3, np.nan, grad(X)))
    # a state whose W is not the state's
    with pytest.raises(ValueError, match='state'):
        tm.sample_mcmc(target, 16, 2, init=dict(info['state'], W=torch.zeros(tm.D, 18, dtype=torch.float64, device=tm._dev)), grad_log_target_pdf=grad)
    # maps without a univariate form
    tmi, _ = make('c2a_int')
    with pytest.raises(NotImplementedError, match='integrated'):
        tmi.sample_mcmc(lambda X: -0.5 * np.sum(X ** 2, axis=1), 16, 2, draw=0, grad_log_target_pdf=lambda X: -X)
    assert tm._draws == 0


# ------------------------------------------------------------------------------------------ the timing tool

@pytest.mark.gpu
def test_timing_tool_runs(tmp_path):
    """tools/langevin_bench.py in a fresh child process on small shapes (as tests/test_mcmc.py: test_timing_tool_runs; the time
    limit ends a hang and gates no speed)."""
    out = tmp_path / 'result.json'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'langevin_bench.py'), '--workloads', 'C2b', '--rows', '65536', '--launches', '4',
                          '--rounds', '2', '--chain-workloads', 'C2b', '--chains', '4096', '--steps', '3', '--rhos', '0.7', '--label', 'small',
                          '--out', str(out)], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    js = json.loads(res.stdout.splitlines()[-1])
    assert js['label'] == 'small' and js['rounds'] == 2 and json.loads(out.read_text()) == js
    wl = js['workloads']['C2b']
    v = wl['versions']
    assert wl['N'] == 65536 and wl['ncols'] == 2
    assert sorted(v) == ['langevin_corr', 'mh_step_langevin', 'mh_step_tempered', 'pull_gradient', 'score_band', 'score_u']
    assert all(len(x['ms_rounds']) == 2 and x['ms'] > 0 for x in v.values())
    assert v['pull_gradient']['kernel'] == 'k_pull_gradient_u' and v['score_u']['kernel'] == 'k_score_u' and v['langevin_corr']['kernel'] == 'k_langevin_corr'
    assert v['mh_step_langevin']['kernel'] == 'k_mh_step<drift>' and v['mh_step_tempered']['kernel'] == 'k_mh_step'
    chain = js['chains']['cases']['C2b']['0.7']
    print('pull %.4f ms, score_u %.4f ms; chains %.3f / %.3f ms per step with / without the gradient, acceptance %.3f / %.3f'
          % (v['pull_gradient']['ms'], v['score_u']['ms'], chain['langevin']['ms_per_step'], chain['plain']['ms_per_step'],
             chain['langevin']['accept_rate'], chain['plain']['accept_rate']))
    assert 0.0 < chain['langevin']['accept_rate'] <= 1.0 and chain['langevin']['msj'] > 0
