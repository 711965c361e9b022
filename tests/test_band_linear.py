"""
Long banded separable maps (more than P_FEW_D components) whose monotone parts carry ONE linear term [k] of the own
variable next to the special-term spline, or instead of it: the order-1 transport filter (monotone [[k]]), example 05's
parameterisation ([k] + iRBFs) stretched to many components, and mixes of both with spline-only components.  Such maps
are planned as banded with lag-2 push records and run on k_band_forward / k_band_density / k_band_logdet /
k_band_inverse(_ring) / k_band_newton (csrc/ttm_band.hip); their hot records carry H_NG_MAX group slots and only feed the
push records, so neither the hot-record kernels nor the host test double's hot sweep take them.

The maps are built as tests/test_band.py::_build builds its own (n = 5003: a full and a partial tile of 4096 rows, an odd
tail); all tolerances are that file's.
"""
import ctypes

import numpy as np
import pytest

from tests.util import relerr


def _nonmon(D, band, hf_order, plain_order):
    non = []
    for k in range(D):
        nm = [[]]
        for j in range(max(0, k - band), k):
            for o in range(1, plain_order + 1):
                nm.append([j] * o)
            for o in range(2, hf_order + 1):
                nm.append([j] * o + ['HF'])
        non.append(nm)
    return non


def _linear_only():
    return [[[k]] for k in range(6)], _nonmon(6, 2, 3, 1)


def _linear_plus_st(D=5, hf_order=3, plain_order=1):
    return [[[k], 'iRBF %d' % k, 'iRBF %d' % k] for k in range(D)], _nonmon(D, 2, hf_order, plain_order)


def _mixed(D=7):
    kinds = (lambda k: ['LET %d' % k, 'iRBF %d' % k, 'RET %d' % k],          # spline only: own1 == 0
             lambda k: [[k]],                                                 # linear only: NI == 0
             lambda k: [[k], 'iRBF %d' % k, 'iRBF %d' % k])                   # both
    return [kinds[k % 3](k) for k in range(D)], _nonmon(D, 2, 3, 1)


CASES = {
    'linear_only': dict(D=6, spec=_linear_only, cls=1),
    'linear_plus_st': dict(D=5, spec=_linear_plus_st, cls=1),
    'mixed': dict(D=7, spec=_mixed, cls=1),
    'class_55': dict(D=5, spec=lambda: _linear_plus_st(5, 5, 3), cls=2),
    # ten components: a sweep that starts inside the map still has more than P_FEW_D of them (the long kernels' column prologue)
    'mixed_long': dict(D=10, spec=lambda: _mixed(10), cls=1),
}
SETTINGS = ((-1, -1), (1, -1), (3, 2), (2, 1))      # (band_cus, rt_block): one tile per chunk | several tiles | several blocks


def _build(case, n=5003, seed=0, **ctor):
    from triangular_transport_toolbox_amd.transport_map import transport_map
    from oracle.ttm_oracle import OracleMap
    c = CASES[case]
    d = c['D']
    rng = np.random.default_rng(seed + 17 * d)
    X = rng.standard_normal((n, d)) @ (np.tril(rng.standard_normal((d, d)) * 0.4) + np.eye(d)).T + 0.3 * rng.standard_normal((n, d)) ** 2
    mon, non = c['spec']()
    kw = dict(monotonicity='separable monotonicity')
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, **kw, **ctor)
    om = OracleMap(X=X, monotone=mon, nonmonotone=non, **kw)
    for k in range(d):
        cm_ = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
        cn_ = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        tm.coeffs_mon[k], om.coeffs_mon[k] = cm_.copy(), cm_.copy()
        tm.coeffs_nonmon[k], om.coeffs_nonmon[k] = cn_.copy(), cn_.copy()
    return tm, om, X, rng


def _targets(rng, N, D):
    Zin = rng.standard_normal((N, D))
    Zin[:40] *= 3.5                                         # (targets beyond the resident window and beyond the tables)
    return Zin


def _last(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


def _forward_from(tm, k0, dens):
    """ttm_forward of the components [k0, D) on the training samples: Z, and with `dens` the log-determinant and the sum of
    squares of the same launch; the kernel's name."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    N, D = tm._N, tm.D
    coef = tm._pack_coeffs()
    Z = tm._cols(D - k0, N)
    ld, ss = (tm._empty(N), tm._empty(N)) if dens else (None, None)
    _capi.check(tm._lib.ttm_forward(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._ptr(tm._Xs), tm._Xs.shape[1], N, k0, D,
                                    tm._ptr(Z), Z.shape[1], tm._ptr(ld), None, tm._ptr(ss), tm._stream()))
    torch.cuda.synchronize()
    out = [Z[:, :N].T.cpu().numpy()] + ([ld[:N].cpu().numpy(), ss[:N].cpu().numpy()] if dens else [])
    return out, _last(tm)


# ---------------------------------------------------------------------------
# CPU: the plan, and the unchanged host test double on these maps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(CASES))
def test_long_maps_with_linear_own_terms_are_planned_as_banded(case):
    from tests.hostemu import emu
    from triangular_transport_toolbox_amd import termtable
    with emu.install():
        tm, om, X, rng = _build(case, n=400)
        cm = tm._cm
        assert cm.D > termtable.P_FEW_D
        assert cm.u_enabled and cm.u_p_lag == 2 and cm.u_h_cls == CASES[case]['cls']
        gp = termtable.H_DB[cm.u_h_cls] + 1 + termtable.H_DA[cm.u_h_cls]
        assert cm.u_p_stride == -(-(termtable.P_HDR + 2 * gp) // 8) * 8       # (ttm_band::record_stride(cls, 2))
        # hot records that no hot-record kernel (and no hot sweep of the host double) is instantiated for
        assert cm.u_h_ng == termtable.H_NG_MAX
        assert cm.u_p_off % 8 == 0 and cm.u_p_off >= cm.u_h_off + cm.D * (termtable.H_HDR + cm.u_h_ng * termtable.H_GS[cm.u_h_cls])
        assert cm.u_size >= cm.u_p_off + (cm.D + cm.u_p_lag) * cm.u_p_stride
        nI = cm.ucomp[:cm.D * termtable.UC_LEN].reshape(-1, termtable.UC_LEN)[:, 4]
        if case == 'linear_only':
            assert not nI.any()
        if case in ('mixed', 'mixed_long'):
            assert [bool(v) for v in nI] == [k % 3 != 1 for k in range(cm.D)]


@pytest.mark.parametrize('own', [['k', 'k', 'k', 'HF'], ['k', 'k']])
def test_other_own_terms_of_a_long_map_are_still_not_banded(own):
    from tests.hostemu import emu
    from triangular_transport_toolbox_amd.transport_map import transport_map
    with emu.install():
        D = 5
        mon = [[[k], [k if e == 'k' else e for e in own], 'iRBF %d' % k] for k in range(D)]
        X = np.random.default_rng(4).standard_normal((300, D))
        tm = transport_map(X=X, monotone=mon, nonmonotone=_nonmon(D, 2, 3, 1), verbose=False, monotonicity='separable monotonicity')
        assert tm._cm.u_p_lag == 0


@pytest.mark.parametrize('case', sorted(CASES))
def test_host_double_on_long_maps_with_linear_own_terms_against_the_oracle(case):
    """The double sweeps hot records where it has an evaluator for their shape; these maps' records have no own term, so it
    must fall through to its U-form evaluator and the generic table lookup."""
    from tests.hostemu import emu
    with emu.install():
        tm, om, X, rng = _build(case, n=600)
        D = tm.D
        assert tm._cm.u_p_lag == 2
        assert relerr(tm.map(X), om.map(X)) < 1e-11
        with np.errstate(all='ignore'):
            pref = om.evaluate_pullback_density(X[:400])
        pgot = tm.evaluate_pullback_density(X[:400])
        ok = np.isfinite(pref)
        assert ok.sum() > 300 and np.array_equal(np.isfinite(pgot), ok) and relerr(pgot[ok], pref[ok]) < 1e-10
        Zin = _targets(rng, len(X), D)
        assert relerr(tm.inverse_map(Zin), om.inverse_map(Zin)) < 1e-11
        assert relerr(tm.inverse_map(Zin[:, 1:], X_star=X[:, :1]), om.inverse_map(Zin[:, 1:], X_star=X[:, :1])) < 1e-11


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_band_kernels_of_long_maps_with_linear_own_terms(case, ttm_opt):
    import torch
    tm, om, X, rng = _build(case)
    D, N = tm.D, len(X)
    Zo = om.map(X)
    with np.errstate(all='ignore'):
        pref = om.evaluate_pullback_density(X[:400])
    ok = np.isfinite(pref)
    Zin = _targets(rng, N, D)
    E = 1
    Xo = om.inverse_map(Zin)
    Xco = om.inverse_map(Zin[:, E:], X_star=X[:, :E])
    Xs = (X - om.X_mean) / om.X_std
    so = {k: om.s(Xs, k) for k in sorted({0, D // 2, D - 1})}
    # the kernels the band kernels replace
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 0); ttm_opt('band_inv', 0)
    Zh = tm.map(X)
    tm.forward_device(tm._Xs, tm._N)
    assert _last(tm) in ('k_forward_ul', 'k_forward_u')     # (never the hot-record kernel: its records have no own term)
    Xh = tm.inverse_map(Zin)
    tm.inverse_device(tm._cols(D, tm._N, zero=True), tm._N)
    assert _last(tm) == 'k_inverse_table'
    Xch = tm.inverse_map(Zin[:, E:], X_star=X[:, :E])
    ph = tm.evaluate_pullback_density(X[:400])
    k_mid = 3 if D - 3 > 4 else None                          # a sweep from inside the map that the long kernels take
    if k_mid:
        (Zmh,), _ = _forward_from(tm, k_mid, False)
        (_, ldmh, ssmh), _ = _forward_from(tm, k_mid, True)
    maps, ring, blk = [], [], []
    for cus, block in SETTINGS:
        ttm_opt('band_fwd', 1); ttm_opt('band_inv', 1); ttm_opt('band_cus', cus); ttm_opt('rt_block', block)
        Z = tm.map(X)
        maps.append(Z)
        tm.forward_device(tm._Xs, tm._N)
        assert _last(tm) == 'k_band_forward'
        assert relerr(Z, Zo) < 1e-11, (cus, block)
        assert relerr(Z, Zh) < 1e-12
        ld, ss = tm._empty(tm._N), tm._empty(tm._N)
        tm.forward_device(tm._Xs, tm._N, logdet=ld, sumsq=ss)
        assert _last(tm) == 'k_band_density'
        torch.cuda.synchronize()
        assert relerr(ss.cpu().numpy(), np.sum(Zo ** 2, axis=1)) < 1e-11
        ld2 = tm._empty(tm._N)
        tm.density_device(tm._Xs, tm._N, logdet=ld2)
        assert _last(tm) == 'k_band_logdet'
        torch.cuda.synchronize()
        assert relerr(ld2.cpu().numpy(), ld.cpu().numpy()) < 1e-12         # (fused pass against the log-det-only pass)
        ld3, ss3 = tm._empty(tm._N), tm._empty(tm._N)
        tm.density_device(tm._Xs, tm._N, logdet=ld3, sumsq=ss3)             # (the fused pass without Z)
        assert _last(tm) == 'k_band_density'
        torch.cuda.synchronize()
        assert relerr(ld3.cpu().numpy(), ld.cpu().numpy()) < 1e-12 and relerr(ss3.cpu().numpy(), ss.cpu().numpy()) < 1e-12
        pgot = tm.evaluate_pullback_density(X[:400])
        assert np.array_equal(np.isfinite(pgot), ok) and relerr(pgot[ok], pref[ok]) < 1e-10 and relerr(pgot[ok], ph[ok]) < 1e-12
        for k, ref in so.items():                             # sweeps that start inside the map: the columns in front are pushed first
            assert relerr(tm.s(Xs, k), ref) < 1e-12
        if k_mid:                                             # ... and one with more than P_FEW_D components left: the long kernels' prologue
            (Zm,), name = _forward_from(tm, k_mid, False)
            assert name == 'k_band_forward'
            assert relerr(Zm, Zo[:, k_mid:]) < 1e-11 and relerr(Zm, Zmh) < 1e-12
            (Zm, ldm, ssm), name = _forward_from(tm, k_mid, True)
            assert name == 'k_band_density'
            assert relerr(Zm, Zo[:, k_mid:]) < 1e-11 and relerr(ssm, np.sum(Zo[:, k_mid:] ** 2, axis=1)) < 1e-11
            assert relerr(ldm, ldmh) < 1e-12 and relerr(ssm, ssmh) < 1e-12
        for r in (0, 1):
            ttm_opt('band_ring', r)
            tm._pack_memo = None                              # (a fresh coefficient vector: tables and images under these options)
            Xi = tm.inverse_map(Zin)
            (ring if r else blk).append(Xi)
            tm.inverse_device(tm._cols(D, tm._N, zero=True), tm._N)
            name = _last(tm)
            # (a ring needs twelve slots, or every component resident: rt_block = 2 / 1 leaves the block kernel)
            assert name == ('k_band_inverse_ring' if r and block < 0 else 'k_band_inverse'), (cus, block, r, name)
            assert relerr(Xi, Xo) < 1e-11, (cus, block, r)
            assert relerr(Xi, Xh) < 1e-11
            Xc = tm.inverse_map(Zin[:, E:], X_star=X[:, :E])
            assert relerr(Xc, Xco) < 1e-11 and relerr(Xc, Xch) < 1e-11
        ttm_opt('band_ring', -1)
    # the bits do not depend on how the rows are cut into chunks and tiles or the components into blocks
    for Z in maps[1:]:
        assert np.array_equal(Z, maps[0])
    for Xi in ring[1:]:
        assert np.array_equal(Xi, ring[0])
    for Xi in blk[1:]:
        # (a tile that re-reads its columns at a block boundary takes exp(-x^2/4) there from the series, not the interval)
        assert relerr(Xi, blk[0]) < 1e-14


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_newton_inverse_of_long_maps_with_linear_own_terms(case, ttm_opt):
    import torch
    from tests.test_band_newton import _newton, _padded
    tm, om, X, rng = _build(case, root_finder='newton', alternate_root_finding=False)
    D, N = tm.D, tm._N
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    Zs = tm.forward_device(tm._Xs, N).clone()
    tm.inverse_device(Zs, N)
    assert _last(tm) == 'k_band_newton'
    res = {}
    for cus, block in SETTINGS:
        ttm_opt('band_cus', cus); ttm_opt('rt_block', block)
        Xb, itb, name = _newton(tm, Zs, N)
        assert name == 'k_band_newton'
        res[(cus, block)] = (Xb[:, :N].clone(), itb)
    ttm_opt('band_cus', -1); ttm_opt('rt_block', -1)
    Xb, itb = res[(-1, -1)]
    for key, (Xk, itk) in res.items():                        # rows do not notice the chunking or the residency blocks
        assert torch.equal(Xk, Xb) and np.array_equal(itk, itb), key
    ttm_opt('band_newton', 0)
    Xg, itg, name = _newton(tm, Zs, N)
    assert name == 'k_inverse_newton'
    Xg = Xg[:, :N].clone()
    ttm_opt('band_newton', -1)
    sane = (Xg.abs() < 50.0).all(dim=0)
    assert float(sane.double().mean()) > 0.99
    # residual |S(x) - z| under the oracle's map and under the library's
    Xraw = (Xb.T.cpu().numpy() * om.X_std + om.X_mean)
    keep = sane.cpu().numpy()
    assert np.abs(om.map(Xraw) - Zs[:, :N].T.cpu().numpy())[keep].max() <= 2e-9
    assert float((tm.forward_device(_padded(tm, Xb, N), N)[:, :N] - Zs[:, :N]).abs()[:, sane].max().item()) <= 2e-9
    assert float(((Xb - Xg).abs() / (1 + Xg.abs()))[:, sane].max().item()) < 1e-6
    print(case, 'trial points', itb.tolist(), 'generic', itg.tolist())
    # (the bounds of tests/test_band_newton.py; a linear monotone part - bracket, secant start, done - is where a search
    # that did not use the slope would show)
    assert itb.max() <= 25 and np.all(itb <= itg + 2)
    # rows are independent: exact under a permutation
    perm = torch.from_numpy(np.random.default_rng(3).permutation(N)).to(Zs.device)
    Zp = tm._cols(D, N)
    Zp[:, :N].copy_(Zs[:, :N][:, perm])
    Xp, _, _ = _newton(tm, Zp, N)
    assert torch.equal(Xp[:, :N], Xb[:, perm])
    # the public path: no tables, the round trip of the whole ensemble
    got = tm.inverse_map(tm.map(X))
    assert not getattr(tm._pack_coeffs(), '_ttm_tables', None)
    assert float(np.max(np.abs(got - X) / tm.X_std)) < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['linear_only', 'linear_plus_st', 'mixed'])
def test_density_pass_with_a_negative_linear_slope_is_nan_where_the_reference_is(case, ttm_opt):
    """As test_band.py::test_density_pass_with_negative_derivatives_is_nan_where_the_reference_is.  The derivative of a
    component without a spline is its slope: every row is NaN.  Next to iRBF terms a negative slope makes the derivative
    negative only away from their centres: rows of both kinds, and the mask has to match row by row."""
    import torch
    tm, om, X, rng = _build(case, n=3001)
    # (component 2 has the linear term in all three maps; next to iRBF terms a slope the Gaussians outweigh near their centres)
    tm.coeffs_mon[2][0] = om.coeffs_mon[2][0] = -0.6 if case == 'linear_only' else -0.05
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    with np.errstate(all='ignore'):
        ref = om.evaluate_pullback_density(X)
    got = tm.evaluate_pullback_density(X)
    assert _last(tm) == 'k_band_logdet'
    bad = ~np.isfinite(ref)
    assert bad.sum() > 20
    if case != 'linear_only':
        assert (~bad).sum() > 20                              # (the case has rows of both kinds)
    assert np.array_equal(~np.isfinite(got), bad)
    assert relerr(got[~bad], ref[~bad]) < 1e-10
    # the fused passes on the standardised samples, with and without Z, against the log-det-only pass: the same rows
    N = tm._N
    ld0 = tm._empty(N)
    tm.density_device(tm._Xs, N, logdet=ld0)
    assert _last(tm) == 'k_band_logdet'
    torch.cuda.synchronize()
    ld0 = ld0.cpu().numpy()
    bad_s = ~np.isfinite(ld0)
    assert bad_s.sum() > 20 and (case == 'linear_only' or (~bad_s).sum() > 20)
    for with_z in (True, False):
        ld, ss = tm._empty(N), tm._empty(N)
        if with_z:
            tm.forward_device(tm._Xs, N, logdet=ld, sumsq=ss)
        else:
            tm.density_device(tm._Xs, N, logdet=ld, sumsq=ss)
        assert _last(tm) == 'k_band_density'
        torch.cuda.synchronize()
        ld = ld.cpu().numpy()
        assert np.array_equal(~np.isfinite(ld), bad_s) and np.isfinite(ss.cpu().numpy()).all()
        assert relerr(ld[~bad_s], ld0[~bad_s]) < 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
def test_nan_and_inf_samples_reach_exactly_the_components_that_read_them(case, ttm_opt):
    tm, om, X, rng = _build(case, n=3001)
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    Z0 = tm.map(X)
    Xb = X.copy()
    Xb[6, 2] = np.nan
    Xb[7, 2] = np.inf
    Z = tm.map(Xb)
    tm.forward_device(tm._Xs, tm._N)
    assert _last(tm) == 'k_band_forward'
    for r in (6, 7):                                          # column 2 is read by its own component and the two behind it
        assert not np.isfinite(Z[r, 2:5]).any()
        assert np.array_equal(Z[r, :2], Z0[r, :2]) and np.array_equal(Z[r, 5:], Z0[r, 5:])
    other = np.ones(len(X), bool)
    other[[6, 7]] = False
    assert np.array_equal(Z[other], Z0[other])
    # the density passes: the rows with the bad sample and no others
    ld, ss = tm._empty(tm._N), tm._empty(tm._N)
    Xd = tm._import((Xb - tm.X_mean) / tm.X_std, False)
    tm.forward_device(Xd, len(X), logdet=ld, sumsq=ss)
    assert _last(tm) == 'k_band_density'
    fin = np.isfinite(ld[:len(X)].cpu().numpy()) & np.isfinite(ss[:len(X)].cpu().numpy())
    assert np.array_equal(fin, other)
    ld2 = tm._empty(tm._N)
    tm.density_device(Xd, len(X), logdet=ld2)
    assert _last(tm) == 'k_band_logdet'
    assert np.array_equal(np.isfinite(ld2[:len(X)].cpu().numpy()), other)
