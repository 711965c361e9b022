"""
The Newton root search of banded separable maps in push form (csrc/ttm_band.hip: k_band_newton, k_band_few_newton),
reached through root_finder='newton', alternate_root_finding=False and the C entry point ttm_inverse_newton.

What is checked, with the tolerances of tests/test_newton_inverse.py and SURVEY section 5 (nothing new):
  * on >= 10^4 rows that include the tails of every column, row 0 excluded, rows kept where the ORACLE's bisection is sane
    (|x| < 50 standardised): residual |S_oracle(x) - z| < 2e-9, positions within 1e-6 (1 + |x_ref|) of the oracle's bisection
    for more than 0.98 of the kept entries, more than 0.8 of the rows kept;
  * round trip of the whole ensemble: max |S^-1(S(x)) - x| / X_std < 1e-7 - what the table inverse (6.7e-5 ... 2.4e-4) cannot do;
  * against the generic kernel (option band_newton = 0): residuals of both under the HIP forward map < 2e-9, positions within
    1e-6 (1 + |x|) on sane rows, trial points <= 25 per component and never more than the generic kernel's + 2;
  * NaN / +-inf targets: the NaN pattern of the generic kernel, its values (same tolerance) wherever its result is sane, a
    search that ran away (|x| >= 50: no x reaches the target) with the same sign where the generic one ran away, every other
    row unchanged.  (The position tolerance is one on sane rows, here as above: the last bracket point of a search for an
    infinite target is where the evaluator's arithmetic overflows - 2^1023 for the term tables, earlier for the spline's
    local coordinate - not a root);
  * rows are independent: a permutation of the rows, another chunking (band_cus) and the host pipeline give the same bits.
"""
import ctypes

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case, make_oracle, record_parity


# ---------------------------------------------------------------------------
# CPU: the option exists in both libraries; the Python side under the host test double
# ---------------------------------------------------------------------------
def test_band_newton_is_an_option_of_the_host_double():
    with emu.install():
        emu._lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        try:
            assert emu._lib.ttm_set_option(b'band_newton', 0) == 0
            assert emu._lib.ttm_set_option(b'band_newton', -1) == 0
            assert emu._lib.ttm_set_option(b'band_newtons', 0) != 0
        finally:
            emu._lib.ttm_reset_options()


@pytest.mark.gpu
def test_band_newton_is_an_option_of_the_device_library(ttm_opt):
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    assert lib.ttm_set_option(b'band_newton', 0) == 0
    ttm_opt('band_newton', -1)


@pytest.mark.parametrize('band_newton', [-1, 0])
@pytest.mark.parametrize('name', ['c3_sep', 'c2b_sep', 'c5_sep', 'ex03_order10'])
def test_newton_roots_of_the_banded_fixtures_under_the_host_double(name, band_newton, ttm_opt):
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    X = case_X(name, npz)
    with emu.install():
        ttm_opt('band_newton', band_newton)
        tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False,
                           root_finder='newton', alternate_root_finding=False, **ctor_kwargs(desc))
        tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
        om = make_oracle(name, npz, desc)
        Zin, ref = npz['inv_Z'], npz['inv_X_bisect']
        got = tm.inverse_map(Zin)
        assert not getattr(tm._pack_coeffs(), '_ttm_tables', None)          # no table build on this path
    assert got.shape == ref.shape
    sane = np.all(np.abs(ref) < 50.0, axis=1)
    sane[0] = False                                                     # (sample 0 of the reference: loop-guard quirk)
    assert sane.mean() > 0.8
    res = np.abs(om.map(got) - Zin)
    assert res[sane].max() < 2e-9
    close = np.abs(got[sane] - ref[sane]) <= 1e-6 * (1 + np.abs(ref[sane]))
    assert close.mean() > 0.98


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------
def _newton(tm, Zs, N, cond=None):
    """ttm_inverse_newton of all components on the column-major device matrix Zs; conditioning columns (standardised, device)
    go into X first.  Returns X (d x ld), the trial-point maxima and the kernel's name."""
    import torch
    from tests.test_full_size import _last_kernel
    coef = tm._pack_coeffs()
    Xs = tm._cols(tm._cm.d_cols, N, zero=True)
    if cond is not None:
        Xs[:cond.shape[0], :N].copy_(cond[:, :N])
    iters = tm._zeros(tm.D, dtype=torch.int32)
    rc = tm._lib.ttm_inverse_newton(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, tm.D, tm._ptr(Zs), Zs.shape[1], tm._ptr(Xs),
                                    Xs.shape[1], N, ctypes.c_void_p(iters.data_ptr()), tm._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not getattr(coef, '_ttm_tables', None)                           # the search builds no tables
    return Xs, iters.cpu().numpy().copy(), _last_kernel(tm)


def _contract(tag, tm, om, X, kernel, ttm_opt, Zr=None, nonfinite=True, rt_bound=1e-7):
    """The contract of the module docstring for the targets Z = S(X) of the training ensemble (conditioning columns: the
    ensemble's own) and, if given, the reference samples Zr.  rt_bound: the bound on the round trip of the whole ensemble."""
    import torch
    from tests.test_full_size import subset_with_tails
    N, D, skip = tm._N, tm.D, tm.skip_dimensions
    cond = tm._Xs[:skip] if skip else None
    std = torch.as_tensor(np.asarray(tm.X_std, dtype=float), device=tm._Xs.device)[:, None]
    mean = torch.as_tensor(np.asarray(tm.X_mean, dtype=float), device=tm._Xs.device)[:, None]
    Zdev = tm.forward_device(tm._Xs, N).clone()
    targets = [('pushed', Zdev, subset_with_tails(X))]
    if Zr is not None:
        Zrd = tm._cols(D, N)
        Zrd[:, :N].copy_(torch.from_numpy(np.ascontiguousarray(Zr.T)))
        targets.append(('reference', Zrd, np.unique(np.concatenate((np.arange(50), subset_with_tails(Zr, 10000))))))
    for what, Zs, idx in targets:
        ttm_opt('band_newton', -1)
        Xb, itb, name = _newton(tm, Zs, N, cond)
        assert name == kernel
        Xb = Xb[:, :N].clone()
        ttm_opt('band_newton', 0)
        Xg, itg, name = _newton(tm, Zs, N, cond)
        assert name == 'k_inverse_newton'
        Xg = Xg[:, :N].clone()
        ttm_opt('band_newton', -1)
        # ---- against the oracle's bisection on a subset with tails ----
        idx = idx[idx > 0]
        assert len(idx) >= 10000
        sel = torch.from_numpy(idx).to(Zs.device)
        Zh = Zs[:, :N].T[sel].cpu().numpy()
        Xraw = (Xb * std + mean).T[sel].cpu().numpy()                       # (d columns, conditioning columns included)
        om.alternate_root_finding = False
        star = Xraw[:, :skip] if skip else None
        Zo = np.vstack((Zh[:1], Zh))                                        # (a row 0 of its own keeps the loop-guard quirk off the subset)
        ref = om.inverse_map(Zo, X_star=None if star is None else np.vstack((star[:1], star)))[1:]
        ref = ref[:, -D:]
        ref_s = (ref - om.X_mean[skip:]) / om.X_std[skip:]
        got_s = Xb[skip:].T[sel].cpu().numpy()
        sane = np.all(np.abs(ref_s) < 50.0, axis=1)
        record_parity('%s/%s/rows_kept' % (tag, what), 1.0 - sane.mean(), 0.2)
        assert sane.mean() > 0.8
        res = float(np.abs(om.map(Xraw) - Zh)[sane].max())
        record_parity('%s/%s/newton(%s)_residual_under_the_oracle_map' % (tag, what, kernel), res, 2e-9)
        assert res < 2e-9
        far = 1.0 - float((np.abs(got_s[sane] - ref_s[sane]) <= 1e-6 * (1 + np.abs(ref_s[sane]))).mean())
        record_parity('%s/%s/newton(%s)_positions_beyond_1e-6_of_oracle_bisection' % (tag, what, kernel), far, 0.02)
        assert far < 0.02
        # ---- against the generic kernel, whole ensemble ----
        ok = (Xg[skip:].abs() < 50.0).all(dim=0)
        rb = float((tm.forward_device(_padded(tm, Xb, N), N)[:, :N] - Zs[:, :N]).abs()[:, ok].max().item())
        rg = float((tm.forward_device(_padded(tm, Xg, N), N)[:, :N] - Zs[:, :N]).abs()[:, ok].max().item())
        record_parity('%s/%s/newton(%s)_residual_under_the_HIP_map' % (tag, what, kernel), rb, 2e-9)
        record_parity('%s/%s/newton(k_inverse_newton)_residual_under_the_HIP_map' % (tag, what), rg, 2e-9)
        assert rb < 2e-9 and rg < 2e-9
        dx = float(((Xb - Xg).abs() / (1 + Xg.abs()))[:, ok].max().item())
        record_parity('%s/%s/newton(%s)_vs_k_inverse_newton' % (tag, what, kernel), dx, 1e-6)
        assert dx < 1e-6
        record_parity('%s/%s/newton(%s)_trial_points' % (tag, what, kernel), float(itb.max()), 25)
        print(tag, what, 'trial points', itb.tolist(), 'generic', itg.tolist())
        assert itb.max() <= 25 and np.all(itb <= itg + 2)
        if what == 'pushed':
            rt = float((Xb - tm._Xs[:, :N]).abs().max().item())
            rtg = float((Xg - tm._Xs[:, :N]).abs().max().item())
            record_parity('%s/newton(%s)_round_trip_of_the_whole_ensemble' % (tag, kernel), rt, rt_bound)
            record_parity('%s/newton(k_inverse_newton)_round_trip_of_the_whole_ensemble' % tag, rtg)
            print(tag, 'round trip', rt, 'generic', rtg, 'bound', rt_bound)
            assert rt < rt_bound
            perm = torch.from_numpy(np.random.default_rng(3).permutation(N)).to(Zs.device)
            Zp = tm._cols(D, N)
            Zp[:, :N].copy_(Zs[:, :N][:, perm])
            condp = None
            if skip:
                condp = tm._cols(skip, N)
                condp[:, :N].copy_(cond[:, :N][:, perm])
            Xp, _, _ = _newton(tm, Zp, N, condp)
            assert torch.equal(Xp[:, :N], Xb[:, perm])                      # rows are independent: exact
    if nonfinite:
        Zs = Zdev
        Zn = Zs.clone()
        rows = [5, 1001, 2049, 4098, N - 1, N - 2]
        col = min(1, D - 1)
        for r, v in zip(rows, [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]):
            Zn[col, r] = v
        ttm_opt('band_newton', -1)
        Xc, _, _ = _newton(tm, Zs, N, cond)
        Xb, _, name = _newton(tm, Zn, N, cond)
        assert name == kernel
        ttm_opt('band_newton', 0)
        Xg, _, _ = _newton(tm, Zn, N, cond)
        ttm_opt('band_newton', -1)
        Xc, Xb, Xg = Xc[:, :N], Xb[:, :N], Xg[:, :N]
        other = torch.ones(N, dtype=torch.bool, device=Zs.device)
        other[rows] = False
        assert torch.equal(Xb[:, other], Xc[:, other])                      # every other row unchanged
        b, g = Xb[:, rows].cpu().numpy(), Xg[:, rows].cpu().numpy()
        print(tag, 'non-finite targets: push form\n', b, '\ngeneric\n', g)
        record_parity('%s/non_finite_targets/NaN_pattern_mismatches_vs_k_inverse_newton' % tag, float(np.sum(np.isnan(b) != np.isnan(g))), 1)
        assert np.array_equal(np.isnan(b), np.isnan(g))
        sane = np.abs(g) < 50.0
        dx = float(np.max(np.abs(b[sane] - g[sane]) / (1 + np.abs(g[sane]))))
        record_parity('%s/non_finite_targets/newton(%s)_vs_k_inverse_newton_where_sane' % (tag, kernel), dx, 1e-6)
        assert dx <= 1e-6
        away = ~sane & ~np.isnan(g)
        with np.errstate(over='ignore', invalid='ignore'):
            nearest = float(np.min(np.abs(b[away]))) if away.any() else np.inf
        record_parity('%s/non_finite_targets/entries_where_the_generic_search_ran_away' % tag, float(away.sum()))
        record_parity('%s/non_finite_targets/smallest_|x|_of_newton(%s)_there (at least 50)' % (tag, kernel), min(nearest, 1e308))
        assert nearest >= 50.0 and np.array_equal(np.sign(b[away]), np.sign(g[away]))


def _padded(tm, Xc, N):
    """d x N device matrix -> the padded column-major matrix the entry points take"""
    out = tm._cols(Xc.shape[0], N, zero=True)
    out[:, :N].copy_(Xc)
    return out


def _reference_samples(N, D):
    Zr = np.random.default_rng(1).standard_normal((N, D))
    Zr[:50] *= 2.5
    return Zr


def _as_newton(tm):
    tm.alternate_root_finding = False
    tm.root_finder = 'newton'
    return tm


@pytest.mark.gpu
def test_c5_at_1e6_takes_k_band_newton(ttm_opt):
    """C5 (d = 40, band 2, N = 1e6): k_band_newton by name (band_newton = 0: k_inverse_newton), the whole contract for
    pushed and reference samples, and inverse_map through the host pipeline."""
    from tests.test_full_size import build
    N = 1000000
    tm, om, X = build('C5', 'c5_sep', N)
    _as_newton(tm)
    from tests.test_full_size import _last_kernel
    Zdev = tm.forward_device(tm._Xs, tm._N)
    tm.inverse_device(Zdev, tm._N)
    assert _last_kernel(tm) == 'k_band_newton'
    ttm_opt('band_newton', 0)
    tm.inverse_device(Zdev, tm._N)
    assert _last_kernel(tm) == 'k_inverse_newton'
    ttm_opt('band_newton', -1)
    _contract('c5_1e6', tm, om, X, 'k_band_newton', ttm_opt, Zr=_reference_samples(N, tm.D))
    # inverse_map of host samples: chunks of rows through the pipeline = one copy in, one copy out
    Z = tm.map(X)
    tm.host_pipeline = True
    Xa = tm.inverse_map(Z)
    tm.host_pipeline = False
    Xb = tm.inverse_map(Z)
    tm.host_pipeline = True
    assert np.array_equal(Xa, Xb)
    rt = float(np.max(np.abs(Xa - X) / tm.X_std))
    record_parity('c5_1e6/inverse_map(newton)_round_trip', rt, 1e-7)
    assert rt < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize('cfg, fixture, N', [('C2b', 'c2b_sep', 1000000), ('C3', 'c3_sep', 500000), ('EX03', 'ex03_order10', 100000)])
def test_few_component_maps_take_k_band_few_newton(cfg, fixture, N, ttm_opt):
    from tests.test_full_size import build
    tm, om, X = build(cfg, fixture, N)
    _as_newton(tm)
    _contract('%s_%g' % (cfg.lower(), N), tm, om, X, 'k_band_few_newton', ttm_opt,
              Zr=_reference_samples(N, tm.D) if cfg != 'EX03' else None)
    if N >= (1 << 18):
        Z = tm.map(X)
        Xa = tm.inverse_map(Z)
        tm.host_pipeline = False
        Xb = tm.inverse_map(Z)
        assert np.array_equal(Xa, Xb)


@pytest.mark.gpu
def test_filter_map_with_its_conditioning_column_takes_k_band_few_newton(ttm_opt):
    """The 4-column filter map of example 06 at N = 1e5 (the construction of test_c4_filter_update_at_1e5...): conditioned on
    its first column."""
    from triangular_transport_toolbox_amd import entf, specs
    from oracle.ttm_oracle import OracleMap
    N = 100000
    rng = np.random.default_rng(0)
    ens = rng.standard_normal((N, 3)) * [8, 9, 8] + [0, 0, 25]
    ens = entf.rk4(ens, 0.05, 20)
    inp = np.column_stack((ens[:, 0] + 2.0 * rng.standard_normal(N), ens[:, entf.PERMUTATIONS[0]]))
    tm = entf.make_filter_map(N, root_finder='newton', alternate_root_finding=False)
    tm.reset(inp.copy())
    tm.optimize()
    mon, non = specs.entf_filter_spec(3)
    om = OracleMap(X=inp.copy(), monotone=mon, nonmonotone=non, polynomial_type='hermite function',
                   monotonicity='separable monotonicity', regularization='l2', regularization_lambda=0.05)
    om.coeffs_mon, om.coeffs_nonmon = [c.copy() for c in tm.coeffs_mon], [c.copy() for c in tm.coeffs_nonmon]
    assert tm.skip_dimensions == 1
    # This map is optimised on the spot; the first monotone part it ends with has a nearly flat piece, where the stopping rule
    # |S - z| <= 1e-9 pins x only to 1e-9 / (dS/dx), whoever searches.  What the rule allows on THIS ensemble is measured with
    # the oracle (CPU, the reference's bisection, no code of the library): its own round trip S^-1(S(x)) of every row but the
    # first (loop-guard quirk) - 1e-7 on top of that is the bound.  (The fixture maps and the block map keep the plain 1e-7.)
    om.alternate_root_finding = False
    Zo = om.map(inp)
    xo = om.inverse_map(np.vstack((Zo[:1], Zo)), X_star=np.vstack((inp[:1, :1], inp[:, :1])))[1:]
    rto = float(np.max(np.abs(xo[:, -tm.D:] - inp[:, 1:]) / om.X_std[1:]))
    record_parity('c4_filter_1e5/oracle_bisection_round_trip_of_the_whole_ensemble', rto)
    print('c4_filter_1e5 oracle bisection round trip', rto)
    _contract('c4_filter_1e5', tm, om, inp, 'k_band_few_newton', ttm_opt, rt_bound=1e-7 + rto)
    got = tm.inverse_map(X_star=inp[:, :1].copy(), Z=tm.map(inp))           # the public path with X_star
    rt = float(np.max(np.abs(got - inp[:, 1:]) / tm.X_std[1:]))
    record_parity('c4_filter_1e5/inverse_map(newton, X_star)_round_trip', rt, 1e-7 + rto)
    assert rt < 1e-7 + rto


@pytest.mark.gpu
def test_block_map_with_its_conditioning_columns_takes_k_band_few_newton(ttm_opt):
    """The 6-column block map of example 07 at N = 1e5 (the construction of test_c4_block_map_backward_step_at_1e5...):
    push records of five groups, conditioned on its first three columns."""
    from triangular_transport_toolbox_amd import entf, specs
    from oracle.ttm_oracle import OracleMap
    N = 100000
    rng = np.random.default_rng(0)
    ana = rng.standard_normal((N, 3)) * [8.0, 9.0, 8.0] + [0.0, 0.0, 25.0]
    ana = entf.rk4(ana, 0.05, 20)
    fc_next = entf.rk4(ana, 0.05, 2)
    inp = np.column_stack((fc_next, ana))
    tm = entf.make_smoother_map(N, maxorder=3, lmbda=0.05, root_finder='newton', alternate_root_finding=False)
    tm.reset(inp.copy())
    tm.optimize()
    mon, non = specs.ents_smoother_spec(3)
    om = OracleMap(X=inp.copy(), monotone=mon, nonmonotone=non, polynomial_type="probabilist's hermite",
                   monotonicity='separable monotonicity', regularization='l2', regularization_lambda=0.05)
    om.coeffs_mon, om.coeffs_nonmon = [c.copy() for c in tm.coeffs_mon], [c.copy() for c in tm.coeffs_nonmon]
    assert tm.skip_dimensions == 3
    _contract('c4_block_1e5', tm, om, inp, 'k_band_few_newton', ttm_opt)


@pytest.mark.gpu
def test_c5_newton_with_several_tiles_per_workgroup_and_an_odd_tail(ttm_opt):
    """C5 at N = 2 100 003 (as test_c5_ring_inverse_with_several_tiles_per_workgroup): band_cus = 64 gives every workgroup a
    chunk of nine tiles, the default plan three; rt_block cuts the components into several residency blocks; the rows do not
    notice - nor a permutation of them."""
    import torch
    from tests.test_full_size import build
    N = 2100003
    tm, om, X = build('C5', 'c5_sep', N)
    _as_newton(tm)
    Z = tm.forward_device(tm._Xs, N).clone()
    Xd, itd, name = _newton(tm, Z, N)
    assert name == 'k_band_newton'
    Xd = Xd[:, :N].clone()
    ttm_opt('band_cus', 64)
    Xc, itc, name = _newton(tm, Z, N)
    assert name == 'k_band_newton'
    assert torch.equal(Xc[:, :N], Xd) and np.array_equal(itc, itd)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(N)).to(Z.device)
    Zp = tm._cols(tm.D, N)
    Zp[:, :N].copy_(Z[:, :N][:, perm])
    Xp, _, _ = _newton(tm, Zp, N)
    assert torch.equal(Xp[:, :N], Xd[:, perm])
    # two residency blocks of 20 components (rt_block), nine tiles per chunk: a tile re-reads the two columns in front of the
    # second block and pushes them again - the same bits, the same trial-point maxima
    ttm_opt('rt_block', 20)
    Xk, itk, name = _newton(tm, Z, N)
    assert name == 'k_band_newton'
    assert torch.equal(Xk[:, :N], Xd) and np.array_equal(itk, itd)
    ttm_opt('rt_block', -1)
    ttm_opt('band_cus', -1)
    ttm_opt('rt_block', 13)                                                 # (blocks of 13, 13, 13 and 1 with the default chunks)
    Xk, itk, name = _newton(tm, Z, N)
    assert name == 'k_band_newton'
    assert torch.equal(Xk[:, :N], Xd) and np.array_equal(itk, itd)
    ttm_opt('rt_block', -1)
    rt = float((Xd - tm._Xs[:, :N]).abs().max().item())
    record_parity('c5_2.1e6/newton(k_band_newton)_round_trip_of_the_whole_ensemble', rt, 1e-7)
    assert rt < 1e-7
