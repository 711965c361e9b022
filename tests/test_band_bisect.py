"""
The reference's bisection of banded separable maps in push form (csrc/ttm_band.hip: k_band_bisect, k_band_few_bisect), reached
through alternate_root_finding=False with the default root_finder='reference' and the C entry point ttm_inverse_bisect.

The push form takes the monotone part from the component's spline (fit error <= 2e-13 (1 + |exact|), termtable.U_TOL_VALUE), the
generic kernel from erf itself: the sign of a midpoint's residual can differ only where |fm| < 1e-9, where both searches have
stopped; the stop decision only where |fm| lies within the fit error of 1e-9 - a share of about 4 eps / 1e-9 <= 4e-3 of the
entries, which then end one midpoint earlier or later.  Hence, per target set (S(X) of the ensemble, and reference samples with
50 rows scaled by 2.5: window shifts):

  * against k_inverse_bisect in the same process (option band_bisect = 0), standardised device coordinates, rows where the
    generic result is sane (|x| < 50): >= 0.98 of the entries bit-identical, all within 1e-6 (1 + |x|), the residual of both
    under the HIP forward map < 2e-9, per-component iters within +-1 of the generic kernel's and >= 25 somewhere (it is the
    bisection: tests/test_newton_inverse.py);
  * dyadic grid (pushed targets): where no window shift happened (|x| < 2) every x is a midpoint of [-2, 2] - with n = iters[k],
    x 2^(n-2) is an integer, exactly.  A Newton step or a secant start fails this;
  * against the oracle's bisection (CPU) on a subset with tails that gets a row 0 of its own, rows kept where the oracle is sane:
    more than 0.8 kept, residual under the oracle's map < 2e-9, positions within 1e-6 (1 + |x_ref|) for more than 0.98 of the
    kept entries (the figures of tests/test_band_newton.py);
  * NaN / +-inf targets in a few rows, the last two among them: the NaN pattern of the generic kernel, its values wherever its
    result is sane (a NaN target: the first midpoint, 0, in both), the same sign where the generic search ran away, every other
    row bit-identical to the launch without them;
  * rows are independent: a permutation, another chunking (band_cus) and other residency blocks (rt_block) give the same bits
    in X and the same iters;
  * row ownership as tests/test_row_ownership.py (its harness, imported): padded leading dimension, canary-filled allocation,
    NaN / 1e300 in the pad rows of the inputs - nothing outside rows [0, N) of X changes, results and iters bit-identical to
    the tight layout;
  * the call that starts on an odd row (what the host class passes: Z + 1 row, X + 1 row, N - 1 rows): the push-form kernel by
    name, the row in front of the pointers neither written (canary) nor read (NaN there changes no bit).

The kernels are forced at small N with option u_loader = 1 (tests/test_band_dispatch.py).  After a public inverse_map the last
launch is the replay of sample 0 with the cap - k_inverse_bisect by design - so names are asserted on direct calls.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case, make_oracle, record_parity, relerr


# ---------------------------------------------------------------------------
# CPU: the option exists in both libraries; the Python side under the host test double
# ---------------------------------------------------------------------------
def test_band_bisect_is_an_option_of_the_host_double():
    with emu.install():
        emu._lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        try:
            assert emu._lib.ttm_set_option(b'band_bisect', 0) == 0
            assert emu._lib.ttm_set_option(b'band_bisect', -1) == 0
            assert emu._lib.ttm_set_option(b'band_bisects', 0) != 0
        finally:
            emu._lib.ttm_reset_options()


@pytest.mark.gpu
def test_band_bisect_is_an_option_of_the_device_library(ttm_opt):
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    assert lib.ttm_set_option(b'band_bisect', 0) == 0
    assert lib.ttm_set_option(b'band_bisects', 0) != 0
    ttm_opt('band_bisect', -1)


@pytest.mark.parametrize('band_bisect', [-1, 0])
@pytest.mark.parametrize('name', ['c3_sep', 'c2b_sep', 'c5_sep', 'ex03_order10'])
def test_bisection_of_the_banded_fixtures_under_the_host_double(name, band_bisect, ttm_opt):
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    X = case_X(name, npz)
    with emu.install():
        ttm_opt('band_bisect', band_bisect)
        tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False,
                           alternate_root_finding=False, **ctor_kwargs(desc))
        tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
        got = tm.inverse_map(npz['inv_Z'])
    assert relerr(got, npz['inv_X_bisect']) < 1e-6                          # (the bound of tests/test_transport_map.py)


# ---------------------------------------------------------------------------
# GPU: direct calls
# ---------------------------------------------------------------------------
def _call(tm, Z, ldz, X, ldx, n, iters=None, cap=None, zrow=0, xrow=0):
    """ttm_inverse_bisect of all components on n rows that start at row zrow of Z / xrow of X.  Returns iters and the name."""
    import torch
    from tests.test_full_size import _last_kernel
    coef = tm._pack_coeffs()
    if iters is None:
        iters = tm._zeros(tm.D, dtype=torch.int32)
    rc = tm._lib.ttm_inverse_bisect(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, tm.D, tm._ptr(Z, zrow), int(ldz), tm._ptr(X, xrow),
                                    int(ldx), int(n), ctypes.c_void_p(iters.data_ptr()),
                                    None if cap is None else ctypes.c_void_p(cap.data_ptr()), tm._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return iters.cpu().numpy().copy(), _last_kernel(tm)


def _bisect(tm, Zs, N, cond=None):
    """All components on the column-major device matrix Zs; conditioning columns (standardised, device) go into X first.
    Returns X[:, :N] (d rows), the midpoint maxima and the kernel's name."""
    Xs = tm._cols(tm._cm.d_cols, N, zero=True)
    if cond is not None:
        Xs[:cond.shape[0], :N].copy_(cond[:, :N])
    it, name = _call(tm, Zs, Zs.shape[1], Xs, Xs.shape[1], N)
    return Xs[:, :N].clone(), it, name


def _padded(tm, Xc, N):
    out = tm._cols(Xc.shape[0], N, zero=True)
    out[:, :N].copy_(Xc)
    return out


def _reference_samples(N, D):
    Zr = np.random.default_rng(1).standard_normal((N, D))
    Zr[:50] *= 2.5
    return Zr


def _contract(tag, tm, om, X, kernel, ttm_opt, settings=(), oracle_on_reference=True):
    """The contract of the module docstring for one map; settings: (band_cus, rt_block) pairs that must give the same bits.
    oracle_on_reference: hold the reference samples against the oracle too; False (test_long_bisection, two maps that are not
    monotone): the oracle runs there as well, its kept share is recorded and asserted to be at most 0.8 - the reason for the
    exception - and the rest of the oracle contract is recorded only."""
    import torch
    from tests.test_full_size import subset_with_tails
    N, D, skip = tm._N, tm.D, tm.skip_dimensions
    cond = tm._Xs[:skip] if skip else None
    dev = tm._Xs.device
    std = torch.as_tensor(np.asarray(tm.X_std, dtype=float), device=dev)[:, None]
    mean = torch.as_tensor(np.asarray(tm.X_mean, dtype=float), device=dev)[:, None]
    Zdev = tm.forward_device(tm._Xs, N).clone()
    Zr = _reference_samples(N, D)
    Zrd = tm._cols(D, N, zero=True)
    Zrd[:, :N].copy_(torch.from_numpy(np.ascontiguousarray(Zr.T)))
    n_sub = min(2000, N - 1)
    targets = [('pushed', Zdev, subset_with_tails(X, n_sub)),
               ('reference', Zrd, np.unique(np.concatenate((np.arange(50), subset_with_tails(Zr, n_sub)))))]
    for what, Zs, idx in targets:
        key = '%s/%s/bisect(%s)' % (tag, what, kernel)
        ttm_opt('band_bisect', -1)
        Xb, itb, name = _bisect(tm, Zs, N, cond)
        assert name == kernel
        ttm_opt('band_bisect', 0)
        Xg, itg, name = _bisect(tm, Zs, N, cond)
        assert name == 'k_inverse_bisect'
        ttm_opt('band_bisect', -1)
        print(tag, what, 'midpoints', itb.tolist(), 'generic', itg.tolist())
        # ---- against the generic kernel, whole ensemble ----
        ok = (Xg[skip:].abs() < 50.0).all(dim=0)
        same = float((Xb[skip:] == Xg[skip:])[:, ok].double().mean().item())
        record_parity(key + '_share_not_bit_identical_to_k_inverse_bisect', 1.0 - same, 0.02)
        print(tag, what, 'bit-identical share', same)
        assert same >= 0.98
        dx = float(((Xb - Xg).abs() / (1 + Xg.abs()))[:, ok].max().item())
        record_parity(key + '_vs_k_inverse_bisect', dx, 1e-6)
        assert dx < 1e-6
        rb = float((tm.forward_device(_padded(tm, Xb, N), N)[:, :N] - Zs[:, :N]).abs()[:, ok].max().item())
        rg = float((tm.forward_device(_padded(tm, Xg, N), N)[:, :N] - Zs[:, :N]).abs()[:, ok].max().item())
        record_parity(key + '_residual_under_the_HIP_map', rb, 2e-9)
        print(tag, what, 'residuals', rb, rg, 'dx', dx)
        assert rb < 2e-9 and rg < 2e-9
        assert np.all(np.abs(itb - itg) <= 1) and itb.max() >= 25
        # ---- against the oracle's bisection on a subset with tails ----
        held = what == 'pushed' or oracle_on_reference
        idx = idx[idx > 0]
        sel = torch.from_numpy(idx).to(dev)
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
        record_parity('%s/%s/rows_the_oracle_bisection_loses' % (tag, what), 1.0 - sane.mean(), 0.2 if held else None)
        print(tag, what, 'rows kept by the oracle', sane.mean())
        if not held:
            # (the oracle does not keep 0.8 of these rows - asserted, so that the exception ends when it no longer holds; what it
            # gives on the rows it keeps is recorded, not asserted)
            assert sane.mean() <= 0.8
            with np.errstate(all='ignore'):
                res = float(np.nanmax(np.abs(om.map(Xraw) - Zh)[sane])) if sane.any() else 0.0
            record_parity(key + '_residual_under_the_oracle_map_where_the_oracle_is_sane (not asserted)', min(res, 1e308))
            continue
        assert sane.mean() > 0.8
        res = float(np.abs(om.map(Xraw) - Zh)[sane].max())
        record_parity(key + '_residual_under_the_oracle_map', res, 2e-9)
        assert res < 2e-9
        far = 1.0 - float((np.abs(got_s[sane] - ref_s[sane]) <= 1e-6 * (1 + np.abs(ref_s[sane]))).mean())
        record_parity(key + '_positions_beyond_1e-6_of_oracle_bisection', far, 0.02)
        assert far < 0.02
        if what == 'pushed':
            # ---- dyadic grid: no tolerance ----
            for k in range(D):
                x = Xb[skip + k]
                x = x[x.abs() < 2.0]
                assert x.numel() > N // 2
                v = x * (2.0 ** (int(itb[k]) - 2))
                assert bool((v == v.round()).all()), (k, int(itb[k]))
            # ---- rows are independent ----
            perm = torch.from_numpy(np.random.default_rng(3).permutation(N)).to(dev)
            Zp = tm._cols(D, N, zero=True)
            Zp[:, :N].copy_(Zs[:, :N][:, perm])
            condp = None
            if skip:
                condp = tm._cols(skip, N, zero=True)
                condp[:, :N].copy_(cond[:, :N][:, perm])
            Xp, itp, _ = _bisect(tm, Zp, N, condp)
            assert torch.equal(Xp, Xb[:, perm]) and np.array_equal(itp, itb)
            for cus, block in settings:
                ttm_opt('band_cus', cus); ttm_opt('rt_block', block)
                Xk, itk, name = _bisect(tm, Zs, N, cond)
                ttm_opt('band_cus', -1); ttm_opt('rt_block', -1)
                assert name == kernel
                assert torch.equal(Xk, Xb) and np.array_equal(itk, itb), (cus, block)
    # ---- NaN / +-inf targets ----
    Zn = Zdev.clone()
    rows = [5, 1001, 2049, 4098, N - 1, N - 2]
    col = min(1, D - 1)
    for r, v in zip(rows, [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]):
        Zn[col, r] = v
    Xc, _, _ = _bisect(tm, Zdev, N, cond)
    Xb, _, name = _bisect(tm, Zn, N, cond)
    assert name == kernel
    ttm_opt('band_bisect', 0)
    Xg, _, _ = _bisect(tm, Zn, N, cond)
    ttm_opt('band_bisect', -1)
    other = torch.ones(N, dtype=torch.bool, device=dev)
    other[rows] = False
    assert torch.equal(Xb[:, other], Xc[:, other])                          # every other row unchanged
    b, g = Xb[skip:, rows].cpu().numpy(), Xg[skip:, rows].cpu().numpy()
    print(tag, 'non-finite targets: push form\n', b, '\ngeneric\n', g)
    assert np.array_equal(np.isnan(b), np.isnan(g))
    sane = np.abs(g) < 50.0
    assert np.max(np.abs(b[sane] - g[sane]) / (1 + np.abs(g[sane]))) <= 1e-6
    nan_rows = [i for i, r in enumerate(rows) if np.isnan(float(Zn[col, r].item()))]
    assert np.all(b[col, nan_rows] == 0.0) and np.all(g[col, nan_rows] == 0.0)  # (a NaN target: the first midpoint)
    away = ~sane & ~np.isnan(g)
    assert np.all(np.abs(b[away]) >= 50.0) and np.array_equal(np.sign(b[away]), np.sign(g[away]))


# The few-component kernel: a trimmed table (not the 80 combinations of tests/test_band_dispatch.py) - every degree class 1-4 x
# every record lag 2 / 3 / 5, i.e. each of the twelve instantiations of k_band_few_bisect<CLS, LAG> at least once, with and without
# conditioning columns, with and without plain terms:
# (class, groups per record, reach, D, plain) of tests/test_band_dispatch.py ...
FEW_TABLE = [(1, 2, 1, 2, False), (2, 2, 1, 4, True), (3, 3, 1, 2, False), (4, 3, 2, 4, True), (1, 3, 3, 4, False), (2, 3, 3, 2, True),
             (3, 5, 5, 4, False), (4, 5, 5, 2, True), (4, 2, 1, 2, False), (2, 5, 5, 4, True), (3, 2, 1, 4, True), (1, 5, 5, 2, False)]
# ... and the maps of tests/test_band.py with a linear own term beside the spline (filter map, example 05) and with linear-only
# components and records of five groups (the smoother's block map)
FEW_CASES = ['few_entf', 'few_ex05', 'few_ents', 'few_c3']
N_FEW = 5003                                        # two full tiles of 2048 rows, a partial one, an odd tail
N_LONG = 9001                                       # three tiles of 4096 rows, the last partial and odd
LONG_SETTINGS = ((1, -1), (2, -1), (-1, 2), (2, 4))  # (band_cus, rt_block): several tiles per chunk, several residency blocks


@pytest.mark.gpu
@pytest.mark.parametrize('cls,lag,reach,D,plain', FEW_TABLE, ids=['cls%d-lag%d-reach%d-D%d-%s' % (c, lg, r, D, 'plain' if p else 'hf')
                                                                   for c, lg, r, D, p in FEW_TABLE])
def test_few_component_bisection_over_the_table(cls, lag, reach, D, plain, ttm_opt):
    from tests.test_band_dispatch import _build, _planned
    tm, om, X, rng, E = _build(cls, lag, reach, D, plain, n=N_FEW)
    _planned(tm, cls, lag, reach, plain)
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    _contract('few_table_%d%d%d%d%d' % (cls, lag, reach, D, plain), tm, om, X, 'k_band_few_bisect', ttm_opt, settings=((1, -1),))


@pytest.mark.gpu
@pytest.mark.parametrize('case', FEW_CASES)
def test_few_component_bisection_with_linear_own_terms(case, ttm_opt):
    from tests.test_band import _build
    tm, om, X, rng = _build(case, n=N_FEW)
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    _contract(case, tm, om, X, 'k_band_few_bisect', ttm_opt, settings=((1, -1),))


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['c5_shape', 'class_55', 'class_77', 'mixed'])
def test_long_bisection(case, ttm_opt):
    if case == 'mixed':
        from tests.test_band_linear import _build                           # (linear own terms: the OWN instantiations)
    else:
        from tests.test_band import _build
    tm, om, X, rng = _build(case, n=N_LONG)
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    # class_55 and class_77 with these coefficients are not monotone (tests/test_band.py notes it for the tables of class_55): no
    # x reaches many of the reference samples, the ORACLE's own bisection keeps 0.62 / 0.19 of those rows (measured; below the
    # 0.8 the oracle contract starts from) and both kernels stop at 100 midpoints in two / three components.  That is a property of map and targets, whoever searches: there the reference samples are
    # held against the generic kernel only (bit identity, residuals, iters), the pushed ensemble against the oracle as everywhere.
    _contract('long_' + case, tm, om, X, 'k_band_bisect', ttm_opt, settings=LONG_SETTINGS, oracle_on_reference=case not in ('class_55', 'class_77'))


# ---------------------------------------------------------------------------
# row ownership: the harness of tests/test_row_ownership.py
# ---------------------------------------------------------------------------
OWN_LONG = [(1, 'alt', -1, -1), (2, 'nan', -1, -1), (33, 'inf', -1, -1), (65, 'big', 2, -1), (1025, 'alt', -1, 2), (4097, 'nan', 1, -1)]
OWN_FEW = [(1, 'alt'), (2, 'nan'), (2047, 'inf'), (2049, 'big'), (4097, 'alt')]


@pytest.mark.gpu
@pytest.mark.parametrize('N,poison,cus,block', OWN_LONG)
@pytest.mark.parametrize('kind', ['c5_shape', 'mixed'])
def test_row_ownership_of_the_long_kernel(kind, N, poison, cus, block, ttm_opt):
    from tests.test_row_ownership import _band_case, _band_on
    _band_on(ttm_opt, cus=cus, block=block)
    _band_case(kind, N).search('k_band_bisect', poison, newton=False, rt_bound=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize('N,poison', OWN_FEW)
@pytest.mark.parametrize('kind', ['few2', 'few4c'])
def test_row_ownership_of_the_few_component_kernel(kind, N, poison, ttm_opt):
    from tests.test_row_ownership import _band_case, _band_on
    _band_on(ttm_opt)
    _band_case(kind, N).search('k_band_few_bisect', poison, newton=False, rt_bound=1e-6)


# ---------------------------------------------------------------------------
# the call that starts on an odd row
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _odd_map(long):
    from tests.test_band import _build
    return _build('c5_shape', n=N_LONG) if long else _build('few_c2b', n=N_FEW)


def _odd_buffers(tm, N, Zdev, ldx=None):
    """Z (data in rows [0, N)) and X of the class's layout in canary-filled allocations; row 0 of X stays canary."""
    from tests.test_row_ownership import PAD, even_rows, guarded
    ld = even_rows(N) + PAD
    Z, _, _ = guarded(tm, N, tm.D, ld, PAD, Zdev, tm.D, poison='alt')
    X, raw, owned = guarded(tm, N, tm._cm.d_cols, ldx or ld, PAD, None, 0, poison='alt')
    owned[:tm._cm.d_cols * (ldx or ld)].view(tm._cm.d_cols, ldx or ld)[:, 0] = False
    return Z, ld, X, raw, owned


@pytest.mark.gpu
@pytest.mark.parametrize('long', [False, True], ids=['few', 'long'])
def test_a_call_that_starts_on_an_odd_row_is_split(long, ttm_opt):
    import torch
    tm, om, X, rng = _odd_map(long)
    kernel = 'k_band_bisect' if long else 'k_band_few_bisect'
    N, D = tm._N, tm.D
    ttm_opt('u_loader', 1); ttm_opt('band_fwd', 1)
    Zdev = tm.forward_device(tm._Xs, N)[:, :N].clone()
    # the aligned launch on a copy shifted down by one row
    Zsh = tm._cols(D, N - 1, zero=True)
    Zsh[:, :N - 1].copy_(Zdev[:, 1:])
    Xa, ita, name = _bisect(tm, Zsh, N - 1)
    assert name == kernel
    ttm_opt('band_bisect', 0)
    Xg, itg, name = _bisect(tm, Zsh, N - 1)
    assert name == 'k_inverse_bisect'
    ttm_opt('band_bisect', -1)
    # Z + 1 row, X + 1 row, N - 1 rows: both pointers 8 bytes past a 16-byte boundary, even leading dimensions
    res = []
    for row0 in (None, float('nan')):
        Z, ld, Xo, raw, owned = _odd_buffers(tm, N, Zdev)
        if row0 is not None:
            Z[:, 0] = row0
        assert tm._ptr(Z, 1).value % 16 == 8 and tm._ptr(Xo, 1).value % 16 == 8 and ld % 2 == 0
        before = raw.clone()
        it, name = _call(tm, Z, ld, Xo, ld, N - 1, zrow=1, xrow=1)
        assert name == kernel
        moved = (raw != before) & ~owned
        assert not bool(moved.any()), moved.nonzero().flatten()[:8].tolist()   # (row 0 of X among them: still the canary)
        res.append((Xo[:, 1:N].clone(), it))
    (X1, it1), (X2, it2) = res
    assert torch.equal(X1, X2) and np.array_equal(it1, it2)                 # NaN in the row in front changes no bit
    assert torch.equal(X1[:, 1:], Xa[:, 1:])                                # rows 2.. : the bits of the aligned launch
    assert float(((X1[:, 0] - Xg[:, 0]).abs() / (1 + Xg[:, 0].abs())).max().item()) < 1e-6
    assert np.all(np.abs(it1 - ita) <= 1) and np.all(np.abs(it1 - itg) <= 1)
    # only Z misaligned / an odd ldx: declined, not misread - the generic kernel's bits
    Z, ld, Xo, raw, owned = _odd_buffers(tm, N, Zdev)
    it, name = _call(tm, Z, ld, Xo, ld, N - 1, zrow=1, xrow=0)
    assert name == 'k_inverse_bisect'
    assert torch.equal(Xo[:, :N - 1], Xg)
    Z, ld, Xo, raw, owned = _odd_buffers(tm, N, Zdev, ldx=N if N % 2 else N + 1)
    before = raw.clone()
    it, name = _call(tm, Z, ld, Xo, Xo.shape[1], N - 1, zrow=1, xrow=1)
    assert name == 'k_inverse_bisect'
    assert torch.equal(Xo[:, 1:N], Xg)
    assert not bool(((raw != before) & ~owned).any())


# ---------------------------------------------------------------------------
# the default gate (no u_loader) and the public path
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _gate_map():
    from tests.test_band import _build
    return _build('c5_shape', n=65537)


@pytest.mark.gpu
def test_default_gate_of_the_direct_call(ttm_opt):
    import torch
    tm, om, X, rng = _gate_map()
    N, D = tm._N, tm.D
    Z = tm.forward_device(tm._Xs, N).clone()
    Xs = tm._cols(tm._cm.d_cols, N, zero=True)
    it, name = _call(tm, Z, Z.shape[1], Xs, Xs.shape[1], N - 1, zrow=1, xrow=1)      # 65 536 rows
    assert name == 'k_band_bisect'
    it, name = _call(tm, Z, Z.shape[1], Xs, Xs.shape[1], N - 2, zrow=1, xrow=1)      # 65 535 rows: below the gate
    assert name == 'k_inverse_bisect'
    it, name = _call(tm, Z, Z.shape[1], Xs, Xs.shape[1], N)                          # aligned, 65 537 rows
    assert name == 'k_band_bisect'
    cap = torch.full((D,), 100, dtype=torch.int32, device=Z.device)
    it, name = _call(tm, Z, Z.shape[1], Xs, Xs.shape[1], N, cap=cap)                 # a cap: the generic kernel at any size
    assert name == 'k_inverse_bisect'
    ttm_opt('band_bisect', 0)
    it, name = _call(tm, Z, Z.shape[1], Xs, Xs.shape[1], N)
    assert name == 'k_inverse_bisect'


@pytest.mark.gpu
def test_inverse_map_at_65537_runs_the_push_form_bisection(ttm_opt):
    """The public path: rows 1.. by the oracle contract on a subset; row 0 (the loop-guard quirk depends on the batch) finite,
    with the residual its cap allows.  The bound is 4 / 2^cap max dS where sample 0 was searched in [-2, 2]; it is LOOSER than
    that in two reasoned ways: a row that one window shift moved to [2, 10] / [-10, -2] has a bracket 8 wide (8 / 2^cap max dS;
    |x_0| < 10 is asserted, which rules out a second shift: that bracket starts at +-10), and a row that met the stopping rule
    before the cap stopped at |fm| <= 1e-9, which can exceed 4 / 2^cap max dS for cap >= 32: the floor is 2e-9, the contract's
    residual bound for every converged row."""
    import torch
    from tests.test_full_size import _last_kernel, subset_with_tails
    tm, om, X, rng = _gate_map()
    N, D = tm._N, tm.D
    tm.alternate_root_finding = False
    om.alternate_root_finding = False
    names, lib = [], tm._lib

    class Spy:                                              # (the name after each launch of the class: rows 1.., then sample 0)
        def __getattr__(self, attr):
            return getattr(lib, attr)

        def ttm_inverse_bisect(self, *args):
            rc = lib.ttm_inverse_bisect(*args)
            tm._sync_stream()
            names.append(_last_kernel(tm))
            return rc
    Z = tm.map(X)
    try:
        tm._lib = Spy()
        got = tm.inverse_map(Z)
    finally:
        tm._lib = lib
        tm.alternate_root_finding = True
    assert names == ['k_band_bisect', 'k_inverse_bisect'], names
    idx = subset_with_tails(X, 2000)
    idx = idx[idx > 0]
    ref = om.inverse_map(np.vstack((Z[:1], Z[idx])))[1:]
    ref_s, got_s = (ref - om.X_mean) / om.X_std, (got[idx] - om.X_mean) / om.X_std
    sane = np.all(np.abs(ref_s) < 50.0, axis=1)
    assert sane.mean() > 0.8
    assert np.abs(om.map(got[idx]) - Z[idx])[sane].max() < 2e-9
    assert (np.abs(got_s[sane] - ref_s[sane]) <= 1e-6 * (1 + np.abs(ref_s[sane]))).mean() > 0.98
    # row 0 under the cap the other rows set
    Zd = tm.forward_device(tm._Xs, N).clone()
    Xs = tm._cols(tm._cm.d_cols, N, zero=True)
    cap, _ = _call(tm, Zd, Zd.shape[1], Xs, Xs.shape[1], N - 1, zrow=1, xrow=1)
    assert np.all(np.isfinite(got[0]))
    x0 = (got[0] - om.X_mean) / om.X_std
    res0 = np.abs(om.map(got[:1]) - Z[:1])[0]
    for k in range(D):
        # the bracket of sample 0: [-2, 2], or the one a single window shift leaves ([2, 10] / [-10, -2], 8 wide)
        assert abs(x0[k]) < 10.0
        lo, hi = (-2.0, 2.0) if abs(x0[k]) < 2.0 else ((2.0, 10.0) if x0[k] > 0 else (-10.0, -2.0))
        g = np.linspace(lo, hi, 4001)
        pts = np.repeat(got[:1], len(g), axis=0)
        pts[:, k] = om.X_mean[k] + om.X_std[k] * g
        dS = float(np.max(np.abs(np.diff(om.map(pts)[:, k]) / (g[1] - g[0]))))
        bound = max((hi - lo) / 2.0 ** int(cap[k]) * dS, 2e-9)
        print('row 0, component', k, 'cap', int(cap[k]), 'max dS', dS, 'residual', res0[k], 'bound', bound)
        assert res0[k] <= bound
