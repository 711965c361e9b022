"""
Row ownership and padding independence of the per-sample entry points (include/ttm.h: "ldx >= N").

Every entry point is launched on GUARDED buffers: column-major matrices with ld = even_rows(N) + 64 in an allocation that is
one canary bit pattern (a quiet NaN with a payload) throughout, data in rows [0, N) of the input columns, POISON (NaN, +inf,
1e300, alternating +-1e300) in rows [N, ld) of the input columns; output vectors of N + 64 elements.  After the launch, in
this order:

  1. the kernel's name (ttm_last_kernel) is the expected one, and the same for the second launch of 3;
  2. ownership: everything but rows [0, N) of the outputs is unchanged as int64 - canary in the pads of the outputs and in the
     slack behind the last column, inputs bit for bit, pads included;
  3. padding independence: rows [0, N) of every output and every reduction result (iters, objective sums) equal, bit for bit,
     a second launch on the tight layout of the Python side (ld = even_rows(N), zero pads);
  4. correctness of rows [0, N) against the oracle, at the tolerance of the test that owns the kernel (tests/test_band.py,
     test_band_dispatch.py, test_band_newton.py, test_newton_inverse.py, test_kernels.py; smoke() for the objective).

Maps are trained on max(N, 64) rows and evaluated on their first N (tests/test_wide_conditioning.py).  The host test double
runs the generic, integrated and layout cases on the CPU, so the harness itself is exercised there; the band entry points
exist on the device only.

k_objective_sep_direct is not in here: ttm_objective_sep_direct_* take one column `xk` of exactly N rows and no leading
dimension, and tm.separable_objective hands them a column of the training ensemble the map object keeps (tm._Xs, tight
layout) - there is no pad row the caller could poison.
k_band_logdet's two instantiations (2 / 4 rows per thread, the switch at 3072 rows per chunk) have one kernel name and the
library has no hook that tells them apart: band_cus = 1 with N = 3071 and N = 3073 covers both sides of the switch.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case, make_oracle, relerr

PAD = 64
CANARY = 0x7FF8C0DEC0DEC0DE                         # quiet NaN, payload c0dec0dec0de
POISONS = ('nan', 'inf', 'big', 'alt')


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


def even_rows(N):
    return (int(N) + 1) & ~1


def _poison(kind, n):
    if kind == 'nan':
        return np.full(n, np.nan)
    if kind == 'inf':
        return np.full(n, np.inf)
    if kind == 'big':
        return np.full(n, 1e300)
    assert kind == 'alt'
    return 1e300 * (1.0 - 2.0 * (np.arange(n) % 2))


class Buf:
    """One buffer of a launch.  role 'in' | 'out' | 'inout' (the first `n_in` columns are inputs, the others outputs);
    `data`: ncols_in x N array (torch or NumPy) for the input columns; vec: a vector of N (+ PAD) elements, not a matrix."""

    def __init__(self, role, ncols=1, data=None, n_in=None, vec=False):
        self.role, self.ncols, self.data, self.vec = role, int(ncols), data, vec
        self.n_in = {'in': self.ncols, 'out': 0}.get(role, n_in)
        assert self.n_in is not None


def guarded(tm, N, ncols, ld, slack, data=None, n_in=0, poison=None, byte_offset=0):
    """(tensor ncols x ld, int64 view of the whole allocation, int64 mask of the elements a launch may write).  The whole
    allocation is CANARY; rows [0, N) of the first n_in columns hold `data`, their rows [N, ld) the poison (None: zeros
    everywhere instead of canary and poison - the tight layout of the Python side)."""
    import torch
    total = ncols * ld + slack + 2
    raw = torch.empty(total, dtype=torch.int64, device=tm._dev)
    assert raw.data_ptr() % 16 == 0
    raw.fill_(0 if poison is None else CANARY)
    off = byte_offset // 8
    whole = raw[off:]
    t = whole[:ncols * ld].view(torch.float64).view(ncols, ld)
    if n_in:
        src = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)).to(tm._dev)
        t[:n_in, :N].copy_(src[:n_in, :N])
        if poison is not None and ld > N:
            t[:n_in, N:] = torch.from_numpy(_poison(poison, ld - N)).to(tm._dev)
    owned = torch.zeros(total, dtype=torch.bool, device=tm._dev)
    owned[off:off + ncols * ld].view(ncols, ld)[n_in:, :N] = True
    return t, raw, owned


def run_guarded(tm, N, bufs, launch, kernel, poison, pad=PAD, check=None):
    """The four checks of the module docstring for one entry point.  launch(dict name -> tensor) -> dict of reduction results
    (NumPy arrays); kernel: the expected name or a collection of allowed names; check(dict name -> N-row NumPy outputs)."""
    from tests.test_full_size import _last_kernel
    res = {}
    for layout in ('guarded', 'tight'):
        t, raws = {}, {}
        for name, b in bufs.items():
            rows = N if b.vec else even_rows(N)
            ld = rows + (pad if layout == 'guarded' else 0)
            t[name], raw, owned = guarded(tm, N, b.ncols, ld, PAD if layout == 'guarded' else 0, b.data, b.n_in,
                                          poison if layout == 'guarded' else None)
            raws[name] = (raw, raw.clone(), owned)
            if b.vec:
                t[name] = t[name][0]
        red = launch(t)
        tm._sync_stream()
        name_ran = _last_kernel(tm)
        # 1. the kernel
        allowed = (kernel,) if isinstance(kernel, str) else tuple(kernel)
        assert name_ran in allowed, (name_ran, allowed)
        if layout == 'tight':
            assert name_ran == res['kernel'], (name_ran, res['kernel'])
        if layout == 'guarded':
            # 2. ownership
            for name, (raw, before, owned) in raws.items():
                moved = (raw != before) & ~owned
                if bool(moved.any()):
                    idx = moved.nonzero().flatten()[:8].tolist()
                    ld = t[name].shape[-1]
                    raise AssertionError('%s wrote outside rows [0, %d) of %r (ld %d): elements %s of the allocation, now %s'
                                         % (name_ran, N, name, ld, idx, [hex(v & (2 ** 64 - 1)) for v in raw[idx].tolist()]))
        out = {}
        for name, b in bufs.items():
            if b.role != 'in':
                out[name] = (t[name][:N] if b.vec else t[name][b.n_in:, :N]).contiguous().cpu().numpy()
        if layout == 'guarded':
            res = dict(kernel=name_ran, out=out, red=red)
        else:
            # 3. padding independence, bit for bit
            for name in out:
                a, b_ = res['out'][name].view(np.int64), out[name].view(np.int64)
                assert np.array_equal(a, b_), '%s: %r depends on the pad rows (%d elements differ)' % (name_ran, name, int((a != b_).sum()))
            assert sorted(red) == sorted(res['red'])
            for name in red:
                a, b_ = np.ascontiguousarray(res['red'][name]), np.ascontiguousarray(red[name])
                assert a.tobytes() == b_.tobytes(), '%s: reduction %r depends on the pad rows: %s / %s' % (name_ran, name, a, b_)
    # 4. correctness
    if check is not None:
        check(res['out'], res['red'])
    return res


# ---------------------------------------------------------------------------
# maps (one per case and training size) and their launches
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _band_map(kind, n):
    """(tm, om, X, E) of a banded separable map trained on n rows: 'c5_shape' / 'ring10' (tests/test_band.py), 'mixed'
    (tests/test_band_linear.py), 'few2' / 'few4' / 'few4c' (tests/test_band_dispatch.py; few4c: two conditioning columns)."""
    if kind == 'c5_shape':
        from tests.test_band import _build
        tm, om, X, _ = _build('c5_shape', n=n)
        return tm, om, X, 0
    if kind == 'ring10':
        from tests.test_band import _ring_map
        tm, om, X, _ = _ring_map(10, n=n)
        return tm, om, X, 0
    if kind == 'mixed':
        from tests.test_band_linear import _build
        tm, om, X, _ = _build('mixed', n=n)
        return tm, om, X, 0
    from tests.test_band_dispatch import _build
    cls, lag, reach, D, plain = {'few2': (1, 2, 1, 2, True), 'few4': (2, 3, 3, 4, False), 'few4c': (1, 5, 5, 4, True)}[kind]
    tm, om, X, _, E = _build(cls, lag, reach, D, plain, n=n)
    return tm, om, X, E


@functools.lru_cache(maxsize=4)
def _fixture_map(name, n, backend):
    """(tm, om, X, E) of a golden fixture's map on the first n of its training rows (backend: part of the cache key only)."""
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    X = case_X(name, npz)
    reps = -(-n // len(X))
    X = np.concatenate([X + 0.01 * i for i in range(reps)])[:n]
    tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **ctor_kwargs(desc))
    tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
    om = make_oracle(name, npz, desc, X=X)
    return tm, om, X, tm._cm.d_cols - tm.D, ctor_kwargs(desc)


class Case:
    """The launches of one map on the first N rows of its training ensemble."""

    def __init__(self, tm, om, X, E, N, okw=None):
        self.tm, self.om, self.E, self.N, self.okw = tm, om, E, N, okw
        self.D, self.d = tm.D, tm._cm.d_cols
        self.X = X[:N]
        self.Xs = tm._Xs[:, :N]                                            # standardised device columns
        self.sigma = tm._to_dev(np.asarray(tm.X_std[E:E + self.D], dtype=float))
        self.sep = tm.monotonicity.lower() == 'separable monotonicity'

    # ---- oracle results, once per case ----
    @functools.cached_property
    def Zo(self):
        return self.om.map(self.X)

    @functools.cached_property
    def ldo(self):
        with np.errstate(all='ignore'):
            return self.om._log_determinant((self.X - self.om.X_mean) / self.om.X_std, skip_in_std=True)

    @functools.cached_property
    def om_rows(self):
        """An oracle whose training ensemble is the N standardised rows themselves (no special terms, no regularisation in the
        fixture it is used for): its objective and gradient are the reference of the kernels' sums over these rows."""
        from oracle.ttm_oracle import OracleMap
        om = self.om
        assert om.regularization is None
        rows = ((self.X - om.X_mean) / om.X_std).copy()
        return OracleMap(X=rows, monotone=om.monotone, nonmonotone=om.nonmonotone, standardize_samples=False, **self.okw)

    @functools.cached_property
    def Zin(self):
        Zin = np.random.default_rng(7 + self.N).standard_normal((self.N, self.D))
        Zin[:max(1, self.N // 50)] *= 3.5                                   # (targets beyond the resident window and the tables)
        return Zin

    @functools.cached_property
    def Xo_table(self):
        return self.om.inverse_map(self.Zin, X_star=self.X[:, :self.E] if self.E else None)

    @functools.cached_property
    def Zdev(self):
        """S(x) of the rows by the library, tight layout: the targets of the root searches' round trips."""
        return self.tm.forward_device(self._tight(self.Xs), self.N)[:, :self.N].clone()

    def _tight(self, cols):
        out = self.tm._cols(cols.shape[0], self.N, zero=True)
        out[:, :self.N].copy_(cols)
        return out

    def _raw(self, Xstd):
        """standardised d-column output (NumPy, columns x N) -> raw samples N x D of the map's own columns"""
        return (Xstd * np.asarray(self.tm.X_std)[self.E:, None] + np.asarray(self.tm.X_mean)[self.E:, None]).T

    # ---- forward ----
    def forward(self, kernel, poison, Z=True, logdet=False, sumsq=False, tol_z=1e-11):
        tm, N = self.tm, self.N
        bufs = {'X': Buf('in', self.d, self.Xs)}
        if Z:
            bufs['Z'] = Buf('out', self.D)
        if logdet:
            bufs['logdet'] = Buf('out', vec=True)
        if sumsq:
            bufs['sumsq'] = Buf('out', vec=True)

        def launch(t):
            if Z:
                tm.forward_device(t['X'], N, Z=t['Z'], logdet=t.get('logdet'), sigma=self.sigma if logdet else None, sumsq=t.get('sumsq'))
            else:
                tm.density_device(t['X'], N, logdet=t.get('logdet'), sigma=self.sigma if logdet else None, sumsq=t.get('sumsq'))
            return {}

        def check(out, red):
            if Z:
                assert relerr(out['Z'].T, self.Zo) < tol_z, ('forward', relerr(out['Z'].T, self.Zo))
            if logdet:
                ok = np.isfinite(self.ldo)
                assert np.array_equal(np.isfinite(out['logdet']), ok)
                assert relerr(out['logdet'][ok], self.ldo[ok]) < 1e-10
            if sumsq:
                assert relerr(out['sumsq'], np.sum(self.Zo ** 2, axis=1)) < 1e-11
        return run_guarded(tm, N, bufs, launch, kernel, poison, check=check)

    # ---- table inverse ----
    def inverse_table(self, kernel, poison, tol=1e-11):
        tm, N = self.tm, self.N
        bufs = {'Z': Buf('in', self.D, self.Zin.T), 'X': Buf('inout', self.d, self.Xs, n_in=self.E)}

        def launch(t):
            tm.inverse_device(t['Z'], N, X=t['X'], table=True)
            return {}

        def check(out, red):
            assert relerr(self._raw(out['X']), self.Xo_table) < tol, ('table inverse', relerr(self._raw(out['X']), self.Xo_table))
        return run_guarded(tm, N, bufs, launch, kernel, poison, check=check)

    # ---- forward + table inverse in one launch ----
    def roundtrip(self, kernel, poison, dens):
        tm, N = self.tm, self.N
        bufs = {'X': Buf('in', self.d, self.Xs), 'Z': Buf('out', self.D), 'Xr': Buf('out', self.d)}
        if dens:
            bufs['logdet'], bufs['sumsq'] = Buf('out', vec=True), Buf('out', vec=True)

        def launch(t):
            tm.roundtrip_device(t['X'], N, Z=t['Z'], Xr=t['Xr'], logdet=t.get('logdet'), sigma=self.sigma if dens else None, sumsq=t.get('sumsq'))
            return {}

        def check(out, red):
            assert relerr(out['Z'].T, self.Zo) < 1e-11
            star = self.X[:, :self.E] if self.E else None
            assert relerr(self._raw(out['Xr'][self.E:]), self.om.inverse_map(out['Z'].T.copy(), X_star=star)) < 1e-11
            if self.E:
                assert np.array_equal(out['Xr'][:self.E], self.Xs[:self.E].cpu().numpy())
            if dens:
                ok = np.isfinite(self.ldo)
                assert relerr(out['logdet'][ok], self.ldo[ok]) < 1e-10 and relerr(out['sumsq'], np.sum(self.Zo ** 2, axis=1)) < 1e-11
        return run_guarded(tm, N, bufs, launch, kernel, poison, check=check)

    # ---- root searches: targets S(x), so that the roots are the rows themselves ----
    def search(self, kernel, poison, newton, rt_bound):
        import torch
        tm, N = self.tm, self.N
        bufs = {'Z': Buf('in', self.D, self.Zdev), 'X': Buf('inout', self.d, self.Xs, n_in=self.E)}
        coef = tm._pack_coeffs()

        def launch(t):
            iters = tm._zeros(self.D, dtype=torch.int32)
            args = (tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, self.D, tm._ptr(t['Z']), t['Z'].shape[1], tm._ptr(t['X']),
                    t['X'].shape[1], N, ctypes.c_void_p(iters.data_ptr()))
            rc = tm._lib.ttm_inverse_newton(*args, tm._stream()) if newton else tm._lib.ttm_inverse_bisect(*args, None, tm._stream())
            assert rc == 0, rc
            tm._sync_stream()
            return {'iters': iters.cpu().numpy().copy()}

        def check(out, red):
            # the stopping rule |S - z| <= 1e-9 under the ORACLE's forward map (tests/test_newton_inverse.py: < 2e-9), and the
            # round trip of the rows (tests/test_band_newton.py: < 1e-7 for the Newton searches)
            got = np.column_stack((self.X[:, :self.E], self._raw(out['X'])))
            assert np.abs(self.om.map(got) - self.Zdev.T.cpu().numpy()).max() < 2e-9
            rt = float(np.abs(out['X'] - self.Xs[self.E:].cpu().numpy()).max())
            assert rt < rt_bound, ('round trip', rt)
            # (a 1e300 target in a pad row would send its search to the 100-point limit)
            assert 0 < red['iters'].max() < 100, red['iters']
        return run_guarded(tm, N, bufs, launch, kernel, poison, check=check)

    # ---- objective + gradient sums of component k: ttm_objective_host (coefficients as kernel arguments; the X-program kernel
    # k_int_objective where the component has one) or ttm_objective (coefficients on the device) ----
    def objective(self, kernel, poison, k=None, host=False):
        import torch
        tm, N = self.tm, self.N
        k = self.D - 1 if k is None else k
        div = len(tm.coeffs_nonmon[k])
        c = np.ascontiguousarray(0.2 * np.random.default_rng(k).standard_normal(div + len(tm.coeffs_mon[k])))
        nout = 1 + int(tm._cm.n_mon[k]) + (0 if self.sep else int(tm._cm.n_nm[k]))
        assert not self.sep and nout == 1 + len(c)
        ck = tm._to_dev(c)

        def launch(t):
            work = tm._empty(int(tm._lib.ttm_reduce_work_size(nout)))
            if host:
                out = torch.zeros(256, dtype=torch.float64, pin_memory=tm._dev.type == 'cuda')
                cnt = tm._zeros(16, dtype=torch.int32)
                rc = tm._lib.ttm_objective_host(tm._pp, int(k), ctypes.c_void_p(c.ctypes.data), tm._ptr(t['X']), t['X'].shape[1], N,
                                                tm._ptr(work), ctypes.c_void_p(cnt.data_ptr()), ctypes.c_void_p(out.data_ptr()), tm._stream())
            else:
                out = tm._empty(nout)
                rc = tm._lib.ttm_objective(tm._pp, int(k), tm._ptr(ck), tm._ptr(t['X']), t['X'].shape[1], N, tm._ptr(work), tm._ptr(out), tm._stream())
            assert rc == 0, rc
            tm._sync_stream()
            return {'sums': out[:nout].cpu().numpy().copy()}

        def check(out, red):
            # J = sums[0] / N, grad J = sums[1:] / N (transport_map._objective_and_gradient; the fixtures have no regularisation)
            o = self.om_rows
            assert relerr(red['sums'][0] / N, o.objective_function(c, k, div)) < 1e-10
            assert relerr(red['sums'][1:] / N, o.objective_function_jacobian(c, k, div)) < 1e-10
        return run_guarded(tm, N, {'X': Buf('in', self.d, self.Xs)}, launch, kernel, poison, check=check)


def _band_case(kind, N):
    tm, om, X, E = _band_map(kind, max(N, 64))
    return Case(tm, om, X, E, N)


def _band_on(ttm_opt, cus=-1, block=-1, ring=-1):
    for name, v in (('u_loader', 1), ('band_fwd', 1), ('band_inv', 1), ('band_cus', cus), ('rt_block', block), ('band_ring', ring)):
        ttm_opt(name, v)


# every N with one poison kind, every poison kind at one odd and one even N
def _sweep(Ns, odd, even):
    return [(n, 'alt') for n in Ns] + [(n, p) for n in (odd, even) for p in POISONS if p != 'alt']


LONG_DEFAULT = _sweep((1, 2, 3, 31, 32, 33, 65, 1023, 1025, 2049), 33, 32)
LONG_ONE_WG = [(n, 'alt') for n in (1023, 1024, 1025, 2047, 2049, 3071, 3073, 4097)]
LONG_FEW_WG = [(2, 33), (2, 65), (3, 33), (3, 65), (2, 2 * 1056 - 1), (3, 2 * 1056 - 1)]
FEW_NS = _sweep((1, 2, 2047, 2048, 2049, 4097), 2049, 2048)
GENERIC_NS = _sweep((1, 2, 63, 65, 257, 1025), 65, 2)


def _long(case, poison):
    """Every long-band forward and search kernel on one case."""
    case.forward('k_band_forward', poison)
    case.forward('k_band_density', poison, logdet=True, sumsq=True)
    case.forward('k_band_density', poison, Z=False, logdet=True, sumsq=True)
    case.forward('k_band_logdet', poison, Z=False, logdet=True)
    case.search('k_band_newton', poison, newton=True, rt_bound=1e-7)


def _long_inverse(case, poison, ttm_opt, ring, block=-1):
    ttm_opt('band_ring', ring)
    case.tm._pack_memo = None                               # (a fresh coefficient vector: tables and images under these options)
    # (a ring needs twelve slots, or every component resident: a small rt_block leaves the block kernel)
    case.inverse_table('k_band_inverse_ring' if ring and block < 0 else 'k_band_inverse', poison)
    ttm_opt('band_ring', -1)


@pytest.mark.gpu
@pytest.mark.parametrize('N,poison', LONG_DEFAULT)
@pytest.mark.parametrize('kind', ['c5_shape', 'mixed'])
def test_long_band_kernels_default_chunks(kind, N, poison, ttm_opt):
    """A chunk of 32 rows per workgroup at these sizes: N = 32 k + 1 leaves the last workgroup a single row."""
    _band_on(ttm_opt)
    case = _band_case(kind, N)
    _long(case, poison)
    _long_inverse(case, poison, ttm_opt, ring=0)


@pytest.mark.gpu
@pytest.mark.parametrize('N,poison', LONG_DEFAULT)
def test_ring_inverse_default_chunks(N, poison, ttm_opt):
    _band_on(ttm_opt)
    case = _band_case('ring10', N)
    _long_inverse(case, poison, ttm_opt, ring=1)
    _long_inverse(case, poison, ttm_opt, ring=0)


@pytest.mark.gpu
@pytest.mark.parametrize('N,poison', LONG_ONE_WG)
def test_long_band_kernels_one_workgroup_several_tiles(N, poison, ttm_opt):
    """band_cus = 1: one workgroup walks the tiles; 3071 / 3073 rows are the two sides of k_band_logdet's switch from two to
    four rows per thread (3072 rows per chunk)."""
    _band_on(ttm_opt, cus=1)
    case = _band_case('c5_shape', N)
    _long(case, poison)
    _long_inverse(case, poison, ttm_opt, ring=0)
    ring = _band_case('ring10', N)
    _long_inverse(ring, poison, ttm_opt, ring=1)


@pytest.mark.gpu
@pytest.mark.parametrize('cus,N', LONG_FEW_WG)
def test_long_band_kernels_two_and_three_workgroups(cus, N, ttm_opt):
    """The last chunk has one row (N = 33, 65) or is one row short (N = 2 x 1056 - 1)."""
    _band_on(ttm_opt, cus=cus)
    case = _band_case('mixed', N)
    _long(case, 'alt')
    _long_inverse(case, 'alt', ttm_opt, ring=0)
    _long_inverse(_band_case('ring10', N), 'alt', ttm_opt, ring=1)


@pytest.mark.gpu
@pytest.mark.parametrize('block', [-1, 1, 2])
def test_long_band_kernels_with_block_boundaries(block, ttm_opt):
    """rt_block cuts the components into residency blocks: a block boundary inside the sweep, an odd N, several tiles."""
    _band_on(ttm_opt, cus=2, block=block)
    case = _band_case('c5_shape', 2049)
    _long(case, 'alt')
    _long_inverse(case, 'alt', ttm_opt, ring=0, block=block)
    _long_inverse(_band_case('ring10', 2049), 'alt', ttm_opt, ring=1, block=block)


@pytest.mark.gpu
@pytest.mark.parametrize('N,poison', FEW_NS)
@pytest.mark.parametrize('kind', ['few2', 'few4c'])
def test_few_component_kernels(kind, N, poison, ttm_opt):
    """Tiles of 2048 rows; few4c has conditioning columns (inputs of the inverse kernels' in/out X: poisoned pads)."""
    _band_on(ttm_opt)
    case = _band_case(kind, N)
    case.forward('k_band_few', poison)
    case.forward('k_band_few<density>', poison, logdet=True, sumsq=True)
    case.inverse_table('k_band_few_inverse', poison)
    case.search('k_band_few_newton', poison, newton=True, rt_bound=1e-7)
    ttm_opt('roundtrip_fused', 1)
    case.roundtrip('k_band_few_roundtrip', poison, dens=False)
    case.roundtrip('k_band_few_roundtrip<density>', poison, dens=True)


@pytest.mark.gpu
def test_few_component_kernels_reach_three(ttm_opt):
    _band_on(ttm_opt)
    case = _band_case('few4', 2049)
    case.forward('k_band_few', 'alt')
    case.inverse_table('k_band_few_inverse', 'alt')
    case.search('k_band_few_newton', 'alt', newton=True, rt_bound=1e-7)


# ---------------------------------------------------------------------------
# generic kernels (bands off) and integrated-rectifier kernels: the host test double too
# ---------------------------------------------------------------------------
def _fixture_case(name, N, backend):
    tm, om, X, E, okw = _fixture_map(name, max(N, 64), backend)
    return Case(tm, om, X, E, N, okw)


def _names(backend, *names):
    return ('hostemu',) if backend == 'hostemu' else names


def _bands_off(ttm_opt):
    for name in ('band_fwd', 'band_inv', 'band_newton'):
        ttm_opt(name, 0)


# What ttm_forward / ttm_inverse_table take for a fixture with the bands off, aligned buffers and N < 65 536 follows from its plan
# (csrc/ttm_kernels.hip): u - it has a U-form; hot - the hot-record kernels sweep its records themselves (hot_sweepable:
# classes 1-3, records of 2 or 4 groups, lag <= 2); fast - no component needs the generic evaluator (all_fast: bit 0 of `complex`).
#   c3_sep   U-form, records of lag 3: k_forward_u / k_forward_ul by u_loader, the table inverse always k_inverse_table;
#   c5_sep   U-form, hot records of two groups, band 2: under u_loader = 1 k_forward_hl and k_inverse_rt<band>
#            (option rt_band = 0: k_inverse_rt);
#   misc_sep no U-form, components the planned cache cannot take: k_forward.
# A U-form map with option no_uform = 1 takes k_forward_plan, with no_plan = 1 k_forward.
GENERIC_PLAN = {'c3_sep': dict(u=True, hot=False, fast=True), 'c5_sep': dict(u=True, hot=True, fast=True),
                'misc_sep': dict(u=False, hot=False, fast=False)}
HOT_NS = [(1, 'alt'), (2, 'alt'), (65, 'alt'), (513, 'alt'), (1025, 'alt'), (65, 'nan'), (2, 'inf')]


def _plan(case, name):
    cm = case.tm._cm
    u = bool(cm.u_enabled)
    plan = dict(u=u, hot=u and 1 <= cm.u_h_cls <= 3 and cm.u_h_ng in (2, 4) and cm.u_p_lag <= 2,
                fast=not any(int(c) & 1 for c in np.asarray(cm.complex)[:case.D]))
    assert plan == GENERIC_PLAN[name], (name, plan)
    return plan


def _forward_and_table_inverse(case, backend, poison, fwd, inv):
    case.forward(_names(backend, fwd), poison)
    case.forward(_names(backend, fwd), poison, logdet=True, sumsq=True)
    case.inverse_table(_names(backend, inv), poison)


@pytest.mark.parametrize('N,poison', GENERIC_NS)
@pytest.mark.parametrize('name', ['c3_sep', 'misc_sep'])
def test_generic_separable_kernels(backend, name, N, poison, ttm_opt):
    _bands_off(ttm_opt)
    case = _fixture_case(name, N, backend)
    plan = _plan(case, name)
    for loader in (0, 1):
        ttm_opt('u_loader', loader)
        fwd = ('k_forward_ul' if loader else 'k_forward_u') if plan['u'] else 'k_forward'
        _forward_and_table_inverse(case, backend, poison, fwd, 'k_inverse_table')
    ttm_opt('u_loader', -1)
    if plan['u']:
        ttm_opt('no_uform', 1)
        case.forward(_names(backend, 'k_forward_plan'), poison)
        case.forward(_names(backend, 'k_forward_plan'), poison, logdet=True, sumsq=True)
        ttm_opt('no_uform', 0)
        ttm_opt('no_plan', 1)
        case.forward(_names(backend, 'k_forward'), poison)
        ttm_opt('no_plan', 0)
    # (the rows as targets: the reference's bisection and the generic Newton search find them again; tests/test_newton_inverse.py)
    case.search(_names(backend, 'k_inverse_bisect'), poison, newton=False, rt_bound=1e-6)
    case.search(_names(backend, 'k_inverse_newton'), poison, newton=True, rt_bound=1e-6)


@pytest.mark.parametrize('N,poison', HOT_NS)
def test_hot_record_kernels(backend, N, poison, ttm_opt):
    """c5_sep with the bands off and u_loader = 1: k_forward_hl with two and four samples per evaluating thread (hl_ns: tiles of
    512 / 1024 rows, so N = 513 and 1025 leave a tile one row) and k_inverse_rt with the register shift and with the LDS
    column cache (rt_band = 0)."""
    _bands_off(ttm_opt)
    case = _fixture_case('c5_sep', N, backend)
    assert _plan(case, 'c5_sep')['hot']
    ttm_opt('u_loader', 1)
    for hl_ns in (-1, 2, 4):
        ttm_opt('hl_ns', hl_ns)
        _forward_and_table_inverse(case, backend, poison, 'k_forward_hl', 'k_inverse_rt<band>')
    ttm_opt('hl_ns', -1)
    ttm_opt('rt_band', 0)
    case.inverse_table(_names(backend, 'k_inverse_rt'), poison)
    ttm_opt('rt_band', -1)
    ttm_opt('u_loader', 0)
    _forward_and_table_inverse(case, backend, poison, 'k_forward_u', 'k_inverse_table')


@pytest.mark.parametrize('ns', [2, 4])
@pytest.mark.parametrize('name', ['c3_sep', 'c2a_int'])
def test_multi_sample_variants(backend, name, ns, ttm_opt):
    """The TTM_NS kernels of tests/test_kernels.py::test_multi_sample_kernel_variants at N = 2 ns x 64 + 1: a last thread
    with one row of its ns.  (Its hl_ns = 2 / 4 part: test_hot_record_kernels - c3_sep has no hot-record kernel.)"""
    _bands_off(ttm_opt)
    for opt, v in (('forward_ns', ns), ('inverse_ns', 2), ('u_ns', ns), ('u_loader', 0)):
        ttm_opt(opt, v)
    case = _fixture_case(name, 2 * ns * 64 + 1, backend)
    if case.sep:
        _forward_and_table_inverse(case, backend, 'alt', 'k_forward_u', 'k_inverse_table')
        ttm_opt('no_uform', 1)
        case.forward(_names(backend, 'k_forward_plan'), 'alt')               # (two samples per thread at most)
        ttm_opt('no_uform', 0)
        ttm_opt('no_plan', 1)
    else:
        ttm_opt('int_dense', 0)
    case.forward(_names(backend, 'k_forward'), 'alt')                        # (ns samples per thread)


@pytest.mark.parametrize('N,poison', GENERIC_NS)
def test_integrated_kernels(backend, N, poison, ttm_opt):
    case = _fixture_case('c2a_int', N, backend)
    case.forward(_names(backend, 'k_int_forward'), poison)
    ttm_opt('int_xprog', 0)
    case.forward(_names(backend, 'k_int_forward<walk>'), poison)
    ttm_opt('int_xprog', -1)
    case.search(_names(backend, 'k_int_root<bisect>'), poison, newton=False, rt_bound=1e-6)
    ttm_opt('int_xprog', 2)                                                 # (the root searches on the X program)
    case.search(_names(backend, 'k_int_root_x<bisect>'), poison, newton=False, rt_bound=1e-6)
    ttm_opt('int_xprog', -1)
    a = case.objective(_names(backend, 'k_int_objective'), poison, host=True)
    w = case.objective(_names(backend, 'k_int_objective_walk'), poison)
    ttm_opt('int_dense', 0)
    b = case.objective(_names(backend, 'k_objective'), poison)
    bh = case.objective(_names(backend, 'k_objective'), poison, host=True)
    case.forward(_names(backend, 'k_forward'), poison)                      # (the device library runs c2a_int's generic forward map on k_forward)
    # (each launch was held against an oracle on these N rows, 1e-10; and against each other - the sums' order differs)
    for other in (a, w, bh):
        assert relerr(other['red']['sums'], b['red']['sums']) < 1e-10


def test_objective_sums_against_the_oracle(backend, ttm_opt):
    """Every component on the whole training ensemble: the guarded launch against an oracle on the rows (Case.objective), the
    class against the fixture's oracle (1e-10, as smoke()), and the guarded launch gives the sums the class works with."""
    case = _fixture_case('c2a_int', 257, backend)
    tm, om = case.tm, case.om
    for k in range(tm.D):
        div = len(tm.coeffs_nonmon[k])
        got = case.objective(_names(backend, 'k_int_objective'), 'alt', k=k, host=True)['red']['sums']
        c = 0.2 * np.random.default_rng(k).standard_normal(div + len(tm.coeffs_mon[k]))
        assert abs(tm.objective_function(c, k, div) - om.objective_function(c, k, div)) < 1e-10
        assert relerr(tm.objective_function_jacobian(c, k, div), om.objective_function_jacobian(c, k, div)) < 1e-10
        # ... and the guarded launch gives the sums objective_function is made of, bit for bit
        assert np.array_equal(got, tm._device_sums(k, c))


# ---------------------------------------------------------------------------
# layout kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('N,d,poison', [(257, 63, 'alt'), (257, 64, 'nan'), (257, 65, 'alt'), (1, 3, 'inf'), (2, 65, 'big'), (1025, 5, 'alt')])
def test_layout_kernels(backend, N, d, poison):
    """ttm_import / ttm_export (tiles of 64 columns: blockIdx.y tiles and a partial one at d = 63, 64, 65),
    ttm_standardize_cols and ttm_map_columns: the same IEEE operations as NumPy, element for element."""
    from tests.test_kernels import small_map
    tm = small_map()
    rng = np.random.default_rng(N + d)
    X = rng.standard_normal((N, d)) * rng.uniform(0.5, 3, d) + rng.uniform(-2, 2, d)
    mean, sd = X.mean(axis=0), X.std(axis=0) + 0.5
    mean_d, sd_d = tm._to_dev(mean), tm._to_dev(sd)
    Xrow = tm._to_dev(X)
    st = tm._stream()
    ref = (X - mean) / sd
    flat = '_flat' if d <= 64 else ''                                       # (up to 64 columns: one tile of columns per workgroup)

    def imp(t):
        assert tm._lib.ttm_import(tm._ptr(Xrow), N, d, tm._ptr(mean_d), tm._ptr(sd_d), tm._ptr(t['Xs']), t['Xs'].shape[1], st) == 0
        return {}
    run_guarded(tm, N, {'Xs': Buf('out', d)}, imp, _names(backend, 'k_import' + flat), poison,
                check=lambda out, red: np.testing.assert_array_equal(out['Xs'], ref.T))

    def exp(t):
        back = tm._empty(N + 1, d).fill_(-7.0)                             # (a row behind the row-major result)
        assert tm._lib.ttm_export(tm._ptr(t['Xs']), t['Xs'].shape[1], N, 0, d, tm._ptr(mean_d), tm._ptr(sd_d), tm._ptr(back), st) == 0
        tm._sync_stream()
        return {'rows': back.cpu().numpy().copy()}

    def exp_check(out, red):
        assert np.array_equal(red['rows'][:N], ref * sd + mean) and np.all(red['rows'][N] == -7.0)
    run_guarded(tm, N, {'Xs': Buf('in', d, ref.T)}, exp, _names(backend, 'k_export' + flat), poison, check=exp_check)

    def std(t):
        assert tm._lib.ttm_standardize_cols(tm._ptr(t['Xc']), t['Xc'].shape[1], N, d, tm._ptr(mean_d), tm._ptr(sd_d), tm._ptr(t['Xs']),
                                            t['Xs'].shape[1], st) == 0
        return {}
    run_guarded(tm, N, {'Xc': Buf('in', d, X.T), 'Xs': Buf('out', d)}, std, _names(backend, 'k_standardize_cols'), poison,
                check=lambda out, red: np.testing.assert_array_equal(out['Xs'], ref.T))

    nc = min(d, 16)
    src = (np.arange(nc)[::-1] % d).astype(np.int32)
    if nc > 2:
        src[1] = -1                                                          # a constant column
    scale, shift = rng.uniform(0.5, 2, nc), rng.uniform(-1, 1, nc)

    def mapc(t):
        tm.map_columns(src, nc, N, source=t['in'], scale=scale, shift=shift, out=t['out'])
        return {}

    def mapc_check(out, red):
        want = np.where(src[:, None] >= 0, X.T[np.maximum(src, 0)] * scale[:, None], 0.0) + shift[:, None]
        assert np.array_equal(out['out'], want)
    run_guarded(tm, N, {'in': Buf('in', d, X.T), 'out': Buf('out', nc)}, mapc, _names(backend, 'k_map_columns'), poison, check=mapc_check)


# ---------------------------------------------------------------------------
# buffers the vector kernels cannot take: the entry points decline to the generic kernels (or say TTM_E_UNSUPPORTED)
# ---------------------------------------------------------------------------
def _loose(tm, N, ncols, ld, data, n_in, byte_offset=0):
    return guarded(tm, N, ncols, ld, PAD, data, n_in, poison='alt' if ld > N else 'nan', byte_offset=byte_offset)


def _untouched(raw, before, owned, what):
    moved = (raw != before) & ~owned
    assert not bool(moved.any()), '%s: wrote outside its rows at %s' % (what, moved.nonzero().flatten()[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize('layout', ['odd_ld', 'offset8', 'odd_ldz_only'])
@pytest.mark.parametrize('kind', ['c5_shape', 'few2'])
def test_buffers_the_band_kernels_cannot_take_go_to_the_generic_kernels(kind, layout, ttm_opt):
    """N = 2049.  odd_ld: every matrix with ld = N, columns back to back ("beyond" is the slack behind the last column);
    offset8: even ld, base pointers 8 bytes into an aligned allocation; odd_ldz_only: only the Z of ttm_forward / ttm_roundtrip
    and the Z of the inverses has ld = N (ttm_band::forward passes need = 0 for Z: the parity of ldz must decline it).
    ttm_forward, ttm_inverse_table and ttm_inverse_newton return 0 and run a generic kernel; ttm_roundtrip returns
    TTM_E_UNSUPPORTED and writes nothing - for both maps."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    from tests.test_full_size import _last_kernel
    N = 2049
    _band_on(ttm_opt)
    ttm_opt('roundtrip_fused', 1)
    case = _band_case(kind, N)
    tm, D, d, E = case.tm, case.D, case.d, case.E
    coef = tm._pack_coeffs()
    p, c, f, st = tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._stream()

    def geom(is_z):
        if layout == 'odd_ld':
            return N, 0
        if layout == 'offset8':
            return even_rows(N) + PAD, 8
        return (N, 0) if is_z else (even_rows(N) + PAD, 0)

    def alloc(ncols, data, n_in, is_z=False):
        ld, off = geom(is_z)
        t, raw, owned = _loose(tm, N, ncols, ld, data, n_in, byte_offset=off)
        assert (t.data_ptr() % 16 == 0) == (off == 0)
        return t, raw, raw.clone(), owned, ld

    def band_ok(*bufs):
        return all(t.data_ptr() % 16 == 0 and ld % 2 == 0 and ld >= even_rows(N) for t, _, _, _, ld in bufs)

    def settle(what, bufs, rc=0):
        tm._sync_stream()
        name = _last_kernel(tm)
        assert rc == 0, (what, rc)
        assert band_ok(*bufs) or not name.startswith('k_band'), (what, name)
        for t, raw, before, owned, ld in bufs:
            _untouched(raw, before, owned, what + ' -> ' + name)
        return name

    # ---- ttm_forward ----
    Xb = alloc(d, case.Xs, d)
    Zb = alloc(D, None, 0, is_z=True)
    rc = tm._lib.ttm_forward(p, c, f, tm._ptr(Xb[0]), Xb[4], N, 0, D, tm._ptr(Zb[0]), Zb[4], None, None, None, st)
    settle('ttm_forward', (Xb, Zb), rc)
    Zgot = Zb[0][:, :N].cpu().numpy()
    assert relerr(Zgot.T, case.Zo) < 1e-11
    # ---- ttm_inverse_table on the default tables ----
    Zi = alloc(D, case.Zin.T, D, is_z=True)
    Xi = alloc(d, case.Xs, E)
    tm.inverse_device(Zi[0], N, X=Xi[0], table=True)
    settle('ttm_inverse_table', (Zi, Xi))
    assert relerr(case._raw(Xi[0][E:, :N].cpu().numpy()), case.Xo_table) < 1e-11
    # ---- ttm_inverse_newton: the rows as roots ----
    Zn = alloc(D, case.Zdev, D, is_z=True)
    Xn = alloc(d, case.Xs, E)
    iters = tm._zeros(D, dtype=torch.int32)
    rc = tm._lib.ttm_inverse_newton(p, c, f, 0, D, tm._ptr(Zn[0]), Zn[4], tm._ptr(Xn[0]), Xn[4], N, ctypes.c_void_p(iters.data_ptr()), st)
    settle('ttm_inverse_newton', (Zn, Xn), rc)
    assert float((Xn[0][E:, :N] - case.Xs[E:]).abs().max().item()) < 1e-6
    assert 0 < int(iters.max().item()) < 100
    # ---- ttm_roundtrip: the documented TTM_E_UNSUPPORTED (the caller then makes the two calls), nothing written.  None of the
    # three layouts satisfies col_ok for all of X, Z and Xr, so the one launch is never taken; the long map is declined for its
    # number of components whatever the buffers (ttm_band::roundtrip: more than TTM_P_FEW_D).  Return code 0 with the fused
    # kernel by name is test_few_component_kernels' ----
    resolution, start_distance, nb = 1001, 10, tm._inv_nb()
    tm._inverse_table(coef, 0, D, None, None, 0, resolution, start_distance)
    out_d, tmin_d, tmax_d, bkt_d, is_sorted, _ = coef._ttm_tables[(0, D, resolution, start_distance, nb)]
    assert is_sorted
    Xb = alloc(d, case.Xs, d)
    Zb = alloc(D, None, 0, is_z=True)
    Xr = alloc(d, None, 0)
    assert not band_ok(Xb, Zb, Xr)
    rc = tm._lib.ttm_roundtrip(p, c, f, tm._ptr(Xb[0]), Xb[4], N, tm._ptr(Zb[0]), Zb[4], tm._ptr(Xr[0]), Xr[4], None, None, None,
                               tm._ptr(out_d), resolution, tm._pts_affine, tm._ptr(tmin_d), tm._ptr(tmax_d),
                               ctypes.c_void_p(bkt_d.data_ptr()), nb, st)
    assert rc == _capi.TTM_E_UNSUPPORTED, rc
    tm._sync_stream()
    for t, raw, before, owned, ld in (Xb, Zb, Xr):
        _untouched(raw, before, torch.zeros_like(owned), 'ttm_roundtrip (declined)')
