"""
The table inverse's index (ttm_inverse_table_index) and every lookup kernel behind ttm_inverse_table, held to NumPy at
every node of their tables.

The other tests feed the lookup kernels random Gaussian targets and compare at relerr < 1e-11.  Linear interpolation is
continuous across a node, so that check cannot see a neighbouring interval picked for a target at or next to a node, and
its 5000 rows almost never contain the targets at which a bucket edge or a window edge picks an interval far off.  Here:

1. the index against its definition - tmin / tmax, the sortedness flag and bkt[q] = #{entries whose bucket is below q}
   with the bucket function restated in exact rational arithmetic (`bucket_of`) - on tables with ties, flat ends, one
   value, ranges whose scale degenerates, a crowded bucket, a descending pair and a NaN;
2. exact-target sweeps: a separable banded map whose nonmonotone coefficients are all 0.0 has offset +-0, so that the
   search target IS Z[n, k] to the bit.  Column k of Z holds every entry of component k's table and its two neighbours in
   double precision, every interval midpoint, every bucket boundary with its neighbours, the table's and the resident
   windows' ends with theirs, points beyond both ends, +-inf and NaN; every kernel (its name asserted after every call)
   is held to np.searchsorted + the slope form in np.longdouble under a bound derived below, with and without
   clipping where the kernel takes both, and to itself under another split of rows / components;
3. the same targets with the map's nonzero nonmonotone coefficients against the oracle and kernel against kernel.

THE BOUND of part 2 (`bound`).  With i the located interval, x the reference value, delta = x - y[i-1], u = 2^-53:

    |got - x| <= |delta| (e_slope + c1 u) + c2 u max(|y[i-1]|, |x|)

 * generic kernel (k_inverse_table, csrc/ttm_kernels.hip: `slope = fast_div(y_hi - y_lo, fmax(x_hi - x_lo, 1e-300))`,
   `re = slope * (target - x_lo) + y_lo`) and the host test double (the same statements): the operations that round and
   scale delta are y_hi - y_lo, x_hi - x_lo, target - x_lo and the product: c1 = 4; e_slope = 2 u, the 1 ulp that
   tests/test_device_math.py holds fast_div to; the abscissa (i - 1) * step + y0 is np.linspace's to the bit (the host
   checks that before it passes h_y_affine, the build does not contract), so only the sum rounds: c2 = 1.
 * resident kernels (k_inverse_rt, k_band_inverse, k_band_inverse_ring, k_band_few_inverse: `dx = x_hi - x_lo`, `rc` =
   v_rcp_f64 + one Newton step, `slope = (y_hi - y_lo) * rc`, `delta = slope * (tgt - x_lo)`, `rr = delta + y_lo`):
   y_hi - y_lo, dx, the product with rc, tgt - x_lo and the product with it: c1 = 5; e_slope = 2^-46 (the comment at the
   interp lambda of k_inverse_rt); y_lo and y_hi are np.linspace's to the bit ((i - 1) * step + y0 in two roundings, the
   last point forced; from the {E_i, y_i} pair table where the kernel has one), so only the sum rounds: c2 = 1

The resident kernels interpolate on np.linspace's abscissae to the bit since this file exists: until then they took the
abscissa as fma(i, step, y0 - step) (6.3e-16 at the grid point 0, where the reference has 0; 478 u |y| off at y[501]) and
the slope as step / dx (y[i] - y[i-1] is the step only to 800 u) and missed this bound by 1.24e-15 (1.29e-12 at
|x| = 4e3 in unclipped searches) without ever picking a wrong interval.  Measured on an MI355X, worst error / bound of
every kernel over all its table sets and variants: 0.93 - 1.000 for all six, the host double 0.985 - 1.000 (the final
rounding of x at a node reaches the bound).

WHAT THE TARGETS EXERCISE, kernel by kernel (by reading; the mutations of the host double - `<=` in either search, bkt
shifted by one, the clip to [0, T-1] - were each built into a copy and each fail the CPU tests here: `<=` only on the
tables with ties, as continuity hides it everywhere else even at this bound):
 * k_inverse_table: nodes +-1 ulp the compare `xs[mid] < target` and the clip of a to [1, T-1]; bucket boundaries
   +-1 ulp the bracket `bk[q - 1] .. bk[q + 2]` around q = (int)((target - lo) * scale), which is not the index's fma;
 * k_inverse_rt: bucket boundaries `bkl[min((int)fma(tg, scale, bias), nb - 1)]`; nodes the compares `q0 < tg` .. `q3 < tg`
   of the three `per` branches (le2 / 3to4 / mixed); wl, wh +-1 ulp `traw != tg` (resident or outlier); beyond the table
   and the degenerate components the search in memory behind `if (outl != 0)`;
 * k_band_inverse / k_band_inverse_ring (csrc/ttm_band.hip: band_inverse_tile) and k_band_few_inverse (its own copy of the
   step): the same three places - the bucket read behind `traw[e] != tg[e]`, the phases of compares of the target's own
   bucket, the search in memory behind `if (deg || traw[e] != tg[e])` - the ring kernel on the image's wl / wh / per /
   degenerate words, which the test reads back and compares with `resident_range`.

The worst error / bound of every kernel and table class goes to record_parity('lookup/<kernel>/<tables>/error_over_bound').
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import record_parity, relerr

U = 2.0 ** -53
T_DEF, NB_DEF = 1001, 1023
Y_DEF = np.linspace(-10.0, 10.0, T_DEF)
WINDOWS = (0, 64, 200)                                  # rt_window: whole tables, and two small even windows
BOUNDS = {                                              # kernel -> (e_slope, c1, c2): the module docstring
    'hostemu': (2 * U, 4, 1), 'k_inverse_table': (2 * U, 4, 1),
    'k_inverse_rt': (2.0 ** -46, 5, 1), 'k_inverse_rt<band>': (2.0 ** -46, 5, 1), 'k_band_inverse': (2.0 ** -46, 5, 1),
    'k_band_inverse_ring': (2.0 ** -46, 5, 1), 'k_band_few_inverse': (2.0 ** -46, 5, 1),
}


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


# ---------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------
def bucket_params(lo, hi, nb):
    """scale = nb / (hi - lo) in IEEE double - 0 where that is not in (0, 1e300) - and bias = -lo * scale."""
    with np.errstate(all='ignore'):
        scale = np.float64(nb) / (np.float64(hi) - np.float64(lo))
        if not (scale > 0.0 and scale < 1.0e300):
            scale = np.float64(0.0)
        return float(scale), float(-np.float64(lo) * scale)


def bucket_of(x, scale, bias, nb):
    """clamp(trunc(fma(x, scale, bias)), 0, nb - 1): the fma as ONE correctly rounded operation (float() of a Fraction)."""
    try:
        v = float(Fraction(float(x)) * Fraction(scale) + Fraction(bias))
    except OverflowError:
        v = np.inf if (x > 0) == (scale > 0) else -np.inf
    return int(min(max(np.trunc(v), 0), nb - 1))


def index_of(row, nb):
    """(tmin, tmax, bkt, entries per bucket at most) of one sorted row by the definition."""
    T = len(row)
    scale, bias = bucket_params(row[0], row[-1], nb)
    q = np.array([bucket_of(x, scale, bias, nb) for x in row])
    bkt = np.array([int(np.sum(q < b)) for b in range(nb)] + [T], dtype=np.int32)
    return row[0], row[-1], bkt, int(np.bincount(q, minlength=nb).max())


def synthetic_rows(T, nb):
    """name -> row: the classes of table the index and the lookups must handle."""
    t = np.linspace(-1.0, 1.0, T)
    smooth = np.sinh(2.5 * t) + 0.3 * t + 0.125
    rows = {'smooth': smooth}
    r = smooth.copy()
    for a, n in ((T // 3, 2), (T // 2, 3), (T // 2 + 7, max(2, T // 100)), (2 * T // 3, 5)):
        if a + n < T - 1:
            r[a:a + n] = r[a]
    rows['runs'] = r
    r = smooth.copy(); r[:5] = r[4]; rows['flat_start'] = r
    r = smooth.copy(); r[-5:] = r[-5]; rows['flat_end'] = r
    rows['one_value'] = np.full(T, 0.75)
    r = smooth.copy()                                   # nine tenths of the entries inside one bucket in the middle
    m = min((9 * T) // 10, T - 2)
    a = (T - m) // 2
    bw = (smooth[-1] - smooth[0]) / nb
    start = smooth[0] + (np.floor((smooth[a] - smooth[0]) / bw) + 1.1) * bw      # a tenth into the next bucket, eight tenths wide
    r[a:a + m] = start + 0.8 * bw * np.arange(m) / m
    rows['crowded'] = r
    rows['scale_zero'] = 1.5e308 * np.linspace(-1.0, 1.0, T)        # hi - lo overflows: nb / inf = 0
    rows['scale_inf'] = np.arange(T) * 5e-324                       # subnormal range: nb / (hi - lo) overflows
    rows['scale_huge'] = np.linspace(0.0, 1e-300, T)                # nb / (hi - lo) >= 1e300
    rows['signed_zeros'] = np.concatenate((np.full(3, -0.0), np.full(2, 0.0), 0.01 * np.arange(1, T - 4)))
    r = smooth.copy(); r[T // 2], r[T // 2 + 1] = smooth[T // 2 + 1], smooth[T // 2]; rows['descending_pair'] = r
    r = smooth.copy(); r[T // 3] = np.nan; rows['nan'] = r
    for k, v in rows.items():
        assert v.shape == (T,)
        if k not in ('descending_pair', 'nan'):
            assert np.all(np.diff(v) >= 0), k
    return rows


UNSORTED = ('descending_pair', 'nan')


class Dev:
    """The library of a backend with arrays where it reads them."""

    def __init__(self, backend):
        import torch
        from triangular_transport_toolbox_amd import _capi
        self.torch = torch
        self.lib = emu.lib() if backend == 'hostemu' else _capi.load()
        self.device = 'cpu' if backend == 'hostemu' else 'cuda'

    def put(self, a, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(a).copy())
        return (t if dtype is None else t.to(dtype)).to(self.device)

    def empty(self, *shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.torch.float64, device=self.device)

    @staticmethod
    def ptr(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())

    def index(self, tab, nb):
        """ttm_inverse_table_index of the rows of `tab` -> (tmin, tmax, bkt, unsorted) as the library wrote them (device arrays)."""
        ncomp, T = tab.shape
        tab_d = self.put(tab)
        tmin, tmax = self.empty(ncomp), self.empty(ncomp)
        bkt = self.empty(ncomp, nb + 1, dtype=self.torch.int32)
        uns = self.empty(ncomp, dtype=self.torch.int32)
        rc = self.lib.ttm_inverse_table_index(self.ptr(tab_d), ncomp, T, nb, self.ptr(tmin), self.ptr(tmax), self.ptr(bkt), self.ptr(uns), None)
        assert rc == 0
        if self.device == 'cuda':
            self.torch.cuda.synchronize()
        return tab_d, tmin, tmax, bkt, uns


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---------------------------------------------------------------------------
# 1. the index against its definition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('T,nb', [(T_DEF, NB_DEF), (8, 4), (2048, 4096)])
def test_index_is_the_definition(backend, T, nb):
    """tmin / tmax = first / last entry to the bit (include/ttm.h), unsorted exactly for the rows with a descending pair or
    a NaN, and for the sorted rows bkt[0] = 0, bkt[nb] = T, bkt non-decreasing, bkt[q] = #{entries with bucket(x) < q} -
    smallest (T = 8, nb = 4), default and largest (T = 2048, nb = 4096) geometry, all rows of a geometry in ONE call."""
    dev = Dev(backend)
    rows = synthetic_rows(T, nb)
    names = sorted(rows)
    tab = np.stack([rows[n] for n in names])
    _, tmin, tmax, bkt, uns = dev.index(tab, nb)
    tmin, tmax, bkt, uns = tmin.cpu().numpy(), tmax.cpu().numpy(), bkt.cpu().numpy(), uns.cpu().numpy()
    assert [n for n, f in zip(names, uns) if f == 1] == sorted(UNSORTED) and set(uns.tolist()) == {0, 1}
    crowded = {}
    for c, n in enumerate(names):
        if n in UNSORTED:
            continue
        lo, hi, want, per = index_of(rows[n], nb)
        crowded[n] = per
        assert bits(tmin[c]) == bits(lo) and bits(tmax[c]) == bits(hi), n
        assert bkt[c, 0] == 0 and bkt[c, nb] == T and np.all(np.diff(bkt[c]) >= 0), n
        bad = np.nonzero(bkt[c] != want)[0]
        assert bad.size == 0, '%s: bkt[%d] = %d, definition %d (%d differ)' % (n, bad[0], bkt[c, bad[0]], want[bad[0]], bad.size)
    # the classes are what their names say
    for n in ('one_value', 'scale_zero', 'scale_inf', 'scale_huge'):
        assert crowded[n] == T and bucket_params(rows[n][0], rows[n][-1], nb)[0] == 0.0, n
    assert crowded['crowded'] >= min((9 * T) // 10, T - 2) and crowded['smooth'] <= max(3, T // 100)


# ---------------------------------------------------------------------------
# 2. exact-target sweeps
# ---------------------------------------------------------------------------
# monotone coefficients {LET, iRBF, iRBF, RET} per component of test_band.py's c5_shape: with equal weights the table is
# close to a straight line (a bucket holds 2 entries at most); iRBF weights that are small against the edge terms'
# flatten the middle of the table, where the entries then crowd into few buckets
MONOTONE = {
    'le2': [[1.0, 1.0, 1.0, 1.0]] * 6,
    '3to4': [[1.0, 0.12, 0.12, 1.0]] * 6,
    'mixed': [[1.0, 1e-3, 1e-3, 1.0], [1.0, 1.0, 1.0, 1.0]] * 3,
}
PER_CLASS = {'le2': lambda p: max(p) <= 2, '3to4': lambda p: 3 <= max(p) <= 4, 'mixed': lambda p: max(p) > 4 and min(p) <= 4}


def window_of(T, window):
    """[w0, w0 + W) of a pinned rt_window (csrc/ttm_band_image.h: band_ring_plan; 0 = whole tables)."""
    if window <= 0:
        return 0, T
    W = min(max(window, 16), T - 1) & ~1
    return (T - W) // 2, W


def resident_range(row, bkt, window):
    """(wl, wh, entries per bucket at most over the buckets that reach the window, degenerate) as band_image_write lays them out."""
    T = len(row)
    w0, W = window_of(T, window)
    n = np.diff(bkt.astype(np.int64))
    reach = (bkt[1:] > w0) & (bkt[:-1] < w0 + W)
    per = int(n[reach].max()) if reach.any() else 0
    pm = max(per, 1)
    deg = pm + 3 >= W or per > 4
    xw = lambda i: row[w0 + i] if i < W else np.inf
    return (xw(1), xw(1), per, True) if deg else (xw(pm), xw(W - 2), per, False)


def targets_of(row, nb, bkt):
    """The targets of one component's column: see the module docstring."""
    lo, hi = row[0], row[-1]
    span = max(hi - lo, 1.0)
    both = lambda v: np.concatenate((v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)))
    edges = lo + np.arange(nb + 1) * ((hi - lo) / nb)
    ends = [lo, hi]
    for w in WINDOWS:
        ends += list(resident_range(row, bkt, w)[:2])
    beyond = np.concatenate(([0.01, 1.0, 10.0], np.geomspace(1e-9, 5.0, 27))) * span
    return np.concatenate((both(row), 0.5 * (row[:-1] + row[1:]), both(edges), both(np.array([e for e in ends if np.isfinite(e)])),
                           lo - beyond, hi + beyond))


def expected(row, y, t, truncate):
    """x, interval, tie mask by np.searchsorted (left) + the slope form in np.longdouble; the tie x_hi == x_lo gives y[i-1]."""
    T = len(row)
    lo, hi = row[0], row[-1]
    tt = np.where(np.isnan(t), t, np.clip(t, lo, hi)) if truncate else t
    a = np.searchsorted(row, tt, 'left')
    i = np.clip(a, 1, T - 1)
    L = np.longdouble
    xl, xh = row[i - 1], row[i]
    tie = (xh == xl) & ~np.isnan(tt)
    with np.errstate(all='ignore'):
        slope = (y[i].astype(L) - y[i - 1].astype(L)) / np.where(tie, 1.0, xh.astype(L) - xl.astype(L))
        x = y[i - 1].astype(L) + slope * (tt.astype(L) - xl.astype(L))
        x = np.where(tie & (tt == xl), y[i - 1].astype(L), x)
        # a tied end interval has no slope: beyond it (unclipped searches only) interp1d's infinity of the side the target is on
        x = np.where(tie & (tt != xl) & ~np.isnan(tt), np.sign(tt - xl) * np.inf, x)
    x = np.where(np.isnan(tt), np.nan, x)
    return x, i, tie


def bound(kernel, x, yl):
    e_slope, c1, c2 = BOUNDS[kernel]
    with np.errstate(all='ignore'):
        return (np.abs(x - yl) * (e_slope + c1 * U) + c2 * U * np.maximum(np.abs(yl), np.abs(x))).astype(np.float64)



class Sweep:
    """One table set: its map (nonmonotone coefficients 0.0), the tables as the library read them back, the matrix of
    targets, the reference for both clipping modes and the coverage conditions - all before any lookup result."""

    def __init__(self, backend, tables):
        from tests.test_band import _build
        self.backend, self.tables = backend, tables
        self.few = tables.startswith('few')
        self.synthetic = tables.endswith('synthetic')
        self.tm, self.om, self.X, _ = _build('few_c2b' if self.few else 'c5_shape', n=400)
        tm = self.tm
        self.real_nonmon = [c.copy() for c in tm.coeffs_nonmon]
        self.lib = tm._lib
        self.lib.ttm_last_kernel.restype = ctypes.c_char_p
        self.D, self.T, self.nb = tm.D, T_DEF, NB_DEF
        for k in range(tm.D):
            tm.coeffs_nonmon[k] = np.zeros(len(tm.coeffs_nonmon[k]))
            if not self.few:
                tm.coeffs_mon[k] = np.asarray(MONOTONE[tables.split('_')[0] if self.synthetic else tables][k], dtype=float)
            self.om.coeffs_mon[k] = tm.coeffs_mon[k].copy()
        tm._ensure_pts(self.T, 10)                         # (the abscissae np.linspace(-10, 10, T) and their affine restatement)
        self.coef = self.pack()
        if self.synthetic:
            rows = synthetic_rows(self.T, self.nb)
            names = ['smooth', 'runs', 'flat_start', 'flat_end', 'crowded', 'one_value'][:self.D] if not self.few else ['runs', 'flat_start']
            dev = Dev(backend)
            self.tab_d, self.tmin_d, self.tmax_d, self.bkt_d, uns = dev.index(np.stack([rows[n] for n in names]), self.nb)
            assert int(uns.cpu().max()) == 0
        else:
            self.tab_d, self.tmin_d, self.tmax_d, self.bkt_d = self.entry(self.coef)[:4]
        self.tab = self.tab_d.cpu().numpy().copy()
        self.bkt = self.bkt_d.cpu().numpy().copy()
        assert np.all(np.diff(self.tab, axis=1) >= 0)
        # the index the lookups are handed is the definition's (part 1 on these very tables), `per` by the restatement
        self.per = []
        for k in range(self.D):
            lo, hi, want, per = index_of(self.tab[k], self.nb)
            assert np.array_equal(self.bkt[k], want), k
            self.per.append(per)
        cols = [targets_of(self.tab[k], self.nb, self.bkt[k]) for k in range(self.D)]
        n = max(len(c) for c in cols)
        n += 1 - n % 2                                  # odd
        rng = np.random.default_rng(20240607)
        Z = np.empty((n + 3 * self.D, self.D))
        for k, c in enumerate(cols):
            mid = self.tab[k][self.T // 2]
            Z[:, k] = mid
            Z[:len(c), k] = c
            # +-inf and NaN: one row per component, finite targets in its other columns (a non-finite x_k spoils the offsets behind it)
            Z[n + 3 * k:n + 3 * k + 3, k] = (np.inf, -np.inf, np.nan)
        self.Z = Z[rng.permutation(len(Z))]
        self.N = len(self.Z)
        assert self.N % 2 == 1
        self.ref = {}
        for truncate in (1, 0):
            x = np.empty(self.Z.shape, dtype=np.longdouble)
            i = np.empty(self.Z.shape, dtype=np.int64)
            tie = np.empty(self.Z.shape, dtype=bool)
            for k in range(self.D):
                x[:, k], i[:, k], tie[:, k] = expected(self.tab[k], Y_DEF, self.Z[:, k], truncate)
            # what is held: everything up to and including a row's first non-finite result
            dirty = ~np.isfinite(x.astype(np.float64))
            held = np.cumsum(np.concatenate((np.zeros((self.N, 1), bool), dirty[:, :-1]), axis=1), axis=1) == 0
            self.ref[truncate] = (x, i, tie, held)
        x, i, tie, held = self.ref[1]
        assert np.all(i[tie] == 1), 'clipped searches meet a tie at the flat start only (csrc/ttm_eval.h: table_lookup)'
        assert self.synthetic or not tie.any()
        self.coverage()

    # -- the map's own launches ------------------------------------------------------------------------------------
    def pack(self):
        self.tm._pack_memo = None
        return self.tm._pack_coeffs()

    def entry(self, coef):
        self.tm._inverse_table(coef, 0, self.D, None, None, 0)
        return next(iter(coef._ttm_tables.values()))

    def lookup(self, truncate, expect, image=False, Z=None):
        """One ttm_inverse_table over the targets under the options in force -> N x D; the kernel that ran must be `expect`."""
        tm = self.tm
        Z = self.Z if Z is None else Z
        N = len(Z)
        coef, img, per = self.coef, None, 0
        if image:                                        # tables and images laid out under these options: a fresh vector
            coef = self.pack()
            e = self.entry(coef)
            assert np.array_equal(e[0].cpu().numpy(), self.tab) and e[5] is not None
            img, per = e[5], e[5].numel() // self.D
            self.image = img.cpu().numpy().reshape(self.D, per)
        Zd = tm._cols(self.D, N, zero=True)
        Zd[:, :N] = tm._to_dev(np.ascontiguousarray(Z.T))
        Xd = tm._cols(self.D, N, zero=True)
        rc = self.lib.ttm_inverse_table(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, self.D, tm._ptr(Zd), Zd.shape[1], tm._ptr(Xd),
                                        Xd.shape[1], N, tm._ptr(self.tab_d), tm._ptr(tm._pts_d), 0, self.T, tm._pts_affine, tm._ptr(self.tmin_d),
                                        tm._ptr(self.tmax_d), ctypes.c_void_p(self.bkt_d.data_ptr()), self.nb, truncate, tm._ptr(img), per, tm._stream())
        assert rc == 0
        try:
            got = Xd[:, :N].cpu().numpy().T.copy()
        except RuntimeError as e:                      # a HIP error: nothing more is launched on a device that faulted
            pytest.exit('device error behind %s: %s' % (self.lib.ttm_last_kernel().decode(), e), returncode=3)
        name = self.lib.ttm_last_kernel().decode()
        assert name == expect, 'ran %s, not %s' % (name, expect)
        return got

    # -- conditions on the targets, from the reference alone ---------------------------------------------------------
    def coverage(self):
        deg_any = {}
        for w in WINDOWS:
            degs = []
            for k in range(self.D):
                row, z = self.tab[k], self.Z[:, k]
                wl, wh, per, deg = resident_range(row, self.bkt[k], w)
                degs.append(deg)
                inside = (z >= row[0]) & (z <= row[-1])
                n_res = int(np.sum(inside & (z >= wl) & (z <= wh)))
                n_win = int(np.sum(inside & ((z < wl) | (z > wh))))
                n_tab = int(np.sum((z < row[0]) | (z > row[-1])))
                assert n_tab >= 50, (w, k, n_tab)
                if not deg:
                    assert n_res >= 50, (w, k, n_res)
                    # (whole tables: the window ends one entry inside the table, so only the outermost nodes lie beyond it)
                    assert n_win >= (50 if w else 3), (w, k, n_win)
                if w == 0:
                    assert per == self.per[k]
                # first, middle and last buckets
                scale, bias = bucket_params(row[0], row[-1], self.nb)
                if scale > 0:
                    zi = z[inside & (z > row[0]) & (z < row[-1])]           # (strictly inside: a product one rounding off stays in its bucket's neighbourhood)
                    qs = np.clip(np.trunc(zi * scale + bias), 0, self.nb - 1)
                    assert np.sum(qs == 0) > 0 and np.sum(qs == self.nb - 1) > 0 and np.sum(np.abs(qs - self.nb // 2) <= 1) > 0, (w, k)
            deg_any[w] = degs
        self.degenerate = deg_any
        if not self.few and not self.synthetic:
            assert PER_CLASS[self.tables](self.per), self.per
        if self.tables in ('mixed', 'mixed_synthetic'):
            assert any(deg_any[0]) and not all(deg_any[0])      # degenerate and resident components within one launch

    # -- the comparison ------------------------------------------------------------------------------------------------
    def check(self, kernel, got, truncate, what):
        x, i, tie, held = self.ref[truncate]
        xf = x.astype(np.float64)
        yl = Y_DEF[i - 1]
        nan = np.isnan(xf) & held
        assert np.all(np.isnan(got[nan])), (kernel, what, 'a NaN target gives NaN')
        inf = np.isinf(xf) & held
        open_tie = inf & tie                             # (beyond a tied end interval: sign, and beyond every finite abscissa)
        assert np.all(got[inf & ~tie] == xf[inf & ~tie]), (kernel, what, 'infinite targets')
        assert np.all(np.sign(got[open_tie]) == np.sign(xf[open_tie])) and np.all(np.abs(got[open_tie]) > 1e250), (kernel, what)
        fin = np.isfinite(xf) & held
        assert np.all(np.isfinite(got[fin])), (kernel, what)
        with np.errstate(all='ignore'):
            err = np.abs(got.astype(np.longdouble) - x).astype(np.float64)
        at_tie = fin & tie
        assert np.array_equal(got[at_tie], yl[at_tie]), (kernel, what, 'the tie returns the first abscissa')
        b = bound(kernel, x, yl)
        with np.errstate(all='ignore'):
            ratio = np.where(fin & (b > 0), err / b, 0.0)
            excess = float(np.max(np.where(fin, err - b, 0.0)))
        zero = fin & (b == 0)
        ratio[zero] = np.where(err[zero] == 0, 0.0, np.inf)
        worst = float(ratio.max())
        n, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print('lookup/%s/%s %s truncate=%d: error / bound = %.3f (component %d: target %r, interval %d, got %r, reference %r, excess %.2e)'
              % (kernel, self.tables, what, truncate, worst, k, self.Z[n, k], i[n, k], got[n, k], float(x[n, k]), excess))
        return worst


@functools.lru_cache(maxsize=8)
def sweep_of(backend, tables):
    return Sweep(backend, tables)


TABLES = ['le2', '3to4', 'mixed', 'mixed_synthetic']
FEW_TABLES = ['few', 'few_synthetic']
_WINDOWED = {'w%d' % w: dict(rt_window=w) for w in WINDOWS}

# kernel -> (options that pin it, clipping modes it takes, variants {what: options}, another split of the rows, of the components)
PINS = {
    # (the generic kernel has no split of its own: its variants - one or two rows per thread, planned or not - are held to each other)
    'k_inverse_table': (dict(rt_off=1), (1, 0), {'ns1': dict(inverse_ns=1), 'ns2': dict(inverse_ns=2), 'unplanned': dict(no_plan=1)}, None, None),
    'k_inverse_rt<band>': (dict(band_inv=0), (1, 0), _WINDOWED, dict(rt_ns=2), None),      # (six components do not split into blocks of four)
    'k_inverse_rt': (dict(band_inv=0, rt_band=0), (1, 0), _WINDOWED, dict(rt_ns=4), None),
    'k_band_inverse': (dict(band_inv=1, band_ring=0), (1,), _WINDOWED, dict(band_cus=1), dict(rt_block=2)),
    'k_band_inverse_ring': (dict(band_inv=1, band_ring=1), (1,), _WINDOWED, dict(band_cus=1), None),   # (a ring of two slots is no ring: k_band_inverse)
    'k_band_few_inverse': (dict(band_inv=1), (1,), {'whole': {}}, dict(band_cus=1), None),
}


def _pin(ttm_opt, *sets):
    ttm_opt('u_loader', 1)
    for s in sets:
        for name, v in (s or {}).items():
            ttm_opt(name, v)


def _unpin(ttm_opt, *sets):
    for s in sets:
        for name in (s or {}):
            ttm_opt(name, 0 if name in ('rt_off', 'no_plan', 'u_no_hot') else -1)


def _run(sw, kernel, ttm_opt):
    """Every variant and clipping mode of one kernel over one table set: the kernel's name after every call, NaN / infinite
    targets, the tie, the image header (ring), the same bits under another split (the generic kernel: from every variant).
    Returns the worst error / bound."""
    base, modes, variants, rows, comps = PINS[kernel]
    ring = kernel == 'k_band_inverse_ring'
    worst = 0.0
    first = {}
    for what, opts in variants.items():
        for truncate in modes:
            _pin(ttm_opt, base, opts)
            got = sw.lookup(truncate, kernel, image=ring)
            if kernel == 'k_inverse_table':             # the same bits from every variant (the offsets are +-0 whatever evaluates them)
                assert np.array_equal(got, first.setdefault(truncate, got), equal_nan=True), (what, truncate)
            if ring:                                    # the image header agrees with the restatement: per [8], degenerate [10]
                for k in range(sw.D):
                    wl, wh, per, deg = resident_range(sw.tab[k], sw.bkt[k], opts['rt_window'])
                    hdr = sw.image[k, :6].view(np.int32)
                    assert (int(hdr[8]), int(hdr[10])) == (per, int(deg)), (k, hdr[8:12], per, deg)
                    assert sw.image[k, 0] == wl and sw.image[k, 1] == wh
            worst = max(worst, sw.check(kernel, got, truncate, what))
            if rows:
                _pin(ttm_opt, rows)
                assert np.array_equal(sw.lookup(truncate, kernel, image=ring), got, equal_nan=True), (what, truncate, rows)
                _unpin(ttm_opt, rows)
            if comps:                                   # (tests/test_band.py: a tile that re-reads its columns at a block boundary, 1e-14)
                _pin(ttm_opt, comps)
                again = sw.lookup(truncate, kernel)
                x, _, _, held = sw.ref[truncate]
                ok = np.isfinite(x.astype(np.float64)) & held
                assert relerr(again[ok], got[ok]) < 1e-14, (what, truncate, comps)
                _unpin(ttm_opt, comps)
            _unpin(ttm_opt, base, opts)
    return worst


@pytest.mark.parametrize('tables', TABLES)
def test_exact_targets_through_the_host_double(tables, ttm_opt):
    """Part 2 on the CPU: the double's accelerated search over the bucket index (hot records) and its full search, held to the bound."""
    with emu.install():
        sw = sweep_of('hostemu', tables)
        worst = 0.0
        for what, opts in (('bucket search', {}), ('full search', dict(u_no_hot=1))):
            _pin(ttm_opt, opts)
            for truncate in (1, 0):
                worst = max(worst, sw.check('hostemu', sw.lookup(truncate, 'hostemu'), truncate, what))
            _unpin(ttm_opt, opts)
        assert worst <= 1.0, worst


def _cases():
    return [(k, t) for k in sorted(PINS) for t in (FEW_TABLES if k == 'k_band_few_inverse' else TABLES)
            if not (k == 'k_band_inverse_ring' and t.endswith('synthetic'))] + [('k_inverse_table', t) for t in FEW_TABLES]
    # (the ring kernel reads images, which only ttm_inverse_table_build_index writes: no synthetic tables for it)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel,tables', _cases())
def test_exact_targets_through_every_lookup_kernel(kernel, tables, ttm_opt):
    """Part 2 on the device.  Every call asserts the kernel that ran; every variant (samples per thread, planned or not,
    whole and windowed tables) and both clipping modes where the kernel takes them; another split of the rows gives the
    same bits, another split of the components 1e-14; every result within the bound of the module docstring."""
    sw = sweep_of('hip', tables)
    worst = _run(sw, kernel, ttm_opt)
    record_parity('lookup/%s/%s/error_over_bound' % (kernel, tables), worst, 1.0)
    assert worst <= 1.0, worst


def test_an_unsorted_table_takes_the_gathered_abscissae(backend, ttm_opt):
    """The host detour of a table that is not sorted (tab_y gathered, ldy != 0, no h_y_affine) once through the generic
    kernel: the descending pair of part 1 after interp1d's stable sort, held to the generic bound."""
    sw = sweep_of(backend, 'le2')
    tm = sw.tm
    dev = Dev(backend)
    raw = np.stack([synthetic_rows(sw.T, sw.nb)['descending_pair']] * sw.D)
    order = np.argsort(raw, axis=1, kind='mergesort')
    tab = np.take_along_axis(raw, order, axis=1)
    ys = np.ascontiguousarray(Y_DEF[order])
    tab_d, tmin_d, tmax_d, bkt_d, uns = dev.index(tab, sw.nb)
    assert int(uns.cpu().max()) == 0
    Z = np.stack([targets_of(tab[k], sw.nb, bkt_d.cpu().numpy()[k]) for k in range(sw.D)], axis=1)
    Z = Z[np.random.default_rng(5).permutation(len(Z))]
    N = len(Z)
    Zd = tm._cols(sw.D, N, zero=True)
    Zd[:, :N] = tm._to_dev(np.ascontiguousarray(Z.T))
    Xd = tm._cols(sw.D, N, zero=True)
    ys_d = dev.put(ys)
    _pin(ttm_opt, {})
    rc = sw.lib.ttm_inverse_table(tm._pp, tm._ptr(sw.coef), tm._ptr(sw.coef._ttm_fold), 0, sw.D, tm._ptr(Zd), Zd.shape[1], tm._ptr(Xd), Xd.shape[1], N,
                                  dev.ptr(tab_d), dev.ptr(ys_d), sw.T, sw.T, None, dev.ptr(tmin_d), dev.ptr(tmax_d), dev.ptr(bkt_d), sw.nb, 1, None, 0,
                                  tm._stream())
    assert rc == 0
    name = sw.lib.ttm_last_kernel().decode()
    assert name == ('hostemu' if backend == 'hostemu' else 'k_inverse_table')
    got = Xd[:, :N].cpu().numpy().T
    for k in range(sw.D):
        x, i, tie, = expected(tab[k], ys[k], Z[:, k], 1)
        assert not tie.any()
        err = np.abs(got[:, k].astype(np.longdouble) - x).astype(np.float64)
        e_slope, c1, c2 = BOUNDS[name]
        yl = ys[k][i - 1]
        b = np.abs((x - yl).astype(np.float64)) * (e_slope + c1 * U) + c2 * U * np.maximum(np.abs(yl), np.abs(x.astype(np.float64)))
        assert np.all(err <= b), (k, float(np.max(err / b)))


# ---------------------------------------------------------------------------
# 3. the same targets with the map's real coefficients
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('tables', ['le2', '3to4', 'mixed', 'few'])
def test_node_targets_with_the_real_coefficients(tables, ttm_opt):
    """The targets of part 2 with nonzero nonmonotone coefficients (tests/test_band.py's) through every kernel - the four of
    the six-component map on its three table sets, k_band_few_inverse on the two-component map: the oracle at relerr <
    1e-11, and no row further than 1e-12 from the generic kernel's - thousands of rows whose targets now lie within an
    offset's rounding of a node, a bucket boundary or a window end, with the E-table / push feedback live."""
    sw = sweep_of('hip', tables)
    tm, om = sw.tm, sw.om
    keep = np.isfinite(sw.Z).all(axis=1)
    Z = sw.Z[keep][:-1] if keep.sum() % 2 == 0 else sw.Z[keep]
    zero = [c.copy() for c in tm.coeffs_nonmon]
    zero_om = [np.asarray(c).copy() for c in om.coeffs_nonmon]
    kernels = ['k_band_few_inverse'] if sw.few else [k for k in sorted(PINS) if k not in ('k_inverse_table', 'k_band_few_inverse')]
    try:
        for k in range(sw.D):
            tm.coeffs_nonmon[k] = sw.real_nonmon[k].copy()
            om.coeffs_nonmon[k] = sw.real_nonmon[k].copy()
        real = Sweep.__new__(Sweep)
        real.__dict__.update(sw.__dict__)
        real.coef = sw.pack()
        Xo = (om.inverse_map(Z) - om.X_mean) / om.X_std
        _pin(ttm_opt, dict(rt_off=1))
        generic = real.lookup(1, 'k_inverse_table', Z=Z)
        e_o = relerr(generic, Xo)
        record_parity('lookup/k_inverse_table/%s/real_coefficients_vs_oracle' % tables, e_o, 1e-11)
        assert e_o < 1e-11, e_o
        ttm_opt('rt_off', 0)
        for kernel in kernels:
            base, _, variants, _, _ = PINS[kernel]
            for what, opts in variants.items():
                _pin(ttm_opt, base, opts)
                got = real.lookup(1, kernel, image=kernel == 'k_band_inverse_ring', Z=Z)
                e_o, e_g = relerr(got, Xo), relerr(got, generic)
                record_parity('lookup/%s/%s/%s/real_coefficients_vs_oracle' % (kernel, tables, what), e_o, 1e-11)
                record_parity('lookup/%s/%s/%s/real_coefficients_vs_k_inverse_table' % (kernel, tables, what), e_g, 1e-12)
                assert e_o < 1e-11 and e_g < 1e-12, (kernel, what, e_o, e_g)
                _unpin(ttm_opt, opts)
            _unpin(ttm_opt, base)
    finally:
        for k in range(sw.D):
            tm.coeffs_nonmon[k] = zero[k]
            om.coeffs_nonmon[k] = zero_om[k]
        tm._pack_memo = None
        for base, _, variants, _, _ in PINS.values():   # (a failure in the middle leaves nothing pinned for the code below)
            _unpin(ttm_opt, base, *variants.values())
