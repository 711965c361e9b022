"""
Quasi-Monte Carlo reference draws: qmc.tables, ttm_sobol_normal_fill / k_sobol_normal_fill (include/ttm.h, csrc/ttm_rng.h:
normal_quantile, sobol_low / sobol_high) and the `sequence='sobol'` keyword of transport_map.reference_device / sample_device /
sample, on the host test double and on the GPU.

The expected points come from a NumPy restatement of the Gray-code XOR in this file (`points`), the expected deviates from
scipy.special.ndtri of them; a GPU process never loads the host double.  Every figure is printed before it is held.

Bound of the normal quantile function, PHI_BOUND = 8 * 2^-52 = 1.78e-15 relative: the host build of normal_quantile (AS 241 PPND16) differs
from mpmath (40 digits, sqrt(2) erfinv(2 u - 1)) by at most 3.97e-16 = 1.79 * 2^-52 on the probe set of this file (PROBES: the
ends u = 2^-31 and 1 - 2^-31, the two values beside 1/2, both sides of the branch points |u - 1/2| = 0.425, a ladder down both
tails); four times that, rounded up to a multiple of 2^-52, leaves room for the device's log, sqrt and division, which differ from
libm's by a few ulp.  It may never exceed 64 * 2^-52 (the published approximations are below 2.1e-15).  Where the reference is
scipy's ndtri, its own largest error against mpmath on the probe set, measured here, is added.  Comparisons of two fills of one
backend are bitwise.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

from tests.hostemu import emu
from tests.test_sample import DEVICE_CASES, E_ARG, ROOT, SENTINEL, _free_port, backend, host, last_kernel, make  # noqa: F401

HOST_WORST = 3.97e-16                                             # host build against mpmath on PROBES (printed by the probe test)
PHI_BOUND = float(np.ceil(4.0 * HOST_WORST / 2.0 ** -52)) * 2.0 ** -52
assert PHI_BOUND == 8 * 2.0 ** -52 and PHI_BOUND <= 64 * 2.0 ** -52
BITS = 30
TOP = 2 ** BITS - 1


# ------------------------------------------------------------------------------------------ the restatement (NumPy alone)

def points(dirs, shift, row0, N):
    """q[j, n] = shift[j] XOR (XOR over the set bits b of the Gray code of row0 + n of dirs[j, b])."""
    i = np.uint64(row0) + np.arange(N, dtype=np.uint64)
    g = i ^ (i >> np.uint64(1))
    q = np.repeat(np.asarray(shift, dtype=np.uint64)[:, None], N, axis=1)
    for b in range(BITS):
        q ^= np.where((g >> np.uint64(b)) & np.uint64(1), np.uint64(1), np.uint64(0))[None, :] * np.asarray(dirs, dtype=np.uint64)[:, b:b + 1]
    return q


def uniforms(q):
    return (q.astype(np.float64) + 0.5) * 2.0 ** -30


def tables(*a, **kw):
    from triangular_transport_toolbox_amd import qmc
    return qmc.tables(*a, **kw)


@functools.lru_cache(maxsize=None)
def probes():
    """(the probe points q, sorted; mpmath's z of (q + 0.5) 2^-30 at 40 digits) - about 200 points, computed once."""
    import mpmath
    edge = int(np.ceil(0.075 * 2.0 ** 30 - 0.5))                 # u = (q + 0.5) 2^-30 crosses 1/2 - 0.425 between edge - 1 and edge
    qs = {0, 1, 2 ** 29, 2 ** 29 - 1}
    qs.update(edge + k for k in (-2, -1, 0, 1))
    for k in range(BITS):
        qs.update((2 ** k, 3 * 2 ** k // 2, 2 ** k - 1))
    qs = {q for q in qs if 0 <= q <= TOP}
    qs |= {TOP - q for q in qs}
    qs = np.array(sorted(qs), dtype=np.int64)
    u = uniforms(qs)
    central = np.abs(u - 0.5) <= 0.425
    k = int(np.searchsorted(qs, edge))
    assert not central[k - 1] and central[k] and qs[k - 1] == edge - 1, 'the probes straddle the branch point'
    assert central[np.searchsorted(qs, TOP - edge)] and not central[np.searchsorted(qs, TOP - edge + 1)]
    with mpmath.workdps(40):
        ref = [mpmath.sqrt(2) * mpmath.erfinv(2 * mpmath.mpf(float(x)) - 1) for x in u]
    return qs, ref


def rel_to_mpmath(z, ref):
    import mpmath
    with mpmath.workdps(40):
        return max(float(abs((mpmath.mpf(float(a)) - b) / b)) for a, b in zip(z, ref))


@functools.lru_cache(maxsize=None)
def scipy_error():
    """scipy's ndtri against mpmath on the probe set."""
    from scipy.special import ndtri
    qs, ref = probes()
    return rel_to_mpmath(ndtri(uniforms(qs)), ref)


def expected(dirs, shift, row0, N):
    from scipy.special import ndtri
    return ndtri(uniforms(points(dirs, shift, row0, N)))


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


SCRAMBLES = [None, (0, 0), (5, 0), (5, 3), (2 ** 40 + 7, 1)]           # None: plain; (seed, draw)


def tables_of(which, col0, ncols):
    return tables(0, 0, col0, ncols, scramble=False) if which is None else tables(which[0], which[1], col0, ncols, scramble=True)


# ------------------------------------------------------------------------------------------ A: the tables

def test_plain_points_are_torchs():
    from torch.quasirandom import SobolEngine
    import torch
    dirs, shift = tables(1, 2, 0, 40, scramble=False)
    assert dirs.shape == (40, BITS) and dirs.dtype == np.uint32 and shift.shape == (40,) and shift.dtype == np.uint32 and not shift.any()
    q = points(dirs, shift, 0, 4096)
    ref = SobolEngine(40, scramble=False).draw(4096, dtype=torch.float64).numpy().T
    assert np.array_equal(q.astype(np.float64) * 2.0 ** -30, ref)
    assert np.array_equal(uniforms(q), ref + 2.0 ** -31)


@pytest.mark.parametrize('which', SCRAMBLES, ids=lambda w: 'plain' if w is None else 'seed%d_draw%d' % w)
def test_columns_are_stratified_and_the_first_two_form_a_net(which):
    dirs, shift = tables_of(which, 0, 40)
    assert dirs.max() < 2 ** BITS and shift.max() < 2 ** BITS
    for row0 in (0, 4096):
        q = points(dirs, shift, row0, 4096)
        assert np.array_equal(np.sort(q >> np.uint64(18), axis=1), np.tile(np.arange(4096, dtype=np.uint64), (40, 1))), row0
        for a in range(13):                                    # elementary intervals 2^-a x 2^-(12 - a): one point each
            cell = ((q[0] >> np.uint64(BITS - a)) << np.uint64(12 - a)) | (q[1] >> np.uint64(BITS - (12 - a)))
            assert np.array_equal(np.sort(cell), np.arange(4096, dtype=np.uint64)), (row0, a)


def test_a_columns_tables_do_not_depend_on_the_columns_of_the_call():
    for which in SCRAMBLES:
        d5, s5 = tables_of(which, 0, 5)
        d3, s3 = tables_of(which, 2, 3)
        assert np.array_equal(d3, d5[2:5]) and np.array_equal(s3, s5[2:5]), which


def test_draw_and_seed_select_the_scrambling():
    d0, s0 = tables(5, 0, 0, 4)
    assert all(np.array_equal(a, b) for a, b in zip((d0, s0), tables(5, 0, 0, 4)))
    for other in (tables(5, 1, 0, 4), tables(6, 0, 0, 4)):
        assert not np.array_equal(other[0], d0) and not np.array_equal(other[1], s0)
    plain = tables(5, 0, 0, 4, scramble=False)
    assert all(np.array_equal(a, b) for a, b in zip(plain, tables(9, 7, 0, 4, scramble=False)))
    assert not np.array_equal(plain[0], d0)
    # dimension 0 has the identity as its generator matrix, so its scrambled direction number b is column b of the unit
    # lower-triangular scramble matrix itself: 2^(29 - b) + lower bits
    assert np.array_equal(plain[0][0], 1 << (BITS - 1 - np.arange(BITS, dtype=np.uint32)))
    assert np.array_equal(d0[0] >> (BITS - 1 - np.arange(BITS, dtype=np.uint32)), np.ones(BITS, dtype=np.uint32))


def test_table_limits():
    from triangular_transport_toolbox_amd import qmc
    assert qmc.tables(0, 0, qmc.MAX_COLUMNS - 1, 1)[0].shape == (1, BITS)
    with pytest.raises(ValueError):
        qmc.tables(0, 0, qmc.MAX_COLUMNS - 1, 2)
    with pytest.raises(ValueError):
        qmc.tables(0, 0, 0, 0)
    with pytest.raises(ValueError):
        qmc.tables(0, 0, -1, 2)


# ------------------------------------------------------------------------------------------ B: the entry point

def fill(backend, N, dirs, shift, row0=0, ldz=None, offset=0, ncols=None, null=()):
    """ttm_sobol_normal_fill into a sentinel-filled buffer, laid out as test_sample.fill's.  Returns (rc, whole buffer on the
    host, the matrix as an (ncols + 1, ldz) view of it)."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    dev = 'cpu' if backend == 'hostemu' else 'cuda'
    cols = len(dirs)
    ncols = cols if ncols is None else ncols
    ldz = N + (N & 1) if ldz is None else ldz
    buf = torch.full((offset + (cols + 1) * max(ldz, 1) + 2,), SENTINEL, dtype=torch.float64, device=dev)
    assert buf.data_ptr() % 16 == 0
    d = torch.from_numpy(np.ascontiguousarray(dirs, dtype=np.uint32).view(np.int32)).to(dev)
    s = None if shift is None else torch.from_numpy(np.ascontiguousarray(shift, dtype=np.uint32).view(np.int32)).to(dev)
    rc = lib.ttm_sobol_normal_fill(None if 'Z' in null else ctypes.c_void_p(buf.data_ptr() + 8 * offset), ldz, N, ncols,
                                   None if 'dirs' in null else ctypes.c_void_p(d.data_ptr()),
                                   None if s is None else ctypes.c_void_p(s.data_ptr()), row0, None)
    if backend == 'hip':
        torch.cuda.synchronize()
    hostbuf = buf.cpu().numpy().copy()
    return rc, hostbuf, hostbuf[offset:offset + (cols + 1) * max(ldz, 1)].reshape(cols + 1, max(ldz, 1))


def filled(backend, N, dirs, shift, **kw):
    """The N filled rows of every column, after the checks every fill gets: return code 0, nothing written outside."""
    rc, hostbuf, M = fill(backend, N, dirs, shift, **kw)
    assert rc == 0
    offset, ncols = kw.get('offset', 0), len(dirs)
    assert np.all(hostbuf[:offset] == SENTINEL) and np.all(M[:ncols, N:] == SENTINEL) and np.all(M[ncols] == SENTINEL) and np.all(hostbuf[-2:] == SENTINEL)
    return M[:ncols, :N]


def test_fill_against_the_restatement(backend):
    N = 4099
    bound = PHI_BOUND + scipy_error()
    print('ndtri against mpmath on the probes: %.3e; bound of the comparison %.3e' % (scipy_error(), bound))
    for which in (None, (5, 3)):
        for ncols in (1, 3, 70):
            dirs, shift = tables_of(which, 0, ncols)
            for row0 in (0, 1, 2 ** 29 + 5):
                Z = filled(backend, N, dirs, shift, row0=row0)
                err = rel(Z, expected(dirs, shift, row0, N))
                print('%s %s ncols %d row0 %d: max |a - b| / |b| = %.3e' % (backend, which, ncols, row0, err))
                assert err <= bound


def test_the_last_rows_of_the_sequence(backend):
    dirs, shift = tables(3, 1, 0, 2)
    Z = filled(backend, 1500, dirs, shift, row0=2 ** 30 - 1500)
    assert rel(Z, expected(dirs, shift, 2 ** 30 - 1500, 1500)) <= PHI_BOUND + scipy_error()


def test_a_window_of_rows_equals_those_rows_of_the_whole(backend):
    dirs, shift = tables(9, 2, 0, 3)
    whole = filled(backend, 2101, dirs, shift)
    for start in (337, 338, 1023, 1024):                    # both parities, and both sides of a workgroup's block of rows
        part = filled(backend, 1050, dirs, shift, row0=start)
        assert np.array_equal(part, whole[:, start:start + 1050]), start


def test_a_column_does_not_depend_on_the_columns_of_the_call(backend):
    dirs, shift = tables(3, 1, 0, 70)
    many = filled(backend, 777, dirs, shift)
    for j in (0, 1, 15, 16, 17, 69):
        assert np.array_equal(filled(backend, 777, dirs[j:j + 1], shift[j:j + 1])[0], many[j]), j
    assert np.array_equal(filled(backend, 777, dirs[14:37], shift[14:37]), many[14:37])


def test_small_and_odd_shapes_alignment_and_padding(backend):
    dirs, shift = tables(11, 5, 0, 2)
    whole = filled(backend, 4200, dirs, shift)
    for N in (1, 2, 3, 4097):
        for row0 in (0, 1, 6, 7):
            ref = whole[:, row0:row0 + N]
            assert np.array_equal(filled(backend, N, dirs, shift, row0=row0), ref), (N, row0)
            # the matrix 8 bytes past a 16-byte boundary; an odd leading dimension with padding rows (sentinels: `filled`)
            assert np.array_equal(filled(backend, N, dirs, shift, row0=row0, offset=1), ref), (N, row0)
            assert np.array_equal(filled(backend, N, dirs, shift, row0=row0, ldz=N + 3), ref), (N, row0)
            assert np.array_equal(filled(backend, N, dirs, shift, row0=row0, ldz=N + 3, offset=1), ref), (N, row0)


def test_a_null_shift_is_a_zero_shift(backend):
    dirs, shift = tables(0, 0, 0, 3, scramble=False)
    assert np.array_equal(filled(backend, 1001, dirs, None, row0=5), filled(backend, 1001, dirs, shift, row0=5))
    scr, _ = tables(4, 4, 0, 3)
    assert np.array_equal(filled(backend, 1001, scr, None, row0=5), filled(backend, 1001, scr, np.zeros(3, dtype=np.uint32), row0=5))


def test_argument_errors(backend):
    dirs, shift = tables(1, 1, 0, 2)
    good = dict(N=10, row0=0, ldz=10)
    assert fill(backend, dirs=dirs, shift=shift, **good)[0] == 0
    bad = [dict(N=0), dict(N=-1), dict(ncols=0), dict(ncols=-1), dict(ldz=9), dict(row0=-1), dict(row0=2 ** 30 - 9), dict(row0=2 ** 30 + 1),
           dict(row0=2 ** 62), dict(null=('Z',)), dict(null=('dirs',))]
    for change in bad:
        rc, hostbuf, _ = fill(backend, dirs=dirs, shift=shift, **dict(good, **change))
        print('%s %s: %d' % (backend, change, rc))
        assert rc == E_ARG, change
        assert np.all(hostbuf == SENTINEL), change            # nothing was launched
    assert fill(backend, dirs=dirs, shift=shift, N=10, ldz=10, row0=2 ** 30 - 10)[0] == 0


# ------------------------------------------------------------------------------------------ C: the quantile function at chosen arguments

def test_normal_quantile_at_chosen_arguments(backend):
    """The identity table dirs[b] = 1 << b makes q = gray(row) XOR shift: row 0 of column j is the point shift[j]."""
    qs, ref = probes()
    assert 150 <= len(qs) <= 260 and qs[0] == 0 and qs[-1] == TOP
    dirs = np.tile((1 << np.arange(BITS)).astype(np.uint32), (len(qs), 1))
    z = filled(backend, 1, dirs, qs.astype(np.uint32))[:, 0]
    err = rel_to_mpmath(z, ref)
    print('%s: normal_quantile against mpmath on %d probes: %.3e = %.2f * 2^-52 (bound %.3e = %d * 2^-52; host build %.2e)'
          % (backend, len(qs), err, err / 2.0 ** -52, PHI_BOUND, round(PHI_BOUND / 2.0 ** -52), HOST_WORST))
    assert err <= PHI_BOUND
    assert np.all(np.diff(z) > 0)                              # increasing in q
    anti = float(np.max(np.abs(z + z[::-1]) / np.abs(z)))       # the probe set is its own mirror image: q <-> 2^30 - 1 - q
    print('%s: antisymmetry %.3e' % (backend, anti))
    assert np.array_equal(qs, TOP - qs[::-1]) and anti <= PHI_BOUND
    # a row of the same table beside 1/2: gray(n) XOR shift with a shift that lands on 2^29 - 1 and 2^29
    for n in (5, 2 ** 29 + 77):
        g = n ^ (n >> 1)
        pair = filled(backend, 1, dirs[:2], np.array([g ^ (2 ** 29 - 1), g ^ 2 ** 29], dtype=np.uint32), row0=n)[:, 0]
        k = int(np.searchsorted(qs, 2 ** 29 - 1))
        assert np.array_equal(pair, z[k:k + 2]), n


# ------------------------------------------------------------------------------------------ D: the class

def expected_draws(seed, draw, col0, ncols, row0, N, scramble=True):
    dirs, shift = tables(seed, draw, col0, ncols, scramble=scramble)
    return expected(dirs, shift, row0, N)


@pytest.mark.parametrize('name,N,override', DEVICE_CASES, ids=['c3_sep', 'c2b_sep', 'c5_sep', 'c5_sep_newton', 'c2a_int'])
def test_sample_device_is_fill_plus_inverse(backend, name, N, override):
    tm, _ = make(name, **override)
    seed, draw = 17, 4
    Z = tm.reference_device(N, seed=seed, draw=draw, sequence='sobol')
    assert tuple(Z.shape) == (tm.D, N + (N & 1))
    assert last_kernel(tm) == ('hostemu' if backend == 'hostemu' else 'k_sobol_normal_fill')
    Zh = host(Z, N)
    err = rel(Zh, expected_draws(seed, draw, 0, tm.D, 0, N))
    print('%s %s: reference_device against the restatement %.3e (bound %.3e)' % (backend, name, err, PHI_BOUND + scipy_error()))
    assert err <= PHI_BOUND + scipy_error()
    Xa = host(tm.inverse_device(Z, N), N)
    kernel_a = last_kernel(tm)
    Xb = host(tm.sample_device(N, seed=seed, draw=draw, sequence='sobol'), N)
    kernel_b = last_kernel(tm)
    print('%s %s: inverse kernel %s / %s' % (backend, name, kernel_a, kernel_b))
    assert kernel_a == kernel_b
    assert np.all(np.isfinite(Xb)) and np.array_equal(Xa, Xb)
    assert tm._draws == 0                                     # explicit draws leave the map's counter alone
    assert not np.array_equal(Zh, host(tm.reference_device(N, seed=seed, draw=draw), N))          # 'random' stays the default


def draws_host(tm, N, seed, draw, ncols, col0=0, row0=0, **kw):
    """The host copy (N x ncols, as inverse_map takes it) of reference_device(..., sequence='sobol')."""
    Z = tm.reference_device(N, seed=seed, draw=draw, ncols=ncols, col0=col0, row0=row0, sequence='sobol', **kw)
    return np.ascontiguousarray(host(Z, N).T)


@pytest.mark.parametrize('N', [1, 2, 1001])
def test_sample_is_inverse_map_of_the_draws(backend, N):
    tm, _ = make('c3_sep')
    X = tm.sample(N, seed=2, draw=7, sequence='sobol')
    assert X.shape == (N, tm.D)
    assert np.array_equal(X, tm.inverse_map(draws_host(tm, N, 2, 7, tm.D)))
    Xp = tm.sample(N, seed=2, draw=7, sequence='sobol', scramble=False)
    assert np.array_equal(Xp, tm.inverse_map(draws_host(tm, N, 2, 7, tm.D, scramble=False)))


def test_sample_with_conditioning_columns_in_front(backend):
    tm, _ = make('ex02_partial')
    assert tm.skip_dimensions == 1 and tm.D == 1
    N = 501
    X_star = np.linspace(-0.8, 0.9, N)[:, None]
    X = tm.sample(N, X_star=X_star, seed=1, draw=0, sequence='sobol')
    assert X.shape == (N, 1)
    assert np.array_equal(X, tm.inverse_map(draws_host(tm, N, 1, 0, 1), X_star=X_star))


def test_conditional_sample_is_the_tail_of_the_unconditional_one(backend):
    tm, npz = make('c3_sep')
    N, E = 501, 2
    X_star = np.asarray(npz['X'][:N, :E], dtype=float)
    X = tm.sample(N, X_star=X_star, seed=8, draw=1, sequence='sobol')
    assert X.shape == (N, tm.D)
    assert np.array_equal(X, tm.inverse_map(draws_host(tm, N, 8, 1, tm.D - E, col0=E), X_star=X_star))
    assert np.array_equal(draws_host(tm, N, 8, 1, tm.D - E, col0=E), draws_host(tm, N, 8, 1, tm.D)[:, E:])
    # one conditioning point, as (E,), (1, E) and repeated
    point = X_star[3]
    ref = tm.sample(N, X_star=np.repeat(point[None, :], N, axis=0), seed=8, draw=1, sequence='sobol')
    assert np.array_equal(ref, tm.inverse_map(draws_host(tm, N, 8, 1, tm.D - E, col0=E), X_star=np.repeat(point[None, :], N, axis=0)))
    assert np.array_equal(tm.sample(N, X_star=point, seed=8, draw=1, sequence='sobol'), ref)
    assert np.array_equal(tm.sample(N, X_star=point[None, :], seed=8, draw=1, sequence='sobol'), ref)


def test_draw_counter_explicit_draws_and_errors(backend):
    tm, _ = make('c3_sep')
    kw = dict(sequence='sobol')
    a, b = tm.sample(64, seed=4, **kw), tm.sample(64, seed=4, **kw)
    assert tm._draws == 2 and not np.array_equal(a, b)
    assert np.array_equal(a, tm.sample(64, seed=4, draw=0, **kw)) and np.array_equal(b, tm.sample(64, seed=4, draw=1, **kw))
    assert tm._draws == 2
    assert np.array_equal(tm.sample(64, seed=4, draw=9, **kw), tm.sample(64, seed=4, draw=9, **kw))
    assert not np.array_equal(tm.sample(64, seed=5, draw=9, **kw), tm.sample(64, seed=4, draw=9, **kw))
    Z = host(tm.reference_device(64, seed=4, **kw), 64)      # the third draw of the map's counter
    assert tm._draws == 3 and np.array_equal(Z, host(tm.reference_device(64, seed=4, draw=2, **kw), 64))
    # the plain sequence: neither draw nor seed has an effect
    plain = tm.sample(64, seed=4, draw=0, scramble=False, **kw)
    assert np.array_equal(plain, tm.sample(64, seed=11, draw=5, scramble=False, **kw)) and not np.array_equal(plain, a)
    assert np.array_equal(plain, tm.sample(64, scramble=False, **kw)) and tm._draws == 4
    for call in (tm.sample, tm.sample_device, tm.reference_device):
        with pytest.raises(ValueError, match='sequence'):
            call(64, sequence='halton')
        with pytest.raises(ValueError, match='2\\^30'):
            call(64, row0=2 ** 30 - 63, **kw)
    with pytest.raises(ValueError):
        tm.sample(64, draw=2 ** 31, **kw)
    assert tm._draws == 4
    assert tm.sample(64, row0=2 ** 30 - 64, draw=0, **kw).shape == (64, tm.D)


def test_column_means_of_a_stratified_sample(backend):
    """One point per stratum of width 1 / N: the mean of N = 4096 deviates is within (z(1 - 2^-31) - z(2^-31)) / N = 2.99e-3 of 0
    (each point moved to the worst end of its stratum: the sum telescopes).  Random draws have a standard deviation of 1.56e-2."""
    from scipy.special import ndtri
    tm, _ = make('c3_sep')
    N = 4096
    cap = float(ndtri(1 - 2.0 ** -31) - ndtri(2.0 ** -31)) / N
    assert abs(cap - 2.99e-3) < 1e-5
    for kw in (dict(scramble=False), dict(seed=0, draw=0), dict(seed=5, draw=3), dict(seed=12345, draw=1), dict(seed=5, draw=4)):
        Z = host(tm.reference_device(N, ncols=40, sequence='sobol', **kw), N)
        worst = float(np.max(np.abs(Z.mean(axis=1))))
        print('%s %s: largest |column mean| %.3e (cap %.3e)' % (backend, kw, worst, cap))
        assert worst <= cap


# ------------------------------------------------------------------------------------------ E: rows sharded over two ranks (CPU)

SHARD_N, SHARD_SEED, SHARD_DRAW = 801, 21, 5


def _worker(rank, world, port, override, outdir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        with emu.install():
            tm, _ = make('c3_sep', **override)
            tm.shard_samples = True
            cut = SHARD_N // 2 + 3                                          # an odd offset
            lo, hi = (0, cut) if rank == 0 else (cut, SHARD_N)
            X = tm.sample(hi - lo, seed=SHARD_SEED, draw=SHARD_DRAW, row0=lo, sequence='sobol')
        np.savez(os.path.join(outdir, 'rank%d.npz' % rank), X=X)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('override', [{}, dict(alternate_root_finding=False)], ids=['table', 'bisection'])
def test_two_ranks_draw_what_one_rank_draws(override, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), override, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    with emu.install():
        one = make('c3_sep', **override)[0].sample(SHARD_N, seed=SHARD_SEED, draw=SHARD_DRAW, sequence='sobol')
    both = np.vstack((r0['X'], r1['X']))
    assert both.shape == one.shape and np.all(np.isfinite(one)) and np.array_equal(both, one)
