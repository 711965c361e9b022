"""
Reference draws on the device and sampling from a fitted map: ttm_normal_fill / k_normal_fill (include/ttm.h, csrc/ttm_rng.h:
normal_pair) and transport_map.reference_device / sample_device / sample, on the host test double and on the GPU.

The expected deviates come from a NumPy restatement of the counter layout in this file (`philox4x32_10`, `expected`): Philox on
uint64 arrays, np.log, np.sqrt, np.cos, np.sin - a GPU process never loads the host double.  Every figure is printed before it
is held.

Bound of the comparison with the restatement: |a - b| <= 256 * 2^-52 * (1 + |b|).  Derived, not measured: with log, sqrt, sin
and cos each within 4 ulp on either side the error is at most R (pi + 4) ulp from the angle 2 pi u2 and the trigonometric call
plus a few ulp relative from log and sqrt; R <= sqrt(2 * 54 * ln 2) = 8.66, so both sides together stay below 130 * 2^-52
absolute, and 256 leaves a factor of two.  Comparisons of two fills of one backend are bitwise.

The caps of the distribution test are conditions on a deterministic generator (each figure is a standardised statistic of
N = 65 536 deviates: 4 is four standard deviations, 1.95 the 0.1 % point of the Kolmogorov distribution); the restatement itself
is held to them by a test that needs no library - it gives at most 1.96, 2.95, 2.94, 1.47, 1.70 and 2.12 on these inputs, and a
largest |z| of 5.02 (seed 5, draw 0).
"""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 256.0 * 2.0 ** -52
SENTINEL = -7.25e300
E_ARG = -1


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


# ------------------------------------------------------------------------------------------ the restatement (NumPy alone)

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint64 arrays / scalars that hold 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def expected(seed, draw, col, rows):
    """The deviates of column `col` at the global rows `rows` (any integers < 2^63) of draw `draw` under `seed`."""
    rows = np.asarray(rows, dtype=np.uint64)
    p = rows >> np.uint64(1)
    seed = np.uint64(seed)
    r0, r1, r2, r3 = philox4x32_10(p & M32, p >> np.uint64(32), np.uint64(col), np.uint64(0x80000000 | draw), seed & M32, seed >> np.uint64(32))
    u1 = ((((r0 << np.uint64(32)) | r1) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    u2 = ((((r2 << np.uint64(32)) | r3) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    R, t = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586477 * u2
    return np.where((rows & np.uint64(1)) == 0, R * np.cos(t), R * np.sin(t))


def expected_matrix(seed, draw, col0, ncols, row0, N):
    rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
    return np.stack([expected(seed, draw, col0 + j, rows) for j in range(ncols)])


KNOWN = {0: [-0.93970707, -2.05455670, 1.16710235, 0.37488446], 1: [-0.46600936, 0.72985492]}     # seed 5, draw 0


def test_restatement_reproduces_the_known_answer():
    for col, vals in KNOWN.items():
        got = expected(5, 0, col, np.arange(len(vals)))
        print('restatement, column %d: %s' % (col, ' '.join('%.8f' % v for v in got)))
        assert np.max(np.abs(got - np.array(vals))) <= 1e-8


# ------------------------------------------------------------------------------------------ A / B: the entry point

def fill(backend, N, ncols, col0=0, seed=0, draw=0, row0=0, ldz=None, offset=0):
    """ttm_normal_fill into a sentinel-filled buffer: `offset` doubles of slack in front (offset = 1: the matrix starts 8 bytes
    past a 16-byte boundary), ncols + 1 columns of ldz doubles behind.  Returns (rc, whole buffer on the host, the matrix
    as an (ncols + 1, ldz) view of it)."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    ldz = N + (N & 1) if ldz is None else ldz
    buf = torch.full((offset + (ncols + 1) * max(ldz, 1) + 2,), SENTINEL, dtype=torch.float64, device='cpu' if backend == 'hostemu' else 'cuda')
    assert buf.data_ptr() % 16 == 0
    rc = lib.ttm_normal_fill(ctypes.c_void_p(buf.data_ptr() + 8 * offset), ldz, N, ncols, col0, seed, draw, row0, None)
    if backend == 'hip':
        torch.cuda.synchronize()
    host = buf.cpu().numpy().copy()
    return rc, host, host[offset:offset + (ncols + 1) * max(ldz, 1)].reshape(ncols + 1, max(ldz, 1))


def filled(backend, N, ncols, **kw):
    """The N filled rows of every column, after the checks every fill gets: return code 0, nothing written outside."""
    rc, host, M = fill(backend, N, ncols, **kw)
    assert rc == 0
    offset = kw.get('offset', 0)
    assert np.all(host[:offset] == SENTINEL) and np.all(M[:ncols, N:] == SENTINEL) and np.all(M[ncols] == SENTINEL) and np.all(host[-2:] == SENTINEL)
    return M[:ncols, :N]


def test_known_answer(backend):
    Z = filled(backend, 4, 2, seed=5, draw=0)
    print('%s, column 0: %s; column 1: %s' % (backend, ' '.join('%.8f' % v for v in Z[0]), ' '.join('%.8f' % v for v in Z[1, :2])))
    assert np.max(np.abs(Z[0] - np.array(KNOWN[0]))) <= 1e-8
    assert np.max(np.abs(Z[1, :2] - np.array(KNOWN[1]))) <= 1e-8


def test_fill_against_the_restatement(backend):
    N, ncols = 4099, 3
    worst = 0.0
    for seed in (5, 2 ** 40 + 7):
        for draw in (0, 3):
            for col0 in (0, 2):
                for row0 in (0, 1, 2 ** 33 + 5):
                    Z = filled(backend, N, ncols, col0=col0, seed=seed, draw=draw, row0=row0)
                    ref = expected_matrix(seed, draw, col0, ncols, row0, N)
                    err = float(np.max(np.abs(Z - ref) / (1.0 + np.abs(ref))))
                    print('%s seed %d draw %d col0 %d row0 %d: max |a - b| / (1 + |b|) = %.3e (bound %.3e)' % (backend, seed, draw, col0, row0, err, TOL))
                    worst = max(worst, err)
                    assert err <= TOL
    assert worst <= TOL


def test_a_window_of_rows_equals_those_rows_of_the_whole(backend):
    whole = filled(backend, 1001, 3, seed=9, draw=2)
    for start in (337, 338):                                # both parities
        part = filled(backend, 200, 3, seed=9, draw=2, row0=start)
        assert np.array_equal(part, whole[:, start:start + 200]), start


def test_a_column_does_not_depend_on_the_columns_of_the_call(backend):
    five = filled(backend, 777, 5, seed=3, draw=1)
    for j in range(5):
        assert np.array_equal(filled(backend, 777, 1, col0=j, seed=3, draw=1)[0], five[j]), j


def test_small_and_odd_shapes_alignment_and_padding(backend):
    whole = filled(backend, 4200, 2, seed=11, draw=5)
    for N in (1, 2, 3, 4097):
        for row0 in (0, 1, 6, 7):
            ref = whole[:, row0:row0 + N]
            assert np.array_equal(filled(backend, N, 2, seed=11, draw=5, row0=row0), ref), (N, row0)
            # the matrix 8 bytes past a 16-byte boundary; an odd leading dimension with padding rows (sentinels: `filled`)
            assert np.array_equal(filled(backend, N, 2, seed=11, draw=5, row0=row0, offset=1), ref), (N, row0)
            assert np.array_equal(filled(backend, N, 2, seed=11, draw=5, row0=row0, ldz=N + 3), ref), (N, row0)
            assert np.array_equal(filled(backend, N, 2, seed=11, draw=5, row0=row0, ldz=N + 3, offset=1), ref), (N, row0)


def test_argument_errors(backend):
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    good = dict(N=10, ncols=2, col0=0, draw=0, row0=0, ldz=10)
    bad = [dict(N=0), dict(N=-1), dict(ncols=0), dict(col0=-1), dict(ldz=9), dict(row0=-1), dict(draw=2 ** 31), dict(draw=2 ** 32 - 1)]
    assert fill(backend, **good)[0] == 0
    for change in bad:
        kw = dict(good, **change)
        rc, host, _ = fill(backend, **kw)
        print('%s %s: %d' % (backend, change, rc))
        assert rc == E_ARG, change
        assert np.all(host == SENTINEL), change            # nothing was launched
    assert lib.ttm_normal_fill(None, 10, 10, 2, 0, 0, 0, 0, None) == E_ARG
    if backend == 'hip':
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ C: the distribution

CAPS = {'mean': 4.0, 'var': 4.0, 'kurt': 4.0, 'ks': 1.95, 'cross': 4.0, 'lag1': 4.0, 'max': 8.7}
DIST_N, DIST_COLS = 65536, 4
DIST_CASES = [(seed, row0, draw) for seed in (0, 5, 12345) for row0 in (0, 1) for draw in (0, 3)]


def figures(Z):
    """The standardised statistics of a (columns, N) matrix of deviates, the largest over the columns of each."""
    from scipy.special import ndtr
    n = Z.shape[1]
    grid = np.arange(1, n + 1) / n
    ks = 0.0
    for z in Z:
        cdf = ndtr(np.sort(z))
        ks = max(ks, float(np.max(grid - cdf)), float(np.max(cdf - (grid - 1.0 / n))))
    cross = np.corrcoef(Z)
    return {'mean': float(np.max(np.abs(Z.mean(axis=1))) * np.sqrt(n)),
            'var': float(np.max(np.abs(Z.var(axis=1) - 1.0)) * np.sqrt(n / 2.0)),
            'kurt': float(np.max(np.abs((Z ** 4).mean(axis=1) - 3.0)) * np.sqrt(n / 96.0)),
            'ks': ks * np.sqrt(n),
            'cross': float(np.max(np.abs(cross[np.triu_indices(Z.shape[0], 1)])) * np.sqrt(n)),
            'lag1': float(max(abs(np.corrcoef(z[:-1], z[1:])[0, 1]) for z in Z) * np.sqrt(n)),
            'max': float(np.max(np.abs(Z)))}


def hold_caps(label, fig):
    print('%s: %s' % (label, ', '.join('%s %.3f' % (k, fig[k]) for k in CAPS)))
    for k, cap in CAPS.items():
        assert (fig[k] < cap) if k == 'max' else (fig[k] <= cap), (label, k, fig[k], cap)


def test_the_restatement_meets_the_distribution_caps():
    worst = dict.fromkeys(CAPS, 0.0)
    for seed, row0, draw in DIST_CASES:
        fig = figures(expected_matrix(seed, draw, 0, DIST_COLS, row0, DIST_N))
        hold_caps('restatement seed %d row0 %d draw %d' % (seed, row0, draw), fig)
        worst = {k: max(worst[k], fig[k]) for k in CAPS}
    print('restatement, largest over the cases: %s' % ', '.join('%s %.2f' % (k, worst[k]) for k in CAPS))


def test_distribution(backend):
    for seed, row0, draw in DIST_CASES:
        Z = filled(backend, DIST_N, DIST_COLS, seed=seed, draw=draw, row0=row0)
        hold_caps('%s seed %d row0 %d draw %d' % (backend, seed, row0, draw), figures(Z))


# ------------------------------------------------------------------------------------------ D / E: the class

def make(name, n_train=None, **override):
    """A map of a golden case with the fixture's coefficients; n_train: the first rows of the training ensemble only."""
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    if name == 'c5_sep':
        X = specs.sample_mixture(n_train or 4000)
    else:
        X = case_X(name, npz)
        X = X if n_train is None else X[:n_train]
    kw = ctor_kwargs(desc)
    kw.update(override)
    tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **kw)
    tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
    return tm, npz


def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


def host(t, N):
    return t[:, :N].cpu().numpy().copy()


DEVICE_CASES = [('c3_sep', 1001, {}), ('c2b_sep', 4097, {}), ('c5_sep', 65539, {}),
                ('c5_sep', 65539, dict(alternate_root_finding=False, root_finder='newton')), ('c2a_int', 1001, {})]


@pytest.mark.parametrize('name,N,override', DEVICE_CASES, ids=['c3_sep', 'c2b_sep', 'c5_sep', 'c5_sep_newton', 'c2a_int'])
def test_sample_device_is_fill_plus_inverse(backend, name, N, override):
    tm, _ = make(name, **override)
    seed, draw = 17, 4
    Z = tm.reference_device(N, seed=seed, draw=draw)
    assert tuple(Z.shape) == (tm.D, N + (N & 1))
    assert last_kernel(tm) == ('hostemu' if backend == 'hostemu' else 'k_normal_fill')
    Zh = host(Z, N)
    ref = expected_matrix(seed, draw, 0, tm.D, 0, N)
    err = float(np.max(np.abs(Zh - ref) / (1.0 + np.abs(ref))))
    print('%s %s: reference_device against the restatement %.3e (bound %.3e)' % (backend, name, err, TOL))
    assert err <= TOL
    Xa = host(tm.inverse_device(Z, N), N)
    kernel_a = last_kernel(tm)
    Xb = host(tm.sample_device(N, seed=seed, draw=draw), N)
    kernel_b = last_kernel(tm)
    print('%s %s: inverse kernel %s / %s' % (backend, name, kernel_a, kernel_b))
    assert kernel_a == kernel_b
    assert np.all(np.isfinite(Xb)) and np.array_equal(Xa, Xb)
    assert tm._draws == 0                                     # explicit draws leave the map's counter alone


def draws_host(tm, N, seed, draw, ncols, col0=0, row0=0):
    """The host copy (N x ncols, as inverse_map takes it) of reference_device(...)."""
    return np.ascontiguousarray(host(tm.reference_device(N, seed=seed, draw=draw, ncols=ncols, col0=col0, row0=row0), N).T)


@pytest.mark.parametrize('N', [1, 2, 1001])
def test_sample_is_inverse_map_of_the_draws(backend, N):
    tm, _ = make('c3_sep')
    assert N < tm.PIPE_MIN_ROWS
    X = tm.sample(N, seed=2, draw=7)
    assert X.shape == (N, tm.D)
    assert np.array_equal(X, tm.inverse_map(draws_host(tm, N, 2, 7, tm.D)))


def test_sample_with_conditioning_columns_in_front(backend):
    """skip_dimensions = 1 (Example 02: the integrated second spiral component alone, bisection with the sample-0 replay)."""
    tm, _ = make('ex02_partial')
    assert tm.skip_dimensions == 1 and tm.D == 1
    N = 501
    X_star = np.linspace(-0.8, 0.9, N)[:, None]
    X = tm.sample(N, X_star=X_star, seed=1, draw=0)
    assert X.shape == (N, 1)
    assert np.array_equal(X, tm.inverse_map(draws_host(tm, N, 1, 0, 1), X_star=X_star))


def test_sample_with_more_conditioning_columns_than_map_columns_takes(backend):
    """Example 04: 20 conditioning columns (ttm_map_columns takes 16); varying rows, then one point in its three shapes."""
    tm, npz = make('ex04_monod')
    assert tm.skip_dimensions == 20 and tm.D == 2
    N = 501
    X_star = np.resize(npz['inv_Xstar'], (N, 20))
    Z = draws_host(tm, N, 6, 2, 2)
    assert np.array_equal(tm.sample(N, X_star=X_star, seed=6, draw=2), tm.inverse_map(Z, X_star=X_star))
    obs = np.asarray(npz['obs'], dtype=float)
    ref = tm.inverse_map(Z, X_star=np.repeat(obs[None, :], N, axis=0))
    assert np.array_equal(tm.sample(N, X_star=np.repeat(obs[None, :], N, axis=0), seed=6, draw=2), ref)
    assert np.array_equal(tm.sample(N, X_star=obs[None, :], seed=6, draw=2), ref)
    assert np.array_equal(tm.sample(N, X_star=obs, seed=6, draw=2), ref)


def test_conditional_sample_is_the_tail_of_the_unconditional_one(backend):
    """The skip_dimensions == 0 shape with a 2-column X_star: component k draws from column k."""
    tm, npz = make('c3_sep')
    N, E = 501, 2
    X_star = np.asarray(npz['X'][:N, :E], dtype=float)
    X = tm.sample(N, X_star=X_star, seed=8, draw=1)
    assert X.shape == (N, tm.D)
    assert np.array_equal(X, tm.inverse_map(draws_host(tm, N, 8, 1, tm.D - E, col0=E), X_star=X_star))
    assert np.array_equal(draws_host(tm, N, 8, 1, tm.D - E, col0=E), draws_host(tm, N, 8, 1, tm.D)[:, E:])
    # one conditioning point, as (E,), (1, E) and repeated
    point = X_star[3]
    ref = tm.sample(N, X_star=np.repeat(point[None, :], N, axis=0), seed=8, draw=1)
    assert np.array_equal(tm.sample(N, X_star=point, seed=8, draw=1), ref)
    assert np.array_equal(tm.sample(N, X_star=point[None, :], seed=8, draw=1), ref)


def test_draw_counter_and_explicit_draws(backend):
    tm, _ = make('c3_sep')
    a, b = tm.sample(64, seed=4), tm.sample(64, seed=4)
    assert tm._draws == 2 and not np.array_equal(a, b)
    assert np.array_equal(a, tm.sample(64, seed=4, draw=0)) and np.array_equal(b, tm.sample(64, seed=4, draw=1))
    assert tm._draws == 2
    assert np.array_equal(tm.sample(64, seed=4, draw=9), tm.sample(64, seed=4, draw=9))
    assert not np.array_equal(tm.sample(64, seed=5, draw=9), tm.sample(64, seed=4, draw=9))
    Z = host(tm.reference_device(64, seed=4), 64)            # the third draw of the map's counter
    assert tm._draws == 3 and np.array_equal(Z, host(tm.reference_device(64, seed=4, draw=2), 64))
    with pytest.raises(ValueError):
        tm.sample(64, draw=2 ** 31)
    with pytest.raises(ValueError):
        tm.sample(0)


def test_sample_without_standardisation(backend):
    tm, _ = make('c3_sep', standardize_samples=False)
    N = 501
    assert np.array_equal(tm.sample(N, seed=3, draw=3), tm.inverse_map(draws_host(tm, N, 3, 3, tm.D)))


def test_x_star_shape_errors_are_those_of_inverse_map(backend):
    tm, npz = make('c3_sep')
    N = 50
    Z = draws_host(tm, N, 0, 0, tm.D)
    with pytest.raises(ValueError, match='together'):                         # more columns than the map has
        tm.inverse_map(Z, X_star=np.zeros((N, tm.D + 1)))
    for width in (tm.D, tm.D + 1):                                            # no component left to draw
        with pytest.raises(ValueError, match='together'):
            tm.sample(N, X_star=np.zeros((N, width)))
    # a conditioning block with another number of rows: the copy into the columns fails in both
    with pytest.raises(RuntimeError) as e_inv:
        tm.inverse_map(Z[:, 2:], X_star=np.zeros((N - 7, 2)))
    with pytest.raises(RuntimeError) as e_smp:
        tm.sample(N, X_star=np.zeros((N - 7, 2)))
    assert str(e_inv.value) == str(e_smp.value)
    # conditioning columns in front (skip_dimensions > 0) and an X_star of another width: the reference's UnboundLocalError
    tm2, _ = make('ex04_monod')
    with pytest.raises(UnboundLocalError):
        tm2.inverse_map(np.zeros((N, 2)), X_star=np.zeros((N, 3)))
    with pytest.raises(UnboundLocalError):
        tm2.sample(N, X_star=np.zeros((N, 3)))


# ------------------------------------------------------------------------------------------ F: rows sharded over two ranks (CPU)

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


SHARD_N, SHARD_SEED, SHARD_DRAW = 801, 21, 5


def _shard_map(override):
    """The map of both ranks and of the single process: built from the whole training ensemble, so all three hold the same bits;
    the ranks then share the ROWS OF THE DRAW (shard_samples switches on the all-reduced iteration caps and the replay of global
    sample 0 on rank 0)."""
    tm, _ = make('c3_sep', **override)
    return tm


def _worker(rank, world, port, override, outdir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        with emu.install():
            tm = _shard_map(override)
            tm.shard_samples = True
            cut = SHARD_N // 2 + 3                                          # an odd offset
            lo, hi = (0, cut) if rank == 0 else (cut, SHARD_N)
            before = emu.lib().ttm_hostemu_allreduce_calls()
            X = tm.sample(hi - lo, seed=SHARD_SEED, draw=SHARD_DRAW, row0=lo)
            calls = emu.lib().ttm_hostemu_allreduce_calls() - before
        np.savez(os.path.join(outdir, 'rank%d.npz' % rank), X=X, calls=calls)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('override', [{}, dict(alternate_root_finding=False)], ids=['table', 'bisection'])
def test_two_ranks_draw_what_one_rank_draws(override, tmp_path):
    import torch.multiprocessing as mp
    assert (SHARD_N // 2 + 3) % 2 == 1
    mp.spawn(_worker, args=(2, _free_port(), override, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    with emu.install():
        one = _shard_map(override).sample(SHARD_N, seed=SHARD_SEED, draw=SHARD_DRAW)
    both = np.vstack((r0['X'], r1['X']))
    print('all-reduces per rank: %d / %d' % (int(r0['calls']), int(r1['calls'])))
    assert int(r0['calls']) == int(r1['calls']) == (1 if override else 0)      # the iteration caps of the bisection
    assert both.shape == one.shape and np.all(np.isfinite(one)) and np.array_equal(both, one)
