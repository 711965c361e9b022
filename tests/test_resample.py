"""
Importance weights in fixed point and resampling: ttm_weight_scan / ttm_resample (include/ttm.h, csrc/ttm_resample.h, the kernels
k_weight_max .. k_weight_apply and k_resample of csrc/ttm_kernels.hip) and transport_map.weights_device / importance_summary /
resample_device / resample / sample_importance, on the host test double and on the GPU.

The scan tile of the kernels is 1024 rows (256 threads x 4 rows) and one pass of the tile-sum scan holds 256 tiles, so the row
counts are 1, 2, 63, 64, 65, 1023, 1024, 1025, 100 003 and 263 169 = 256 * 1024 + 1025 (258 tiles: the second pass of the tile-sum
scan holds two tiles, the last tile one row).  Offspring counts: 1, 2, N, 3 N + 1, 65 537.

What is exact and what has a bound (every bound is derived, none measured; every figure is printed before it is held):
  * K, the Philox words, the thresholds and the ancestor rule are restated here in NumPy on uint64 (`restated_ancestors`) and held
    against `fractions.Fraction` / Python integers at small sizes by a test that needs no library;
  * q against floor(exp(logw - m) 2^K) with mpmath's exponential at 80 bits: |difference| <= 1.  The kernels use fast_exp of
    csrc/ttm_math.h, held to 1 ulp by tests/test_device_math.py::test_fast_exp_device ('fast_exp/ulp_vs_mpmath'); any exponential
    within 4096 ulp puts exp(.) 2^K within 4096 * 2^-53 * 2^40 = 1/2 of the exact product, and the rounding of logw - m (half an ulp
    of a number below 1024: a relative 5.7e-14 of the exponential) adds 0.07 - below one unit together.  For speed mpmath is called
    where NumPy's exponential (within 2^-11 of the product) leaves the floor open and on the first 512 rows of every case;
    everywhere else the floor of NumPy's product IS the exact floor;
  * the rows of the maximum are 2^K, -inf / NaN / +inf rows are 0, m and the bad count are exact;
  * cum == np.cumsum(q) on uint64, T == cum[N - 1]: exact;
  * S2 against the exact rational sum q^2 / 4^K (integer arithmetic): relative (depth + 2) 2^-52 with depth = 18 + ceil(tiles / 256),
    the documented depth of the summation tree (10 levels inside a tile, one addition per pass, 8 levels over the running sums);
  * the ancestors equal the restatement applied to the backend's OWN cum for every offspring, the gathered entries are bitwise
    those of the source rows, padding around every output keeps its sentinel.
The host double and the GPU are never compared with each other (their exponentials may differ in the last bit).
"""
import ctypes
import fractions
import math

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case

E_ARG = -1
SENT_U64 = np.uint64(0xDEADBEEFCAFEF00D)
SENT_I32 = np.int32(-777)
SENT_F64 = -7.25e300
TILE, PASS = 1024, 256
N_ALL = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 100003, PASS * TILE + TILE + 1]
SCHEMES = {'systematic': 0, 'stratified': 1, 'multinomial': 2}
KINDS = ['gauss', 'spread', 'neginf', 'dominant', 'equal']


def m_list(N):
    return sorted({1, 2, N, 3 * N + 1, 65537})


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


# ------------------------------------------------------------------------------------------ the restatement (NumPy / Python integers)

M32 = np.uint64(0xFFFFFFFF)
U32 = np.uint64(32)


def weight_bits(N):
    c = 0
    while (1 << c) < N:
        c += 1
    return min(40, 62 - c)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint64 arrays / scalars that hold 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> U32) ^ c1 ^ k0, p1 & M32, (p0 >> U32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(seed, draw, scheme, j):
    """R_j = r[0] << 32 | r[1] of the block {lo32(j), hi32(j), 0xFFFFFFFF - scheme, 0x80000000 | draw} under the key of `seed`."""
    j = np.asarray(j, dtype=np.uint64)
    seed = np.uint64(seed)
    r0, r1, _, _ = philox4x32_10(j & M32, j >> U32, np.uint64(0xFFFFFFFF - scheme), np.uint64(0x80000000 | draw), seed & M32, seed >> U32)
    return (r0 << U32) | r1


def mulhi64(a, b):
    """High 64 bits of the 128-bit product of uint64 arrays (schoolbook on 32-bit halves, no intermediate leaves 64 bits)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    a0, a1, b0, b1 = a & M32, a >> U32, b & M32, b >> U32
    mid = a1 * b0 + ((a0 * b0) >> U32)
    mid2 = a0 * b1 + (mid & M32)
    return a1 * b1 + (mid >> U32) + (mid2 >> U32)


def restated_thresholds(T, M, scheme, seed, draw):
    j = np.arange(M, dtype=np.uint64)
    T64, M64 = np.uint64(T), np.uint64(M)
    R = words(seed, draw, scheme, np.zeros(M, dtype=np.uint64) if scheme == 0 else j)
    V = mulhi64(R, np.full(M, T64))
    if scheme == 2:
        return V
    a, b = T64 // M64, T64 % M64
    return j * a + (j * b + V) // M64


def restated_ancestors(cum, M, scheme, seed, draw):
    """idx_j = min { i : cum_i > t_j }, -1 for every j when T = 0."""
    cum = np.asarray(cum, dtype=np.uint64)
    T = int(cum[-1])
    if T == 0:
        return np.full(M, -1, dtype=np.int64)
    return np.searchsorted(cum, restated_thresholds(T, M, scheme, seed, draw), side='right').astype(np.int64)


def test_restatement_against_python_integers_and_fractions():
    """K, mulhi64, the words' layout, the thresholds and the ancestor rule of the NumPy restatement against Python integers and
    fractions.Fraction at small sizes; the thresholds stay below T and do not decrease for the two ordered schemes."""
    assert [weight_bits(n) for n in (1, 2, 3, 4, 2 ** 22, 2 ** 22 + 1, 2 ** 30)] == [40, 40, 40, 40, 40, 39, 32]
    rng = np.random.default_rng(1)
    a = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    b = np.concatenate((rng.integers(0, 2 ** 64, 196, dtype=np.uint64), np.array([0, 1, 2 ** 62, 2 ** 64 - 1], dtype=np.uint64)))
    assert [int(v) for v in mulhi64(a, b)] == [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    # known words (Philox-4x32-10 of the Random123 known-answer set: counter 0, key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8)
    r = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in r] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    checked = 0
    for N, M in [(1, 1), (1, 7), (5, 5), (7, 3), (13, 40), (64, 193)]:
        for kind in range(3):
            K = weight_bits(N)
            if kind == 0:
                q = rng.integers(0, 2 ** K + 1, N, dtype=np.uint64)
            elif kind == 1:
                q = np.where(rng.random(N) < 0.6, 0, rng.integers(0, 2 ** 20, N)).astype(np.uint64)
                q[rng.integers(N)] = 2 ** K
            else:
                q = np.full(N, 2 ** K, dtype=np.uint64)
            cum = np.cumsum(q, dtype=np.uint64)
            T = int(cum[-1])
            for scheme in range(3):
                for seed, draw in ((0, 0), (2 ** 40 + 7, 5)):
                    t = restated_thresholds(T, M, scheme, seed, draw)
                    idx = restated_ancestors(cum, M, scheme, seed, draw)
                    for j in range(M):
                        R = int(words(seed, draw, scheme, 0 if scheme == 0 else j))
                        V = (R * T) >> 64
                        want = V if scheme == 2 else math.floor(fractions.Fraction(j * T + V, M))
                        assert int(t[j]) == want and 0 <= want < T
                        anc = min(i for i in range(N) if int(cum[i]) > want)
                        assert int(idx[j]) == anc and int(q[anc]) > 0
                        checked += 1
                    if scheme < 2:
                        assert np.all(np.diff(t.astype(np.int64)) >= 0)
    print('restatement: %d thresholds and ancestors equal the Fraction / integer brute force' % checked)


# ------------------------------------------------------------------------------------------ inputs

def log_weights(kind, N, seed=0):
    rng = np.random.default_rng(1000 * N + seed)
    if kind == 'gauss':                       # the maximum is near -1e4: it has to be subtracted
        return 3.0 * rng.standard_normal(N) - 1.0e4
    if kind == 'spread':                      # 800 in log-weight: many q underflow to 0
        w = -800.0 * rng.random(N)
        w[rng.integers(N)] = 0.25
        return w
    if kind == 'neginf':
        w = rng.standard_normal(N)
        w[rng.random(N) < 0.4] = -np.inf
        w[rng.integers(N)] = 1.5
        return w
    if kind == 'dominant':                    # one row, all others -inf
        w = np.full(N, -np.inf)
        w[(7 * N) // 11] = -3.0
        return w
    assert kind == 'equal'
    return np.full(N, 0.7)


# ------------------------------------------------------------------------------------------ the entry points

def _lib():
    from triangular_transport_toolbox_amd import _capi
    return _capi.load()


def _dev(backend):
    return 'cpu' if backend == 'hostemu' else 'cuda'


def _sync(backend):
    if backend == 'hip':
        import torch
        torch.cuda.synchronize()


def padded(backend, n, dtype, sentinel, offset=0):
    """A sentinel-filled device buffer with 2 + offset words of 8 bytes in front of the n payload entries and 16 bytes behind;
    offset = 1: the payload starts 8 bytes past a 16-byte boundary.  Returns (tensor, byte address of the payload, view function)."""
    import torch
    item = np.dtype(dtype).itemsize
    front = 8 * (2 + offset)
    nbytes = front + item * n + 16
    nbytes += (-nbytes) % 8
    host = np.empty(nbytes // item, dtype=dtype)
    host[:] = sentinel
    t = torch.from_numpy(host.view(np.uint8)).to(_dev(backend))
    assert t.data_ptr() % 16 == 0
    lo = front // item

    def read():
        h = t.cpu().numpy().view(dtype)
        pay, pad = h[lo:lo + n], np.concatenate((h[:lo], h[lo + n:]))
        assert np.all(pad.view(np.uint8).reshape(-1, item) == np.array([sentinel], dtype=dtype).view(np.uint8)), 'padding overwritten'
        return pay.copy()
    return t, t.data_ptr() + front, read


def scan(backend, logw, offset=0, want_q=True, poison=None):
    """ttm_weight_scan on sentinel-padded buffers.  Returns (rc, q, cum, summary dict)."""
    import torch
    from triangular_transport_toolbox_amd import weights
    N = len(logw)
    lw_host = np.full(N + 2 + offset, SENT_F64)
    lw_host[1 + offset:1 + offset + N] = logw
    lw = torch.from_numpy(lw_host).to(_dev(backend))
    tc, pc, rc_ = padded(backend, N, np.uint64, SENT_U64, offset)
    tq, pq, rq = padded(backend, N, np.uint64, SENT_U64, offset)
    ts, ps, rs = padded(backend, 4, np.uint64, SENT_U64)
    nwork = weights.work_words(N)
    assert nwork == 4 * ((N + TILE - 1) // TILE)
    work_host = np.zeros(nwork + 2) if poison is None else np.full(nwork + 2, poison)
    work_host[-2:] = SENT_F64
    work = torch.from_numpy(work_host).to(_dev(backend))
    rc = _lib().ttm_weight_scan(ctypes.c_void_p(lw.data_ptr() + 8 * (1 + offset)), N, ctypes.c_void_p(pc), ctypes.c_void_p(pq) if want_q else None,
                                ctypes.c_void_p(ps), ctypes.c_void_p(work.data_ptr()), None)
    _sync(backend)
    assert np.all(work.cpu().numpy()[-2:] == SENT_F64), 'ttm_weight_scan wrote behind its workspace'
    assert np.array_equal(lw.cpu().numpy().view(np.uint64), lw_host.view(np.uint64)), 'ttm_weight_scan wrote to logw'
    s = rs()
    summary = {'m': float(s.view(np.float64)[0]), 'T': int(s[1]), 'S2': float(s.view(np.float64)[2]), 'bad': int(s[3])}
    q = rq()
    if not want_q:
        assert np.all(q == SENT_U64)
    return rc, q, rc_(), summary


_SCANS = {}


def scanned(backend, kind, N):
    """(logw, q, cum, summary) of an input, computed once per backend and shared by the tests (never modified)."""
    key = (backend, kind, N)
    if key not in _SCANS:
        logw = log_weights(kind, N)
        rc, q, cum, s = scan(backend, logw)
        assert rc == 0
        for a in (logw, q, cum):
            a.setflags(write=False)
        _SCANS[key] = (logw, q, cum, s)
    return _SCANS[key]


def exact_q(logw, m, K):
    """floor(exp(logw - m) 2^K) clamped to 2^K with mpmath's exponential (80 bits) - called where NumPy's product is within 2^-11 of
    an integer from either side and on the first 512 rows; elsewhere NumPy's exponential (1 ulp: the product within 2^-12) fixes the
    same floor, and exp(0) 2^K = 2^K needs none."""
    import mpmath
    ok = np.isfinite(logw)
    y = np.where(ok, logw - m, -np.inf)
    with np.errstate(under='ignore'):
        x = np.exp(y) * 2.0 ** K
    ref = np.minimum(np.floor(x), 2.0 ** K).astype(np.uint64)
    err = 2.0 ** -11                                          # (twice the 2^-12 that 1 ulp of a product <= 2^40 is)
    open_ = ok & (y != 0.0) & ((np.floor(np.maximum(x - err, 0.0)) != np.floor(x + err)) | (np.arange(len(logw)) < 512))
    with mpmath.workprec(80):
        for i in np.nonzero(open_)[0]:
            ref[i] = min(int(mpmath.floor(mpmath.exp(mpmath.mpf(float(y[i]))) * 2 ** K)), 2 ** K)
    ref[~ok] = 0
    return ref, int(open_.sum())


def sum_of_squares(q):
    """sum q^2 as a Python integer, exactly (q <= 2^40 split into 20-bit halves: every partial sum stays below 2^64)."""
    q = np.asarray(q, dtype=np.uint64)
    h, l = q >> np.uint64(20), q & np.uint64(0xFFFFF)
    hh, hl, ll = (int(np.sum(a * b, dtype=np.uint64)) for a, b in ((h, h), (h, l), (l, l)))
    return (hh << 40) + (hl << 21) + ll


@pytest.mark.parametrize('N', N_ALL)
def test_weights_scan_and_sums(backend, N):
    """Tests 2, 3 and 4 of the issue at one N, all five inputs: q within 1 of the exact floor, special rows and m and bad exact,
    cum == cumsum(q) exactly, S2 within (depth + 2) 2^-52 of the exact rational."""
    from triangular_transport_toolbox_amd import weights
    K = weight_bits(N)
    assert K == weights.weight_bits(N)
    depth = 18 + ((N + TILE - 1) // TILE + PASS - 1) // PASS
    assert depth == weights.s2_depth(N)
    tol = (depth + 2) * 2.0 ** -52
    for kind in KINDS:
        logw, q, cum, s = scanned(backend, kind, N)
        valid = ~np.isnan(logw) & (logw != np.inf)
        m = np.max(logw[valid])
        ref, n_mp = exact_q(logw, m, K)
        dq = int(np.max(np.abs(q.astype(np.int64) - ref.astype(np.int64))))
        zeros = int(np.sum(q == 0))
        exact = fractions.Fraction(sum_of_squares(q), 4 ** K)
        rel = float(abs(fractions.Fraction(s['S2']) - exact) / exact)
        print('%s N %d %s: K %d, max |q - floor| %d (mpmath on %d rows), %d zero weights, m %.17g, T %d, S2 rel. error %.3e (bound %.3e, depth %d)'
              % (backend, N, kind, K, dq, n_mp, zeros, s['m'], s['T'], rel, tol, depth))
        assert dq <= 1
        assert s['m'] == m and s['bad'] == 0
        assert np.all(q[logw == m] == 2 ** K) and np.all(q[logw == -np.inf] == 0) and np.all(q <= 2 ** K)
        assert np.array_equal(cum, np.cumsum(q, dtype=np.uint64))
        assert s['T'] == int(cum[-1]) and s['T'] >= 2 ** K
        assert rel <= tol
        if kind == 'spread' and N >= 63:
            assert zeros > 0                                      # the input does underflow
        if kind == 'equal':
            assert s['T'] == N * 2 ** K and s['S2'] == float(N)


def test_bad_entries_are_counted_and_get_no_weight(backend):
    N = 3001
    logw = log_weights('gauss', N)
    nan_rows, inf_rows, ninf_rows = [0, 5, 1024, 3000], [1, 1023, 2047], [2, 77]
    logw[nan_rows], logw[inf_rows], logw[ninf_rows] = np.nan, np.inf, -np.inf
    rc, q, cum, s = scan(backend, logw)
    valid = ~np.isnan(logw) & (logw != np.inf)
    print('%s: bad %d, m %.17g' % (backend, s['bad'], s['m']))
    assert rc == 0 and s['bad'] == 7 and s['m'] == np.max(logw[valid])
    assert np.all(q[nan_rows] == 0) and np.all(q[inf_rows] == 0) and np.all(q[ninf_rows] == 0)
    assert np.all(q[logw == s['m']] == 2 ** 40) and np.array_equal(cum, np.cumsum(q, dtype=np.uint64))


def test_scan_alignment_optional_q_workspace_and_repeat(backend):
    """Buffers 8 bytes past a 16-byte boundary, q left out, a poisoned workspace and a second call: the same bits."""
    for N in (1, 2, 65, TILE + 1, 5000):
        logw = log_weights('gauss', N, seed=3)
        rc, q, cum, s = scan(backend, logw)
        assert rc == 0
        for kw in (dict(offset=1), dict(want_q=False), dict(poison=np.nan), dict(poison=-1.0), dict(offset=1, poison=1e300), {}):
            rc2, q2, cum2, s2 = scan(backend, logw, **kw)
            assert rc2 == 0 and np.array_equal(cum2, cum) and s2['T'] == s['T'] and s2['bad'] == s['bad'] and s2['m'] == s['m'], (N, kw)
            assert np.float64(s2['S2']).view(np.uint64) == np.float64(s['S2']).view(np.uint64), (N, kw)
            if kw.get('want_q', True):
                assert np.array_equal(q2, q), (N, kw)


def test_scan_phase_c_option_gives_the_same_bits(backend):
    """Option wscan_reread (phase C rereads the parked q instead of forming exp again): the same cum, q and summary."""
    from triangular_transport_toolbox_amd import _capi
    for N in (65, TILE + 1, 5000):
        logw = log_weights('spread', N, seed=4)
        rc, q, cum, s = scan(backend, logw)
        _capi.set_option('wscan_reread', 1)
        try:
            rc2, q2, cum2, s2 = scan(backend, logw)
            rc3, _, cum3, s3 = scan(backend, logw, want_q=False)
        finally:
            _capi.reset_options()
        assert rc == rc2 == rc3 == 0 and np.array_equal(q, q2) and np.array_equal(cum, cum2) and np.array_equal(cum, cum3) and s == s2 == s3


def resample(backend, cum, M, scheme, seed=0, draw=0, X=None, ldx=None, ldy=None, offset=0, want_idx=True, N=None):
    """ttm_resample on sentinel-padded buffers; X: (ncols, N) host matrix or None (ncols = 0).  Returns (rc, idx, Y (ncols, M))."""
    import torch
    N = len(cum) if N is None else N
    cum_t = torch.from_numpy(np.ascontiguousarray(cum).view(np.int64).copy()).to(_dev(backend))
    ncols = 0 if X is None else X.shape[0]
    ldx = N if ldx is None else ldx
    ldy = M if ldy is None else ldy
    ti, pi, ri = padded(backend, M, np.int32, SENT_I32)
    px = py = None
    if ncols:
        xh = np.full(ncols * ldx, SENT_F64)
        xh.reshape(ncols, ldx)[:, :N] = X
        tx, px, rx = padded(backend, ncols * ldx, np.float64, SENT_F64, offset)
        tx.view(torch.float64)[2 + offset:2 + offset + ncols * ldx] = torch.from_numpy(xh).to(_dev(backend))
        ty, py, ry = padded(backend, ncols * ldy, np.float64, SENT_F64, offset)
    rc = _lib().ttm_resample(ctypes.c_void_p(cum_t.data_ptr()), N, M, scheme, seed, draw, ctypes.c_void_p(px) if px else None, ldx, ncols,
                             ctypes.c_void_p(py) if py else None, ldy, ctypes.c_void_p(pi) if want_idx else None, None)
    _sync(backend)
    idx = ri()
    Y = None
    if ncols:
        Yfull = ry().reshape(ncols, ldy)
        assert np.all(Yfull[:, M:] == SENT_F64) or rc != 0, 'rows behind M were written'
        assert np.array_equal(rx().view(np.uint64), xh.view(np.uint64)), 'the source was written'
        Y = Yfull[:, :M].copy()
    return rc, idx, Y


@pytest.mark.parametrize('N', N_ALL)
def test_ancestors_equal_the_restatement(backend, N):
    """Test 5 of the issue at one N: the three schemes at M in {1, 2, N, 3 N + 1, 65 537}, every offspring, against the restatement
    applied to the backend's own cum; all five inputs (up to N = 1025 at every M, above it at M = N and one further M each, so
    that a case stays within seconds).  Rows without weight never appear; the systematic offspring counts are within 1 of
    M q_i / T in exact integer arithmetic."""
    checked = 0
    for a, kind in enumerate(KINDS):
        logw, q, cum, s = scanned(backend, kind, N)
        Ms = m_list(N)
        if N > TILE + 1:
            Ms = sorted({N, m_list(N)[a % len(m_list(N))]})
        for M in Ms:
            for name, scheme in SCHEMES.items():
                seed, draw = (5, 3) if (M + scheme) % 2 else (2 ** 40 + 7, 0)
                rc, idx, _ = resample(backend, cum, M, scheme, seed=seed, draw=draw)
                assert rc == 0
                want = restated_ancestors(cum, M, scheme, seed, draw)
                bad = int(np.sum(idx.astype(np.int64) != want))
                checked += M
                if bad:
                    j = int(np.nonzero(idx.astype(np.int64) != want)[0][0])
                    print('%s N %d M %d %s %s: %d ancestors differ, first j = %d: %d, restatement %d' % (backend, N, M, kind, name, bad, j, idx[j], want[j]))
                assert bad == 0, (N, M, kind, name)
                assert np.all(idx >= 0) and np.all(idx < N) and np.all(q[idx] > 0)
                if scheme < 2:
                    assert np.all(np.diff(idx) >= 0)
                if scheme == 0:
                    counts = np.bincount(idx, minlength=N).astype(object)
                    dev = np.abs(counts * s['T'] - M * q.astype(object))       # |c_i - M q_i / T| T, Python integers
                    assert np.all(dev <= s['T']), (N, M, kind)
                if kind == 'dominant':
                    assert np.all(idx == (7 * N) // 11)
                if kind == 'equal' and M == N and scheme == 0:
                    assert np.array_equal(idx, np.arange(N))
    print('%s N %d: %d ancestors equal the restatement' % (backend, N, checked))


def test_known_answers_need_no_restatement(backend):
    """Equal weights, M = N, systematic: idx_j = j whatever V is (every seed and draw).  One dominant row: that row M times."""
    for N in (1, 2, 65, TILE + 1, 4099):
        cum = np.cumsum(np.full(N, 2 ** weight_bits(N), dtype=np.uint64), dtype=np.uint64)
        for seed, draw in ((0, 0), (1, 0), (0, 1), (2 ** 63 + 11, 2 ** 31 - 1)):
            rc, idx, _ = resample(backend, cum, N, 0, seed=seed, draw=draw)
            assert rc == 0 and np.array_equal(idx, np.arange(N)), (N, seed, draw)
        q = np.zeros(N, dtype=np.uint64)
        q[N // 3] = 2 ** weight_bits(N)
        for scheme in range(3):
            for M in (1, 5, 2 * N + 1):
                rc, idx, _ = resample(backend, np.cumsum(q, dtype=np.uint64), M, scheme, seed=9, draw=2)
                assert rc == 0 and np.all(idx == N // 3), (N, scheme, M)


@pytest.mark.parametrize('ncols', [1, 3, 40])
def test_gather_is_bitwise_and_touches_nothing_else(backend, ncols):
    """Test 6 of the issue: Y[c, j] is bitwise X[c, idx_j]; odd leading dimensions, buffers 8 bytes past a 16-byte boundary, idx
    left out, sentinels around Y and idx (`padded`, `resample`); two calls agree."""
    rng = np.random.default_rng(ncols)
    for N, M in ((65, 131), (TILE + 1, TILE + 1), (5001, 777), (20011, 3 * 20011 + 1) if ncols == 3 else (333, 1)):
        logw, q, cum, s = scanned(backend, 'neginf', N) if N in N_ALL else (None,) + scan(backend, log_weights('neginf', N))[1:]
        X = rng.standard_normal((ncols, N))
        X.view(np.uint64)[0, ::7] = rng.integers(0, 2 ** 64, len(X[0, ::7]), dtype=np.uint64)       # any bit pattern, NaN payloads included
        for scheme in range(3):
            rc0, idx0, Y0 = resample(backend, cum, M, scheme, seed=3, draw=1, X=X)
            assert rc0 == 0 and np.array_equal(idx0.astype(np.int64), restated_ancestors(cum, M, scheme, 3, 1))
            assert np.array_equal(Y0.view(np.uint64), X[:, idx0].view(np.uint64)), (N, M, scheme)
            for kw in (dict(ldx=N + 3, ldy=M + 5), dict(offset=1), dict(ldx=N + 1, ldy=M + 1, offset=1), dict(want_idx=False), {}):
                rc, idx, Y = resample(backend, cum, M, scheme, seed=3, draw=1, X=X, **kw)
                assert rc == 0 and np.array_equal(Y.view(np.uint64), Y0.view(np.uint64)), (N, M, scheme, kw)
                if kw.get('want_idx', True):
                    assert np.array_equal(idx, idx0)
                else:
                    assert np.all(idx == SENT_I32)


def test_no_valid_weight(backend):
    """Test 7: all -inf or all NaN gives return code 0, T = 0, idx = -1 and NaN entries; the Python layer raises ValueError."""
    tm, _ = make('c3_sep')
    for N in (1, 65, TILE + 1, 3000):
        for fill, bad in ((-np.inf, 0), (np.nan, N), (np.inf, N)):
            logw = np.full(N, fill)
            rc, q, cum, s = scan(backend, logw)
            print('%s N %d all %s: rc %d, T %d, bad %d, m %s' % (backend, N, fill, rc, s['T'], s['bad'], s['m']))
            assert rc == 0 and s['T'] == 0 and s['bad'] == bad and s['S2'] == 0.0 and np.all(q == 0) and np.all(cum == 0)
            assert s['m'] == -np.inf
            for scheme in range(3):
                for M in (1, N, 2 * N + 3):
                    X = np.arange(2.0 * N).reshape(2, N)
                    rc, idx, Y = resample(backend, cum, M, scheme, X=X)
                    assert rc == 0 and np.all(idx == -1) and np.all(np.isnan(Y))
            with pytest.raises(ValueError, match='NaN or' if bad else 'total weight'):
                tm.importance_summary(logw)
            with pytest.raises(ValueError):
                tm.resample(np.zeros((N, 2)), logw)


def test_argument_errors(backend):
    """Every TTM_E_ARG case of include/ttm.h returns -1 and nothing is written."""
    import torch
    lib = _lib()
    dev = _dev(backend)
    N, M = 10, 12
    lw = torch.zeros(N, dtype=torch.float64, device=dev)
    cum = torch.full((N,), 7, dtype=torch.int64, device=dev)
    summ = torch.full((4,), 7, dtype=torch.int64, device=dev)
    work = torch.zeros(8, dtype=torch.float64, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    assert lib.ttm_weight_scan(p(lw), N, p(cum), None, p(summ), p(work), None) == 0
    _sync(backend)
    assert cum.cpu().numpy()[-1] == N * 2 ** 40
    cum0 = cum.clone()
    for args in ((None, N, p(cum), None, p(summ), p(work)), (p(lw), N, None, None, p(summ), p(work)), (p(lw), N, p(cum), None, None, p(work)),
                 (p(lw), N, p(cum), None, p(summ), None), (p(lw), 0, p(cum), None, p(summ), p(work)), (p(lw), -1, p(cum), None, p(summ), p(work)),
                 (p(lw), 2 ** 30 + 1, p(cum), None, p(summ), p(work))):
        assert lib.ttm_weight_scan(*args, None) == E_ARG, args
    X = torch.arange(3.0 * N, dtype=torch.float64, device=dev)
    Y = torch.full((3 * M + N,), SENT_F64, dtype=torch.float64, device=dev)
    idx = torch.full((M,), -777, dtype=torch.int32, device=dev)
    good = dict(cum=p(cum), N=N, M=M, scheme=0, seed=0, draw=0, X=p(X), ldx=N, ncols=3, Y=p(Y), ldy=M, idx=p(idx))
    order = ['cum', 'N', 'M', 'scheme', 'seed', 'draw', 'X', 'ldx', 'ncols', 'Y', 'ldy', 'idx']
    bad = [dict(cum=None), dict(N=0), dict(N=2 ** 30 + 1), dict(M=0), dict(M=-3), dict(M=2 ** 30 + 1), dict(scheme=3), dict(scheme=-1), dict(draw=2 ** 31),
           dict(draw=2 ** 32 - 1), dict(X=None), dict(Y=None), dict(ldx=N - 1), dict(ldy=M - 1), dict(ncols=-1), dict(ncols=0, idx=None),
           dict(Y=p(X)), dict(Y=p(X, 8 * (3 * N - 1))), dict(X=p(Y, 8 * (3 * M - 1)), ldx=N), dict(X=p(Y, 8 * 5))]
    for change in bad:
        kw = dict(good, **change)
        rc = lib.ttm_resample(*[kw[k] for k in order], None)
        print('%s %s: %d' % (backend, {k: (v if not isinstance(v, ctypes.c_void_p) else 'ptr') for k, v in change.items()}, rc))
        assert rc == E_ARG, change
    _sync(backend)
    assert np.all(Y.cpu().numpy() == SENT_F64) and np.all(idx.cpu().numpy() == -777) and torch.equal(cum, cum0)
    assert lib.ttm_resample(*[good[k] for k in order], None) == 0                              # the good call, last
    assert lib.ttm_resample(*[dict(good, ncols=0, X=None, Y=None)[k] for k in order], None) == 0   # ancestors alone
    _sync(backend)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), restated_ancestors(cum.cpu().numpy().view(np.uint64), M, 0, 0, 0))
    assert np.all(Y.cpu().numpy()[3 * M:] == SENT_F64)


# ------------------------------------------------------------------------------------------ the class

def make(name):
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    tm = transport_map(X=case_X(name, npz), monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **ctor_kwargs(desc))
    tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
    return tm, npz


def log_target(X):
    """An unnormalised log-density on the raw draws with NumPy operations that torch repeats bit for bit (products and sums)."""
    return -0.5 * ((X * X).sum(axis=1)) * 0.81 + 0.3 * X[:, 0]


def log_target_device(Xt):
    return -0.5 * ((Xt * Xt).sum(dim=0)) * 0.81 + 0.3 * Xt[0]


PY_N = 4096


@pytest.mark.parametrize('name,kw', [('c3_sep', {}), ('c3_sep', dict(sequence='sobol')), ('c2a_int', {}), ('c3_sep', dict(scheme='multinomial', M=1000)),
                                     ('c3_sep', dict(scheme='stratified', M=3 * PY_N + 1))],
                         ids=['c3_sep', 'c3_sep_sobol', 'c2a_int', 'c3_sep_multinomial', 'c3_sep_stratified'])
def test_sample_importance_on_a_fitted_map(backend, name, kw):
    """Test 8: the resampled rows are rows idx of sample(N, draw=d), logw is log p(X) - logq of sample(..., logdensity=True) bit for
    bit, ess is that of importance_summary(logw), idx is the restatement's on the weights' own cum."""
    tm, _ = make(name)
    N, seed, draw = PY_N, 11, 6
    skw = {k: v for k, v in kw.items() if k == 'sequence'}
    X, logq = tm.sample(N, seed=seed, draw=draw, logdensity=True, **skw)
    assert np.array_equal(X, tm.sample(N, seed=seed, draw=draw, **skw))
    Xr, info = tm.sample_importance(N, log_target, seed=seed, draw=draw, **kw)
    M = kw.get('M', N)
    logw = log_target(X) - logq
    summ = tm.importance_summary(logw)
    print('%s %s %s: ess %.6f of %d, log mean weight %.12f, max %.6f, %d distinct ancestors of %d'
          % (backend, name, kw, info['ess'], N, info['log_mean_weight'], info['max'], len(np.unique(info['idx'])), M))
    assert tm._draws == 0
    assert np.array_equal(info['logw'].view(np.uint64), logw.view(np.uint64))
    assert info['ess'] == summ['ess'] and info['log_mean_weight'] == summ['log_mean_weight'] and 1.0 <= info['ess'] <= N
    assert Xr.shape == (M, tm.D) and info['idx'].shape == (M,)
    assert np.array_equal(Xr.view(np.uint64), X[info['idx']].view(np.uint64))
    w = tm.weights_device(tm._to_dev(logw), N, q=True)
    cum = w.cum.cpu().numpy().view(np.uint64)
    assert np.array_equal(cum, np.cumsum(w.q.cpu().numpy().view(np.uint64), dtype=np.uint64))
    assert np.array_equal(info['idx'].astype(np.int64), restated_ancestors(cum, M, SCHEMES[kw.get('scheme', 'systematic')], seed, draw))
    # the float formulas of the summary from the exact integers: ess and the log of the mean weight to 1e-12
    q = w.q.cpu().numpy().view(np.uint64)
    ess = float(fractions.Fraction(int(cum[-1]) ** 2, sum_of_squares(q)))
    lmw = np.max(logw) + math.log(int(cum[-1])) - 40 * math.log(2.0) - math.log(N)
    assert abs(info['ess'] - ess) <= 1e-12 * ess and abs(info['log_mean_weight'] - lmw) <= 1e-12 * max(1.0, abs(lmw))
    # the target on the device: the same operations, so the same weights and the same ancestors; only M rows return
    Xd, infod = tm.sample_importance(N, log_target_device, seed=seed, draw=draw, target_on_device=True, **kw)
    same = np.array_equal(infod['logw'].view(np.uint64), logw.view(np.uint64))
    print('%s %s: device target gives the same log-weights: %s; ess %.12f / %.12f' % (backend, name, same, infod['ess'], info['ess']))
    assert abs(infod['ess'] - info['ess']) <= 1e-12 * info['ess']
    if same:
        assert np.array_equal(infod['idx'], info['idx']) and np.array_equal(Xd.view(np.uint64), Xr.view(np.uint64))
    else:
        assert np.array_equal(Xd.view(np.uint64), X[infod['idx']].view(np.uint64))


def test_the_maps_own_density_as_target_gives_equal_weights(backend):
    tm, _ = make('c3_sep')
    N = PY_N
    X, logq = tm.sample(N, seed=2, draw=1, logdensity=True)
    Xr, info = tm.sample_importance(N, lambda x: logq, seed=2, draw=1)
    print('%s: ess %r, log mean weight %r' % (backend, info['ess'], info['log_mean_weight']))
    assert np.all(info['logw'] == 0.0) and info['ess'] == float(N)
    assert abs(info['log_mean_weight']) <= 1e-13             # (log(N 2^40) - 40 log 2 - log N: three roundings of numbers below 40)
    assert np.array_equal(info['idx'], np.arange(N)) and np.array_equal(Xr, X)


def test_conditional_sample_importance_and_the_draw_counter(backend):
    tm, npz = make('c3_sep')
    N, E = PY_N, 2
    point = np.asarray(npz['X'][3, :E], dtype=float)
    X, logq = tm.sample(N, X_star=point, seed=8, draw=1, logdensity=True)
    Xr, info = tm.sample_importance(N, log_target, M=500, X_star=point, seed=8, draw=1)
    assert np.array_equal(info['logw'].view(np.uint64), (log_target(X) - logq).view(np.uint64))
    assert Xr.shape == (500, tm.D) and np.array_equal(Xr, X[info['idx']])
    Xd, infod = tm.sample_importance(N, log_target_device, M=500, X_star=point, seed=8, draw=1, target_on_device=True)
    assert abs(infod['ess'] - info['ess']) <= 1e-12 * info['ess'] and np.array_equal(Xd, X[infod['idx']])
    # draw None: the map's counter, one draw number per call, shared by the draws and the thresholds
    a, ia = tm.sample_importance(256, log_target, seed=4)
    b, ib = tm.sample_importance(256, log_target, seed=4)
    assert tm._draws == 2 and not np.array_equal(ia['logw'], ib['logw'])
    a0, ia0 = tm.sample_importance(256, log_target, seed=4, draw=0)
    assert np.array_equal(a, a0) and np.array_equal(ia['idx'], ia0['idx']) and tm._draws == 2


def test_resample_and_resample_device(backend):
    import torch
    tm, _ = make('c3_sep')
    rng = np.random.default_rng(12)
    N, d = 5003, 5
    X, logw = rng.standard_normal((N, d)), 2.0 * rng.standard_normal(N)
    for scheme in SCHEMES:
        for M in (None, 17, 2 * N + 1):
            Y, idx = tm.resample(X, logw, M=M, scheme=scheme, seed=3, draw=4)
            w = tm.weights_device(tm._to_dev(logw), N)
            want = restated_ancestors(w.cum.cpu().numpy().view(np.uint64), M or N, SCHEMES[scheme], 3, 4)
            assert Y.shape == (M or N, d) and np.array_equal(idx.astype(np.int64), want) and np.array_equal(Y.view(np.uint64), X[idx].view(np.uint64))
    # the device form: a Weights object or a tensor of log-weights, the same ancestors; the counter when draw is None
    Xc = tm._import(X, False)
    lw = tm._to_dev(logw)
    Y1, i1 = tm.resample_device(Xc, N, lw, seed=3, draw=4, idx=True)
    Y2, i2 = tm.resample_device(Xc, N, tm.weights_device(lw, N), seed=3, draw=4, idx=True)
    assert torch.equal(i1, i2) and torch.equal(Y1[:, :N], Y2[:, :N]) and tuple(Y1.shape) == (d, N + (N & 1))
    assert np.array_equal(Y1[:, :N].cpu().numpy().T, X[i1.cpu().numpy()])
    before = tm._draws
    tm.resample_device(Xc, N, lw)
    assert tm._draws == before + 1
    s = tm.importance_summary(lw)
    w = np.exp(logw - logw.max())
    print('%s: ess %.9f (float64 formula %.9f), log mean weight %.12f (%.12f)' % (backend, s['ess'], w.sum() ** 2 / (w * w).sum(), s['log_mean_weight'],
                                                                                    logw.max() + np.log(w.mean())))
    # against the plain float formulas: the truncation takes less than one unit of 2^-40 from every weight, i.e. at most N / T of the
    # sum and 2 N / T of the sum of squares (T in units): 4 N / T relative for ess, N / T absolute for the log; 1e-12 for the roundings
    T = tm.weights_device(lw, N).summary()['T']
    print('%s: N / T = %.3e' % (backend, N / T))
    assert abs(s['ess'] - w.sum() ** 2 / (w * w).sum()) <= (4.0 * N / T + 1e-12) * s['ess']
    assert abs(s['log_mean_weight'] - (logw.max() + np.log(w.mean()))) <= 2.0 * N / T + 1e-12
    assert s['max'] == logw.max() and s['n_bad'] == 0


def test_python_argument_errors(backend):
    tm, _ = make('c3_sep')
    X, logw = np.zeros((10, 2)), np.zeros(10)
    for call in (lambda: tm.resample(X, logw, scheme='residual'), lambda: tm.resample(X, logw, M=0), lambda: tm.resample(X, logw[:9]),
                 lambda: tm.resample(X[0], logw), lambda: tm.resample(X, logw, draw=2 ** 31), lambda: tm.sample_importance(0, log_target),
                 lambda: tm.sample_importance(16, log_target, M=0), lambda: tm.sample_importance(16, log_target, scheme='best'),
                 lambda: tm.sample_importance(16, lambda x: np.zeros(15)), lambda: tm.importance_summary(np.zeros((2, 2))),
                 lambda: tm.importance_summary(np.array([0.0, np.nan])), lambda: tm.sample_importance(16, lambda x: np.full(16, np.inf))):
        with pytest.raises(ValueError):
            call()
