"""
Sequential Monte Carlo with adaptive tempering from a fitted map: ttm_temper_scan / k_temper_sums / k_temper_finish
(include/ttm.h, csrc/ttm_smc.h), ttm_mh_step_tempered (csrc/ttm_mcmc.h), weights.temper_search and
transport_map.temper_device / smc_device / sample_smc, on the host test double and on the GPU.

The temper scan is held to the SAME backend's ttm_weight_scan of the pre-multiplied vector (NumPy product: one correctly rounded
multiply), all four words bit for bit.  The tempered step is held bit for bit to ttm_mh_step at beta = 1 and, at beta < 1, to a
NumPy restatement (Philox on uint64 arrays, the counter layout of the accept uniforms and the accept rule: `accept_uniform` and
`decide`, copied from tests/test_mcmc.py with the exponent added).  A decision is compared with the restatement only where
|log u - beta (lp - lc)| > 64 * 2^-52 * (1 + |beta (lp - lc)|) - the logarithms of the device and of NumPy may differ by a few ulp -
and the cap on rows excluded this way is ZERO: test_restatement_has_no_knife_edge_rows, which needs no library, asserts that the
inputs used here have none.  The driver is held bit for bit to the same run composed by hand from the public pieces.  A GPU
process never loads the host double.  Every figure is printed before it is held.
"""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNIFE = 64.0 * 2.0 ** -52
SENTINEL = -7.25e300
ISENT = -77777
E_ARG = -1
TILE = 1024


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def library(backend):
    from triangular_transport_toolbox_amd import _capi
    return _capi.load(), ('cpu' if backend == 'hostemu' else 'cuda')


# ------------------------------------------------------------------------------------------ ttm_temper_scan

def weight_work_words(N):
    return 4 * ((N + TILE - 1) // TILE)


def temper_work_words(N, C):
    return 4 + (2 + 2 * C) * ((N + TILE - 1) // TILE)


def weight_scan_words(backend, v):
    """The four summary words of this backend's ttm_weight_scan of the vector v, as uint64."""
    import torch
    lib, dev = library(backend)
    N = v.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    cum = torch.empty(N, dtype=torch.int64, device=dev)
    words = torch.full((4,), SENTINEL, dtype=torch.float64, device=dev)
    work = torch.empty(weight_work_words(N), dtype=torch.float64, device=dev)
    rc = lib.ttm_weight_scan(ctypes.c_void_p(x.data_ptr()), N, ctypes.c_void_p(cum.data_ptr()), None, ctypes.c_void_p(words.data_ptr()),
                             ctypes.c_void_p(work.data_ptr()), None)
    assert rc == 0
    return words.cpu().numpy().view(np.uint64).copy()


def temper_scan(backend, logw, deltas, offset=0, work_byte=0xFF, null=(), N=None, C=None):
    """ttm_temper_scan on logw placed `offset` doubles behind a 16-byte boundary, a workspace filled with `work_byte` bytes and
    summaries with two sentinel entries behind them.  Returns (rc, (C, 4) uint64 words, the sentinel tail is intact)."""
    import torch
    lib, dev = library(backend)
    n = logw.shape[0]
    d = np.ascontiguousarray(deltas, dtype=np.float64)
    c = d.shape[0]
    N = n if N is None else N
    C = c if C is None else C
    x = torch.from_numpy(np.concatenate((np.full(offset, np.nan), logw))).to(dev)
    assert x.data_ptr() % 16 == 0
    out = torch.full((4 * (c + 2),), SENTINEL, dtype=torch.float64, device=dev)
    work = torch.from_numpy(np.full(8 * temper_work_words(n, c), work_byte, dtype=np.uint8)).to(dev)
    args = dict(logw=ctypes.c_void_p(x.data_ptr() + 8 * offset), delta=ctypes.c_void_p(d.ctypes.data), summaries=ctypes.c_void_p(out.data_ptr()),
                work=ctypes.c_void_p(work.data_ptr()))
    for name in null:
        args[name] = None
    rc = lib.ttm_temper_scan(args['logw'], N, args['delta'], C, args['summaries'], args['work'], None)
    if backend == 'hip':
        torch.cuda.synchronize()
    h = out.cpu().numpy()
    return rc, h[:4 * c].view(np.uint64).reshape(c, 4).copy(), bool(np.all(h[4 * c:] == SENTINEL)), bool(np.all(h == SENTINEL))


def temper_deltas():
    """64 candidates: 1.0, 2^-20, the non-dyadic 0.3 (where a contracted FMA shows), values above 1 and a spread over (0, 1)."""
    rng = np.random.default_rng(5)
    d = np.concatenate(([1.0, 2.0 ** -20, 0.3, 1.7, 1.0 / 3.0, 0.7, 1e-3], rng.uniform(1e-3, 1.0, 57)))
    assert d.shape == (64,)
    return d


def temper_logw(N, case):
    """case 0: finite values spread over +-60 and several -inf; case 1: NaN and +inf entries as well."""
    rng = np.random.default_rng(100 * N + case)
    v = rng.uniform(-60.0, 60.0, N)
    if N >= 3:
        v[rng.choice(N, size=min(5, N // 3), replace=False)] = -np.inf
    if case == 1:
        if N == 1:
            v[0] = np.nan                                  # no valid entry at all
        elif N == 2:
            v[0] = np.inf
        else:
            pick = rng.choice(N, size=min(6, 2 * (N // 3)), replace=False)
            v[pick[0::2]] = np.nan
            v[pick[1::2]] = np.inf
    return v


TEMPER_N = (1, 2, 3, 1023, 1024, 1025, 2049, 256 * 1024 + 1)


@pytest.mark.parametrize('N', TEMPER_N)
def test_temper_scan_against_weight_scan(backend, N):
    """All four words of every candidate equal the same backend's ttm_weight_scan of delta[c] * logw, for C in {1, 7, 64}, an
    even and an odd alignment of logw, with and without NaN / +inf entries, whatever the workspace held; nothing behind
    summaries[C] is written.  (On the parent the symbol does not exist.)"""
    deltas = temper_deltas()
    compared = 0
    for case in (0, 1):
        logw = temper_logw(N, case)
        ref = np.stack([weight_scan_words(backend, d * logw) for d in deltas])
        for C in (1, 7, 64):
            for offset in ((0, 1) if C < 64 else (1,)):            # (all 64 candidates once, at the odd alignment: the host double's time)
                rc, got, tail, _ = temper_scan(backend, logw, deltas[:C], offset=offset)
                assert rc == 0 and tail
                diff = np.argwhere(got != ref[:C])
                if diff.size:
                    c, w = diff[0]
                    print('%s N %d case %d C %d offset %d: candidate %d (delta %.17g) word %d: %#x, ttm_weight_scan %#x'
                          % (backend, N, case, C, offset, c, deltas[c], w, got[c, w], ref[c, w]))
                assert diff.size == 0
                compared += got.size
        rc, zero, tail, _ = temper_scan(backend, logw, deltas[:7], offset=1, work_byte=0)      # (NaN bytes above, zeros here)
        assert rc == 0 and tail and np.array_equal(zero, ref[:7])
    ess = [(float(r[1]) / 2.0 ** min(40, 62 - (N - 1).bit_length())) ** 2 / r[2:3].view(np.float64)[0] for r in ref if r[1] > 0]
    print('%s N %d: %d words equal those of ttm_weight_scan; ESS of the last case over the candidates %.4g .. %.4g'
          % (backend, N, compared, min(ess, default=0.0), max(ess, default=0.0)))


def test_temper_scan_argument_errors(backend):
    logw = temper_logw(10, 0)
    good = np.array([0.5, 1.0])
    rc, _, tail, _ = temper_scan(backend, logw, good)
    assert rc == 0 and tail
    nan, inf = float('nan'), float('inf')
    cases = [dict(null=('logw',)), dict(null=('delta',)), dict(null=('summaries',)), dict(null=('work',)), dict(N=0), dict(N=-1), dict(N=2 ** 30 + 1),
             dict(C=0), dict(C=-1), dict(C=65)]
    for kw in cases:
        d = np.full(65, 0.5) if kw.get('C') == 65 else good
        rc, _, _, untouched = temper_scan(backend, logw, d, **kw)
        print('%s %s: %d' % (backend, kw, rc))
        assert rc == E_ARG and untouched, kw
    for bad in (nan, inf, -inf, 0.0, -0.0, -1.0):
        for pos in (0, 1):
            d = good.copy()
            d[pos] = bad
            rc, _, _, untouched = temper_scan(backend, logw, d)
            print('%s delta[%d] = %r: %d' % (backend, pos, bad, rc))
            assert rc == E_ARG and untouched, (bad, pos)


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


def accept_uniform(seed, draw, rows):
    """The accept uniforms of the global rows `rows`: block p = row >> 1 with the third counter word 0xFFFFFFFF - 4; the even
    row from r[0], r[1], the odd one from r[2], r[3]."""
    rows = np.asarray(rows, dtype=np.uint64)
    p = rows >> np.uint64(1)
    seed = np.uint64(seed)
    r = philox4x32_10(p & M32, p >> np.uint64(32), np.uint64(0xFFFFFFFB), np.uint64(0x80000000 | draw), seed & M32, seed >> np.uint64(32))
    ua = ((((r[0] << np.uint64(32)) | r[1]) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    ub = ((((r[2] << np.uint64(32)) | r[3]) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    return np.where((rows & np.uint64(1)) == 0, ua, ub)


def decide(lp, lc, u, beta):
    """(accept, bad, knife, margin): the tempered accept rule log u < beta (lp - lc), the rows whose comparison is too close to
    hold a backend to, and |log u - beta (lp - lc)| of every row that compares (inf elsewhere)."""
    lp, lc = np.asarray(lp, dtype=float), np.asarray(lc, dtype=float)
    with np.errstate(invalid='ignore'):
        bad = np.isnan(lp) | (lp == np.inf)
        diff = beta * (lp - lc)
        compared = ~bad & (lp > -np.inf) & (lc != -np.inf)
        logu = np.log(u)
        accept = ~bad & (lp > -np.inf) & ((lc == -np.inf) | (logu < diff))
        margin = np.where(compared & np.isfinite(diff), np.abs(logu - diff), np.inf)
        knife = margin <= KNIFE * (1.0 + np.where(np.isfinite(diff), np.abs(diff), 0.0))
    return accept, bad, knife, margin


# ------------------------------------------------------------------------------------------ the step on padded buffers

MATS = ('Zcur', 'Xcur', 'Zprop', 'Xprop', 'Znext', 'Xrec')
VECS = ('logw_cur', 'logw_out', 'logw_prop')
CNTS = ('n_acc', 'n_bad')
ORDER = ('Zcur', 'ldzc', 'Xcur', 'ldxc', 'logw_cur', 'logw_out', 'Zprop', 'ldzp', 'Xprop', 'ldxp', 'logw_prop', 'Znext', 'ldzn', 'rho', 'beta', 'Xrec',
         'ldxr', 'n_acc', 'n_bad', 'N', 'ncols', 'col0', 'seed', 'draw_accept', 'draw_propose', 'row0')
LD_OF = {'Zcur': 'ldzc', 'Xcur': 'ldxc', 'Zprop': 'ldzp', 'Xprop': 'ldxp', 'Znext': 'ldzn', 'Xrec': 'ldxr'}


def make_inputs(N, ncols, seed, planted=True, scale=1.0):
    """Host inputs of one step (tests/test_mcmc.py: make_inputs); scale widens the weight differences, so that a small beta still
    rejects a share of the rows."""
    rng = np.random.default_rng(seed)
    inp = {k: rng.standard_normal((ncols, N)) for k in ('Zcur', 'Xcur', 'Zprop', 'Xprop')}
    inp['logw_cur'] = rng.standard_normal(N)
    inp['logw_prop'] = inp['logw_cur'] + scale * rng.normal(-0.8, 1.5, N)
    inp['n_acc'] = rng.integers(0, 9, N).astype(np.int32)
    inp['n_bad'] = rng.integers(0, 9, N).astype(np.int32)
    if planted and N >= 16:
        inp['logw_cur'][3] = -np.inf
        inp['logw_prop'][4] = -np.inf
        inp['logw_prop'][5] = np.nan
        inp['logw_prop'][6] = np.inf
        inp['logw_prop'][7] = inp['logw_cur'][7]
        inp['logw_cur'][8] = inp['logw_prop'][8] = -np.inf
    return inp


def step(backend, inp, N, ncols, beta, accept=True, propose=True, rho=0.0, col0=0, row0=0, seed=0, da=1, dp=2, offset=0, pad=3, null=(), override=None):
    """ttm_mh_step_tempered (beta None: ttm_mh_step) on sentinel-padded buffers, as tests/test_mcmc.py: step.  Returns
    (rc, {name: whole host buffer}, {name: (columns + 1, ld) view})."""
    import torch
    lib, dev = library(backend)
    ld = max(N, 1) + pad
    bufs, ptrs = {}, {}
    for name in MATS + VECS + CNTS:
        cols = ncols if name in MATS else 1
        fp = name not in CNTS
        h = np.full(offset + (cols + 1) * ld + 2, SENTINEL if fp else ISENT, dtype=np.float64 if fp else np.int32)
        if name in inp:
            h[offset:offset + (cols + 1) * ld].reshape(cols + 1, ld)[:cols, :N] = inp[name]
        t = torch.from_numpy(h).to(dev)
        assert t.data_ptr() % 16 == 0
        bufs[name] = t
        ptrs[name] = t.data_ptr() + (8 if fp else 4) * offset
    args = {name: ctypes.c_void_p(ptrs[name]) for name in MATS + VECS + CNTS}
    args.update({v: ld for v in LD_OF.values()})
    args.update(N=N, ncols=ncols, col0=col0, row0=row0, seed=seed, draw_accept=da, draw_propose=dp, rho=rho, beta=beta)
    if not accept:
        args.update(Zprop=None, Xprop=None, logw_prop=None)
    if not propose:
        args.update(Znext=None)
    for name in null:
        args[name] = None
    args.update(override or {})
    if beta is None:
        rc = lib.ttm_mh_step(*[args[k] for k in ORDER if k != 'beta'], None)
    else:
        rc = lib.ttm_mh_step_tempered(*[args[k] for k in ORDER], None)
    if backend == 'hip':
        torch.cuda.synchronize()
    host, view = {}, {}
    for name, t in bufs.items():
        cols = ncols if name in MATS else 1
        host[name] = t.cpu().numpy().copy()
        view[name] = host[name][offset:offset + (cols + 1) * ld].reshape(cols + 1, ld)
    return rc, host, view


STEP_SHAPES = [(N, row0, offset) for N in (1, 2, 65) for row0 in (0, 7) for offset in (0, 1)]
PHASES = [(True, True), (True, False), (False, True)]
BETAS = (0.25, 2.0 ** -10)
STEP_SEEDS = (11, 2 ** 40 + 7)
STEP_SCALE = {0.25: 4.0, 2.0 ** -10: 1000.0}


def test_restatement_has_no_knife_edge_rows():
    """The inputs of the tempered-step test: no row's comparison lies within the knife-edge margin, so no row is excluded."""
    smallest, total, accepted, rows_seen = np.inf, 0, 0, 0
    for N, row0, offset in STEP_SHAPES:
        for beta in BETAS:
            for seed in STEP_SEEDS:
                inp = make_inputs(N, 3, seed, scale=STEP_SCALE[beta])
                rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
                u = accept_uniform(seed, 3, rows)
                assert np.all((u > 0.0) & (u < 1.0))
                acc, _, knife, margin = decide(inp['logw_prop'], inp['logw_cur'], u, beta)
                smallest, total = min(smallest, float(margin.min())), total + int(knife.sum())
                accepted, rows_seen = accepted + int(acc.sum()), rows_seen + N
    print('restatement: %d knife-edge rows, smallest margin |log u - beta (lp - lc)| = %.3e; %d of %d rows accept' % (total, smallest, accepted, rows_seen))
    assert total == 0
    assert 0.2 < accepted / rows_seen < 0.8


def test_tempered_step_at_beta_one_is_the_plain_step(backend):
    """beta = 1.0: every buffer of ttm_mh_step_tempered - outputs, state, counts and the padding around them - holds the bits of
    ttm_mh_step on the same inputs."""
    calls = 0
    for N, row0, offset in STEP_SHAPES:
        for accept, propose in PHASES:
            for seed in STEP_SEEDS:
                inp = make_inputs(N, 3, seed)
                kw = dict(accept=accept, propose=propose, rho=0.5, col0=1, row0=row0, seed=seed, da=3, dp=4, offset=offset)
                rc0, plain, _ = step(backend, inp, N, 3, None, **kw)
                rc1, temp, _ = step(backend, inp, N, 3, 1.0, **kw)
                assert rc0 == 0 and rc1 == 0
                for name in plain:
                    a, b = plain[name], temp[name]
                    assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), (N, row0, name)
                calls += 1
    print('%s: %d calls at beta = 1.0 equal ttm_mh_step bit for bit' % (backend, calls))


def test_tempered_step_against_the_restatement(backend):
    """beta in {0.25, 2^-10}: the decisions are those of log u < beta (lp - lc), accepted rows take the proposal's bits, and
    logw_out carries the UNTEMPERED log-weight of the row that stands."""
    accepted = rows_seen = 0
    for N, row0, offset in STEP_SHAPES:
        for beta in BETAS:
            for seed in STEP_SEEDS:
                inp = make_inputs(N, 3, seed, scale=STEP_SCALE[beta])
                rc, host, view = step(backend, inp, N, 3, beta, rho=0.5, col0=1, row0=row0, seed=seed, da=3, dp=4, offset=offset)
                assert rc == 0
                rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
                lc, lp = inp['logw_cur'], inp['logw_prop']
                acc, bad, knife, _ = decide(lp, lc, accept_uniform(seed, 3, rows), beta)
                assert int(knife.sum()) == 0
                assert np.array_equal(view['n_acc'][0, :N] - inp['n_acc'], acc.astype(np.int32)), ('decisions', N, row0, beta)
                assert np.array_equal(view['n_bad'][0, :N] - inp['n_bad'], bad.astype(np.int32))
                Zpost, Xpost = np.where(acc, inp['Zprop'], inp['Zcur']), np.where(acc, inp['Xprop'], inp['Xcur'])
                assert same_bits(view['Zcur'][:3, :N], Zpost) and same_bits(view['Xcur'][:3, :N], Xpost) and same_bits(view['Xrec'][:3, :N], Xpost)
                assert same_bits(view['logw_out'][0, :N], np.where(acc, lp, lc))                 # untempered bits
                for name in host:                                                                # nothing outside rows [0, N) is written
                    cols = 3 if name in MATS else 1
                    s = ISENT if name in CNTS else SENTINEL
                    assert np.all(host[name][:offset] == s) and np.all(host[name][-2:] == s) and np.all(view[name][:cols, N:] == s) and np.all(view[name][cols] == s)
                if N == 65:
                    accepted, rows_seen = accepted + int(acc.sum()), rows_seen + N
    print('%s: tempered decisions equal the restatement; %d of %d rows accepted' % (backend, accepted, rows_seen))
    assert 0.2 < accepted / rows_seen < 0.8


def test_tempered_step_argument_errors(backend):
    N, ncols = 10, 2
    inp = make_inputs(N, ncols, 1, planted=False)
    nan = float('nan')
    cases = [dict(null=('Zcur',)), dict(null=('Xcur',)), dict(null=('logw_cur',)), dict(accept=False, propose=False),
             dict(null=('Zprop',)), dict(null=('Xprop',)), dict(null=('logw_out',)),
             dict(override={'N': 0}), dict(override={'N': -1}), dict(override={'ncols': 0}), dict(col0=-1), dict(row0=-1),
             dict(override={'ldzc': N - 1}), dict(override={'ldxc': N - 1}), dict(override={'ldzp': N - 1}), dict(override={'ldxp': N - 1}),
             dict(override={'ldzn': N - 1}), dict(override={'ldxr': N - 1}), dict(da=2 ** 31), dict(dp=2 ** 31),
             dict(rho=nan), dict(rho=1.0), dict(rho=-1.0),
             dict(beta=nan), dict(beta=0.0), dict(beta=-0.5), dict(beta=1.0 + 2.0 ** -52), dict(beta=2.0), dict(beta=float('inf'))]
    for beta in (0.5, 1.0, 5e-324):
        rc, _, _ = step(backend, inp, N, ncols, beta, rho=0.5)
        assert rc == 0, beta
    for kw in cases:
        kw = dict(dict(rho=0.5, beta=0.5), **kw)
        beta = kw.pop('beta')
        rc, host, view = step(backend, inp, N, ncols, beta, **kw)
        print('%s beta %r %s: %d' % (backend, beta, kw, rc))
        assert rc == E_ARG, kw
        for name in ('Zcur', 'Xcur', 'n_acc', 'n_bad'):                                   # the state is as it was
            cols = ncols if name in MATS else 1
            assert np.array_equal(view[name][:cols, :N], np.reshape(inp[name], (cols, N))), (kw, name)
        for name in ('logw_out', 'Znext', 'Xrec'):                                        # nothing was launched
            assert np.all(host[name] == SENTINEL), (kw, name)


# ------------------------------------------------------------------------------------------ the search rule (no library)

class Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, deltas):
        self.calls.append(list(deltas))
        return [self.fn(d) for d in deltas]


def test_temper_search():
    from triangular_transport_toolbox_amd.weights import temper_search
    target = 50.0
    # a step function at a known delta: the largest grid point span k / 64^3 not above it, from 64 + 63 + 63 candidates
    for span, edge in ((1.0, 0.3), (0.25, 0.1), (0.5, 0.5 * 77 / 262144), (1.0, 1.0 - 2.0 ** -30)):
        rec = Recorder(lambda d, edge=edge: 100.0 if d <= edge else 10.0)
        got = temper_search(rec, span, target)
        want = span * math.floor(edge / span * 262144) / 262144
        print('step at %.17g of span %g: %.17g (grid %.17g) after %s candidates' % (edge, span, got, want, [len(c) for c in rec.calls]))
        assert got == want and [len(c) for c in rec.calls] == [64, 63, 63]
        assert rec.calls[0][-1] == span and rec.calls[0][0] == span / 64
        assert all(0.0 < d < span for c in rec.calls[1:] for d in c) and all(c == sorted(c) for c in rec.calls)
    # a constant above the target: the whole span, from one call
    for span in (1.0, 0.3, 1.0 - 0.7):
        rec = Recorder(lambda d: 51.0)
        assert temper_search(rec, span, target) == span and len(rec.calls) == 1
    rec = Recorder(lambda d: 50.0)                                    # (ESS == target passes)
    assert temper_search(rec, 1.0, target) == 1.0
    # a constant below: the smallest candidate tried, so that the run still moves
    for span in (1.0, 0.25, 0.3):
        rec = Recorder(lambda d: 1.0)
        got = temper_search(rec, span, target)
        smallest = min(d for c in rec.calls for d in c)
        print('nothing passes, span %g: %.17g' % (span, got))
        assert got == smallest and got > 0.0 and len(rec.calls) == 3
        if span != 0.3:
            assert got == span / 262144
    # the prefix rule: candidate 12 / 64 passes out of order behind the failing 11 / 64 - the result stays in front of the failure
    rec = Recorder(lambda d: 100.0 if (d <= 10.0 / 64 or d == 12.0 / 64) else 10.0)
    assert temper_search(rec, 1.0, target) == 10.0 / 64
    rec = Recorder(lambda d: 100.0 if d == 12.0 / 64 else 10.0)       # nothing leads: the fallback, not the stray pass
    assert temper_search(rec, 1.0, target) == 1.0 / 262144
    # C and rounds
    rec = Recorder(lambda d: 100.0 if d <= 0.3 else 10.0)
    assert temper_search(rec, 1.0, target, C=4, rounds=2) == 0.25 and [len(c) for c in rec.calls] == [4, 3]
    rec = Recorder(lambda d: 100.0 if d <= 0.3 else 10.0)
    assert temper_search(rec, 1.0, target, C=8, rounds=1) == 0.25 and len(rec.calls) == 1
    for kw in (dict(span=0.0), dict(span=-1.0), dict(C=1), dict(C=65), dict(rounds=0)):
        with pytest.raises(ValueError):
            temper_search(rec, **dict(dict(span=1.0, target=target), **kw))
    with pytest.raises(ValueError):
        temper_search(lambda ds: [1.0], 1.0, target)


# ------------------------------------------------------------------------------------------ the class

def make(name, **override):
    """A map of a golden case with the fixture's coefficients (tests/test_sample.py: make)."""
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    X = case_X(name, npz)
    kw = ctor_kwargs(desc)
    kw.update(override)
    tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **kw)
    tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
    return tm, X


def gauss_device(tm, shift, scale, logc=0.0):
    """log c + log N(x; mu, diag(s^2)) on the device, mu = X_mean + shift X_std and s = scale X_std per column (raw coordinates):
    its integral is c exactly."""
    mean, std = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    mu, s = mean + shift * std, scale * std
    mu_d, s_d = tm._to_dev(mu)[:, None], tm._to_dev(s)[:, None]
    norm = logc - float(np.sum(np.log(s))) - 0.5 * tm.D * math.log(2.0 * math.pi)

    def target(raw):
        return norm - 0.5 * (((raw - mu_d) / s_d) ** 2).sum(dim=0)
    return target, mu, s


def gauss_host(mu, s, logc=0.0):
    norm = logc - float(np.sum(np.log(s))) - 0.5 * len(mu) * math.log(2.0 * math.pi)
    return lambda X: norm - 0.5 * np.sum(((X - mu) / s) ** 2, axis=1)


def compose(tm, target, N, ess_target, moves, rho, scheme, seed, draw0):
    """The run of smc_device put together from sample_device's pieces, temper_device, temper_search, weights_device,
    resample_device and ttm_mh_step_tempered with the draw numbers of the docstring.  Also holds, at every stage, the summary of
    the chosen candidate's temper scan to the words of weights_device(delta * logw), bit for bit."""
    import torch
    from triangular_transport_toolbox_amd import weights
    D, d = tm.D, tm._cm.d_cols
    c0 = d - D
    ld = N + (N & 1)
    K = weights.weight_bits(N)
    g_scale = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float)[c0:d]) if tm.standardize_samples else None
    const = 0.5 * D * np.log(2 * np.pi)

    def invert(Zdev):
        Xd, logq = tm.inverse_device(Zdev, N, logq=True, g_scale=g_scale)
        raw = Xd[c0:d, :N]
        if tm.standardize_samples:
            raw = raw * tm._std_d[c0:d, None] + tm._mean_d[c0:d, None]
        return Xd, (target(raw).reshape(N).to(torch.float64) - (logq[:N] - const)).contiguous()
    Z = tm.reference_device(N, seed=seed, draw=draw0)
    Xd, logw0 = invert(Z)
    S = torch.zeros((2 * D + 1, ld), dtype=torch.float64, device=Z.device)
    S[:D, :N], S[D:2 * D, :N], S[2 * D, :N] = Z[:, :N], Xd[c0:d, :N], logw0
    beta, logz, stages = 0.0, 0.0, 0
    betas, ess = [0.0], []
    while beta < 1.0:
        r = draw0 + 1 + stages * (moves + 1)
        logw = S[2 * D, :N].clone()
        span = 1.0 - beta
        delta = weights.temper_search(lambda ds: weights.temper_ess(tm.temper_device(logw, N, ds).cpu().numpy(), N, K), span, ess_target * N)
        beta_next = 1.0 if delta == span else beta + delta
        W = tm.weights_device((delta * logw).contiguous(), N)
        seen = tm.temper_device(logw, N, [delta]).cpu().numpy()
        assert same_bits(seen[0], W.words.cpu().numpy()), (stages, delta)
        summ = W.importance_summary()
        assert bits(weights.temper_ess(seen, N, K)[0]) == bits(summ['ess'])
        logz += summ['log_mean_weight']
        ess.append(summ['ess'])
        S = tm.resample_device(S, N, W, scheme=scheme, seed=seed, draw=r, check=False)
        beta = beta_next
        betas.append(beta)
        stages += 1
        lw, lwp, Zp, Xp = [S[2 * D, :N].clone(), torch.empty(N, dtype=torch.float64, device=Z.device)], None, None, None
        for t in range(moves + 1 if moves else 0):
            accept, propose = t >= 1, t < moves
            zn = torch.zeros((D, ld), dtype=torch.float64, device=Z.device) if propose else None
            p = lambda x, off=0: None if x is None else ctypes.c_void_p(x.data_ptr() + 8 * off)
            rc = tm._lib.ttm_mh_step_tempered(p(S), ld, p(S, D * ld), ld, p(lw[0]), p(lw[1]) if accept else None, p(Zp) if accept else None, ld,
                                              p(Xp, c0 * ld) if accept else None, ld, p(lwp) if accept else None, p(zn), ld, rho, beta, None, ld, None, None,
                                              N, D, 0, seed, r + t if accept else 0, r + t + 1 if propose else 0, 0, tm._stream())
            assert rc == 0
            if accept:
                lw.reverse()
            if propose:
                Zp = zn
                Xp, lwp = invert(zn)
        S[2 * D, :N] = lw[0]
    return S, dict(log_evidence=logz, betas=betas, ess=ess, stages=stages)


@pytest.mark.parametrize('name', ['c2b_sep', 'c2a_int'])
def test_composition(backend, name):
    """smc_device equals the run composed by hand (bitwise: particles, log-weights, betas, ess, log_evidence); two calls with the
    same (seed, draw) are identical; draw None advances the counter by 1 + stages (moves + 1)."""
    tm, _ = make(name)
    N, moves, seed, draw0 = 257, 2, 7, 30
    target, mu, s = gauss_device(tm, 1.0, 0.5)
    state, info = tm.smc_device(target, N, ess_target=0.5, moves=moves, rho=0.5, seed=seed, draw=draw0)
    print('%s %s: %d stages, betas %s, ess %s, accept %s, log Z %.6f' % (backend, name, info['stages'], ' '.join('%.5f' % b for b in info['betas']),
                                                                         ' '.join('%.1f' % e for e in info['ess']),
                                                                         ' '.join('%.3f' % a for a in info['accept_rate']), info['log_evidence']))
    assert tm._draws == 0 and info['stages'] >= 2
    assert info['draws'] == (draw0, draw0 + info['stages'] * (moves + 1)) and len(info['accept_rate']) == info['stages']
    S, ref = compose(tm, target, N, 0.5, moves, 0.5, 'systematic', seed, draw0)
    D = tm.D
    assert ref['stages'] == info['stages'] and same_bits(ref['betas'], info['betas']) and same_bits(ref['ess'], info['ess'])
    assert bits(ref['log_evidence']) == bits(info['log_evidence'])
    assert same_bits(S[:D, :N].cpu().numpy(), state['Z'][:, :N].cpu().numpy()) and same_bits(S[D:2 * D, :N].cpu().numpy(), state['X'][:, :N].cpu().numpy())
    assert same_bits(S[2 * D, :N].cpu().numpy(), state['logw'].cpu().numpy())
    # path properties on the backend's own numbers
    b = info['betas']
    assert b[0] == 0.0 and b[-1] == 1.0 and all(x < y for x, y in zip(b, b[1:])) and len(b) == info['stages'] + 1
    assert all(e >= 0.5 * N for e in info['ess'])
    assert all(0.0 < a < 1.0 for a in info['accept_rate']) and info['n_bad'] == 0
    # the same (seed, draw) again, then the map's own counter
    state2, info2 = tm.smc_device(target, N, ess_target=0.5, moves=moves, rho=0.5, seed=seed, draw=draw0)
    assert same_bits(state2['X'][:, :N].cpu().numpy(), state['X'][:, :N].cpu().numpy()) and same_bits(info2['betas'], info['betas'])
    assert bits(info2['log_evidence']) == bits(info['log_evidence'])
    tm._draws = draw0
    state3, info3 = tm.smc_device(target, N, ess_target=0.5, moves=moves, rho=0.5, seed=seed)
    assert tm._draws == draw0 + 1 + info['stages'] * (moves + 1)
    assert same_bits(state3['X'][:, :N].cpu().numpy(), state['X'][:, :N].cpu().numpy())


def test_sample_smc_host_target_and_first_block(backend):
    """sample_smc with a host target: its first call sees sample(N, seed, draw0) bit for bit, the particles are those of the
    device target's run up to the target's own rounding, the returned rows are the raw own columns of the state."""
    tm, _ = make('c2b_sep')
    N, seed, draw0 = 257, 7, 30
    _, mu, s = gauss_device(tm, 1.0, 0.5)
    calls = []

    def target(X):
        calls.append(X.copy())
        return gauss_host(mu, s)(X)
    X, info = tm.sample_smc(target, N, seed=seed, draw=draw0)
    assert X.shape == (N, tm.D) and info['logw'].shape == (N,) and np.all(np.isfinite(X)) and np.all(np.isfinite(info['logw']))
    assert same_bits(calls[0], tm.sample(N, seed=seed, draw=draw0))
    assert len(calls) == 1 + info['stages'] * 2 and all(c.shape == (N, tm.D) for c in calls)
    print('%s: %d stages, betas %s, log Z %.6f' % (backend, info['stages'], info['betas'], info['log_evidence']))
    assert info['betas'][0] == 0.0 and info['betas'][-1] == 1.0 and tm._draws == 0


def test_python_argument_errors(backend):
    tm, Xtrain = make('c2b_sep')
    _, mu, s = gauss_device(tm, 0.2, 0.9)
    target = gauss_host(mu, s)
    X, info = tm.sample_smc(target, 16, seed=1, draw=0)
    assert X.shape == (16, tm.D)
    bad = [dict(N=0), dict(ess_target=0.0), dict(ess_target=1.0), dict(ess_target=float('nan')), dict(moves=-1), dict(rho=1.0), dict(rho=-1.0),
           dict(rho=float('nan')), dict(scheme='residual'), dict(draw=-1), dict(draw=2 ** 31 - 3), dict(max_stages=0),
           dict(X_star=np.zeros((16, 1)))]
    for change in bad:
        kw = dict(dict(N=16, seed=1, draw=0), **change)
        with pytest.raises(ValueError):
            tm.sample_smc(target, **kw)
    with pytest.raises(ValueError, match='return'):
        tm.sample_smc(lambda X: np.zeros(15), 16, draw=0)
    with pytest.raises(ValueError, match='return'):
        tm.sample_smc(lambda raw: raw[0, :15], 16, draw=0, target_on_device=True)
    for value in (np.nan, np.inf):
        def broken(X, value=value):
            out = target(X)
            out[7] = value
            return out
        with pytest.raises(ValueError, match='initial'):
            tm.sample_smc(broken, 16, draw=0)
    assert tm._draws == 0
    # one conditioning point for all particles
    Xc, infoc = tm.sample_smc(gauss_host(mu[1:], s[1:]), 16, X_star=np.asarray(Xtrain[3, :1], dtype=float), seed=1, draw=0)
    assert Xc.shape == (16, tm.D - 1) and infoc['betas'][-1] == 1.0


def test_degenerate_inputs(backend):
    tm, _ = make('c2b_sep')
    near, mu_n, s_n = gauss_device(tm, 0.0, 0.5)
    far, mu_f, s_f = gauss_device(tm, 1.0, 0.5)
    # a fit with ESS(1) >= target from the start: one stage, and the evidence is importance sampling's, bit for bit
    N = 257
    state, info = tm.smc_device(near, N, ess_target=0.05, seed=3, draw=4)
    assert info['stages'] == 1 and info['betas'] == [0.0, 1.0]
    # (the run's own initial log-weights: the moves at beta = 1 change rows, so they are rebuilt from the same pieces)
    import torch
    g_scale = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float))
    Xd, lq = tm.inverse_device(tm.reference_device(N, seed=3, draw=4), N, logq=True, g_scale=g_scale)
    raw = Xd[:tm.D, :N] * tm._std_d[:tm.D, None] + tm._mean_d[:tm.D, None]
    logw0 = (near(raw).reshape(N).to(torch.float64) - (lq[:N] - 0.5 * tm.D * np.log(2 * np.pi))).contiguous()
    ref = tm.importance_summary(logw0)
    print('%s: one stage: log Z %.17g, importance_summary %.17g, ess %.2f' % (backend, info['log_evidence'], ref['log_mean_weight'], info['ess'][0]))
    assert bits(info['log_evidence']) == bits(ref['log_mean_weight']) and bits(info['ess'][0]) == bits(ref['ess'])
    # N = 1: every reweighting leaves ESS = 1 >= target
    state, info = tm.smc_device(far, 1, seed=3, draw=4)
    assert info['stages'] == 1 and info['betas'] == [0.0, 1.0] and info['ess'] == [1.0] and np.isfinite(info['log_evidence'])
    assert np.all(np.isfinite(state['X'][:, :1].cpu().numpy()))
    # moves = 0: pure tempering and resampling - every final particle is one of the initial draws
    X, info = tm.sample_smc(gauss_host(mu_f, s_f), N, moves=0, seed=3, draw=4)
    init = tm.sample(N, seed=3, draw=4)
    assert info['draws'] == (4, 4 + info['stages']) and info['accept_rate'] == [0.0] * info['stages'] and info['stages'] >= 2
    assert all(np.any(np.all(bits(init) == bits(row), axis=1)) for row in X)
    print('%s: moves = 0: %d stages, %d distinct particles of %d' % (backend, info['stages'], len(np.unique(X, axis=0)), N))
    # all but one weight -inf: every search ends in its fallback candidate; the run ends or raises at max_stages, nothing is NaN
    calls = []

    def lonely(Xh):
        calls.append(1)
        out = np.full(Xh.shape[0], -np.inf)
        if len(calls) == 1:
            out[5] = 0.0
        return out
    for max_stages in (3, 100):
        del calls[:]
        try:
            X, info = tm.sample_smc(lonely, 64, ess_target=0.5, moves=1, max_stages=max_stages, seed=3, draw=4)
            print('%s: one positive weight, max_stages %d: %d stages, last betas %s' % (backend, max_stages, info['stages'], info['betas'][-3:]))
            assert np.all(np.isfinite(X)) and np.isfinite(info['log_evidence']) and info['betas'][-1] == 1.0
            assert np.all(bits(X) == bits(X[0]))                      # the one particle with weight
        except RuntimeError as e:
            print('%s: one positive weight, max_stages %d: %s' % (backend, max_stages, e))
            assert 'beta' in str(e) and 'nan' not in str(e).lower()
    # no positive weight at all
    with pytest.raises(ValueError, match='finite'):
        tm.sample_smc(lambda Xh: np.full(Xh.shape[0], -np.inf), 16, draw=0)
    assert tm._draws == 0


# ------------------------------------------------------------------------------------------ statistics

STAT = dict(shift=np.array([1.0, -1.0]), scale=0.5, K=16, N=4096, logc=math.log(3.0))


def test_evidence_is_unbiased_and_no_wider_than_importance_sampling(backend):
    """c2b_sep, target log p(x) = log 3 + log N(x; mu, diag(s^2)) in raw coordinates with mu = X_mean + (1, -1) X_std - one column
    standard deviation off the ensemble mean in each column - and s = X_std / 2, so the integral of p is 3 exactly.  K = 16
    replicates (draws 0, 1000, ...), N = 4096, ess_target 0.5, two moves at rho = 0.5.  A deterministic generator: the outcome at
    these seeds is a fixed number.  Held: the unbiasedness z-tests |mean_k(Z_k / c) - 1| <= 4 std_k / sqrt(K) and the same on every
    column of the particle mean against mu; the spread of the SMC estimate at most TWICE that of exp(log_mean_weight) of plain
    sample_importance over the same draws at the same N (the factor is the margin for K = 16, where an estimated standard
    deviation is uncertain by about 20 %).  Conditions on the choice of mu, asserted too: every replicate takes at least 3 stages,
    plain importance sampling has ESS / N below ess_target, and the importance-sampling reference passes its own z-test.  The
    sign of the offset is chosen for the power of the test: towards (1, 1) the weights are heavy-tailed - the three conditions hold
    there too, but importance sampling has a spread of 0.60 (SMC 0.37), single replicates decide the means and a z-test against
    such a spread can hardly fail; towards (-1, 0) the reference fails its own z-test (6.9).  Towards (1, -1) the spread is 0.034 and
    a bias of 3 % would show.
    The host double gives: 3 stages in all 16 replicates; importance sampling ESS / N 0.122 .. 0.135, Z / c mean 0.99973,
    sd 0.03384 (z 0.03); SMC Z / c mean 0.99096, sd 0.03130 (z 1.16; 0.92 of the reference's spread); particle means z 1.13 and
    2.88.  The MI355X gives the same figures to the digits shown."""
    tm, _ = make('c2b_sep')
    K, N = STAT['K'], STAT['N']
    target, mu, s = gauss_device(tm, STAT['shift'], STAT['scale'], STAT['logc'])
    host = gauss_host(mu, s, STAT['logc'])
    c = math.exp(STAT['logc'])
    z_smc, z_is, means, stages, ess_is = [], [], [], [], []
    for k in range(K):
        draw0 = 1000 * k
        X, info = tm.sample_smc(target, N, ess_target=0.5, moves=2, rho=0.5, seed=9, draw=draw0, target_on_device=True)
        z_smc.append(math.exp(info['log_evidence']) / c)
        means.append(X.mean(axis=0))
        stages.append(info['stages'])
        _, ref = tm.sample_importance(N, host, seed=9, draw=draw0)
        z_is.append(math.exp(ref['log_mean_weight']) / c)
        ess_is.append(ref['ess'] / N)
    z_smc, z_is, means = np.array(z_smc), np.array(z_is), np.array(means)
    sd_smc, sd_is = float(z_smc.std(ddof=1)), float(z_is.std(ddof=1))
    t_smc = abs(float(z_smc.mean()) - 1.0) / (sd_smc / math.sqrt(K))
    t_is = abs(float(z_is.mean()) - 1.0) / (sd_is / math.sqrt(K))
    t_mean = np.abs(means.mean(axis=0) - mu) / (means.std(axis=0, ddof=1) / math.sqrt(K))
    print('%s: stages %s; importance sampling ESS / N %.3f .. %.3f' % (backend, stages, min(ess_is), max(ess_is)))
    print('%s: Z / c: SMC mean %.5f sd %.5f (z %.2f); importance sampling mean %.5f sd %.5f (z %.2f); particle means z %s'
          % (backend, z_smc.mean(), sd_smc, t_smc, z_is.mean(), sd_is, t_is, ' '.join('%.2f' % v for v in t_mean)))
    assert min(stages) >= 3 and max(ess_is) < 0.5          # the test exercises the tempering
    assert t_is <= 4.0                                     # the parent-code reference satisfies its own z-test
    assert t_smc <= 4.0
    assert np.all(t_mean <= 4.0)
    assert sd_smc <= 2.0 * sd_is


# ------------------------------------------------------------------------------------------ the timing tool

@pytest.mark.gpu
def test_timing_tool_runs(tmp_path):
    """tools/smc_bench.py in a fresh child process on small shapes (as tests/test_mcmc.py runs its tool; the time limit ends a
    hang and gates no speed)."""
    out = tmp_path / 'result.json'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'smc_bench.py'), '--workloads', 'C2b', '--rows', '65536', '--launches', '4',
                          '--rounds', '2', '--smc-workloads', 'C2b', '--particles', '4096', '--calls', '1', '--label', 'small', '--out', str(out)],
                         capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    js = json.loads(res.stdout.splitlines()[-1])
    assert js['label'] == 'small' and js['rounds'] == 2 and json.loads(out.read_text()) == js
    v = js['scan']['versions']
    assert js['scan']['N'] == 65536 and sorted(v) == sorted('%s%d' % (k, C) for k in ('temper_', 'scan_x', 'torch_') for C in (1, 8, 64))
    assert all(len(x['ms_rounds']) == 2 and x['ms'] > 0 for x in v.values())
    assert all(v['temper_%d' % C]['kernel'] == 'k_temper_finish' for C in (1, 8, 64)) and js['scan_ess_rel_diff_vs_torch'] < 1e-4
    w = js['workloads']['C2b']['versions']
    assert all(w[k]['kernel'] == 'k_mh_step' and 0.0 < w[k]['accepted_share'] < 1.0 for k in ('mh_step', 'mh_step_tempered'))
    run = js['smc']['cases']['C2b']
    print('temper scan of 64: %.4f ms, 64 weight scans %.4f ms, torch %.4f ms; SMC %d stages, %.3f ms per stage'
          % (v['temper_64']['ms'], v['scan_x64']['ms'], v['torch_64']['ms'], run['stages'], run['ms_per_stage']))
    assert run['stages'] >= 1 and run['ms_per_stage'] > 0 and 0.0 < run['accept_rate'] < 1.0
