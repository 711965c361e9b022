"""
Metropolis-Hastings in the reference space of a fitted map: ttm_mh_step / k_mh_step (include/ttm.h, csrc/ttm_mcmc.h) and
transport_map.mcmc_device / sample_mcmc, on the host test double and on the GPU.

The expected values come from a NumPy restatement in this file: Philox on uint64 arrays as in tests/test_sample.py, the counter
layout of the accept uniforms (`accept_uniform`), the accept rule (`decide`) and the proposal formula (`proposal`).  A GPU
process never loads the host double.  Every figure is printed before it is held.

Bounds.  Values formed from deviates (Znext): |a - b| <= 256 * 2^-52 * (1 + |b|), the bound tests/test_sample.py derives for a
deviate against its restatement (the proposal adds a product, an FMA against a product and a sum, and |rho|, s <= 1: three more
roundings of values no larger than the deviate's bound assumes).  Comparisons between two calls of one backend are bitwise, and so
are copied values (accepted rows, logw_out, Xrec, the counts).  A decision is compared with the restatement only where
|log u - (lp - lc)| > 64 * 2^-52 * (1 + |lp - lc|): the logarithms of the device and of NumPy may differ by a few ulp.  The cap on
rows excluded this way is ZERO: the seeds below are chosen so that the restatement reports none
(test_restatement_has_no_knife_edge_rows, which needs no library; its smallest margin is 1.7e-4; the composition
test counts its own rows and finds 6.5e-5 as its smallest margin on the host double).

The caps of the stationarity test are conditions on a deterministic generator; its docstring records the figures of the host
double.
"""
import ctypes
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import case_X, coeff_lists, ctor_kwargs, load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 256.0 * 2.0 ** -52
KNIFE = 64.0 * 2.0 ** -52
SENTINEL = -7.25e300
ISENT = -77777
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


def _blocks(seed, draw, third, rows):
    rows = np.asarray(rows, dtype=np.uint64)
    p = rows >> np.uint64(1)
    seed = np.uint64(seed)
    r = philox4x32_10(p & M32, p >> np.uint64(32), np.uint64(third), np.uint64(0x80000000 | draw), seed & M32, seed >> np.uint64(32))
    ua = ((((r[0] << np.uint64(32)) | r[1]) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    ub = ((((r[2] << np.uint64(32)) | r[3]) >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)
    return (rows & np.uint64(1)) == 0, ua, ub


def deviates(seed, draw, col, rows):
    """The reference draws of column `col` at the global rows `rows` (tests/test_sample.py: expected)."""
    even, u1, u2 = _blocks(seed, draw, col, rows)
    R, t = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586477 * u2
    return np.where(even, R * np.cos(t), R * np.sin(t))


def accept_uniform(seed, draw, rows):
    """The accept uniforms of the global rows `rows`: block p = row >> 1 with the third counter word 0xFFFFFFFF - 4; the even
    row from r[0], r[1], the odd one from r[2], r[3]."""
    even, ua, ub = _blocks(seed, draw, 0xFFFFFFFB, rows)
    return np.where(even, ua, ub)


def decide(lp, lc, u):
    """(accept, bad, knife, margin): the accept rule, the rows whose comparison is too close to hold a backend to, and
    |log u - (lp - lc)| of every row that compares (inf elsewhere)."""
    lp, lc = np.asarray(lp, dtype=float), np.asarray(lc, dtype=float)
    with np.errstate(invalid='ignore'):
        bad = np.isnan(lp) | (lp == np.inf)
        diff = lp - lc
        compared = ~bad & (lp > -np.inf) & (lc != -np.inf)
        logu = np.log(u)
        accept = ~bad & (lp > -np.inf) & ((lc == -np.inf) | (logu < diff))
        margin = np.where(compared & np.isfinite(diff), np.abs(logu - diff), np.inf)
        knife = margin <= KNIFE * (1.0 + np.where(np.isfinite(diff), np.abs(diff), 0.0))
    return accept, bad, knife, margin


def proposal(rho, z, xi):
    return rho * z + np.sqrt((1.0 - rho) * (1.0 + rho)) * xi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ the entry point on padded buffers

MATS = ('Zcur', 'Xcur', 'Zprop', 'Xprop', 'Znext', 'Xrec')
VECS = ('logw_cur', 'logw_out', 'logw_prop')
CNTS = ('n_acc', 'n_bad')
ORDER = ('Zcur', 'ldzc', 'Xcur', 'ldxc', 'logw_cur', 'logw_out', 'Zprop', 'ldzp', 'Xprop', 'ldxp', 'logw_prop', 'Znext', 'ldzn', 'rho', 'Xrec', 'ldxr',
         'n_acc', 'n_bad', 'N', 'ncols', 'col0', 'seed', 'draw_accept', 'draw_propose', 'row0')
LD_OF = {'Zcur': 'ldzc', 'Xcur': 'ldxc', 'Zprop': 'ldzp', 'Xprop': 'ldxp', 'Znext': 'ldzn', 'Xrec': 'ldxr'}


def make_inputs(N, ncols, seed, planted=True):
    """Host inputs of one step: states, proposals and log-weights with about half the rows accepting, and (N >= 16) planted
    rows 3 .. 7 with lc = -inf, lp = -inf, lp = NaN, lp = +inf, lp == lc."""
    rng = np.random.default_rng(seed)
    inp = {k: rng.standard_normal((ncols, N)) for k in ('Zcur', 'Xcur', 'Zprop', 'Xprop')}
    inp['logw_cur'] = rng.standard_normal(N)
    inp['logw_prop'] = inp['logw_cur'] + rng.normal(-0.8, 1.5, N)
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


def step(backend, inp, N, ncols, accept=True, propose=True, rho=0.0, col0=0, row0=0, seed=0, da=1, dp=2, offset=0, pad=3, null=(), override=None,
         alias=None):
    """ttm_mh_step on sentinel-padded buffers: every matrix has `offset` doubles of slack in front (offset = 1: it starts 8 bytes
    past a 16-byte boundary), ncols + 1 columns of ld = N + pad doubles and two doubles behind; vectors and counts likewise as one
    column.  inp: the host inputs (make_inputs); buffers without an input hold sentinels.  null: names passed as NULL beyond what
    the phases imply; override: raw argument values; alias: {name: (other name, offset in doubles)} pointer substitutions.
    Returns (rc, {name: whole host buffer}, {name: (columns + 1, ld) view})."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    dev = 'cpu' if backend == 'hostemu' else 'cuda'
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
    args.update(N=N, ncols=ncols, col0=col0, row0=row0, seed=seed, draw_accept=da, draw_propose=dp, rho=rho)
    if not accept:
        args.update(Zprop=None, Xprop=None, logw_prop=None)
    if not propose:
        args.update(Znext=None)
    for name in null:
        args[name] = None
    for name, (other, off) in (alias or {}).items():
        args[name] = ctypes.c_void_p(ptrs[other] + 8 * off)
    args.update(override or {})
    rc = lib.ttm_mh_step(*[args[k] for k in ORDER], None)
    if backend == 'hip':
        torch.cuda.synchronize()
    host, view = {}, {}
    for name, t in bufs.items():
        cols = ncols if name in MATS else 1
        host[name] = t.cpu().numpy().copy()
        view[name] = host[name][offset:offset + (cols + 1) * ld].reshape(cols + 1, ld)
    return rc, host, view


def outside_untouched(host, view, N, ncols, offset):
    """Nothing outside rows [0, N) of the columns in use holds anything but the sentinel."""
    for name in host:
        cols = ncols if name in MATS else 1
        s = ISENT if name in CNTS else SENTINEL
        ok = np.all(host[name][:offset] == s) and np.all(host[name][-2:] == s) and np.all(view[name][:cols, N:] == s) and np.all(view[name][cols] == s)
        assert ok, name


def check_step(backend, N, ncols, accept, propose, rho, row0, offset, seed, col0=1):
    """One call against the restatement; returns (rows accepted, rows, knife-edge rows)."""
    inp = make_inputs(N, ncols, seed)
    da, dp = 3, 4
    rc, host, view = step(backend, inp, N, ncols, accept=accept, propose=propose, rho=rho, col0=col0, row0=row0, seed=seed, da=da, dp=dp, offset=offset)
    assert rc == 0
    rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
    lc, lp = inp['logw_cur'], inp['logw_prop']
    if accept:
        acc, bad, knife, _ = decide(lp, lc, accept_uniform(seed, da, rows))
    else:
        acc, bad, knife = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, bool)
    assert int(knife.sum()) == 0
    Zpost, Xpost = np.where(acc, inp['Zprop'], inp['Zcur']), np.where(acc, inp['Xprop'], inp['Xcur'])
    got_acc = view['n_acc'][0, :N] - inp['n_acc']
    assert np.array_equal(got_acc, acc.astype(np.int32)), 'decisions'
    assert np.array_equal(view['n_bad'][0, :N] - inp['n_bad'], bad.astype(np.int32))
    assert same_bits(view['Zcur'][:ncols, :N], Zpost) and same_bits(view['Xcur'][:ncols, :N], Xpost)
    assert same_bits(view['logw_out'][0, :N], np.where(acc, lp, lc))
    assert same_bits(view['Xrec'][:ncols, :N], Xpost)
    for name in ('Zprop', 'Xprop', 'logw_cur', 'logw_prop'):                # the inputs are inputs
        cols = ncols if name in MATS else 1
        assert same_bits(view[name][:cols, :N], np.reshape(inp[name], (cols, N)))
    if propose:
        xi = np.stack([deviates(seed, dp, col0 + j, rows) for j in range(ncols)])
        ref = xi if rho == 0.0 else proposal(rho, Zpost, xi)
        err = float(np.max(np.abs(view['Znext'][:ncols, :N] - ref) / (1.0 + np.abs(ref))))
        assert err <= TOL, (err, TOL)
    else:
        err = 0.0
        assert np.all(view['Znext'] == SENTINEL)
    outside_untouched(host, view, N, ncols, offset)
    return int(acc.sum()), N, err


STEP_SHAPES = [(N, row0, offset) for N in (1, 2, 3, 4099) for row0 in (0, 7) for offset in (0, 1)]
PHASES = [(True, True), (True, False), (False, True)]


def test_restatement_has_no_knife_edge_rows():
    """The inputs of every entry-point test: no row's comparison lies within the knife-edge margin, so no row is excluded."""
    smallest, total = np.inf, 0
    for N, row0, offset in STEP_SHAPES:
        for seed in (11, 2 ** 40 + 7):
            inp = make_inputs(N, 3, seed)
            rows = np.uint64(row0) + np.arange(N, dtype=np.uint64)
            u = accept_uniform(seed, 3, rows)
            assert np.all((u > 0.0) & (u < 1.0))
            _, _, knife, margin = decide(inp['logw_prop'], inp['logw_cur'], u)
            smallest, total = min(smallest, float(margin.min())), total + int(knife.sum())
    print('restatement: %d knife-edge rows, smallest margin |log u - (lp - lc)| = %.3e' % (total, smallest))
    assert total == 0


def test_accept_uniforms_bracketed_by_decisions(backend):
    """The library's accept uniform of every row, pinned from both sides: with lc = 0 a proposal of lp = log u + g accepts and
    one of lp = log u - g rejects, u the restated uniform of (seed, draw, global row) and g = 1e-9 (1 + |log u|) - more than 10^4 knife-edge
    margins, so the logarithms' few ulp do not matter, and small enough that a uniform from any other block, word pair or row
    of the pair fails one side on nearly every row."""
    N, row0, seed, da = 4099, 7, 2 ** 40 + 7, 3
    logu = np.log(accept_uniform(seed, da, np.uint64(row0) + np.arange(N, dtype=np.uint64)))
    gap = 1e-9 * (1.0 + np.abs(logu))
    assert np.all(gap > 1e4 * KNIFE * (1.0 + np.abs(logu) + gap))
    inp = make_inputs(N, 1, 3, planted=False)
    inp['logw_cur'] = np.zeros(N)
    for sign, expect in ((+1.0, 1), (-1.0, 0)):
        inp['logw_prop'] = logu + sign * gap
        rc, _, view = step(backend, inp, N, 1, propose=False, row0=row0, seed=seed, da=da)
        assert rc == 0
        got = view['n_acc'][0, :N] - inp['n_acc']
        print('%s: lp = log u %+.0e (1 + |log u|): %d of %d rows accept' % (backend, sign * 1e-9, int(got.sum()), N))
        assert np.array_equal(got, np.full(N, expect, dtype=np.int32))


def test_step_against_the_restatement(backend):
    accepted = rows = 0
    worst = 0.0
    for N, row0, offset in STEP_SHAPES:
        for rho in (0.0, 0.5):
            for accept, propose in PHASES:
                for seed in (11, 2 ** 40 + 7):
                    a, n, err = check_step(backend, N, 3, accept, propose, rho, row0, offset, seed)
                    worst = max(worst, err)
                    if accept and N == 4099:
                        accepted, rows = accepted + a, rows + n
    print('%s: %d of %d rows accepted (%.3f); Znext against the restatement %.3e (bound %.3e)' % (backend, accepted, rows, accepted / rows, worst, TOL))
    assert 0.3 < accepted / rows < 0.7 and worst <= TOL


def test_rho_zero_proposes_the_reference_draws(backend):
    """rho = 0: Znext is what ttm_normal_fill writes, bit for bit, and a NaN in Zcur does not reach it."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    for N, row0 in ((4099, 0), (1000, 7)):
        inp = make_inputs(N, 3, 5)
        inp['Zcur'] = np.full((3, N), np.nan)
        for accept in (False, True):
            rc, host, view = step(backend, inp, N, 3, accept=accept, rho=0.0, col0=2, row0=row0, seed=9, da=6, dp=7, pad=1)
            assert rc == 0
            ld = N + 1
            Z = torch.full((3 * ld,), SENTINEL, dtype=torch.float64, device='cpu' if backend == 'hostemu' else 'cuda')
            assert lib.ttm_normal_fill(ctypes.c_void_p(Z.data_ptr()), ld, N, 3, 2, 9, 7, row0, None) == 0
            fill = Z.cpu().numpy().reshape(3, ld)[:, :N]
            assert np.all(np.isfinite(view['Znext'][:3, :N])) and same_bits(view['Znext'][:3, :N], fill)


def outputs(view, N, ncols, lo=0):
    return [view[k][:ncols, lo:lo + N].copy() for k in ('Zcur', 'Xcur', 'Znext', 'Xrec')] + \
           [view[k][:1, lo:lo + N].copy() for k in ('logw_out', 'n_acc', 'n_bad')]


def test_a_window_of_rows_equals_those_rows_of_the_whole(backend):
    N, ncols = 4099, 3
    inp = make_inputs(N, ncols, 21)
    rc, _, whole = step(backend, inp, N, ncols, rho=0.5, seed=21)
    assert rc == 0
    for start, n in ((5, 1000), (6, 999)):
        part_inp = {k: v[..., start:start + n] for k, v in inp.items()}
        rc, _, part = step(backend, part_inp, n, ncols, rho=0.5, seed=21, row0=start)
        assert rc == 0
        for a, b in zip(outputs(part, n, ncols), outputs(whole, n, ncols, lo=start)):
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), start


def test_a_column_does_not_depend_on_the_columns_of_the_call(backend):
    """N large enough that the launch spreads the 40 columns over workgroups."""
    N, ncols = 65539, 40
    inp = make_inputs(N, ncols, 33)
    rc, _, all_cols = step(backend, inp, N, ncols, rho=0.5, seed=33, pad=1)
    assert rc == 0
    ref = outputs(all_cols, N, ncols)
    assert 0.3 < float(np.mean(ref[5] - inp['n_acc'])) < 0.7
    for j in range(ncols):
        one_inp = {k: (v[j:j + 1] if v.ndim == 2 else v) for k, v in inp.items()}
        rc, _, one = step(backend, one_inp, N, 1, rho=0.5, seed=33, col0=j, pad=1)
        assert rc == 0
        got = outputs(one, N, 1)
        for a, b in zip(got[:4], ref[:4]):
            assert np.array_equal(a[0].view(np.uint64), b[j].view(np.uint64)), j
        for a, b in zip(got[4:], ref[4:]):
            assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), j


def test_argument_errors(backend):
    N, ncols = 10, 2
    inp = make_inputs(N, ncols, 1, planted=False)
    nan = float('nan')
    cases = [dict(null=('Zcur',)), dict(null=('Xcur',)), dict(null=('logw_cur',)),
             dict(accept=False, propose=False),
             dict(null=('Zprop',)), dict(null=('Xprop',)), dict(null=('logw_out',)),
             dict(alias={'logw_out': ('logw_cur', 0)}), dict(alias={'logw_out': ('logw_cur', N - 1)}), dict(alias={'logw_out': ('logw_cur', 1 - N)}),
             dict(alias={'logw_out': ('logw_prop', 0)}), dict(alias={'logw_out': ('logw_prop', N - 1)}),
             dict(override={'N': 0}), dict(override={'N': -1}), dict(override={'ncols': 0}), dict(col0=-1), dict(row0=-1),
             dict(override={'ldzc': N - 1}), dict(override={'ldxc': N - 1}), dict(override={'ldzp': N - 1}), dict(override={'ldxp': N - 1}),
             dict(override={'ldzn': N - 1}), dict(override={'ldxr': N - 1}),
             dict(accept=False, override={'ldzp': N - 1}), dict(propose=False, override={'ldzn': N - 1}), dict(null=('Xrec',), override={'ldxr': N - 1}),
             dict(da=2 ** 31), dict(dp=2 ** 31), dict(da=2 ** 32 - 1),
             dict(rho=nan), dict(rho=1.0), dict(rho=-1.0), dict(rho=1.5)]
    rc, _, _ = step(backend, inp, N, ncols, rho=0.5)
    assert rc == 0
    for kw in cases:
        rc, host, view = step(backend, inp, N, ncols, **dict(dict(rho=0.5), **kw))
        print('%s %s: %d' % (backend, kw, rc))
        assert rc == E_ARG, kw
        for name in ('Zcur', 'Xcur', 'n_acc', 'n_bad'):                                   # the state is as it was
            cols = ncols if name in MATS else 1
            assert np.array_equal(view[name][:cols, :N], np.reshape(inp[name], (cols, N))), (kw, name)
        for name in ('logw_out', 'Znext', 'Xrec'):                                        # nothing was launched
            assert np.all(host[name] == SENTINEL), (kw, name)


# ------------------------------------------------------------------------------------------ the class

def make(name, **override):
    """A map of a golden case with the fixture's coefficients (tests/test_sample.py: make)."""
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    npz, desc = load_case(name)
    X = specs.sample_mixture(4000) if name == 'c5_sep' else case_X(name, npz)
    kw = ctor_kwargs(desc)
    kw.update(override)
    tm = transport_map(X=X, monotone=desc['monotone'], nonmonotone=desc['nonmonotone'], verbose=False, **kw)
    tm.coeffs_mon, tm.coeffs_nonmon = coeff_lists(npz, tm.D)
    return tm, X


def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


class Forced:
    """A stateful host target: sign * 1000 * (number of the call) for every row."""

    def __init__(self, sign):
        self.sign, self.calls, self.shapes = sign, 0, []

    def __call__(self, X):
        self.calls += 1
        self.shapes.append(X.shape)
        return np.full(X.shape[0], self.sign * 1000.0 * self.calls)


def gauss_host(mu, sd):
    return lambda X: -0.5 * np.sum(((X - mu) / sd) ** 2, axis=1)


FORCED_CASES = [('c3_sep', {}, 0), ('c5_sep', dict(alternate_root_finding=False, root_finder='newton'), 2), ('c2a_int', {}, 0)]


@pytest.mark.parametrize('name,override,E', FORCED_CASES, ids=['c3_sep', 'c5_sep_newton_one_point', 'c2a_int'])
def test_forced_decisions_through_sample_mcmc(backend, name, override, E):
    tm, Xtrain = make(name, **override)
    N, steps, seed, draw0 = 1001, 4, 13, 20
    X_star = np.asarray(Xtrain[3, :E], dtype=float) if E else None
    own = tm.D - E
    draws = [tm.sample(N, X_star=X_star, seed=seed, draw=draw0 + t)[:, E:] for t in range(steps + 1)]
    up = Forced(+1)
    X, info = tm.sample_mcmc(up, N, steps, X_star=X_star, seed=seed, draw=draw0)
    assert X.shape == (steps, N, own) and up.calls == steps + 1 and set(up.shapes) == {(N, own)}
    print('%s %s: forced accepts, rate %.3f .. %.3f; draws %s' % (backend, name, info['accept_rate'].min(), info['accept_rate'].max(), info['draws']))
    assert np.all(info['accept_rate'] == 1.0) and np.all(info['n_bad'] == 0) and info['draws'] == (draw0, draw0 + steps)
    for t in range(1, steps + 1):
        assert same_bits(X[t - 1], draws[t]), t
    down = Forced(-1)
    X, info = tm.sample_mcmc(down, N, steps, X_star=X_star, seed=seed, draw=draw0)
    assert np.all(info['accept_rate'] == 0.0) and down.calls == steps + 1
    for t in range(steps):
        assert same_bits(X[t], draws[0]), t
    assert tm._draws == 0                                     # explicit draws leave the map's counter alone


def test_draw_counter_burn_thin_and_continuation(backend):
    tm, Xtrain = make('c3_sep')
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    target = gauss_host(mu, sd)
    N, seed = 257, 3
    tm._draws = 5
    X, info = tm.sample_mcmc(target, N, 6, rho=0.5, seed=seed)
    assert tm._draws == 5 + 7 and info['draws'] == (5, 11)
    Xe, infoe = tm.sample_mcmc(target, N, 6, rho=0.5, seed=seed, draw=5)
    assert tm._draws == 12 and same_bits(X, Xe) and same_bits(info['logw'], infoe['logw'])
    rate = float(info['accept_rate'].mean())
    print('%s: acceptance rate %.3f' % (backend, rate))
    assert 0.05 < rate < 0.999
    # burn / thin: the states after the steps burn + thin, burn + 2 thin, ...
    for burn, thin, keep in ((0, 2, (2, 4, 6)), (1, 2, (3, 5)), (3, 3, (6,)), (5, 1, (6,))):
        Xb, _ = tm.sample_mcmc(target, N, 6, rho=0.5, seed=seed, draw=5, burn=burn, thin=thin)
        assert Xb.shape == (len(keep), N, tm.D)
        for i, t in enumerate(keep):
            assert same_bits(Xb[i], X[t - 1]), (burn, thin, t)
    # a continued run: the bits of one longer run, with the map's counter (draw None) and with explicit draws
    tm._draws = 5
    Xa, infoa = tm.sample_mcmc(target, N, 2, rho=0.5, seed=seed)
    assert tm._draws == 8
    Xc, infoc = tm.sample_mcmc(target, N, 4, rho=0.5, seed=seed, init=infoa['state'])
    assert tm._draws == 12 and infoc['draws'] == (7, 11)
    assert same_bits(np.concatenate((Xa, Xc)), X) and same_bits(infoc['logw'], info['logw'])
    assert np.array_equal(infoc['accept_rate'], info['accept_rate']) and np.array_equal(infoc['n_bad'], info['n_bad'])
    Xd, _ = tm.sample_mcmc(target, N, 4, rho=0.5, seed=seed, init=infoa['state'], draw=7)
    assert tm._draws == 12 and same_bits(Xd, Xc)


def test_initial_states_from_an_array(backend):
    """init = raw states: z and log q come from one forward pass; an initial -inf weight is allowed, NaN and +inf raise."""
    tm, Xtrain = make('c3_sep', alternate_root_finding=False, root_finder='newton')
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    N = 301
    x0 = np.asarray(Xtrain[:N], dtype=float)
    calls = []

    def target(X):
        calls.append(X.copy())
        out = gauss_host(mu, sd)(X)
        if len(calls) == 1:
            out[4] = -np.inf
        return out
    X, info = tm.sample_mcmc(target, N, 3, rho=0.0, seed=2, draw=0, init=x0)
    err = float(np.max(np.abs(calls[0] - x0)))
    print('%s: initial states as the target sees them, max |x - init| = %.3e' % (backend, err))
    assert err <= 1e-12
    assert info['accept_rate'][4] > 0 and np.all(np.isfinite(info['logw']))
    # rho = 0: the first proposal is the draw of draw0 + 1 whatever the initial state
    assert same_bits(calls[1], tm.sample(N, seed=2, draw=1))
    for value in (np.nan, np.inf):
        def broken(X, value=value):
            out = gauss_host(mu, sd)(X)
            out[7] = value
            return out
        with pytest.raises(ValueError, match='initial'):
            tm.sample_mcmc(broken, N, 3, seed=2, draw=0, init=x0)


def test_initial_state_of_an_array_is_the_maps_own(backend):
    """init = the rows sample() drew: the z that the forward pass over [k0, D) gives them is the reference draw they were made
    from, and their initial log-weight is log p - log q with the log q that sample(logdensity=True) reports.  Bound on both:
    2e-9, what tests/test_newton_inverse.py holds the Newton search's stopping rule |S_k - z_k| <= 1e-9 to (z), and far above
    the roundings of export and import that separate the two evaluations of log q at the same rows - a missing sigma or
    2 pi term is an error of order 1.  The target rejects every proposal (-inf), so the final state is the initial one."""
    for E in (0, 1):
        tm, Xtrain = make('c3_sep', alternate_root_finding=False, root_finder='newton')
        mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
        N, seed, d0 = 301, 6, 9
        X_star = np.asarray(Xtrain[:N, :E], dtype=float) if E else None
        x0, logq = tm.sample(N, X_star=X_star, seed=seed, draw=d0, logdensity=True)
        zref = tm.reference_device(N, seed=seed, draw=d0, ncols=tm.D - E, col0=E)[:, :N].cpu().numpy()
        logp = gauss_host(mu[E:], sd[E:])(x0[:, E:])
        calls = []

        def target(X):
            calls.append(1)
            return gauss_host(mu[E:], sd[E:])(X) if len(calls) == 1 else np.full(X.shape[0], -np.inf)
        X, info = tm.sample_mcmc(target, N, 2, X_star=X_star, rho=0.5, seed=1, draw=0, init=x0[:, E:])
        assert np.all(info['accept_rate'] == 0.0) and np.all(info['n_bad'] == 0)
        ez = float(np.max(np.abs(info['state']['Z'][:, :N].cpu().numpy() - zref)))
        ew = float(np.max(np.abs(info['logw'] - (logp - logq))))
        ex = float(np.max(np.abs(X[-1] - x0[:, E:])))
        print('%s E = %d: init = sample(): max |z - reference draw| = %.3e, max |logw - (log p - log q)| = %.3e, max |x - init| = %.3e (bounds 2e-9, 2e-9, 1e-12)'
              % (backend, E, ez, ew, ex))
        assert ez <= 2e-9 and ew <= 2e-9 and ex <= 1e-12


def test_a_wider_conditioning_matrix(backend):
    """mcmc_device with a caller's Xs wider than the chains' own leading dimension (odd N): the state keeps its own leading
    dimension, so trace and state are those of the default matrix bit for bit, with conditioning columns (k0 = 1) and without;
    a width that is odd, short or not a device matrix of doubles is a ValueError."""
    import torch
    tm, _ = make('c3_sep')
    N, steps = 301, 3
    d = tm._cm.d_cols
    cond = np.random.default_rng(8).standard_normal(N)

    def run(k0, width):
        mu, sd = tm._mean_d[d - tm.D + k0:d, None], tm._std_d[d - tm.D + k0:d, None]
        Xs = None
        if width is not None:
            Xs = torch.full((d, width), 3.5, dtype=torch.float64, device=tm._dev)
            Xs[:d - tm.D + k0] = 0.0
            if k0:
                Xs[d - tm.D, :N] = torch.from_numpy(cond).to(tm._dev)
        elif k0:
            Xs = tm._cols(d, N, zero=True)
            Xs[d - tm.D, :N] = torch.from_numpy(cond).to(tm._dev)
        return tm.mcmc_device(lambda raw: -0.5 * (((raw - mu) / sd) ** 2).sum(dim=0), N, steps, Xs=Xs, rho=0.5, seed=4, draw=2, k0=k0)
    for k0 in (0, 1):
        trace, state = run(k0, None)
        assert tuple(trace.shape) == (steps, tm.D - k0, N + 1)
        moved = float(state['n_acc'].sum().item()) / (N * steps)
        for width in (N + 1, N + 3, 2 * N + 2):
            tw, sw = run(k0, width)
            assert tuple(tw.shape) == tuple(trace.shape) and tuple(sw['X'].shape) == (tm.D - k0, N + 1)
            assert same_bits(tw[:, :, :N].cpu().numpy(), trace[:, :, :N].cpu().numpy()), (k0, width)
            for key in ('Z', 'X'):
                assert same_bits(sw[key][:, :N].cpu().numpy(), state[key][:, :N].cpu().numpy()), (k0, width, key)
            assert same_bits(sw['logw'].cpu().numpy(), state['logw'].cpu().numpy())
            assert np.array_equal(sw['n_acc'].cpu().numpy(), state['n_acc'].cpu().numpy())
        print('%s k0 = %d: widths %d, %d, %d give the bits of the default; acceptance rate %.3f' % (backend, k0, N + 1, N + 3, 2 * N + 2, moved))
        assert 0.05 < moved < 0.999
    for Xs in (torch.zeros((d, N), dtype=torch.float64, device=tm._dev), torch.zeros((d, N + 2), dtype=torch.float64, device=tm._dev),
               torch.zeros((d, N - 1), dtype=torch.float64, device=tm._dev), torch.zeros((d + 1, N + 1), dtype=torch.float64, device=tm._dev),
               torch.zeros((d, N + 1), dtype=torch.float32, device=tm._dev), torch.zeros((d, 2 * N + 2), dtype=torch.float64, device=tm._dev)[:, ::2],
               np.zeros((d, N + 1))):
        with pytest.raises(ValueError, match='Xs'):
            tm.mcmc_device(lambda raw: -0.5 * (raw ** 2).sum(dim=0), N, steps, Xs=Xs, draw=0)
    assert tm._draws == 0


def test_a_continuation_runs_on_its_own_stream(backend):
    """init = state: seed and row0 are the state's, whether the call leaves them out or repeats them, to the bits of one longer
    run; another seed or row0, or a state without its bookkeeping, is a ValueError."""
    tm, _ = make('c3_sep')
    target = gauss_host(np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float))
    N, seed, row0 = 129, 3, 6
    X, info = tm.sample_mcmc(target, N, 5, rho=0.5, seed=seed, draw=4, row0=row0)
    Xa, infoa = tm.sample_mcmc(target, N, 2, rho=0.5, seed=seed, draw=4, row0=row0)
    state = infoa['state']
    assert state['seed'] == seed and state['row0'] == row0
    for kw in (dict(), dict(seed=seed), dict(row0=row0), dict(seed=seed, row0=row0)):
        Xc, infoc = tm.sample_mcmc(target, N, 3, rho=0.5, init=state, **kw)
        assert same_bits(np.concatenate((Xa, Xc)), X) and same_bits(infoc['logw'], info['logw']), kw
        assert infoc['draws'] == (6, 9) and infoc['state']['seed'] == seed and infoc['state']['row0'] == row0
        assert np.array_equal(infoc['accept_rate'], info['accept_rate'])
    for kw in (dict(seed=seed + 1), dict(row0=row0 + 1), dict(seed=seed, row0=1)):
        with pytest.raises(ValueError, match='seed'):
            tm.sample_mcmc(target, N, 3, rho=0.5, init=state, **kw)
    for key in ('steps', 'draws', 'seed', 'row0', 'Z', 'n_bad'):
        broken = {k: v for k, v in state.items() if k != key}
        with pytest.raises(ValueError, match='state'):
            tm.sample_mcmc(target, N, 3, rho=0.5, init=broken)
    for key, value in (('draws', None), ('draws', (4,)), ('steps', 'many'), ('logw', state['logw'].cpu().numpy()), ('n_acc', state['n_acc'].long())):
        with pytest.raises(ValueError, match='state'):
            tm.sample_mcmc(target, N, 3, rho=0.5, init=dict(state, **{key: value}))
    print('%s: a continuation takes seed %d and row0 %d from its state' % (backend, seed, row0))


def exact_fma(a, b, c):
    """fma(a, b, c) entry by entry: exact rational arithmetic, one rounding."""
    out = np.empty(b.shape)
    fa = Fraction(float(a))
    for idx in np.ndindex(*b.shape):
        out[idx] = float(fa * Fraction(float(b[idx])) + Fraction(float(c[idx])))
    return out


def test_composition(backend):
    """mcmc_device against the same chain put together from reference_device, inverse_device(logq=True), the restated uniforms
    and the accept rule in NumPy."""
    import torch
    tm, _ = make('c3_sep')
    N, steps, rho, seed, draw0 = 513, 6, 0.6, 77, 40
    D = tm.D
    mu = tm._to_dev(np.asarray(tm.X_mean, dtype=float))[:, None]
    sd = tm._to_dev(np.asarray(tm.X_std, dtype=float))[:, None]

    def target(raw):
        return -0.5 * (((raw - mu) / sd) ** 2).sum(dim=0)
    trace, state = tm.mcmc_device(target, N, steps, rho=rho, seed=seed, draw=draw0)
    assert last_kernel(tm) == ('hostemu' if backend == 'hostemu' else 'k_mh_step')     # the last launch of a run decides its last step
    assert tuple(trace.shape) == (steps, D, N + (N & 1))
    g_scale = tm._to_dev(1.0 / np.asarray(tm.X_std, dtype=float))
    const = 0.5 * D * np.log(2 * np.pi)
    s = float(np.sqrt((1.0 - rho) * (1.0 + rho)))
    rows = np.arange(N, dtype=np.uint64)

    def invert(Zdev):
        Xd, logq = tm.inverse_device(Zdev, N, logq=True, g_scale=g_scale)
        raw = Xd[:D, :N] * tm._std_d[:D, None] + tm._mean_d[:D, None]
        logw = target(raw).reshape(N).to(torch.float64) - (logq[:N] - const)
        return Xd[:, :N].cpu().numpy().copy(), logw.cpu().numpy().copy()
    Zdev = tm.reference_device(N, seed=seed, draw=draw0)
    Z = Zdev[:, :N].cpu().numpy().copy()
    X, logw = invert(Zdev)
    n_acc = np.zeros(N, dtype=np.int64)
    excluded, smallest = 0, np.inf
    for t in range(1, steps + 1):
        xi = tm.reference_device(N, seed=seed, draw=draw0 + t)[:, :N].cpu().numpy()
        Zp = exact_fma(rho, Z, s * xi)
        Zp_dev = tm._cols(D, N, zero=True)
        Zp_dev[:, :N].copy_(torch.from_numpy(Zp))
        Xp, logwp = invert(Zp_dev)
        acc, bad, knife, margin = decide(logwp, logw, accept_uniform(seed, draw0 + t, rows))
        excluded, smallest = excluded + int(knife.sum()), min(smallest, float(margin.min()))
        assert not bad.any()
        Z, X, logw = np.where(acc, Zp, Z), np.where(acc, Xp, X), np.where(acc, logwp, logw)
        n_acc += acc
        assert same_bits(trace[t - 1][:, :N].cpu().numpy(), X), t
    print('%s: %d rows excluded, smallest margin %.3e, acceptance rate %.3f' % (backend, excluded, smallest, n_acc.mean() / steps))
    assert excluded == 0
    assert np.array_equal(state['n_acc'].cpu().numpy(), n_acc)
    assert same_bits(state['Z'][:, :N].cpu().numpy(), Z) and same_bits(state['X'][:, :N].cpu().numpy(), X)
    err = float(np.max(np.abs(state['logw'].cpu().numpy() - logw)))
    print('%s: final log-weights, max |a - b| = %.3e' % (backend, err))
    assert err <= 1e-12
    assert 0.05 < n_acc.mean() / steps < 0.999


def test_stationarity(backend):
    """c3_sep with the Newton inverse, target N(X_mean, diag(X_std^2)), 8192 independent chains started IN the target
    (np.random.default_rng(2024)), 30 steps at rho = 0.7, seed 1, draws 0 .. 30: if the step leaves the target invariant the final
    states are an exact i.i.d. sample of it, so the standardised errors of every column's mean, sqrt(n) (mean - mu) / sd, and
    second moment, sqrt(n / 2) (mean(((x - mu) / sd)^2) - 1), are standard normal to first order.  Cap 4.5 on each; the
    acceptance rate must lie strictly between 0.05 and 0.999.  The host double gives 0.10 0.84 0.64 1.29 for the means and
    -1.79 0.71 -0.80 -0.72 for the second moments at an acceptance rate of 0.385 (94 % of the chains have moved)."""
    tm, _ = make('c3_sep', alternate_root_finding=False, root_finder='newton')
    mu, sd = np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float)
    n, steps = 8192, 30
    x0 = mu + sd * np.random.default_rng(2024).standard_normal((n, tm.D))
    X, info = tm.sample_mcmc(gauss_host(mu, sd), n, steps, rho=0.7, seed=1, draw=0, init=x0, burn=steps - 1)
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


def test_python_argument_errors(backend):
    tm, Xtrain = make('c3_sep')
    target = gauss_host(np.asarray(tm.X_mean, dtype=float), np.asarray(tm.X_std, dtype=float))
    good = dict(chains=16, steps=4)
    X, _ = tm.sample_mcmc(target, seed=1, draw=0, **good)
    assert X.shape == (4, 16, tm.D)
    bad = [dict(chains=0), dict(steps=0), dict(thin=0), dict(burn=-1), dict(burn=4), dict(burn=2, thin=3), dict(rho=1.0), dict(rho=-1.0),
           dict(rho=float('nan')), dict(draw=2 ** 31 - 4), dict(draw=-1), dict(init=np.zeros((15, tm.D))), dict(init=np.zeros((16, tm.D - 1))),
           dict(init=dict(Z=None))]
    for change in bad:
        kw = dict(dict(good, seed=1, draw=0), **change)
        with pytest.raises(ValueError):
            tm.sample_mcmc(target, **kw)
    assert tm.sample_mcmc(target, 16, 4, draw=2 ** 31 - 5)[1]['draws'] == (2 ** 31 - 5, 2 ** 31 - 1)
    with pytest.raises(ValueError, match='return'):
        tm.sample_mcmc(lambda X: np.zeros(15), 16, 4, draw=0)
    with pytest.raises(ValueError, match='return'):
        tm.sample_mcmc(lambda raw: raw[0, :15], 16, 4, draw=0, target_on_device=True)
    _, state = tm.mcmc_device(lambda raw: -0.5 * (raw ** 2).sum(dim=0), 16, 2, draw=0)
    with pytest.raises(ValueError, match='state'):
        tm.mcmc_device(lambda raw: -0.5 * (raw ** 2).sum(dim=0), 17, 2, init=state)
    assert tm._draws == 0


# ------------------------------------------------------------------------------------------ the timing tool

@pytest.mark.gpu
def test_timing_tool_runs(tmp_path):
    """tools/mcmc_bench.py in a fresh child process on small shapes (as tests/test_bench_tools.py runs its tools; the time limit
    ends a hang and gates no speed)."""
    out = tmp_path / 'result.json'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'mcmc_bench.py'), '--workloads', 'C2b', '--rows', '65536', '--launches', '4',
                          '--rounds', '2', '--chain-workloads', 'C2a', '--chains', '4096', '--steps', '3', '--calls', '1', '--label', 'small',
                          '--out', str(out)], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    js = json.loads(res.stdout.splitlines()[-1])
    assert js['label'] == 'small' and js['rounds'] == 2 and json.loads(out.read_text()) == js
    wl = js['workloads']['C2b']
    v = wl['versions']
    assert wl['N'] == 65536 and wl['ncols'] == 2 and 0.3 < wl['accepted_share'] < 0.7
    assert sorted(v) == ['mh_accept', 'mh_propose', 'mh_step', 'normal_fill', 'torch_step']
    assert all(len(x['ms_rounds']) == 2 and x['ms'] > 0 for x in v.values())
    assert all(v[k]['kernel'] == 'k_mh_step' for k in ('mh_step', 'mh_accept', 'mh_propose')) and v['normal_fill']['kernel'] == 'k_normal_fill'
    chain = js['chains']['cases']['C2a']
    print('fused step %.4f ms, torch %.4f ms; chains %.3f ms per step, acceptance %.3f' % (v['mh_step']['ms'], v['torch_step']['ms'], chain['ms_per_step'],
                                                                                       chain['accept_rate']))
    assert chain['steps_per_second'] > 0 and 0.0 < chain['accept_rate'] < 1.0
