"""
The DEVICE builds of the fp64 primitives (csrc/ttm_math.h, csrc/ttm_dense.h and the ones private to csrc/ttm_band.hip), held to
the bounds DESIGN.md and the header comments quote.  tests/test_math.py runs the host build of the same header; what it cannot
see is here: the v_rcp_f64 + Newton branches of the reciprocal and the divisions (plain IEEE divisions in the host build), the
band kernels' private primitives, the tables as the kernels stage them (LDS copies, constant memory, the pair-table image) and
the device lowering of rint / cvt / ldexp / frexp and of band_expq's inline min(|x|, hi).

Everything goes through the test hook ttm_math_probe (include/ttm.h): one elementwise launch per test on the full operand set.
Reference: mpmath at 30 digits on a fixed subsample of at most 6 000 points plus every listed edge operand; the remaining
points against NumPy at a bound one ulp looser (the divisions against NumPy at the SAME bound: an IEEE quotient is the
correctly rounded one, i.e. the rounded mpmath value).  ulp = |got - ref| / spacing(|ref|), ref rounded to double as in
tests/test_math.py.  Every achieved maximum is recorded under device_math/<function>/<quantity> (tests.util.record_parity).
"""
import ctypes
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest

from tests.hostemu import emu
from tests.util import record_parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ids of include/ttm.h (TTM_PROBE_*)
FAST_EXP, ERF_TAB, GAUSS_TAB, FAST_LOG, FAST_RCP, FAST_DIV, EXP_Q_TAB, EXP_Q_FAST = range(8)
FAST_DIV1, APPROX_RCP, DENSE_EXP_CORE, FAST_EXP_V2, EXP_Q_FAST_V2 = 8, 9, 10, 11, 12
BAND_EXPQ, BAND_EXPQ_SERIES, BAND_EXPQ_FAR, BAND_LOG, BAND_DIV = 32, 33, 34, 35, 36
TWO_OPERANDS = (FAST_DIV, FAST_DIV1, BAND_DIV)
TTM_E_ARG, TTM_E_UNSUPPORTED = -1, -4
SENTINEL = -1.2345e77                      # behind the n results: the kernels write n doubles and nothing else


def header_ids():
    text = open(os.path.join(ROOT, 'include', 'ttm.h')).read()
    return {name: int(val) for name, val in re.findall(r'#define TTM_PROBE_(\w+) (\d+)', text)}


# ---- running a primitive ------------------------------------------------------------------------------------------------

def device(which, a, b=None):
    """out[i] = f(a[i] [, b[i]]) on the GPU: one launch of the probe kernel."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    a = np.ascontiguousarray(a, dtype=float)
    ta = torch.from_numpy(a).cuda()
    tb = None if b is None else torch.from_numpy(np.ascontiguousarray(b, dtype=float)).cuda()
    out = torch.full((a.size + 8,), SENTINEL, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    rc = lib.ttm_math_probe(which, ta.data_ptr(), None if tb is None else tb.data_ptr(), a.size, out.data_ptr(), None)
    assert rc == 0, lib.ttm_last_error_string().decode()
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.all(res[a.size:] == SENTINEL), 'the probe kernel wrote behind its n results'
    return res[:a.size].copy()


def host(which, a, b=None):
    """The same through the host test double (host build of the same headers)."""
    a = np.ascontiguousarray(a, dtype=float)
    bb = None if b is None else np.ascontiguousarray(b, dtype=float)
    out = np.full(a.size + 8, SENTINEL)
    rc = emu.lib().ttm_math_probe(which, emu.ptr(a), emu.ptr(bb), ctypes.c_int64(a.size), emu.ptr(out), None)
    assert rc == 0
    assert np.all(out[a.size:] == SENTINEL)
    return out[:a.size].copy()


# ---- measuring ------------------------------------------------------------------------------------------------------------

def ulps(x, ref):
    with np.errstate(all='ignore'):
        u = np.abs(x - ref) / np.spacing(np.abs(ref))
    u = np.where((x == ref) | (np.isnan(x) & np.isnan(ref)), 0.0, u)       # (equal infinities, NaN for NaN)
    return np.where(np.isnan(u), np.inf, u)                                 # a NaN where a number belongs is a miss


def hold(key, err, tol, operands, got, ref, strict=False, unit='ulp'):
    """Record the maximum of `err` under device_math/<key> and assert it against `tol` (<=, or < when `strict`); tol may be an
    array (a bound per operand: the worst is then the largest err / tol).  The failure names the worst operand."""
    err = np.where(np.isnan(np.asarray(err, dtype=float)), np.inf, np.asarray(err, dtype=float))
    tol_a = np.broadcast_to(np.asarray(tol, dtype=float), err.shape)
    j = int(np.argmax(err / tol_a)) if err.size else 0
    worst = float(err[j]) if err.size else 0.0
    record_parity('device_math/' + key, worst, float(tol_a[j]) if err.size else None)
    print('device_math/%s: max %.4g %s (bound %.4g) at operand %s' % (key, worst, unit, tol_a[j] if err.size else 0.0,
                                                                     operand_str(operands, j) if err.size else '-'))
    ok = (err < tol_a) if strict else (err <= tol_a)
    assert np.all(ok), ('device_math/%s: %d operand(s) miss the bound; worst: operand %s -> %r, reference %r, %.4g %s, bound %s %.4g'
                        % (key, int((~ok).sum()), operand_str(operands, j), float(got[j]), float(ref[j]), worst, unit,
                           '<' if strict else '<=', tol_a[j]))
    return worst


def operand_str(operands, j):
    if isinstance(operands, tuple):
        return '(%r, %r)' % (float(operands[0][j]), float(operands[1][j]))
    return repr(float(operands[j]))


_CACHE = {}


def cached(fn):
    def wrapper(*args):
        key = (fn.__name__,) + args
        if key not in _CACHE:
            _CACHE[key] = fn(*args)
        return _CACHE[key]
    wrapper.__name__ = fn.__name__
    return wrapper


def mp_map(f, x):
    mp.mp.dps = 30
    return np.array([float(f(mp.mpf(float(v)))) for v in x])


def rest_of(n, sub):
    m = np.ones(n, dtype=bool)
    m[sub] = False
    return np.nonzero(m)[0]


# ---- operand sets (those of tests/test_math.py, same seeds and order, plus the edges the issue lists) ----------------------

@cached
def exp_set():
    """test_exp's set: 400 005 operands (odd: the VecD<2> probe pairs the last one with itself); mpmath on its subsample + the edges."""
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(-700, 700, 200000), rng.uniform(-2, 2, 200000), [0.0, -0.0, 1e-300, -745.0, 709.0]])
    sub = np.r_[0:2000, 200000:202000, 400000:400005]
    return a, sub, mp_map(mp.exp, a[sub])


@cached
def exp_q_set(seed):
    """test_exp_q_table's (seed 3) / test_exp_q_fast's (seed 4) set; reference: exp of the ROUNDED argument -x*x/4, as there."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-12, 12, 100000), rng.standard_normal(100000), np.linspace(-60, 60, 4001),
                        [0.0, -0.0, 1e-200, 54.0, -54.0]])
    sub = np.r_[0:1000, 100000:101000, 200000:204006]                      # 6 006 with the 6 edges: the grid and the edges in full
    arg = -0.25 * (x * x)
    return x, sub, mp_map(mp.exp, arg[sub])


@cached
def erf_set():
    rng = np.random.default_rng(1)
    t = np.concatenate([rng.uniform(-6.5, 6.5, 30000), np.linspace(-6, 6, 2049), np.arange(33) * 0.1875,
                        np.nextafter(np.arange(33) * 0.1875, -1), [0.0, -0.0, 7.0, -7.0, 1e300, -1e300]])
    sub = np.r_[0:3000, 30000:len(t)]
    return t, sub, mp_map(mp.erf, t[sub]), mp_map(lambda v: mp.exp(-v * v), t[sub])


@cached
def log_div_sets():
    """test_log_rcp_div's draws in its order: x, then a, then b."""
    rng = np.random.default_rng(2)
    x = np.concatenate([np.exp(rng.uniform(-700, 700, 100000)), rng.uniform(0.5, 2.0, 100000), [1.0, 1e-310, 1e308]])
    a = rng.standard_normal(100000) * np.exp(rng.uniform(-50, 50, 100000))
    b = rng.standard_normal(100000) * np.exp(rng.uniform(-50, 50, 100000))
    return x, a, b


@cached
def log_set():
    x = log_div_sets()[0]
    s = 0.70710678118654752
    edges = [1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), s, np.nextafter(s, 1.0), np.nextafter(s, 0.0), 5e-324, 2.2e-308,
             1e-310, 1e308]
    x = np.concatenate([x, edges])
    sub = np.r_[0:1500, 100000:101500, 200000:len(x)]
    return x, sub, mp_map(mp.log, x[sub])


@cached
def rcp_set():
    b = log_div_sets()[2]
    p2 = 2.0 ** np.arange(-500, 501, 50)
    b = np.concatenate([b, p2, -p2, [1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, 3.0]])
    sub = np.r_[0:5000, 100000:len(b)]
    return b, sub, mp_map(lambda v: 1 / v, b[sub])


@cached
def div_set():
    _, a, b = log_div_sets()
    rng = np.random.default_rng(20)
    m1 = rng.uniform(1, 2, 64) * rng.choice([-1.0, 1.0], 64)
    m2 = rng.uniform(1, 2, 64) * rng.choice([-1.0, 1.0], 64)
    big, small = 2.0 ** 250, 2.0 ** -250
    a = np.concatenate([a, b[:200], np.zeros(200), m1 * big, m1 * small, [big, small]])      # a = b | a = 0 | quotients ~ 2^+-500
    b = np.concatenate([b, b[:200], b[200:400], m2 * small, m2 * big, [small, big]])
    sub = np.r_[0:5000, 100000:len(a)]
    mp.mp.dps = 30
    ref = np.array([float(mp.mpf(float(u)) / mp.mpf(float(v))) for u, v in zip(a[sub], b[sub])])
    return a, b, sub, ref


@cached
def dense_exp_set():
    rng = np.random.default_rng(5)
    y = np.concatenate([rng.uniform(-700, 700, 50000), rng.uniform(-2, 2, 50000)])
    sub = np.r_[0:3000, 50000:53000]
    return y, sub, mp_map(mp.exp, y[sub])


BAND_EDGES = [0.0, -0.0, 16.0, -16.0, 16.5, -16.5, 60.0, -60.0, 1e300, -1e300, np.inf, -np.inf, np.nan]


@cached
def band_expq_set():
    rng = np.random.default_rng(6)
    mid = np.arange(800) * 0.02 + 0.01
    x = np.concatenate([rng.uniform(-16, 16, 100000), mid, np.nextafter(mid, np.inf), BAND_EDGES])
    sub = np.r_[0:4300, 100000:len(x)]                                    # 4 300 + 1 600 + 13 edges
    fin = np.where(np.isfinite(x[sub]), x[sub], 0.0)
    return x, sub, mp_map(lambda v: mp.exp(-v * v / 4), fin)


# ---- GPU: each primitive against its quoted bound ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_fast_exp_device():
    """fast_exp: <= 1 ulp vs mpmath (the rest vs np.exp at <= 2), NaN / underflow / overflow as test_exp, and the VecD<2> form
    bit for bit the scalar one (odd n: the padded partner of the last element is never stored)."""
    a, sub, ref = exp_set()
    ops = np.concatenate([a, [np.nan, -1e9, np.inf]])
    got_all = device(FAST_EXP, ops)
    got, tail = got_all[:a.size], got_all[a.size:]
    hold('fast_exp/ulp_vs_mpmath', ulps(got[sub], ref), 1.0, a[sub], got[sub], ref)
    rest = rest_of(a.size, sub)
    hold('fast_exp/ulp_vs_numpy', ulps(got[rest], np.exp(a[rest])), 2.0, a[rest], got[rest], np.exp(a[rest]))
    assert np.isnan(tail[0])
    assert tail[1] == 0.0 or tail[1] < 1e-300
    assert tail[2] > 1e300
    v2 = device(FAST_EXP_V2, ops)
    assert ops.size % 2 == 0 and a.size % 2 == 1
    assert np.array_equal(v2.view(np.uint64), got_all.view(np.uint64)), 'fast_exp<VecD<2>> differs from the scalar form'
    assert np.array_equal(device(FAST_EXP_V2, a).view(np.uint64), got.view(np.uint64))        # odd n
    record_parity('device_math/fast_exp/v2_bit_differences', 0.0, 0.0)


EXP_Q_CASES = {
    'exp_q_fast': (EXP_Q_FAST, 4, [(1e100, 0.0), (100.0, 0.0), (-1e8, 0.0)]),
    'exp_q_tab': (EXP_Q_TAB, 3, [(np.inf, 0.0), (-np.inf, 0.0), (1e200, 0.0)]),
    'band_expq_series': (BAND_EXPQ_SERIES, 4, [(1e100, 0.0), (100.0, 0.0), (-1e8, 0.0)]),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(EXP_Q_CASES))
def test_exp_q_device(name):
    """exp(-x^2/4) by series / 2^(j/32) table / the band kernels' series: <= 2 ulp of exp of the rounded argument where that is
    > 1e-300, |got| < 1e-299 elsewhere, NaN -> NaN, and the far / infinite results test_exp_q_* assert for the function."""
    which, seed, fixed = EXP_Q_CASES[name]
    x, sub, ref = exp_q_set(seed)
    ops = np.concatenate([x, [np.nan], [v for v, _ in fixed]])
    got_all = device(which, ops)
    got, tail = got_all[:x.size], got_all[x.size:]
    ok = ref > 1e-300
    hold(name + '/ulp_vs_mpmath', ulps(got[sub][ok], ref[ok]), 2.0, x[sub][ok], got[sub][ok], ref[ok])
    hold(name + '/abs_where_underflowed', np.abs(got[sub][~ok]), 1e-299, x[sub][~ok], got[sub][~ok], ref[~ok], strict=True, unit='abs')
    rest = rest_of(x.size, sub)
    with np.errstate(all='ignore'):
        nref = np.exp(-0.25 * (x[rest] * x[rest]))
    okr = nref > 1e-300
    hold(name + '/ulp_vs_numpy', ulps(got[rest][okr], nref[okr]), 3.0, x[rest][okr], got[rest][okr], nref[okr])
    assert np.abs(got[rest][~okr]).max(initial=0.0) < 1e-299
    assert np.isnan(tail[0])
    for (v, want), g in zip(fixed, tail[1:]):
        assert g == want, '%s(%r) = %r, expected %r' % (name, v, g, want)
    if which == EXP_Q_FAST:
        v2 = device(EXP_Q_FAST_V2, ops[:-1])                                # (odd n)
        assert np.array_equal(v2.view(np.uint64), got_all[:-1].view(np.uint64)), 'exp_q_fast<VecD<2>> differs from the scalar form'


@pytest.mark.gpu
def test_erf_and_gauss_table_device():
    """erf_gauss_tab<true> from the LDS copy of the table: erf abs < 2.5e-16, exp(-t^2) abs < 6e-16 and rel < 1e-12 for |t| < 4,
    odd / even symmetry exact, NaN -> NaN, erf(+-inf) = +-1 within the bound."""
    t, sub, e_ref, g_ref = erf_set()
    ops = np.concatenate([t, -t, [np.nan, np.inf, -np.inf]])
    e_all, g_all = device(ERF_TAB, ops), device(GAUSS_TAB, ops)
    n = t.size
    e, g = e_all[:n], g_all[:n]
    hold('erf_gauss_tab/erf_abs', np.abs(e[sub] - e_ref), 2.5e-16, t[sub], e[sub], e_ref, strict=True, unit='abs')
    hold('erf_gauss_tab/gauss_abs', np.abs(g[sub] - g_ref), 6e-16, t[sub], g[sub], g_ref, strict=True, unit='abs')
    inner = np.abs(t[sub]) < 4
    with np.errstate(all='ignore'):
        g_rel = np.abs(g[sub] - g_ref) / g_ref
    hold('erf_gauss_tab/gauss_rel_inside_4', g_rel[inner], 1e-12, t[sub][inner], g[sub][inner], g_ref[inner],
         strict=True, unit='rel')
    # the remaining random points against libm's erf / NumPy's exp, one ulp (of 1: 2.2e-16) looser
    rest = rest_of(n, sub)
    e_np = np.array([math.erf(v) for v in t[rest]])
    g_np = np.exp(-t[rest] * t[rest])
    hold('erf_gauss_tab/erf_abs_vs_libm', np.abs(e[rest] - e_np), 2.5e-16 + 2.2e-16, t[rest], e[rest], e_np, strict=True, unit='abs')
    hold('erf_gauss_tab/gauss_abs_vs_numpy', np.abs(g[rest] - g_np), 6e-16 + 2.2e-16, t[rest], g[rest], g_np, strict=True, unit='abs')
    assert np.array_equal(e_all[n:2 * n], -e) and np.array_equal(g_all[n:2 * n], g)          # odd / even exactly
    assert np.isnan(e_all[2 * n]) and np.isnan(g_all[2 * n])
    assert abs(e_all[2 * n + 1] - 1.0) < 2.5e-16 and abs(e_all[2 * n + 2] + 1.0) < 2.5e-16


@pytest.mark.gpu
@pytest.mark.parametrize('name,which', [('fast_log', FAST_LOG), ('band_log', BAND_LOG)])
def test_log_device(name, which):
    """<= 2 ulp where the reference is not 0 (denormal operands included: the kernels run with fp64 denormals on), log(1) == 0
    exactly, 0 -> -inf, negative -> NaN, NaN -> NaN, +inf -> +inf."""
    x, sub, ref = log_set()
    ops = np.concatenate([x, [0.0, -0.0, -1.0, -1e-310, np.nan, np.inf]])
    got_all = device(which, ops)
    got, tail = got_all[:x.size], got_all[x.size:]
    nz = ref != 0
    hold(name + '/ulp_vs_mpmath', ulps(got[sub][nz], ref[nz]), 2.0, x[sub][nz], got[sub][nz], ref[nz])
    assert np.all(got[x == 1.0] == 0.0) and (x == 1.0).sum() >= 2
    rest = rest_of(x.size, sub)
    nref = np.log(x[rest])
    hold(name + '/ulp_vs_numpy', ulps(got[rest], nref), 3.0, x[rest], got[rest], nref)
    assert tail[0] == -np.inf and tail[1] == -np.inf
    assert np.isnan(tail[2]) and np.isnan(tail[3]) and np.isnan(tail[4])
    assert tail[5] == np.inf


@pytest.mark.gpu
def test_rcp_device():
    """fast_rcp (v_rcp_f64 + two Newton steps): <= 1 ulp of 1/b; approx_rcp: relative error <= 2^-22, twice the 2^-23 the header
    says v_rcp_f64 delivers."""
    b, sub, ref = rcp_set()
    got = device(FAST_RCP, b)
    hold('fast_rcp/ulp_vs_mpmath', ulps(got[sub], ref), 1.0, b[sub], got[sub], ref)
    rest = rest_of(b.size, sub)
    hold('fast_rcp/ulp_vs_ieee', ulps(got[rest], 1.0 / b[rest]), 1.0, b[rest], got[rest], 1.0 / b[rest])
    record_parity('device_math/fast_rcp/correctly_rounded_share', float(np.mean(got == 1.0 / b)), None)
    apx = device(APPROX_RCP, b)
    hold('approx_rcp/rel', np.abs(apx * b - 1.0), 2.0 ** -22, b, apx, 1.0 / b, unit='rel')


@pytest.mark.gpu
@pytest.mark.parametrize('name,which,bound', [('fast_div', FAST_DIV, 1.0), ('band_div', BAND_DIV, 1.0), ('fast_div1', FAST_DIV1, 2.0)])
def test_div_device(name, which, bound):
    """a / b: fast_div and band_div <= 1 ulp, fast_div1 <= 2 ulp (the consumer tolerance its comment names); a = b, a = 0 and
    quotients near 2^+-500 included.  The share of correctly rounded quotients is recorded."""
    a, b, sub, ref = div_set()
    got = device(which, a, b)
    hold(name + '/ulp_vs_mpmath', ulps(got[sub], ref), bound, (a[sub], b[sub]), got[sub], ref)
    rest = rest_of(a.size, sub)
    hold(name + '/ulp_vs_ieee', ulps(got[rest], a[rest] / b[rest]), bound, (a[rest], b[rest]), got[rest], a[rest] / b[rest])
    record_parity('device_math/%s/correctly_rounded_share' % name, float(np.mean(got == a / b)), None)


@pytest.mark.gpu
def test_division_by_zero_inf_nan_is_not_finite():
    """band_div's stated contract - b = 0, infinite or NaN: not a finite quotient - for fast_div, band_div and fast_rcp."""
    a = np.array([1.5, 1.5, 1.5, 1.5, 1.5, -3.0, -3.0, -3.0])
    b = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -np.inf, np.nan])
    for name, got in (('fast_div', device(FAST_DIV, a, b)), ('band_div', device(BAND_DIV, a, b)), ('fast_rcp', device(FAST_RCP, b))):
        assert not np.any(np.isfinite(got)), '%s: finite result for a divisor in %r: %r' % (name, b, got)


DENSE_EXP_BOUND = 2.0


@pytest.mark.gpu
def test_dense_exp_core_device():
    """dense_exp_core (degree-11 near-minimax, coefficients g_exp11 from constant memory).  csrc/ttm_dense.h states no ulp bound
    (only 1.6e-17 for the polynomial in exact arithmetic), so the bound is max(2, ceil(measured) + 1) ulp against mpmath - the
    + 1 for operands the sample missed.  Measured on an MI355X over this operand set: 1 ulp (mpmath subsample and the NumPy
    remainder alike; the device result equals the host build's bit for bit on all 100 000 operands), hence DENSE_EXP_BOUND = 2."""
    y, sub, ref = dense_exp_set()
    got = device(DENSE_EXP_CORE, y)
    hold('dense_exp_core/ulp_vs_mpmath', ulps(got[sub], ref), DENSE_EXP_BOUND, y[sub], got[sub], ref)
    rest = rest_of(y.size, sub)
    hold('dense_exp_core/ulp_vs_numpy', ulps(got[rest], np.exp(y[rest])), DENSE_EXP_BOUND + 1.0, y[rest], got[rest], np.exp(y[rest]))


def band_expq_bound(x):
    """Generator geometry (tools/gen_band_etab.py): entries correctly rounded, degree-7 Taylor series in w,
    |w| <= w_max(x) = 0.01 (2 |x| + 0.01) / 4: relative error <= 1e-15 + 1.25 w_max^8 / 8!."""
    wmax = 0.01 * (2.0 * np.abs(x) + 0.01) / 4.0
    return 1e-15 + 1.25 * wmax ** 8 / math.factorial(8)


@pytest.mark.gpu
def test_band_expq_device():
    """band_expq (pair table staged by the forward kernels' loader, kt = g_band_taylor): relative error vs mpmath exp(-x^2/4)
    <= 1e-15 + 1.25 w_max(x)^8 / 8! for |x| <= 16 (1e-15 at |x| <= 5, 5.3e-14 at 16); beyond 16 and for NaN the value at 16 bit
    for bit; even in x exactly; band_expq_far equal for |x| <= 60 and exactly 0 beyond."""
    x, sub, ref = band_expq_set()
    ops = np.concatenate([x, -x])
    got_all = device(BAND_EXPQ, ops)
    got = got_all[:x.size]
    xs, gs = x[sub], got[sub]
    inside = np.abs(xs) <= 16.0                                             # (NaN: False)
    rel = np.abs(gs[inside] - ref[inside]) / ref[inside]
    hold('band_expq/rel_vs_mpmath', rel, band_expq_bound(xs[inside]), xs[inside], gs[inside], ref[inside], unit='rel')
    core = inside & (np.abs(xs) <= 5.0)
    hold('band_expq/rel_vs_mpmath_inside_5', np.abs(gs[core] - ref[core]) / ref[core], band_expq_bound(xs[core]), xs[core], gs[core],
         ref[core], unit='rel')
    # the remaining points against extended precision (the fp64 product x*x/4 alone would cost 64 ulp at 16), one ulp looser
    rest = rest_of(x.size, sub)
    if np.finfo(np.longdouble).eps < 2e-19:
        xl = x[rest].astype(np.longdouble)
        lref = np.exp(-(xl * xl) / 4)
        lrel = np.abs((got[rest].astype(np.longdouble) - lref) / lref).astype(float)
        hold('band_expq/rel_vs_long_double', lrel, band_expq_bound(x[rest]) + 2.3e-16, x[rest], got[rest], lref.astype(float), unit='rel')
    # held at 16 beyond the table and for NaN
    at16 = device(BAND_EXPQ, np.array([16.0]))[0]
    assert abs(at16 / math.exp(-64.0) - 1.0) < 5.4e-14
    beyond = ~(np.abs(x) <= 16.0)
    assert beyond.sum() >= 9
    assert np.all(got[beyond].view(np.uint64) == np.array([at16]).view(np.uint64)[0]), 'band_expq is not held at 16 beyond the table'
    assert np.array_equal(got_all[x.size:].view(np.uint64), got.view(np.uint64)), 'band_expq is not even in x'
    far = device(BAND_EXPQ_FAR, ops)
    gone = np.abs(ops) > 60.0                                               # (NaN: neither - the value at 16, as band_expq)
    assert np.array_equal(far[~gone].view(np.uint64), got_all[~gone].view(np.uint64))
    assert np.all(far[gone] == 0.0) and gone.sum() >= 8


# ---- GPU + CPU: the device build against the host build of the same source ---------------------------------------------------

def _ops_for(which):
    if which in (FAST_EXP, FAST_EXP_V2):
        return np.concatenate([exp_set()[0], [np.nan, -1e9, np.inf]]), None
    if which == EXP_Q_TAB:
        return np.concatenate([exp_q_set(3)[0], [np.nan, np.inf, -np.inf, 1e200]]), None
    if which in (EXP_Q_FAST, EXP_Q_FAST_V2):
        return np.concatenate([exp_q_set(4)[0], [np.nan, np.inf, -np.inf, 1e100, 100.0, -1e8]]), None
    if which in (ERF_TAB, GAUSS_TAB):
        return np.concatenate([erf_set()[0], [np.nan, np.inf, -np.inf]]), None
    if which == FAST_LOG:
        return np.concatenate([log_set()[0], [0.0, -1.0, np.nan, np.inf]]), None
    if which == FAST_RCP:
        return rcp_set()[0], None
    if which == FAST_DIV:
        return div_set()[0], div_set()[1]
    assert which == DENSE_EXP_CORE
    return dense_exp_set()[0], None


HOST_SERVED = {'fast_exp': FAST_EXP, 'erf_tab': ERF_TAB, 'gauss_tab': GAUSS_TAB, 'fast_log': FAST_LOG, 'fast_rcp': FAST_RCP,
               'fast_div': FAST_DIV, 'exp_q_tab': EXP_Q_TAB, 'exp_q_fast': EXP_Q_FAST, 'dense_exp_core': DENSE_EXP_CORE,
               'fast_exp_v2': FAST_EXP_V2, 'exp_q_fast_v2': EXP_Q_FAST_V2}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(HOST_SERVED))
def test_device_build_against_host_build(name):
    """Every id the host double serves, on its full operand set: device and host results differ by <= 1 ulp.  The number of
    elements that differ in any bit is recorded, not asserted (contraction may legitimately differ).  For fast_rcp / fast_div
    this holds the device branch against IEEE division on every point."""
    which = HOST_SERVED[name]
    a, b = _ops_for(which)
    d, h = device(which, a, b), host(which, a, b)
    hold('%s/ulp_device_vs_host' % name, ulps(d, h), 1.0, a if b is None else (a, b), d, h)
    same = (d.view(np.uint64) == h.view(np.uint64)) | (np.isnan(d) & np.isnan(h))
    record_parity('device_math/%s/bit_differences_device_vs_host' % name, float((~same).sum()), None)
    print('device_math/%s: %d of %d elements differ in some bit between device and host build' % (name, int((~same).sum()), a.size))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_header_ids_are_the_ones_used_here():
    ids = header_ids()
    mine = {k: v for k, v in globals().items() if k.upper() in ids and isinstance(v, int)}
    assert len(ids) == 18 and mine == ids


def test_host_probe_forwards_to_emu_math():
    """ttm_math_probe of the host double gives the values emu_math (what tests/test_math.py drives) gives, id for id."""
    rng = np.random.default_rng(7)
    a = np.concatenate([rng.uniform(-5, 5, 1001), [0.0, -0.0, np.nan, np.inf, -np.inf, 1e300, 1e-310]])
    b = np.concatenate([rng.standard_normal(1001), [3.0, -2.0, 1.0, 5.0, 7.0, 1e10, 1e-10]])
    for which in range(8):
        aa = np.abs(a) if which == FAST_LOG else a
        bb = b if which == FAST_DIV else None
        want = np.empty_like(aa)
        emu.lib().emu_math(which, emu.ptr(aa), emu.ptr(bb), ctypes.c_int64(aa.size), emu.ptr(want))
        got = host(which, aa, bb)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), which
    # the VecD<2> forms are the scalar ones element for element (odd n: the last element pairs with itself)
    assert a.size % 2 == 0
    for n in (a.size, a.size - 1, 1):
        assert np.array_equal(host(FAST_EXP_V2, a[:n]).view(np.uint64), host(FAST_EXP, a[:n]).view(np.uint64))
        assert np.array_equal(host(EXP_Q_FAST_V2, a[:n]).view(np.uint64), host(EXP_Q_FAST, a[:n]).view(np.uint64))
    y = rng.uniform(-700, 700, 2000)
    assert ulps(host(DENSE_EXP_CORE, y), np.exp(y)).max() <= 3.0


def test_host_probe_argument_checks():
    lib = emu.lib()
    a, out = np.ones(4), np.zeros(4)

    def call(which, a_, b_, n, out_):
        return lib.ttm_math_probe(which, emu.ptr(a_), emu.ptr(b_), ctypes.c_int64(n), emu.ptr(out_), None)
    for which in (BAND_EXPQ, BAND_EXPQ_SERIES, BAND_EXPQ_FAR, BAND_LOG):
        assert call(which, a, None, 4, out) == TTM_E_UNSUPPORTED
    assert call(BAND_DIV, a, a, 4, out) == TTM_E_UNSUPPORTED
    assert call(FAST_DIV1, a, a, 4, out) == TTM_E_UNSUPPORTED and call(APPROX_RCP, a, None, 4, out) == TTM_E_UNSUPPORTED
    for bad in (-1, 13, 31, 37, 1000):
        assert call(bad, a, a, 4, out) == TTM_E_ARG
    assert call(FAST_EXP, a, None, -1, out) == TTM_E_ARG
    assert call(FAST_DIV, a, None, 4, out) == TTM_E_ARG                    # b missing for a two-operand id
    assert call(BAND_DIV, a, None, 4, out) == TTM_E_ARG
    assert call(FAST_EXP, None, None, 4, out) == TTM_E_ARG and call(FAST_EXP, a, None, 4, None) == TTM_E_ARG
    assert np.all(out == 0.0)                                               # nothing was written by a refused call
    assert call(FAST_EXP, a, None, 0, out) == 0 and np.all(out == 0.0)     # n = 0: a no-op


@pytest.mark.gpu
def test_device_probe_argument_checks():
    """The device entry refuses the same calls with TTM_E_ARG without launching; n = 0 is a no-op."""
    import torch
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    a = torch.ones(4, dtype=torch.float64, device='cuda')
    out = torch.zeros(4, dtype=torch.float64, device='cuda')
    for bad in (-1, 13, 31, 37, 1000):
        assert lib.ttm_math_probe(bad, a.data_ptr(), a.data_ptr(), 4, out.data_ptr(), None) == TTM_E_ARG
    assert lib.ttm_math_probe(FAST_EXP, a.data_ptr(), None, -1, out.data_ptr(), None) == TTM_E_ARG
    for which in TWO_OPERANDS:
        assert lib.ttm_math_probe(which, a.data_ptr(), None, 4, out.data_ptr(), None) == TTM_E_ARG
    assert lib.ttm_math_probe(FAST_EXP, None, None, 4, out.data_ptr(), None) == TTM_E_ARG
    assert lib.ttm_math_probe(BAND_LOG, a.data_ptr(), None, 4, None, None) == TTM_E_ARG
    assert lib.ttm_math_probe(FAST_EXP, a.data_ptr(), None, 0, out.data_ptr(), None) == 0
    assert lib.ttm_math_probe(BAND_EXPQ, a.data_ptr(), None, 0, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 0.0)


def band_etab_header():
    text = open(os.path.join(ROOT, 'triangular_transport_toolbox_amd', 'csrc', 'ttm_band_etab.h')).read()
    macros = {name: float(val) for name, val in re.findall(r'#define TTM_BAND_ET_(N|STEP|INV_STEP|XMAX) (\S+)', text)}
    body = text[text.index('TTM_BAND_ETAB_VALUES') + len('TTM_BAND_ETAB_VALUES'):]
    vals = np.array([float.fromhex(tok) for tok in re.findall(r'-?0x[0-9a-f.]+p[+-]?\d+', body)])
    return macros, vals


def test_band_pair_table_is_correctly_rounded():
    """csrc/ttm_band_etab.h as text: 801 pairs {E_i, y_i / 4} with y_i = fl(i * 0.02), y_i / 4 exact and E_i = exp(-y_i^2 / 4)
    correctly rounded (what the bound of test_band_expq_device is derived from)."""
    macros, vals = band_etab_header()
    assert vals.size == 2 * 801 == 2 * int(macros['N'])
    E, yq = vals[0::2], vals[1::2]
    y = np.arange(801) * 0.02
    assert np.array_equal(yq * 4.0, y) and np.array_equal(yq, y / 4.0)
    mp.mp.dps = 40
    want = np.array([float(mp.exp(-mp.mpf(float(v)) ** 2 / 4)) for v in y])
    assert np.array_equal(E, want)


def test_band_pair_table_macros_are_consistent():
    macros, _ = band_etab_header()
    n, step, inv, xmax = int(macros['N']), macros['STEP'], macros['INV_STEP'], macros['XMAX']
    assert macros['N'] == n == 801
    assert step * inv == 1.0 and inv == round(inv)
    assert (n - 1) * step == xmax == (n - 1) / inv
    assert int(xmax * inv + 0.5) == n - 1                                  # band_expq's index at the clamp is the last pair
    assert int(np.nextafter(xmax, 0.0) * inv + 0.5) <= n - 1
