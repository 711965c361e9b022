"""
The kernels that differentiate a separable map - ttm_score (k_score_u, k_band_score) and ttm_pull_gradient (k_pull_gradient_u) -
and the forward values on the same rows, against the STORED section evaluated exactly (tests/uform_section.py, mpmath at us.DPS
digits).  tests/test_score.py, test_band_score.py and test_pull_gradient.py tie the stored section to the map by finite
differences of the oracle (1e-8 .. 1e-11); this file ties the kernels to the stored section at a few tens of 2^-53.  On the host
test double (u_score_row / u_pull_row through the host entry points of csrc/ttm_score.h and csrc/ttm_pull.h) and, marked `gpu`,
through each kernel by name (ttm_last_kernel).  k_band_score has no host double: hip only.

Reference (`reference`, built once per stored section and left unwritable; shared by every test; a backend whose ttm_fold writes
other bits than the host double's gets its own - the yardstick is what THAT section stores).  From the doubles of us.read(tm)
alone, per row u (standardised coordinates, every column) and component k with column c(k) = E + k, x = u_c(k):
    S_k   = c0 + sum_g f_g(u_var(g)) + m_k(x),           f = A + exp(-x^2/4) B,   m = own + P_col(s)
    J_kc  = f_g'(u_c) for the group g of k that reads the own column c,   J_kk = m_k'(x)
    m_k', m_k'' at u and at t_k = fl(a_k x + b_k) (ld_affine; the one fma both routines take it with - the correctly rounded
    value, formed here in mpmath and rounded once)
with the sums of |terms| of each, and from them the score G_c = -g_c sum_k S_k J_kc + m_c''(t_c) / m_c'(t_c) and, for the pull,
J and l_k = m_k''(u) / m_k'(u).  Nothing comes from the routines under test or from the oracle.  test_reference_pieces_are_exact
ties the piecewise assembly to us.exact.

The push records.  k_band_score, k_band_forward and k_band_few read the P section, not the group sets.
test_push_records_are_the_group_coefficients reads it back and asserts that every B[0..DB], A[1..DA] and the own slope is, bit for
bit, the group coefficient it stands for and that coefficients beyond the class degrees are zero.  The builder ROUNDS three things
of its own: the chain start [0] = c0 + sum_g A_g[0] (+ the own term's constant), summed in double; [2] = 1 - t_lo/h; and the
columns' local-coordinate offsets s0 = fl(2 sp_a - (2 col - 1)).  So this is the second case of the two: the yardstick of the band
kernels is built from the P numbers (us.read_push: chain start as stored, s = x sp_ds + s0 with s0 the stored double); the test
asserts that the chain start is the double sum in the builder's order and that s0 is the correctly rounded offset.

Bound: derived, per row and per output, from the reference's magnitudes; u = 2^-53.  Counts, statement by statement:
  Horner pass of degree n with fused multiply-adds: a term passes through at most n of them, whichever of the value / first /
  second derivative chains it sits in: n u sum |terms| for each of the three (u_poly, u_horner2, u_spline_d2, band_spline_d2,
  band_group_d alike - the fused passes of the push form do the same fmas in another interleaving).
  e_S   = u [(28 + n_groups) sum |terms| + (2 |u| + |s|) |P'(s)|] + sum_g dE_g |B_g|           (part B of tests/test_uform_spline.py)
  e_J   off the diagonal: u (n + C_g) sum |terms of f'| + dE |B' - x B / 2|, n = max(deg A, deg B);
          u_group_d: fma(-x/2, v, dv), e * (.), df += dv: C_g = 3;   band_group_d: fma(hx, b, db), fma(E, ., da): C_g = 2
  e_m'  = u [C_1 sum |terms of m'| + (2 |u| + |s|) |P''| sp_ds];   u_spline / u_spline_d2: 11 + (x sp_ds) + (dm += dg): C_1 = 13;
          k_band_score: 11 + fma(dm, sp_ds, own1): C_1 = 12
  e_m'' = u [C_2 sum |terms of m''| + (2 |u| + |s|) |P'''| sp_ds^2];   u_spline_d2: 11 + (sp_ds sp_ds) + (2 dda x .) + (d2m += d2g):
          C_2 = 14;   k_band_score: 11 + c2 = 2 (sp_ds sp_ds) + hd2 c2: C_2 = 13
  (the own term of every case is linear - asserted - so m', m'' carry no E term; s = fma(x, sp_ds, s0) rounds once, |s| u, within
  the local-coordinate term of part B, which is kept for both kernels)
  dE: exp_q_fast (u_score_row, u_pull_row, k_forward_u): (4 + x^2/4) u E - 2 ulp of exp of the rounded argument and the argument's
  rounding; band_expq (k_band_*): band_expq_bound(x) E up to |x| = 16, beyond it |E(16) - exp(-x^2/4)| by contract, E(16) within
  band_expq_bound(16) of exp(-64) (tests/test_device_math.py holds both).  The largest beyond-16 allowance relative to 1 + |G| is
  printed per case.  (k_band_few takes band_expq or the series of exp_q_fast's accuracy depending on the sweep: the forward
  families of the push form are allowed the larger of the two.)
  score:  g_c sum_k (e_S |J| + |S| e_J + e_S e_J + 3 u |S J|)      (-(g S) J: two products and the addition / one product and one fma)
        + D u (g_c sum_k |S J| + |q|)                              (the running sum of at most D + 1 terms from zero)
        + (e_m'' + |q| e_m') / (|m'| - e_m') + 2 u |q|             (the quotient at t; one ulp of fast_div / band_div)
  pull:   |sum_j J_ji W_j - (g_i G_i - [logdet] l_i)| <= sum_j (gamma_i |J_ji| + e_J,ji) |W_j| + gamma_i |rhs_i| + [logdet] e_l,i
          gamma_i = (n_open,i + 5) u: g_i G_i (1), one fma per open entry of column i (n_open,i), r -= l (1), the two divisions
          d2m / dm and r / dm at one ulp = 2 u each where the device's are not IEEE's (2, the first in e_l);
          e_l = (e_m'' + |l| e_m') / (|m'| - e_m') + 2 u |l|.
No constant is fitted to what the kernels return.  The reference asserts e_m' < |m'| / 2 at u and at t on every row it holds (a
seeded row that violates it - class_55 is not monotone everywhere - is redrawn from the same generator, in the reference, before
any routine runs; nothing is masked afterwards).

Rows (standardised coordinates; `reference`, `structured_rows`): at most N_SEEDED seeded rows with every column nonzero, and structured rows - a seeded
base row with one column replaced: the own column of every component (of {0, D // 2, D - 1} from D = 40 on) at every knot as the
double it is and its two neighbours, the interval midpoints, t_lo - 50 h, t_hi + 50 h and +-1e6 (exactly linear tail: m'' = 0 and the
quotient's bound is 0 - the launch with g_scale = 0 holds the quotient ALONE on every row, so there it must be exactly 0); a row
whose u is inside the support while t = a u + b is beyond it and one the other way round wherever the map's own (a, b) = (sigma,
mean) allow it (t = a u + b with a > 1 moves away from its fixed point -b / (a - 1): where that lies inside the support no u
beyond the support has its t inside; the SHRUNK call, a = 1/2, b = 0.1, has such rows for every component); every column a group
reads at +-0.0, a pair-table node 37 x 0.02 and its neighbours, 5, 15.99, 16, 16.01, 30, 60.01 and three of them negated.  Within
2^-40 of a knot either adjacent column is accepted (one choice for all outputs of the row).  N = the number of rows made odd; one
further launch repeats them cyclically to N = 4099 (the 1024- and 2048-row tiles of k_band_score), every copy held to the same
bound against the same reference.
"""
import ctypes
import dataclasses
import math

import mpmath as mp
import numpy as np
import pytest

from tests import pull_truth as pt
from tests import test_score as ts
from tests import uform_section as us
from tests.hostemu import emu
from tests.test_device_math import band_expq_bound
from tests.util import record_parity

CASES = ts.ALL_CASES + [pt.STD]
STD_CALL = ['c5_shape', 'few_c2b', 'dense_5']        # the standardised call (g_scale and ld_affine null) as well
SHRUNK_CALL = ['c5_shape', 'few_c2b']                # a call with ld_affine = (1/2, 0.1): u beyond the support, t inside
SHARP = ['few_c2b', 'c5_shape']
K0_CASE = 'c5_shape'
N_BUILD = 600
N_SEEDED = 120                                       # (at most 200)
N_CYCLIC = 4099
U = 2.0 ** -53
NEAR = mp.mpf(2) ** -40
C_U = dict(g=3, m1=13, m2=14)                        # u_score_row / u_pull_row (module docstring)
C_BAND = dict(g=2, m1=12, m2=13)                     # k_band_score
GROUP_POINTS = [0.0, -0.0, np.nextafter(37 * 0.02, 0.0), 37 * 0.02, np.nextafter(37 * 0.02, 1.0), 5.0, 15.99, 16.0, 16.01, 30.0,
                60.01, -5.0, -16.01, -60.01]


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


_MAPS = {}


def case(name, backend):
    """(tm, E, comps) of a case, built once per backend."""
    key = (name, backend)
    if key not in _MAPS:
        tm, om, X, E = pt.build(name) if name == pt.STD else ts.build(name, n=N_BUILD)
        assert tm._cm.u_enabled
        _MAPS[key] = (tm, E, us.read(tm))
    return _MAPS[key]


def affine_of(tm, E):
    """(g_scale, ld_affine) of the raw-coordinate call (evaluate_pullback_score): 1 / sigma, {sigma, mean} of the own columns."""
    std = np.asarray(tm.X_std, dtype=float)[E:E + tm.D]
    mean = np.asarray(tm.X_mean, dtype=float)[E:E + tm.D]
    return np.ascontiguousarray(1.0 / std), np.ascontiguousarray(np.column_stack((std, mean)))


def shrunk_affine(D):
    return np.column_stack((np.full(D, 0.5), np.full(D, 0.1)))


def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


# ---------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------

def components_held(comps):
    D = len(comps)
    return sorted({0, D // 2, D - 1}) if D >= 40 else list(range(D))


def seeded_row(rng, d):
    """One row with every column nonzero (|x| >= 1e-3)."""
    while True:
        row = 1.2 * rng.standard_normal(d)
        if np.all(np.abs(row) >= 1e-3):
            return row


def structured_rows(comps, d, E, base, affines):
    """The structured rows of the module docstring around the seeded row `base`; affines: the (a, b) arrays of the calls that take
    ld_affine, for the rows that put u and t on different sides of a support's end."""
    rows = []

    def put(col, x):
        r = base.copy()
        r[col] = x
        rows.append(r)
    read = set()
    for k in components_held(comps):
        c = comps[k]
        read.update(g.var for g in c.groups)
        if c.nI <= 0:
            for x in (-1e6, 1e6):
                put(c.kc, x)
            continue
        t_hi = c.t_lo + (c.nI - 2) * c.h
        for i in range(c.nI - 1):
            knot = c.t_lo + i * c.h
            for x in (np.nextafter(knot, -np.inf), knot, np.nextafter(knot, np.inf)):
                put(c.kc, x)
            if i < c.nI - 2:
                put(c.kc, c.t_lo + (i + 0.5) * c.h)
        for x in (c.t_lo - 50.0 * c.h, t_hi + 50.0 * c.h, -1e6, 1e6):
            put(c.kc, x)
        inside = lambda v: c.t_lo < v < t_hi                                      # noqa: E731
        for af in affines:
            a, b = float(af[k, 0]), float(af[k, 1])
            # u inside, t beyond / u beyond, t inside: a quarter interval from either end of the support, on either side of it
            cand = [c.t_lo + 0.25 * c.h, t_hi - 0.25 * c.h, c.t_lo - 0.25 * c.h, t_hi + 0.25 * c.h]
            cand += [(v - b) / a for v in (c.t_lo + 0.25 * c.h, t_hi - 0.25 * c.h, c.t_lo - 0.25 * c.h, t_hi + 0.25 * c.h)]
            for want_u in (True, False):
                for x in cand:
                    if inside(x) == want_u and inside(a * x + b) != want_u:
                        put(c.kc, x)
                        break
    for col in sorted(read):
        for x in GROUP_POINTS:
            put(col, x)
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------

_GROUP, _MONO = {}, {}


def group_at(g, x):
    """us.group_terms of a group without its constant A[0] (the push records keep it in the chain start: the two forms share the
    evaluation), memoised on the coefficients' bits."""
    if '_ckey' not in g.__dict__:
        g.__dict__['_ckey'] = (g.B.tobytes(), g.A[1:].tobytes())
    key = (g._ckey, float(x), math.copysign(1.0, float(x)))
    if key not in _GROUP:
        A = g.A.copy()
        A[0] = 0.0
        _GROUP[key] = us.group_terms(us.Group(g.var, g.flags, g.B, A), float(x))
    return _GROUP[key]


def mono_at(c, t, col=None):
    if '_ckey' not in c.__dict__:                        # (a component's numbers are never written after it is read)
        c.__dict__['_ckey'] = (c.table.tobytes() if c.nI > 0 else b'', c.sp_a, c.sp_ds, None if c.s0 is None else c.s0.tobytes(),
                               None if c.own is None else c.own.A.tobytes())
    key = (c._ckey, float(t), col)
    if key not in _MONO:
        _MONO[key] = us.monotone(c, t, col)
    return _MONO[key]


def mono_candidates(c, t):
    """The evaluations of the monotone part an evaluator may agree with at t: its own column, and within 2^-40 of a knot the
    adjacent one."""
    out = [mono_at(c, t)]
    if c.nI > 0:
        u = out[0]['u']
        near = mp.nint(u)
        if abs(u - near) <= NEAR and 0 <= near <= c.nI - 2:
            out += [mono_at(c, t, col) for col in (int(near), int(near) + 1) if col != out[0]['col']]
    return out


def e_fast(x, E):
    return (4.0 + 0.25 * x * x) * U * E


def e_band(x, E):
    """(allowance, the part of it that is the beyond-16 contract)."""
    if abs(x) <= 16.0:
        return float(band_expq_bound(x)) * E, 0.0
    e16 = math.exp(-64.0)
    far = abs(e16 - E) + float(band_expq_bound(16.0)) * e16
    return far, far


def fma_rounded(a, x, b):
    """fl(a x + b): the fma both routines form t with."""
    return float(mp.mpf(float(a)) * mp.mpf(float(x)) + mp.mpf(float(b)))


class Ref:
    """Arrays over V virtual rows (a row near a knot stands once per admissible column choice; real[v] is its row, and a row
    passes when one of its virtual rows does).  mp-valued arrays have dtype object."""


def evaluate(comps, rows, E, affines):
    """The reference of `rows` (R x d, standardised) from the components `comps` (us.read or us.read_push); affines: {call name:
    (D x 2) array or None (t = u)}.  Returns a Ref, or the index of the first row that violates e_m' < |m'| / 2 (at u or at a
    call's t) as an int."""
    D, R = len(comps), len(rows)
    recs, bases = [], {}
    with mp.workdps(us.DPS):
        for n in range(R):
            row = rows[n]
            per_k, variants = [], [[]]
            for k, c in enumerate(comps):
                assert c.own is None or (not (c.own.flags & us.PLAN_HF) and c.own.deg_a <= 1), 'own terms beyond a linear one'
                x = float(row[c.kc])
                bkey = (id(c), tuple(float(row[g.var]) for g in c.groups), tuple(math.copysign(1.0, row[g.var]) for g in c.groups))
                if bkey not in bases:                        # (the structured rows share all but one column)
                    gs = [group_at(g, float(row[g.var])) for g in c.groups]
                    a0 = sum((mp.mpf(float(g.A[0])) for g in c.groups), mp.mpf(0))
                    bases[bkey] = (gs, mp.mpf(c.c0) + a0 + sum((g['d'][0] for g in gs), mp.mpf(0)),
                                   abs(c.c0) + sum(abs(float(g.A[0])) for g in c.groups) + sum(g['mag'][0] for g in gs))
                gs, base, mag_base = bases[bkey]
                ts_ = {name: (x if af is None else fma_rounded(af[k, 0], x, af[k, 1])) for name, af in affines.items()}
                cu = mono_candidates(c, x)
                ct = {name: mono_candidates(c, t) for name, t in ts_.items()}
                per_k.append(dict(c=c, x=x, gs=gs, base=base, mag_base=mag_base, cu=cu, ct=ct))
                # (one admissible choice per evaluation point; a call whose t is x takes the choice made at u)
                choices = [[(k, iu, {name: it for name, it in zip(ct, its)})]
                           for iu in range(len(cu))
                           for its in _product([range(len(ct[name])) if affines[name] is not None else [None] for name in ct])]
                variants = [v + ch for v in variants for ch in choices]
            for var in variants:
                pick = {k: (iu, it) for k, iu, it in var}
                rec = _row_record(per_k, pick, row, D, E, affines)
                if rec is None:
                    return n
                rec['real'] = n
                recs.append(rec)
    return _stack(recs, comps, rows, D, E, affines)


def _product(lists):
    out = [[]]
    for lst in lists:
        out = [o + [v] for o in out for v in lst]
    return out


def _row_record(per_k, pick, row, D, E, affines):
    """One virtual row: the mp values and the float magnitudes of every piece (module docstring), or None where e_m' >= |m'| / 2."""
    rec = dict(S=[None] * D, magS=np.zeros(D), coordS=np.zeros(D), ngr=np.zeros(D), eb_fast=np.zeros(D), eb_band=np.zeros(D),
               eb_far=np.zeros(D), J=[[mp.mpf(0)] * D for _ in range(D)], st=np.zeros((D, D), dtype=bool), magJ=np.zeros((D, D)),
               degJ=np.zeros((D, D)), ej_fast=np.zeros((D, D)), ej_band=np.zeros((D, D)), ej_far=np.zeros((D, D)),
               m1=[None] * D, m2=[None] * D, mag1=np.zeros(D), mag2=np.zeros(D), coord1=np.zeros(D), coord2=np.zeros(D),
               t={name: dict(m1=[None] * D, m2=[None] * D, mag1=np.zeros(D), mag2=np.zeros(D), coord1=np.zeros(D), coord2=np.zeros(D))
                  for name in affines})
    for k, pk in enumerate(per_k):
        c = pk['c']
        iu, it = pick[k]
        mu = pk['cu'][iu]
        rec['S'][k] = pk['base'] + mu['d'][0]
        rec['magS'][k] = pk['mag_base'] + mu['mag'][0]
        rec['ngr'][k] = len(c.groups) + (1 if c.own is not None else 0)

        def fill(dst, m):
            coord = float(2 * abs(m['u']) + abs(m['s'])) if m['u'] is not None else 0.0
            ds = c.sp_ds
            dst['m1'][k], dst['m2'][k] = m['d'][1], m['d'][2]
            dst['mag1'][k], dst['mag2'][k] = float(m['mag'][1]), float(m['mag'][2])
            dst['coord1'][k] = coord * m['dP'][1] * ds
            dst['coord2'][k] = coord * m['dP'][2] * ds * ds
            e1 = U * (C_U['m1'] * dst['mag1'][k] + dst['coord1'][k])
            return e1 < 0.5 * abs(float(m['d'][1]))
        if not fill(rec, mu):
            return None
        rec['coordS'][k] = (float(2 * abs(mu['u']) + abs(mu['s'])) if mu['u'] is not None else 0.0) * mu['dP'][0]
        rec['J'][k][k], rec['st'][k, k] = mu['d'][1], True
        for name in affines:
            mt = mu if it[name] is None else pk['ct'][name][it[name]]
            if not fill(rec['t'][name], mt):
                return None
        for g, gt in zip(c.groups, pk['gs']):
            xg = float(row[g.var])
            Ef = float(gt['E'])
            eb, far = e_band(xg, Ef)
            wB, wB1 = float(gt['w'][0]), float(gt['w'][1])
            rec['eb_fast'][k] += e_fast(xg, Ef) * wB
            rec['eb_band'][k] += eb * wB
            rec['eb_far'][k] += far * wB
            j = g.var - E
            if j >= 0:
                rec['J'][k][j] += gt['d'][1]                 # (one group per column in these maps; += keeps a second one right)
                rec['st'][k, j] = True
                rec['magJ'][k, j] += float(gt['mag'][1])
                rec['degJ'][k, j] = max(rec['degJ'][k, j], max(gt['deg']))
                rec['ej_fast'][k, j] += e_fast(xg, Ef) * wB1
                rec['ej_band'][k, j] += eb * wB1
                rec['ej_far'][k, j] += far * wB1
    return rec


def _stack(recs, comps, rows, D, E, affines):
    ref = Ref()
    ref.D, ref.E, ref.R, ref.V = D, E, len(rows), len(recs)
    ref.rows = np.array(rows, dtype=float)
    ref.real = np.array([r['real'] for r in recs])
    obj = lambda f: np.array([f(r) for r in recs], dtype=object).reshape((len(recs),) + np.shape(f(recs[0])))     # noqa: E731
    flt = lambda key: np.array([r[key] for r in recs], dtype=float)                                                # noqa: E731
    ref.S, ref.J = obj(lambda r: r['S']), obj(lambda r: r['J'])
    ref.m1, ref.m2 = obj(lambda r: r['m1']), obj(lambda r: r['m2'])
    for key in ('magS', 'coordS', 'ngr', 'eb_fast', 'eb_band', 'eb_far', 'magJ', 'degJ', 'ej_fast', 'ej_band', 'ej_far', 'mag1', 'mag2',
                'coord1', 'coord2'):
        setattr(ref, key, flt(key))
    ref.st = np.array([r['st'] for r in recs])
    ref.t = {}
    for name in affines:
        t = Ref()
        t.m1, t.m2 = obj(lambda r: r['t'][name]['m1']), obj(lambda r: r['t'][name]['m2'])
        for key in ('mag1', 'mag2', 'coord1', 'coord2'):
            setattr(t, key, np.array([r['t'][name][key] for r in recs], dtype=float))
        with mp.workdps(us.DPS):
            t.q = t.m2 / t.m1
        ref.t[name] = t
    with mp.workdps(us.DPS):
        ref.l = ref.m2 / ref.m1
    with mp.workdps(us.DPS):
        ref.SJ = (ref.S[:, :, None] * ref.J).sum(axis=1)                          # sum_k S_k J_kc
    ref.absS = np.abs(ref.S).astype(float)
    ref.absJ = np.abs(ref.J).astype(float)
    for a in vars(ref).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


_REF = {}


def calls_of(name, tm, E):
    """{call: (g_scale or None, ld_affine or None)} of a case: raw coordinates always, the standardised and the shrunk call where
    listed."""
    gs, af = affine_of(tm, E)
    calls = {'raw': (gs, af)}
    if name in STD_CALL:
        calls['std'] = (None, None)
    if name in SHRUNK_CALL:
        calls['shrunk'] = (gs, shrunk_affine(tm.D))
    return calls


def reference(name, tm, E, comps, form='u'):
    """The reference of a case for the section `comps` was read from: (Ref, rows).  form 'u': the group sets (u_score_row,
    u_pull_row, k_forward_u); 'p': the push records (k_band_*).  Rows are drawn once per case (from the group-set form, with the
    redraws its condition asks for) and shared by both forms and both backends."""
    calls = calls_of(name, tm, E)
    affines = {c: af for c, (gs, af) in calls.items()}
    d = tm._cm.d_cols
    sig = b''.join(np.ascontiguousarray(a).tobytes() for c in comps for a in ([c.c0, c.sp_a, c.sp_ds], c.table, *[g.B for g in c.groups], *[g.A for g in c.groups]))
    key = (name, form, hash(sig))
    if key in _REF:
        return _REF[key]
    rows_key = (name, 'rows')
    if rows_key not in _REF:
        rng = np.random.default_rng(sum(map(ord, name)))
        base = seeded_row(rng, d)
        rows = structured_rows(comps, d, E, base, [af for af in affines.values() if af is not None])
        bad = evaluate(comps, rows, E, affines)
        assert not isinstance(bad, int), '%s: structured row %d (%r) has e_m\' >= |m\'| / 2' % (name, bad, rows[bad])
        seeded, redrawn = [], 0
        while len(seeded) < N_SEEDED or (len(seeded) + len(rows)) % 2 == 0:
            r = seeded_row(rng, d)
            if isinstance(evaluate(comps, [r], E, affines), int):
                redrawn += 1                                 # (the next draw of the same generator takes its place)
                continue
            seeded.append(r)
        print('%s: %d seeded rows (%d redrawn: e_m\' >= |m\'| / 2), %d structured rows' % (name, len(seeded), redrawn, len(rows)))
        allrows = np.array(seeded + rows)
        allrows.setflags(write=False)
        _REF[rows_key] = allrows
    rows = _REF[rows_key]
    assert len(rows) % 2 == 1 and len(rows) < N_CYCLIC
    ref = evaluate(comps, list(rows), E, affines)
    assert not isinstance(ref, int), '%s (%s): row %d has e_m\' >= |m\'| / 2 - no row is left out' % (name, form, ref)
    assert ref.R == len(rows) and set(ref.real) == set(range(len(rows)))
    _REF[key] = (ref, rows)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------
# bounds and checks
# ---------------------------------------------------------------------------------------------------------------------------

def errors_of(ref, cnt, etype):
    """(e_S [V, D], e_J [V, D, D] with e_m' at u on the diagonal, e_far [V, D], [V, D, D]: the beyond-16 share)."""
    eb, ej = (ref.eb_fast, ref.ej_fast) if etype == 'fast' else ((ref.eb_band, ref.ej_band) if etype == 'band' else
                                                                   (np.maximum(ref.eb_fast, ref.eb_band), np.maximum(ref.ej_fast, ref.ej_band)))
    e_S = U * ((28.0 + ref.ngr) * ref.magS + ref.coordS) + eb
    e_J = U * (ref.degJ + cnt['g']) * ref.magJ + ej
    e_m1 = U * (cnt['m1'] * ref.mag1 + ref.coord1)
    idx = np.arange(ref.D)
    e_J = e_J.copy()
    e_J[:, idx, idx] = e_m1
    far = etype != 'fast'
    return e_S, e_J, (ref.eb_far if far else 0.0 * ref.eb_far), (ref.ej_far if far else 0.0 * ref.ej_far)


def quotient_bound(tref, cnt):
    """(q as floats' magnitude, e_q = (e_m'' + |q| e_m') / (|m'| - e_m') + 2 u |q|) of the quotient m'' / m' at a call's t."""
    e1 = U * (cnt['m1'] * tref.mag1 + tref.coord1)
    e2 = U * (cnt['m2'] * tref.mag2 + tref.coord2)
    aq = np.abs(tref.q).astype(float)
    am1 = np.abs(tref.m1).astype(float)
    assert np.all(e1 < 0.5 * am1)
    return aq, (e2 + aq * e1) / (am1 - e1) + 2.0 * U * aq


def worst_over_rows(ratio, real, R):
    """max over the rows of the min over a row's virtual rows of the max over its outputs."""
    per_v = ratio.reshape(len(ratio), -1).max(axis=1)
    per_r = np.full(R, np.inf)
    np.minimum.at(per_r, real, per_v)
    return per_r


def to_mp(a):
    return np.array([mp.mpf(float(v)) for v in np.ravel(a)], dtype=object).reshape(np.shape(a))


def check_score(label, ref, call, gs, G, cnt, etype, comps_ref=None):
    """G (N x D, N = R or N_CYCLIC: the rows repeated cyclically) against the exact score of the call at the bound of the module
    docstring; returns the largest error / bound.  Prints every figure before it is held."""
    D, R = ref.D, ref.R
    tref = ref.t[call]
    g = np.ones(D) if gs is None else np.asarray(gs, dtype=float)
    e_S, e_J, far_S, far_J = errors_of(ref, cnt, etype)
    aq, e_q = quotient_bound(tref, cnt)
    with mp.workdps(us.DPS):
        Gref = -to_mp(g)[None, :] * ref.SJ + tref.q
    aSJ = ref.absS[:, :, None] * ref.absJ
    st = ref.st
    gauss = g[None, :] * np.sum(np.where(st, e_S[:, :, None] * ref.absJ + ref.absS[:, :, None] * e_J + e_S[:, :, None] * e_J + 3.0 * U * aSJ, 0.0), axis=1)
    acc = D * U * (g[None, :] * aSJ.sum(axis=1) + aq)
    bound = gauss + acc + e_q
    far = g[None, :] * np.sum(np.where(st, far_S[:, :, None] * ref.absJ + ref.absS[:, :, None] * far_J, 0.0), axis=1)
    aG = np.abs(Gref).astype(float)
    far_rel = float(np.max(far / (1.0 + aG)))
    worst = inside = 0.0
    near16 = far.max(axis=1) == 0.0                                               # virtual rows with every group column within 16
    N = G.shape[0]
    assert N in (R, N_CYCLIC) and np.all(np.isfinite(G))
    for m in range(-(-N // R)):
        take = ref.real + m * R < N
        Gm = G[(ref.real + m * R)[take]]
        with mp.workdps(us.DPS):
            err = np.abs(to_mp(Gm) - Gref[take]).astype(float)
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio = np.where(err == 0.0, 0.0, err / bound[take])
        per_r = worst_over_rows(ratio, ref.real[take], R)
        present = np.bincount(ref.real[take], minlength=R) > 0                   # (the last copy of a cyclic launch is cut short)
        worst = max(worst, float(per_r[present].max()))
        inside = max(inside, float(worst_over_rows(np.where(near16[take][:, None], ratio, 0.0), ref.real[take], R)[present].max()))
    print('%s: N %d, %d rows (%d with a column choice), error / bound %.3f (rows within 16: %.3f), beyond-16 allowance / (1 + |G|) %.3e, max bound / (1 + |G|) %.3e'
          % (label, N, R, ref.V - R, worst, inside, far_rel, float(np.max(bound / (1.0 + aG)))))
    return worst


def hold(key, worst):
    record_parity('score_exact/' + key, worst, 1.0)
    assert worst <= 1.0, 'score_exact/%s: error / bound %.3f' % (key, worst)


def device_rows(tm, rows, N):
    """The rows, repeated cyclically to N, as the standardised column-major matrix the entry points take."""
    R, d = rows.shape
    Xh = np.zeros((d, tm._ld(N)))
    Xh[:, :N] = rows[np.arange(N) % R].T
    return tm._to_dev(Xh)


def run_score(tm, Xd, N, gs, af):
    G = tm.score_device(Xd, N, g_scale=None if gs is None else tm._to_dev(gs), ld_affine=None if af is None else tm._to_dev(af))
    return G[:, :N].cpu().numpy().T.copy()


def score_suite(name, tm, E, ref, rows, backend, kernel, cnt, etype):
    """Every call of a case through the routine in place: the call itself, the same call with g_scale = 0 (the quotient alone) and,
    on the device, the raw call on the rows repeated to N_CYCLIC."""
    R = len(rows)
    Xd = device_rows(tm, rows, R)
    fails = []
    for call, (gs, af) in calls_of(name, tm, E).items():
        launches = [(call, gs, R, Xd)]
        if gs is not None:
            launches.append((call + '_g0', np.zeros(tm.D), R, Xd))
        if backend == 'hip' and call == 'raw':
            launches.append((call + '_cyclic', gs, N_CYCLIC, device_rows(tm, rows, N_CYCLIC)))
        for label, g, N, X in launches:
            G = run_score(tm, X, N, g, af)
            if backend == 'hip':
                assert last_kernel(tm) == kernel, (label, last_kernel(tm))
            worst = check_score('%s %s %s' % (kernel, name, label), ref, call, g, G, cnt, etype)
            try:
                hold('%s/%s/%s' % (kernel, name, label), worst)
            except AssertionError as err:
                fails.append(str(err))
    assert not fails, fails


def check_pull(label, ref, k0, gs, logdet, Gin, W, cnt):
    """The residual of W against the exact J (module docstring); returns the largest residual / bound."""
    D = ref.D
    e_S, e_J, _, _ = errors_of(ref, cnt, 'fast')
    lref = Ref()
    lref.m1, lref.m2, lref.mag1, lref.mag2, lref.coord1, lref.coord2, lref.q = ref.m1, ref.m2, ref.mag1, ref.mag2, ref.coord1, ref.coord2, ref.l
    al, e_l = quotient_bound(lref, cnt)
    g = np.ones(D - k0) if gs is None else np.asarray(gs, dtype=float)
    Wv, Gv = W[ref.real], Gin[ref.real]
    assert np.all(np.isfinite(W))
    with mp.workdps(us.DPS):
        J = ref.J[:, k0:, k0:]                                                    # [V, j, i]
        rhs = to_mp(g)[None, :] * to_mp(Gv) - (ref.l[:, k0:] if logdet else 0)
        res = np.abs((J * to_mp(Wv)[:, :, None]).sum(axis=1) - rhs).astype(float)
        arhs = np.abs(rhs).astype(float)
    st = ref.st[:, k0:, k0:]
    n_open = st.sum(axis=1) - 1                                                   # entries of column i below the diagonal
    gamma = (n_open + 5.0) * U
    aW = np.abs(Wv)
    bound = np.sum(np.where(st, (gamma[:, None, :] * ref.absJ[:, k0:, k0:] + e_J[:, k0:, k0:]) * aW[:, :, None], 0.0), axis=1) + gamma * arhs
    if logdet:
        bound = bound + e_l[:, k0:]
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(res == 0.0, 0.0, res / bound)
    per_r = worst_over_rows(ratio, ref.real, ref.R)
    worst = float(per_r.max())
    print('%s: %d rows, residual / bound %.3f' % (label, ref.R, worst))
    return worst


def pull_inputs(name, R, D):
    return np.random.default_rng(7 + sum(map(ord, name))).standard_normal((R, D))


def run_pull(tm, Xd, N, Gin, E, k0, gs, logdet):
    Gh = np.zeros((tm.D - k0, tm._ld(N)))
    Gh[:, :N] = Gin[:, k0:].T
    W = tm.pull_gradient_device(Xd, N, tm._to_dev(Gh), k0=k0, g_scale=None if gs is None else tm._to_dev(gs), logdet=logdet)
    return W[:, :N].cpu().numpy().T.copy()


# ---------------------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['few_c2b', 'few_cond', 'long_own'])
def test_reference_pieces_are_exact(name):
    """The piecewise assembly of the reference (group_terms + monotone) is us.exact's S, dS/dx and d2S/dx2 with `others` = the row,
    to the working precision; the sums of |terms| agree; a group's derivative is the difference quotient of its value."""
    with emu.install():
        tm, E, comps = case(name, 'hostemu')
        rng = np.random.default_rng(5)
        with mp.workdps(us.DPS):
            for _ in range(5):
                row = seeded_row(rng, tm._cm.d_cols)
                for c in comps:
                    ex = us.exact(c, row[c.kc], others={g.var: row[g.var] for g in c.groups})
                    m = us.monotone(c, row[c.kc])
                    gs = [us.group_terms(g, row[g.var]) for g in c.groups]
                    S = mp.mpf(c.c0) + sum((g['d'][0] for g in gs), mp.mpf(0)) + m['d'][0]
                    tol = mp.mpf(10) ** (5 - us.DPS) * (1 + ex['mag'])
                    assert abs(S - ex['value']) <= tol and abs(m['d'][1] - ex['d1']) <= tol * (1 + ex['mag1']) and abs(m['d'][2] - ex['d2']) <= tol * (1 + abs(ex['d2']))
                    assert abs(abs(c.c0) + sum(g['mag'][0] for g in gs) + m['mag'][0] - ex['mag']) <= 1e-13 * ex['mag']
                    assert abs(m['mag'][1] - ex['mag1']) <= 1e-13 * ex['mag1']
                    for g, gt in zip(c.groups, gs):
                        hq = mp.mpf(10) ** -12
                        x = mp.mpf(float(row[g.var]))
                        fd = [(us._group_value(g, x + hq)[0][r] - us._group_value(g, x - hq)[0][r]) / (2 * hq) for r in (0, 1)]
                        assert abs(fd[0] - gt['d'][1]) <= mp.mpf(10) ** -18 * (1 + gt['mag'][2]) * 10
                        assert abs(fd[1] - gt['d'][2]) <= mp.mpf(10) ** -18 * (1 + gt['mag'][2]) * 1e4
                        assert all(gt['mag'][r] * (1 + 1e-13) >= abs(gt['d'][r]) for r in range(3))
                        _, m0, m1 = us._group_value(g, x)
                        assert abs(gt['mag'][0] - m0) <= 1e-13 * m0 and abs(gt['mag'][1] - m1) <= 1e-13 * m1


@pytest.mark.parametrize('name', CASES)
def test_score_against_the_stored_section(backend, name, ttm_opt):
    """u_score_row on the host double / k_score_u on the device, every call of the case."""
    tm, E, comps = case(name, backend)
    ref, rows = reference(name, tm, E, comps)
    if backend == 'hip':
        ttm_opt('band_score', 0)
    score_suite(name, tm, E, ref, rows, backend, 'k_score_u' if backend == 'hip' else 'u_score_row', C_U, 'fast')


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in CASES if n != ts.DENSE])
def test_push_form_score_against_the_push_records(name, ttm_opt):
    """k_band_score against the push records evaluated exactly (every banded case; dense_5 has no push records)."""
    tm, E, comps = case(name, 'hip')
    assert tm._cm.u_p_lag > 0
    reference(name, tm, E, comps)                                                 # (the rows: drawn from the group-set form)
    P, push = us.read_push(tm, comps)
    ref, rows = reference(name, tm, E, push, form='p')
    ttm_opt('band_score', -1)
    score_suite(name, tm, E, ref, rows, 'hip', 'k_band_score', C_BAND, 'band')


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n in CASES if n != ts.DENSE])
def test_push_records_are_the_group_coefficients(name):
    """Second case of the two (module docstring): every coefficient of the P section is bit for bit the group coefficient it stands
    for; the chain start, 1 - t_lo/h and the columns' offsets are the builder's own roundings, checked to be exactly those."""
    from fractions import Fraction
    from triangular_transport_toolbox_amd import termtable
    tm, E, comps = case(name, 'hip')
    cm = tm._cm
    P, push = us.read_push(tm, comps)
    lag, cls = int(cm.u_p_lag), int(cm.u_h_cls)
    DB, DA = termtable.H_DB[cls], termtable.H_DA[cls]
    GP = DB + 1 + DA
    bits = lambda a: np.ascontiguousarray(a, dtype=float).view(np.uint64)         # noqa: E731
    used = np.zeros(P.shape, dtype=bool)
    for k, (c, p) in enumerate(zip(comps, push)):
        start = np.float64(c.c0)
        for g, gp in zip(c.groups, p.groups):
            assert np.array_equal(bits(gp.B[:DB + 1]), bits(g.B[:DB + 1])) and np.all(g.B[DB + 1:] == 0.0), (k, g.var)
            assert np.array_equal(bits(gp.A[1:DA + 1]), bits(g.A[1:DA + 1])) and np.all(g.A[DA + 1:] == 0.0), (k, g.var)
            assert bool(g.flags & us.PLAN_HF) or np.all(g.B == 0.0)
            start = start + np.float64(g.A[0])                                    # (uform_scatter_push_records: in the groups' order)
            lg = c.kc - g.var
            used[k - lg + lag, termtable.P_HDR + (lg - 1) * GP:termtable.P_HDR + lg * GP] = True
        if c.own is not None:
            assert not (c.own.flags & us.PLAN_HF) and np.all(c.own.A[2:] == 0.0)
            start = start + np.float64(c.own.A[0])
            assert bits(P[k + lag, 7]) == bits(c.own.A[1])
        else:
            assert P[k + lag, 7] == 0.0
        assert bits(P[k, 0]) == bits(start), (k, P[k, 0], start)
        rec = P[k + lag]
        if c.nI > 0:
            assert bits(rec[2]) == bits(np.float64(c.sp_a) + 1.0) and bits(rec[3]) == bits(c.sp_b) and bits(rec[4]) == bits(c.sp_ds)
            for col in range(c.nI):
                assert p.s0[col] == float(2 * Fraction(c.sp_a) - (2 * col - 1)), (k, col)
        ni_tab = rec[5:6].view(np.int32)
        assert int(ni_tab[0]) == c.nI and (c.nI == 0 or int(ni_tab[1]) == c.tab_off)
        assert int(rec[6:7].view(np.int32)[0]) == k
    blocks = np.zeros(P.shape, dtype=bool)
    blocks[:, termtable.P_HDR:termtable.P_HDR + lag * GP] = True
    assert np.all(P[blocks & ~used] == 0.0), 'a group block that stands for no group is not zero'


@pytest.mark.parametrize('name', CASES)
def test_pull_against_the_stored_section(backend, name):
    """u_pull_row / k_pull_gradient_u: logdet 0 and 1, g_scale on and off; K0_CASE also from k0 = 2."""
    tm, E, comps = case(name, backend)
    ref, rows = reference(name, tm, E, comps)
    R, D = len(rows), tm.D
    Xd = device_rows(tm, rows, R)
    Gin = pull_inputs(name, R, D)
    sigma = np.asarray(tm.X_std, dtype=float)[E:E + D]
    fails = []
    for k0 in ((0, 2) if name == K0_CASE else (0,)):
        for logdet in (False, True):
            for gs in (sigma[k0:], None):
                W = np.zeros((R, D))
                W[:, k0:] = run_pull(tm, Xd, R, Gin, E, k0, gs, logdet)
                if backend == 'hip':
                    assert last_kernel(tm) == 'k_pull_gradient_u'
                kernel = 'k_pull_gradient_u' if backend == 'hip' else 'u_pull_row'
                label = 'k0_%d_logdet_%d_gscale_%d' % (k0, logdet, gs is not None)
                worst = check_pull('%s %s %s' % (kernel, name, label), ref, k0, gs, logdet, Gin[:, k0:], W[:, k0:], C_U)
                try:
                    hold('%s/%s/%s' % (kernel, name, label), worst)
                except AssertionError as err:
                    fails.append(str(err))
    assert not fails, fails


FAMILIES = {
    'k_forward_u': (dict(band_fwd=0, u_no_hot=1, u_loader=0), ('k_forward_u',), 'u', 'fast'),
    'k_band': (dict(band_fwd=1, u_loader=1), ('k_band_forward', 'k_band_few'), 'p', 'either'),
}


def check_forward(label, ref, Z, etype):
    e_S, _, far_S, _ = errors_of(ref, C_U, etype)
    with mp.workdps(us.DPS):
        err = np.abs(to_mp(Z[ref.real]) - ref.S).astype(float)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0.0, 0.0, err / e_S)
    worst = float(worst_over_rows(ratio, ref.real, ref.R).max())
    inside = float(worst_over_rows(np.where((far_S.max(axis=1) == 0.0)[:, None], ratio, 0.0), ref.real, ref.R).max())
    print('%s: %d rows, error / bound %.3f (rows within 16: %.3f), beyond-16 allowance / (1 + |S|) %.3e'
          % (label, ref.R, worst, inside, float(np.max(far_S / (1.0 + ref.absS)))))
    return worst


def run_forward(tm, Xd, N):
    Z = tm.forward_device(Xd, N, Z=tm._cols(tm.D, N, zero=True))
    return Z[:, :N].cpu().numpy().T.copy()


@pytest.mark.parametrize('name', CASES)
def test_forward_values_on_the_same_rows_on_the_host_double(name):
    with emu.install():
        tm, E, comps = case(name, 'hostemu')
        ref, rows = reference(name, tm, E, comps)
        Z = run_forward(tm, device_rows(tm, rows, len(rows)), len(rows))
        hold('u_component/%s/forward' % name, check_forward('u_component %s' % name, ref, Z, 'fast'))


@pytest.mark.gpu
@pytest.mark.parametrize('family', sorted(FAMILIES))
@pytest.mark.parametrize('name', CASES)
def test_forward_families_on_the_same_rows(name, family, ttm_opt):
    """Z of ttm_forward against the exact S with every column off zero: k_forward_u against the group sets, k_band_forward /
    k_band_few against the push records - a failing score is S's or J's, and part B's "other columns 0" is closed."""
    tm, E, comps = case(name, 'hip')
    opts, names, form, etype = FAMILIES[family]
    if form == 'p' and tm._cm.u_p_lag == 0:
        pytest.skip('%s is not banded: it has no push records, k_band_* cannot be reached' % name)
    ref, rows = reference(name, tm, E, comps)
    if form == 'p':
        ref, rows = reference(name, tm, E, us.read_push(tm, comps)[1], form='p')
    for key, value in opts.items():
        ttm_opt(key, value)
    Z = run_forward(tm, device_rows(tm, rows, len(rows)), len(rows))
    kernel = last_kernel(tm)
    assert kernel in names, (family, kernel)
    hold('%s/%s/forward' % (kernel, name), check_forward('%s %s' % (kernel, name), ref, Z, etype))


def perturbed(comps, what):
    """A copy of the section with ONE number multiplied by 1 + 2^-40: 'c1' the slope coefficient of the spline column of the last
    component that holds t = 0.1, 'B' the largest B coefficient of the last component's first group, 'sp_ds' the last
    component's 2 / h."""
    f = 1.0 + 2.0 ** -40
    out = list(comps)
    k = len(comps) - 1
    c = comps[k]
    assert c.nI > 0 and c.groups
    if what == 'c1':
        col = us.column_of(c, 0.1)[0]
        table = c.table.copy()
        assert table[col, 1] != 0.0
        table[col, 1] *= f
        out[k] = dataclasses.replace(c, table=table)
    elif what == 'B':
        g = c.groups[0]
        B = g.B.copy()
        j = int(np.argmax(np.abs(B)))
        assert B[j] != 0.0
        B[j] *= f
        out[k] = dataclasses.replace(c, groups=[us.Group(g.var, g.flags, B, g.A)] + c.groups[1:])
    else:
        assert what == 'sp_ds'
        out[k] = dataclasses.replace(c, sp_ds=c.sp_ds * f)
    return out


@pytest.mark.parametrize('what', ['c1', 'B', 'sp_ds'])
@pytest.mark.parametrize('name', SHARP)
def test_the_yardstick_is_sharp(name, what):
    """A reference evaluated from a section with one number off by 2^-40 puts the UNPERTURBED routine beyond the bound on at least
    one row, for the score and for the pull: the bound is no wider than 2^-40 of a single stored number."""
    with emu.install():
        tm, E, comps = case(name, 'hostemu')
        _, rows = reference(name, tm, E, comps)
        D = tm.D
        c = comps[-1]
        # the seeded rows, and the last component's own column across the spline column the perturbed slope belongs to
        sub = [r for r in rows[:N_SEEDED]]
        base = rows[0]
        for x in np.linspace(0.0, 1.0, 9)[1:-1]:
            r = base.copy()
            col = us.column_of(c, 0.1)[0]
            r[c.kc] = c.t_lo + (col - 1 + x) * c.h
            sub.append(r)
        sub = np.array(sub)
        gs, af = affine_of(tm, E)
        ref0 = evaluate(comps, list(sub), E, {'raw': af})
        ref1 = evaluate(perturbed(comps, what), list(sub), E, {'raw': af})
        assert not isinstance(ref0, int) and not isinstance(ref1, int)
        R = len(sub)
        Xd = device_rows(tm, sub, R)
        G = run_score(tm, Xd, R, gs, af)
        Gin = pull_inputs(name, R, D)
        sigma = np.asarray(tm.X_std, dtype=float)[E:E + D]
        W = run_pull(tm, Xd, R, Gin, E, 0, sigma, True)
        s0 = check_score('%s unperturbed score' % name, ref0, 'raw', gs, G, C_U, 'fast')
        s1 = check_score('%s %s x (1 + 2^-40) score' % (name, what), ref1, 'raw', gs, G, C_U, 'fast')
        p0 = check_pull('%s unperturbed pull' % name, ref0, 0, sigma, True, Gin, W, C_U)
        p1 = check_pull('%s %s x (1 + 2^-40) pull' % (name, what), ref1, 0, sigma, True, Gin, W, C_U)
        record_parity('score_exact/sharpness/%s/%s/score' % (name, what), s1, None)
        record_parity('score_exact/sharpness/%s/%s/pull' % (name, what), p1, None)
        assert s0 <= 1.0 and p0 <= 1.0
        assert s1 > 1.0, 'the score\'s bound does not see %s off by 2^-40 (error / bound %.3f)' % (what, s1)
        assert p1 > 1.0, 'the pull\'s bound does not see %s off by 2^-40 (residual / bound %.3f)' % (what, p1)
