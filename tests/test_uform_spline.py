"""
The special-term splines of the U section (csrc/ttm_uform.h) against the map's definition in mpmath: value,
slope and curvature of what ttm_fold stores (part A), and the evaluators at the seams of that section (part B).  On the host test
double and, marked `gpu`, on what the device built and through each kernel family by name.

Reference (`reference(name)`, built once per case, shared by every test and both backends, left unchanged).  For component k
the oracle's monotone term list (om.plan_mon[k], om._st_params, om.coeffs_mon[k]) is summed at 40 digits with d = t - mu,
z = d / (sqrt2 sigma), phi = exp(-z^2) / (sqrt(2 pi) sigma):

    LET   (d (1 - erf z) - sigma sqrt(2/pi) exp(-z^2)) / 2     (1 - erf z) / 2      -phi
    RET   (d (1 + erf z) + sigma sqrt(2/pi) exp(-z^2)) / 2     (1 + erf z) / 2      +phi
    RBF   phi                                                  -d / sigma^2 phi     (d^2 / sigma^4 - 1 / sigma^2) phi
    iRBF  (1 + erf z) / 2                                      phi                  -d / sigma^2 phi

(the formulas of oracle/ttm_oracle.py::_factor; nothing comes from the fold's records or from u_st_direct).  The builder moves the
terms' constants (the 1/2 of each iRBF) into c0, so c0 + P is compared with ref = (coefficient of the constant term) + sum G;
where the builder's own denominator 1 + |v| is needed (A4), v = ref - c0: the split stays the builder's business.

Points (A): per interior column s = +-1, the 11 interior extrema of T_12 (together: cos(pi q / 12), q = 0..12 - the builder's own
probe points) and 3 seeded random s; the reference is taken at t = t_lo + (i + 1/2 + s / 2) h EXACTLY (t_lo, h: the host's
geometry doubles), the column's twelve doubles are evaluated exactly at s.  No interval, knot or point is left out.

Ideal interpolant: per interior interval the degree-11 polynomial through the mpmath values at the exact nodes cos(pi (2m+1) / 24)
(tools/gen_cheb_table.py), by an mpmath solve of the 12 x 12 Vandermonde system.  e_ideal,r (r = 0, 1, 2) are reference quantities.

A3, e_built,r <= e_ideal,r + R_r, is the triangle inequality |P - G| <= |I - G| + |P - I| at every point, in the metric
|.| / (1 + |G^(r)|).  P - I is linear in what the builder did differently from the ideal, to first order in u = 2^-53:

  (a) node values.  u_st_direct, statement by statement, for one record {mu, inv, A1, B0, B1, G, DG, DT} of weight w
      (csrc/ttm_eval.h::fold_st8: LET B0 = w/2, B1 = -w/2, G = -w sigma / sqrt(2 pi); RET B0 = B1 = w/2, G = +...; RBF G = w / (sqrt(2 pi)
      sigma), DT = -2 inv G; iRBF A1 = w/2, DG = w / (sqrt(2 pi) sigma)), every product and sum rounding once:
        d  = t - mu                 |dd| <= u |d|
        tt = d inv                  relative error KAPPA u, KAPPA = 5: d, the product, and three roundings in inv = 1 / (sqrt2 sigma)
        e  = erf(tt)                |de|  <= u (8 |e| + KAPPA (2 / sqrt pi) |tt| exp(-tt^2))       4 ulp of the library = 8 u |e|
        gs = exp(-(tt tt))          |dgs| <= u gs (8 + (2 KAPPA + 1) tt^2)                          4 ulp, and the argument's error
        hh = fma(B1, e, B0)         |dhh| <= u (|hh| + |B0| + |B1 e|) + |B1| |de|                   (one rounding in the weight)
        a += A1 e + d hh + G gs     with T1 = |A1 e|, T2 = |d hh|, T3 = |G gs|:
                                    |A1| |de| + 2 u T1 + |d| |dhh| + 2 u T2 + |G| |dgs| + 7 u T3  (G: six roundings from sigma, pi, w)
                                    + 2 u (T1 + T2 + T3) for the two inner sums, and u n_st sum (T1 + T2 + T3) for the accumulation
      and the rounding of the node's abscissa, 2 u |t| |G'(t)|.  The same walk through `da += hh + fma(tt, DT, DG) gs` gives the
      allowance of the derivative that A4 needs.  All magnitudes are taken from the mpmath reference, none from the code under test.
      A node perturbation dy reaches the r-th derivative through the operator norm
        Lambda_r = max_s sum_m | sum_j (d^r s^j / ds^r) Vinv[j][m] | (2 / h)^r      (mpmath inverse Vandermonde, 401 points of [-1, 1]).
  (b) the stored coefficients: one rounding each, 2^-53 sum_j |c_j| |d^r s^j / ds^r| sp_ds^r (the double-double accumulation of
      Vinv . y below it adds 2^-99 sum_m |Vinv[j][m] y_m|, kept in the bound for completeness), the rounding of the stored 2 / h,
      r u |P^(r)| sp_ds^r, and for r = 0 the rounding of the constant split, u (n_iRBF + 1) (|const| + sum |w| / 2).
  R_r is (a) + (b): no measured constant enters the cap.  With 4 ulp allowed to erf and exp, (a) is 40 - 80 u per node and
  Lambda_r (2 / h)^r is 2.5 / ~1.4e3 / ~3e5, so R_r comes to 1 - 14 times e_ideal,r in these cases (long_own's components of two
  or three terms: 0.4 - 0.5 times) - not far below it, as was hoped: the built pieces sit within a few per cent of the ideal ones
  (e_built / e_ideal = 0.9 - 1.3 at r = 1, 2; every figure is printed), and A3 holds them to e_ideal + R, 0.05 - 0.8 of the cap.

B, the evaluators: at every knot t_lo + i h as the double it is and its two neighbouring doubles, every interval midpoint,
t_lo - 50 h, t_hi + 50 h, +-1e6, 0 and 0.123 in column kc, every other column 0, Z_k is compared with the exact value of the
stored section (tests/uform_section.py::exact; within 2^-40 of a knot either adjacent column is right).  Bound
  2^-53 [(28 + n_groups) sum |terms| + (2 |u| + |s|) |P'(s)|]:
a Horner pass of degree 11 with fused multiply-adds rounds 11 times (11 sum |c_j s^j|), the spline is added to the own part and
to the group sum (2), each group's two Horner passes and its fma round at most 11 + 2 times on its own terms (bounded by 13 sum
|terms| once for all groups, since the terms are disjoint) and add one rounding per group on the running sum (n_groups), c0 and
the final store are exact or one rounding (2): 28 + n_groups; the local coordinate rounds twice in u = fma(t, sp_b, sp_a) and
u - floor (2 |u|, reaching s doubled) and once in s = fma(2, ., -1) (|s|), which moves the value by |P'(s)| times that.  The
derivative takes the same bound on the derivative's terms (|P''(s)| sp_ds for the coordinate), relative to dS/dx, plus the
rounding of the density pass's logarithm, 8 u |log| + u (4 ulp of the library).  On the device the families are taken by name
(ttm_last_kernel): k_forward_u, k_forward_hl or k_forward_ul, k_band_forward or k_band_few, each with the density pass of one
component (the log-determinant alone and fused with the value: k_band_logdet, k_band_few<density>); a map of more than P_FEW_D
components also runs the whole map through k_band_density, whose one logarithm is that of the product of all D derivatives (the
relative bounds of the components add, with D u for the products).  A family a case cannot reach is skipped by name.
"""
import ctypes
import math

import mpmath as mp
import numpy as np
import pytest

from tests import test_score as ts
from tests import uform_section as us
from tests.hostemu import emu
from tests.util import check, record_parity
from triangular_transport_toolbox_amd import termtable

CASES = ['few_c2b', 'few_c3', 'few_cond', 'class_55', 'long_own', 'dense_5', 'c5_shape']
N_BUILD = 600
U = 2.0 ** -53
KAPPA, LIB = 5.0, 8.0
N_RANDOM = 3
NQ = 13                                  # extrema of T_12: cos(pi q / 12), q = 0..12
DPS = us.DPS


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


def components_of(name, comps):
    """The components a case tests: {0, D // 2, D - 1} of c5_shape, else every component that has a spline."""
    D = len(comps)
    ks = sorted({0, D // 2, D - 1}) if name == 'c5_shape' else range(D)
    return [k for k in ks if comps[k].nI > 0]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------

def special_terms(om, k):
    """([(kind, mu, sigma, w)], const, own1) of component k from the oracle's term lists: its special terms, the coefficient of the
    constant term of the nonmonotone list, the slope of the polynomial terms of its own variable in the monotone list."""
    kc = k + om.skip_dimensions
    terms, own1 = [], 0.0
    x0 = np.zeros((1, om.X.shape[1]))
    for t, w in zip(om.plan_mon[k], om.coeffs_mon[k]):
        assert len(t) == 1, 'cross terms have no U-form'
        f = t[0]
        if f[0] == 'st':
            _, kind, var, cross, index = f
            assert var == kc and not cross
            mu, sc = om._st_params(kc, var, cross, index)
            terms.append((kind, mp.mpf(float(mu)), mp.mpf(float(sc)), mp.mpf(float(w))))
        else:
            assert f[0] == 'poly' and f[1] == kc and f[2] == 1 and not f[3], 'own terms beyond a linear one'
            own1 += float(w) * float(om._factor(f, x0, kc, derivative_wrt=kc)[0])
    const = sum(float(w) for t, w in zip(om.plan_nonmon[k], om.coeffs_nonmon[k]) if t == [('const',)])
    return terms, mp.mpf(const), own1


def G(terms, t):
    """(G, G', G'') of the summed special terms at t (mpmath) and the first-order rounding allowances of u_st_direct there, value
    and derivative, in units of u = 2^-53 (module docstring, (a))."""
    t = mp.mpf(t)
    g0 = g1 = g2 = mp.mpf(0)
    pv = pd = sum_t = sum_d = 0.0
    sq2, sq2pi = mp.sqrt(2), mp.sqrt(2 * mp.pi)
    for kind, mu, sc, w in terms:
        d = t - mu
        z = d / (sq2 * sc)
        e, gs = mp.erf(z), mp.exp(-z * z)
        phi = gs / (sq2pi * sc)
        r2 = r3 = r4 = r5 = r6 = r7 = mp.mpf(0)
        if kind == 'let':
            v, v1, v2 = (d * (1 - e) - sc * mp.sqrt(2 / mp.pi) * gs) / 2, (1 - e) / 2, -phi
            r3, r4, r5 = w / 2, -w / 2, -w * sc / sq2pi
        elif kind == 'ret':
            v, v1, v2 = (d * (1 + e) + sc * mp.sqrt(2 / mp.pi) * gs) / 2, (1 + e) / 2, phi
            r3, r4, r5 = w / 2, w / 2, w * sc / sq2pi
        elif kind == 'rbf':
            v, v1, v2 = phi, -d / sc ** 2 * phi, (d * d / sc ** 4 - 1 / sc ** 2) * phi
            r5 = w / (sq2pi * sc)
            r7 = -2 / (sq2 * sc) * r5
        else:
            assert kind == 'irbf'
            v, v1, v2 = (1 + e) / 2, phi, -d / sc ** 2 * phi
            r2, r6 = w / 2, w / (sq2pi * sc)
        g0, g1, g2 = g0 + w * v, g1 + w * v1, g2 + w * v2
        # the allowances, in double precision from the reference's magnitudes
        fd, fz, fe, fgs = abs(float(d)), abs(float(z)), abs(float(e)), float(gs)
        a2, a3, a4, a5, a6, a7 = (abs(float(r)) for r in (r2, r3, r4, r5, r6, r7))
        de = LIB * fe + KAPPA * 2.0 / math.sqrt(math.pi) * fz * fgs
        dgs = fgs * (LIB + (2.0 * KAPPA + 1.0) * fz * fz)
        hh = abs(float(r3 + r4 * e))
        dhh = hh + a3 + a4 * fe + a4 * de
        T1, T2, T3 = a2 * fe, fd * hh, a5 * fgs
        pv += a2 * de + 2.0 * T1 + fd * dhh + 2.0 * T2 + a5 * dgs + 7.0 * T3 + 2.0 * (T1 + T2 + T3)
        sum_t += T1 + T2 + T3
        q = abs(float((z * r7 + r6)))
        C = q * fgs
        pd += dhh + (fz * a7 + a6) * dgs + 10.0 * C + KAPPA * fz * a7 * fgs + 2.0 * (hh + C)
        sum_d += hh + C
    n_st = len(terms)
    pv += n_st * sum_t + 2.0 * abs(float(t)) * abs(float(g1))
    pd += n_st * sum_d + 2.0 * abs(float(t)) * abs(float(g2))
    return (g0, g1, g2), pv, pd


_CHEB = {}


def cheb():
    """(nodes, Vinv, Lambda_0..2 per unit (2/h)^r, s of the extrema) - functions of the degree alone, in mpmath."""
    if not _CHEB:
        with mp.workdps(DPS):
            n = us.U_NCOEF
            nodes = [mp.cos(mp.pi * (2 * m + 1) / (2 * n)) for m in range(n)]
            V = mp.matrix(n, n)
            for m in range(n):
                for j in range(n):
                    V[m, j] = nodes[m] ** j
            Vinv = mp.matrix(n, n)
            for m in range(n):                                  # (one solve per unit vector: column m of the inverse)
                rhs = mp.matrix(n, 1)
                rhs[m] = 1
                col = mp.lu_solve(V, rhs)
                for j in range(n):
                    Vinv[j, m] = col[j]
            Vf = np.array([[float(Vinv[j, m]) for m in range(n)] for j in range(n)])
            lam = []
            grid = np.linspace(-1.0, 1.0, 401)
            for r in range(3):
                best = 0.0
                for s in grid:
                    basis = np.array([math.perm(j, r) * s ** (j - r) if j >= r else 0.0 for j in range(n)])
                    best = max(best, float(np.sum(np.abs(basis @ Vf))))
                lam.append(best)
            ext = [float(mp.cos(mp.pi * q / (NQ - 1))) for q in range(NQ)]
            _CHEB.update(nodes=nodes, Vinv=Vinv, Vabs=np.abs(Vf), lam=lam, ext=ext)
    return _CHEB


_REF = {}


def reference(name, om, comps):
    """The mpmath reference of a case: per tested component the special terms, the points of every interior column with (G, G',
    G'') and the allowances there, the ideal interpolant with its errors, the builder's tail probes.  From the oracle and the
    host's geometry alone; computed once per case and left unchanged."""
    if name in _REF:
        return _REF[name]
    ch = cheb()
    ref = {}
    with mp.workdps(DPS):
        for k in components_of(name, comps):
            c = comps[k]
            terms, const, own1 = special_terms(om, k)
            t_lo, h = mp.mpf(c.t_lo), mp.mpf(c.h)
            rng = np.random.default_rng(1000 * k + c.nI)
            cols = {}
            for i in range(c.nI - 2):
                s_pts = ch['ext'] + [float(v) for v in rng.uniform(-1.0, 1.0, N_RANDOM)]
                t_of = lambda s: t_lo + (i + mp.mpf(1) / 2 + mp.mpf(s) / 2) * h            # noqa: E731
                pts = [G(terms, t_of(s)) for s in s_pts]
                nodes = [G(terms, t_of(sm)) for sm in ch['nodes']]
                y = mp.matrix([const + g[0][0] for g in nodes])
                ideal = ch['Vinv'] * y
                cols[i + 1] = dict(s=s_pts, g=[p[0] for p in pts], pv=[p[1] for p in pts], pd=[p[2] for p in pts],
                                   ideal=[ideal[j] for j in range(us.U_NCOEF)], node_pv=max(g[1] for g in nodes),
                                   node_abs=np.array([abs(float(v)) for v in y]))
            tails = {}
            for col in (0, c.nI - 1):                       # uform_spline_verify: the same probes one interval into each tail
                tails[col] = [(s, G(terms, t_lo + (col - 1 + mp.mpf(1) / 2 + mp.mpf(s) / 2) * h)) for s in ch['ext']]
            ref[k] = dict(terms=terms, const=const, own1=own1, cols=cols, tails=tails,
                          split=(sum(1 for t in terms if t[0] == 'irbf') + 1) *
                          (abs(float(const)) + sum(abs(float(t[3])) / 2 for t in terms if t[0] == 'irbf')))
    _REF[name] = ref
    return ref


def case(name):
    """(tm, om, E, comps, ref) of a case under the backend in place."""
    tm, om, X, E = ts.build(name, n=N_BUILD)
    assert tm._cm.u_enabled
    comps = us.read(tm)
    return tm, om, E, comps, reference(name, om, comps)


def rel(a, b):
    return float(abs(a - b) / (1 + abs(b)))


# ---------------------------------------------------------------------------------------------------------------------------
# A: the stored spline
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CASES)
def test_a1_structure_of_the_section(backend, name):
    """Tail columns exactly linear, padding zero, NI even and within its limits.  (Padding slot 12 of a map with push records
    holds the column's local-coordinate offset fma(2, -t_lo/h, -(2c - 1)) where the push records are written - include/ttm.h;
    the host double writes none.)"""
    from fractions import Fraction
    tm, om, E, comps, ref = case(name)
    tested = components_of(name, comps)
    assert tested
    for k in tested:
        c = comps[k]
        assert c.nI % 2 == 0 and 4 <= c.nI <= termtable.U_NI_MAX
        for col in (0, c.nI - 1):
            assert np.all(c.table[col, 2:] == 0.0), (k, col, c.table[col])
        assert np.all(c.padding[:, 1] == 0.0)
        for col in range(c.nI):
            s0 = float(2 * Fraction(c.sp_a) - (2 * col - 1)) if backend == 'hip' and tm._cm.u_p_lag > 0 else 0.0
            assert c.padding[col, 0] == s0, (k, col, c.padding[col, 0], s0)
        assert np.all(np.isfinite(c.table))
        # the header is the geometry the host chose
        assert c.sp_b == 1.0 / c.h and c.sp_ds == 2.0 / c.h and c.sp_a == -c.t_lo / c.h


def stored_at(c, col, s):
    """[P, P' sp_ds, P'' sp_ds^2] of a stored column at local coordinate s, exactly, and [sum_j |c_j d^r s^j| sp_ds^r]."""
    (p, p1, p2), _, _ = us.poly(c.table[col], s)
    ds = mp.mpf(c.sp_ds)
    cabs = np.abs(c.table[col])
    sa = abs(float(s))
    mags = [float(sum(cabs[j] * math.perm(j, r) * sa ** (j - r) for j in range(r, us.U_NCOEF))) * float(ds) ** r for r in range(3)]
    return [p, p1 * ds, p2 * ds * ds], mags


@pytest.mark.parametrize('name', CASES)
def test_a2_value_and_derivative_within_the_acceptance_tolerances(backend, name):
    tm, om, E, comps, ref = case(name)
    worst = [0.0, 0.0]
    with mp.workdps(DPS):
        for k, R in ref.items():
            c = comps[k]
            for col, cr in R['cols'].items():
                for s, g in zip(cr['s'], cr['g']):
                    sp, _ = stored_at(c, col, s)
                    worst[0] = max(worst[0], rel(mp.mpf(c.c0) + sp[0], R['const'] + g[0]))
                    worst[1] = max(worst[1], rel(sp[1], g[1]))
    print('%s %s: value %.3e (tolerance %.1e), derivative %.3e (%.1e)' % (name, backend, worst[0], termtable.U_TOL_VALUE, worst[1],
                                                                          termtable.U_TOL_DERIV))
    check('uform_spline/%s/value/%s' % (name, backend), worst[0], termtable.U_TOL_VALUE, backend)
    check('uform_spline/%s/derivative/%s' % (name, backend), worst[1], termtable.U_TOL_DERIV, backend)


@pytest.mark.parametrize('name', CASES)
def test_a3_all_three_orders_against_the_ideal_interpolant(backend, name):
    """e_built,r <= e_ideal,r + R_r per component, r = 0, 1, 2 (module docstring)."""
    tm, om, E, comps, ref = case(name)
    ch = cheb()
    fails = []
    with mp.workdps(DPS):
        for k, R in ref.items():
            c = comps[k]
            e_built, e_ideal, e_R = [0.0] * 3, [0.0] * 3, [0.0] * 3
            for col, cr in R['cols'].items():
                ds_exact = 2 / mp.mpf(c.h)
                dd = 2.0 ** -99 * (ch['Vabs'] @ cr['node_abs'])                          # (double-double accumulation, per coefficient)
                for s, g in zip(cr['s'], cr['g']):
                    sp, mags = stored_at(c, col, s)
                    i0 = i1 = i2 = mp.mpf(0)
                    for cj in reversed(cr['ideal']):                                       # (the ideal coefficients are mpmath numbers)
                        i2 = i2 * s + 2 * i1
                        i1 = i1 * s + i0
                        i0 = i0 * s + cj
                    ideal = [i0, i1 * ds_exact, i2 * ds_exact ** 2]
                    built = [mp.mpf(c.c0) + sp[0], sp[1], sp[2]]
                    truth = [R['const'] + g[0], g[1], g[2]]
                    sa = abs(float(s))
                    for r in range(3):
                        den = 1 + abs(float(truth[r]))
                        scale = float(ds_exact) ** r
                        Rr = ch['lam'][r] * scale * U * cr['node_pv']
                        Rr += U * mags[r] + scale * float(sum(dd[j] * math.perm(j, r) * sa ** (j - r) for j in range(r, us.U_NCOEF)))
                        Rr += r * U * abs(float(sp[r]))
                        if r == 0:
                            Rr += U * R['split']
                        e_built[r] = max(e_built[r], float(abs(built[r] - truth[r])) / den)
                        e_ideal[r] = max(e_ideal[r], float(abs(ideal[r] - truth[r])) / den)
                        e_R[r] = max(e_R[r], Rr / den)
            for r in range(3):
                ratio = e_built[r] / (e_ideal[r] + e_R[r])
                print('%s %s component %d r=%d: e_built %.3e, e_ideal %.3e, R %.3e, e_built / (e_ideal + R) = %.3f' %
                      (name, backend, k, r, e_built[r], e_ideal[r], e_R[r], ratio))
                try:
                    check('uform_spline/%s/ideal_r%d/%s' % (name, r, backend), ratio, 1.0 + 1e-12, backend)
                except AssertionError as err:
                    fails.append(str(err) + ' (component %d)' % k)
    assert not fails, fails


@pytest.mark.parametrize('name', CASES)
def test_a4_self_reported_fit_errors_are_honest(backend, name):
    """The two doubles at u_err_off are no smaller than the mpmath-measured errors at the builder's own probe points (the extrema of
    T_12 of every column, one interval into each tail), less the rounding allowance of u_st_direct there."""
    tm, om, E, comps, ref = case(name)
    with mp.workdps(DPS):
        for k, R in ref.items():
            c = comps[k]
            worst = [0.0, 0.0]
            probes = [(col, s, g) for col, cr in R['cols'].items() for s, g in zip(cr['s'][:NQ], zip(cr['g'], cr['pv'], cr['pd']))]
            probes += [(col, s, g) for col, pts in R['tails'].items() for s, g in pts]
            for col, s, (g, pv, pd) in probes:
                sp, _ = stored_at(c, col, s)
                v = R['const'] + g[0] - mp.mpf(c.c0)                 # what u_st_direct sums: the moved constants are in c0
                worst[0] = max(worst[0], (float(abs(sp[0] - v)) - U * pv) / (1 + abs(float(v))))
                worst[1] = max(worst[1], (float(abs(sp[1] - g[1])) - U * pd) / (1 + abs(float(g[1]))))
            print('%s %s component %d: reported %.3e / %.3e, measured less allowance %.3e / %.3e' %
                  (name, backend, k, c.err[0], c.err[1], worst[0], worst[1]))
            assert c.err[0] >= worst[0] and c.err[1] >= worst[1], (k, c.err, worst)
            assert c.err[0] <= termtable.U_TOL_VALUE and c.err[1] <= termtable.U_TOL_DERIV


@pytest.mark.parametrize('name', CASES)
def test_a5_tail_columns_to_the_far_field(backend, name):
    """At t_lo and t_hi, 0.37 h, 50 h and 1e6 beyond them, and at -1e6: value and derivative of the stored section within the
    acceptance tolerances of the mpmath reference."""
    tm, om, E, comps, ref = case(name)
    worst = [0.0, 0.0]
    with mp.workdps(DPS):
        for k, R in ref.items():
            c = comps[k]
            t_hi = c.t_lo + (c.nI - 2) * c.h
            pts = [c.t_lo, t_hi, -1e6]
            for off in (0.37 * c.h, 50.0 * c.h, 1e6):
                pts += [c.t_lo - off, t_hi + off]
            for t in pts:
                ex = us.exact(c, t)
                assert t in (c.t_lo, t_hi) or ex['col'] in (0, c.nI - 1)
                g, _, _ = G(R['terms'], mp.mpf(float(t)))
                own0 = ex['value'] - ex['spline'][0] - mp.mpf(c.c0)          # (groups at 0 and own(t): not the spline's business)
                e0 = rel(ex['value'] - own0, R['const'] + g[0])
                e1 = rel(ex['spline'][1], g[1])
                assert e0 <= termtable.U_TOL_VALUE and e1 <= termtable.U_TOL_DERIV, (k, t, e0, e1)
                assert ex['spline'][2] == 0 or ex['col'] not in (0, c.nI - 1)
                worst = [max(worst[0], e0), max(worst[1], e1)]
    print('%s %s: tails, value %.3e, derivative %.3e' % (name, backend, worst[0], worst[1]))
    check('uform_spline/%s/tail_value/%s' % (name, backend), worst[0], termtable.U_TOL_VALUE, backend)
    check('uform_spline/%s/tail_derivative/%s' % (name, backend), worst[1], termtable.U_TOL_DERIV, backend)


@pytest.mark.parametrize('name', CASES)
def test_a6_curvature_quotient_is_recorded(backend, name):
    """P'' sp_ds^2 / (P' sp_ds + own1) on the points of A against mpmath in the metric of tests/test_score.py::E_SPL: recorded beside
    E_SPL[name], not asserted (class_55 has poles where its components are not monotone)."""
    tm, om, E, comps, ref = case(name)
    worst = 0.0
    with mp.workdps(DPS):
        for k, R in ref.items():
            c = comps[k]
            assert abs(c.own_linear_slope - R['own1']) <= 4 * U * abs(R['own1'])
            for col, cr in R['cols'].items():
                for s, g in zip(cr['s'], cr['g']):
                    sp, _ = stored_at(c, col, s)
                    q_u = sp[2] / (sp[1] + mp.mpf(c.own_linear_slope))
                    q_ref = g[2] / (g[1] + mp.mpf(R['own1']))
                    worst = max(worst, rel(q_u, q_ref))
    print('%s %s: curvature quotient %.3e beside E_SPL %.1e (ratio %.2f)' % (name, backend, worst, ts.E_SPL[name], worst / ts.E_SPL[name]))
    assert math.isfinite(worst)
    record_parity('uform_spline/%s/quotient/%s' % (name, backend), worst, 8.0 * ts.E_SPL[name])


# ---------------------------------------------------------------------------------------------------------------------------
# B: the evaluators at the seams
# ---------------------------------------------------------------------------------------------------------------------------

FAMILIES = {
    # options, names of the forward pass, names of the one-component density pass (the log-determinant alone / with the value)
    'k_forward_u': (dict(band_fwd=0, u_no_hot=1, u_loader=0), ('k_forward_u',), ('k_forward_u',)),
    'k_forward_hl_ul': (dict(band_fwd=0, u_loader=1), ('k_forward_hl', 'k_forward_ul'), ('k_forward_hl', 'k_forward_ul')),
    'k_band': (dict(band_fwd=1, u_loader=1), ('k_band_forward', 'k_band_few'),
               ('k_band_logdet', 'k_band_density', 'k_band_few<density>')),
}


def seam_points(c):
    """Column kc of B: every knot as the double it is with its two neighbours, every midpoint, the far field, 0 and 0.123."""
    t_hi = c.t_lo + (c.nI - 2) * c.h
    pts = []
    for i in range(c.nI - 1):
        knot = c.t_lo + i * c.h
        pts += [np.nextafter(knot, -np.inf), knot, np.nextafter(knot, np.inf)]
        if i < c.nI - 2:
            pts.append(c.t_lo + (i + 0.5) * c.h)
    pts += [c.t_lo - 50.0 * c.h, t_hi + 50.0 * c.h, -1e6, 1e6, 0.0, 0.123]
    return np.array(pts, dtype=float)


def candidates(c, t):
    """The exact evaluations an evaluator may agree with at t: its own column, and within 2^-40 of a knot the adjacent one."""
    ex = us.exact(c, t)
    out = [ex]
    near = mp.nint(ex['u'])
    if abs(ex['u'] - near) <= mp.mpf(2) ** -40 and 0 <= near <= c.nI - 2:
        for col in (int(near), int(near) + 1):
            if col != ex['col']:
                out.append(us.exact(c, t, col=col))
    return out


def forward(tm, coef, Xs, N, k0, k1, want_z, want_logdet):
    from triangular_transport_toolbox_amd import _capi
    Z = tm._cols(k1 - k0, N, zero=True) if want_z else None
    ld = tm._zeros(tm._ld(N)) if want_logdet else None
    _capi.check(tm._lib.ttm_forward(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), tm._ptr(Xs), Xs.shape[1], N, int(k0), int(k1),
                                    tm._ptr(Z), Z.shape[1] if want_z else N, tm._ptr(ld), None, None, tm._stream()))
    return (Z[:, :N].cpu().numpy() if want_z else None), (ld[:N].cpu().numpy() if want_logdet else None)


def last_kernel(tm):
    tm._lib.ttm_last_kernel.restype = ctypes.c_char_p
    return tm._lib.ttm_last_kernel().decode()


def seams(tm, comps, name, backend, label, fwd_names=None, dens_names=None, whole_name=None):
    """B for every tested component of a case through the evaluator the options in place select; returns the worst ratios
    error / bound of the value and of the derivative.  whole_name: the kernel of a density pass over the WHOLE map (value and
    log-determinant in one launch) to hold as well: its log-determinant is the sum over the components, every other column at 0."""
    coef = tm._pack_coeffs()
    d = tm._cm.d_cols
    worst_v = worst_d = 0.0
    reached = set()
    with mp.workdps(DPS):
        for k in components_of(name, comps):
            c = comps[k]
            pts = seam_points(c)
            N = len(pts)
            Xh = np.zeros((d, tm._ld(N)))
            Xh[c.kc, :N] = pts
            Xs = tm._to_dev(Xh)
            Z, _ = forward(tm, coef, Xs, N, 0, tm.D, True, False)
            if fwd_names is not None:
                assert last_kernel(tm) in fwd_names, (label, last_kernel(tm))
                reached.add(last_kernel(tm))
            # the one-component density pass: the log-determinant alone and, through the kernels by name, fused with the value
            values, logdets = [Z[k]], []
            for fused in ((False,) if dens_names is None else (False, True)):
                Zk, ld = forward(tm, coef, Xs, N, k, k + 1, fused, True)
                if dens_names is not None:
                    assert last_kernel(tm) in dens_names, (label, last_kernel(tm))
                    reached.add(last_kernel(tm) + (' (value + density)' if fused else ' (density)'))
                logdets.append(ld)
                if fused:
                    values.append(Zk[0])
            n_groups = len(c.groups) + (1 if c.own is not None else 0)
            for n, t in enumerate(pts):
                cand = candidates(c, t)
                for z in values:
                    best_v = np.inf
                    for ex in cand:
                        coord = 2 * abs(ex['u']) + abs(ex['s'])
                        bound_v = U * ((28 + n_groups) * ex['mag'] + coord * abs(ex['dP_ds']))
                        best_v = min(best_v, float(abs(mp.mpf(float(z[n])) - ex['value']) / bound_v))
                    assert best_v <= 1.0, (label, k, n, t, best_v)
                    worst_v = max(worst_v, best_v)
                for ld in logdets:
                    best_d = np.inf
                    for ex in cand:
                        coord = 2 * abs(ex['u']) + abs(ex['s'])
                        bound_d = U * ((28 + n_groups) * ex['mag1'] + coord * abs(ex['d2P_ds2']) * mp.mpf(c.sp_ds))
                        if ex['d1'] > 2 * bound_d:
                            lg = mp.log(ex['d1'])
                            bound_d = bound_d / ex['d1'] + U * (LIB * abs(lg) + 1)
                            if math.isfinite(ld[n]):                  # (NaN or infinite where the derivative is positive: best_d stays inf)
                                best_d = min(best_d, float(abs(mp.mpf(float(ld[n])) - lg) / bound_d))
                        else:
                            best_d = min(best_d, 0.0)                 # (not monotone there: the logarithm has no value to hold)
                    assert best_d <= 1.0, (label, k, n, t, best_d)
                    worst_d = max(worst_d, best_d)
            if whole_name is not None:
                # one logarithm of the product of the D derivatives: the relative bounds add, D - 1 products round, then the log
                Zw, ldw = forward(tm, coef, Xs, N, 0, tm.D, True, True)
                assert last_kernel(tm) == whole_name, (label, last_kernel(tm))
                reached.add(whole_name + ' (whole map, value + density)')
                rest_rel, rest_log = mp.mpf(0), mp.mpf(0)
                for j, cj in enumerate(comps):
                    if j != k:
                        e0 = us.exact(cj, 0.0)
                        b0 = U * ((28 + len(cj.groups) + (1 if cj.own is not None else 0)) * e0['mag1'] +
                                  (2 * abs(e0['u'] or 0) + abs(e0['s'] or 0)) * abs(e0['d2P_ds2']) * mp.mpf(cj.sp_ds))
                        assert e0['d1'] > 2 * b0, '%s: component %d is not monotone at 0' % (name, j)
                        rest_rel += b0 / e0['d1']
                        rest_log += mp.log(e0['d1'])
                for n, t in enumerate(pts):
                    best_v = best_d = np.inf
                    for ex in candidates(c, t):
                        coord = 2 * abs(ex['u']) + abs(ex['s'])
                        bound_v = U * ((28 + n_groups) * ex['mag'] + coord * abs(ex['dP_ds']))
                        best_v = min(best_v, float(abs(mp.mpf(float(Zw[k, n])) - ex['value']) / bound_v))
                        bound_d = U * ((28 + n_groups) * ex['mag1'] + coord * abs(ex['d2P_ds2']) * mp.mpf(c.sp_ds))
                        if ex['d1'] > 2 * bound_d:
                            lg = rest_log + mp.log(ex['d1'])
                            bound_d = bound_d / ex['d1'] + rest_rel + U * (tm.D + LIB * abs(lg) + 1)
                            if math.isfinite(ldw[n]):
                                best_d = min(best_d, float(abs(mp.mpf(float(ldw[n])) - lg) / bound_d))
                        else:
                            best_d = min(best_d, 0.0)
                    assert best_v <= 1.0 and best_d <= 1.0, (label, whole_name, k, n, t, best_v, best_d)
                    worst_v, worst_d = max(worst_v, best_v), max(worst_d, best_d)
    print('%s %s %s: error / bound, value %.3f, derivative %.3f%s' % (name, backend, label, worst_v, worst_d,
                                                                        '; reached ' + ', '.join(sorted(reached)) if reached else ''))
    key = 'uform_spline/%s/seams/%s' % (name, label)
    check(key + '/value', worst_v, 1.0 + 1e-12, backend)
    check(key + '/derivative', worst_d, 1.0 + 1e-12, backend)
    return worst_v, worst_d


@pytest.mark.parametrize('name', CASES)
def test_b_evaluator_at_the_seams_on_the_host_double(name):
    with emu.install():
        tm, om, X, E = ts.build(name, n=N_BUILD)
        comps = us.read(tm)
        seams(tm, comps, name, 'hostemu', 'hostemu')


@pytest.mark.gpu
@pytest.mark.parametrize('family', sorted(FAMILIES))
@pytest.mark.parametrize('name', CASES)
def test_b_kernel_families_at_the_seams(name, family, ttm_opt):
    tm, om, X, E = ts.build(name, n=N_BUILD)
    if family == 'k_band' and tm._cm.u_p_lag == 0:
        pytest.skip('%s is not banded: it has no push records, k_band_* cannot be reached' % name)
    opts, fwd_names, dens_names = FAMILIES[family]
    comps = us.read(tm)
    for key, value in opts.items():
        ttm_opt(key, value)
    # (a sweep of at most P_FEW_D components takes k_band_few<density>: the long maps also run the whole map for k_band_density)
    whole = 'k_band_density' if family == 'k_band' and tm.D > termtable.P_FEW_D else None
    seams(tm, comps, name, 'hip', family, fwd_names, dens_names, whole)
