"""
Reader and exact evaluator of the U section ttm_fold writes (include/ttm.h "U-form", csrc/ttm_uform.h) - test infrastructure.

read(tm) takes the fold buffer of the current coefficient vector (on the device backend: what the device wrote) and returns, per
component, the numbers a U-form evaluator reads: the `ucomp` record, the header {c0, -t_lo/h, 1/h, 2/h}, the group coefficient
sets B[0..11] | A[0..11] (the own group of a monotone list with polynomial terms last), the spline columns of U_TSTRIDE doubles
(12 coefficients + padding) and the two self-reported fit errors at u_err_off.

exact(comp, t, ...) evaluates, in mpmath and from those stored doubles alone,

    S(t) = c0 + sum_groups (A(x_j) + exp(-x_j^2 / 4) B(x_j)) + own(t) + P_col(s),     u = t sp_b + sp_a,  col = floor(clip(u, -1, NI - 2)) + 1,
                                                                                       s = 2 (u - (col - 1)) - 1

with its first and second derivative in t and the sum of the absolute values of every term that enters the value: it is exact on
what is stored (no rounding of u, s or the Horner passes), so it is the yardstick of an evaluator's rounding, not of the fit.

group_terms / monotone give the pieces of the same sum one by one with their first and second derivatives and the sums of |terms|
of each (what tests/test_score_exact.py assembles S, dS/du and m'' / m' from); read_push reads the push records of a banded map
back and returns the components as the band kernels read them.
"""
from dataclasses import dataclass, field

import mpmath as mp
import numpy as np

from triangular_transport_toolbox_amd import termtable

UC_LEN, UG_LEN = termtable.UC_LEN, termtable.UG_LEN                 # include/ttm.h: TTM_UC_LEN, TTM_UG_LEN
U_TSTRIDE, U_GSTRIDE = termtable.U_TSTRIDE, termtable.U_GSTRIDE     # TTM_U_TSTRIDE, TTM_U_GSTRIDE
U_GHALF = U_GSTRIDE // 2                                            # TTM_U_GHALF
U_DEG = 11                                                          # TTM_U_DEG
U_NCOEF = U_DEG + 1
UCF_OWN, UGF_POLY, PLAN_HF = termtable.UCF_OWN, termtable.UGF_POLY, termtable.PLAN_HF

DPS = 40


@dataclass
class Group:
    var: int                 # the column the group reads
    flags: int
    B: np.ndarray            # monomial coefficients of the exp(-x^2/4) part
    A: np.ndarray            # of the plain part

    @property
    def deg_b(self):
        return (self.flags >> 16) & 15

    @property
    def deg_a(self):
        return (self.flags >> 24) & 15


@dataclass
class Component:
    k: int
    kc: int
    c0: float
    sp_a: float              # -t_lo / h
    sp_b: float              # 1 / h
    sp_ds: float             # 2 / h
    nI: int
    tab_off: int
    dbl_off: int
    flags: int
    table: np.ndarray        # NI x 12
    padding: np.ndarray      # NI x (U_TSTRIDE - 12)
    groups: list = field(default_factory=list)
    own: Group = None        # the polynomial / Hermite-function terms of the monotone list (UCF_OWN), or None
    err: tuple = (0.0, 0.0)  # self-reported fit errors {value, derivative}
    t_lo: float = 0.0        # host geometry (cm.ugeo): what the builder placed its nodes with
    h: float = 0.0
    s0: np.ndarray = None    # read_push: the stored local-coordinate offset of every column (None: s from u, as the U-form evaluators)

    @property
    def own_linear_slope(self):
        """Slope of a linear own term (0.0: no own group); asserts that the own group is no more than that."""
        if self.own is None:
            return 0.0
        assert not (self.own.flags & PLAN_HF) and self.own.deg_a <= 1, 'own terms beyond a linear one'
        return float(self.own.A[1])


def u_section(tm):
    """(U, coef): the U section of the current coefficient vector as a host array."""
    coef = tm._pack_coeffs()
    fold = coef._ttm_fold.cpu().numpy()
    off = int(tm._lib.ttm_uform_offset(tm._pp))
    assert off >= 0, 'the map has no U-form'
    return fold[off:], coef


def read(tm):
    """The components of the U section of tm's current coefficient vector."""
    cm = tm._cm
    U, _ = u_section(tm)
    uc = np.asarray(cm.ucomp[:cm.D * UC_LEN]).reshape(-1, UC_LEN)
    ug = np.asarray(cm.ugrp).reshape(-1, UG_LEN)
    geo = np.asarray(cm.ugeo, dtype=float).reshape(-1, 2)
    err_off = int(cm.u_err_off)
    comps = []
    for k in range(cm.D):
        kc, _, n_grp, grp_off, nI, tab_off, dbl_off, flags = (int(v) for v in uc[k])
        cd = U[dbl_off:]

        def group(g):
            rec = cd[4 + U_GSTRIDE * g:4 + U_GSTRIDE * (g + 1)]
            return Group(int(ug[grp_off + g, 0]), int(ug[grp_off + g, 1]), rec[:U_GHALF].copy(), rec[U_GHALF:].copy())
        cols = U[tab_off:tab_off + nI * U_TSTRIDE].reshape(nI, U_TSTRIDE)
        comps.append(Component(
            k=k, kc=kc, c0=float(cd[0]), sp_a=float(cd[1]), sp_b=float(cd[2]), sp_ds=float(cd[3]), nI=nI, tab_off=tab_off,
            dbl_off=dbl_off, flags=flags, table=cols[:, :U_NCOEF].copy(), padding=cols[:, U_NCOEF:].copy(),
            groups=[group(g) for g in range(n_grp)], own=group(n_grp) if flags & UCF_OWN else None,
            err=(float(U[err_off + 2 * k]), float(U[err_off + 2 * k + 1])), t_lo=float(geo[k, 0]), h=float(geo[k, 1])))
    return comps


def column_of(comp, t):
    """The spline column an exact evaluator takes at t, and the exact (u, s) there."""
    u = mp.mpf(float(t)) * mp.mpf(comp.sp_b) + mp.mpf(comp.sp_a)
    fl = mp.floor(min(max(u, mp.mpf(-1)), mp.mpf(comp.nI - 2)))
    return int(fl) + 1, u, 2 * (u - fl) - 1


def poly(coefs, x):
    """([p, p', p''], sum |c_j x^j|, sum |j c_j x^(j-1)|) of the monomial coefficients `coefs` (doubles) at x, in mpmath."""
    c = [mp.mpf(float(v)) for v in coefs]
    x = mp.mpf(x)
    p = d1 = d2 = mp.mpf(0)
    for cj in reversed(c):
        d2 = d2 * x + 2 * d1
        d1 = d1 * x + p
        p = p * x + cj
    ax = abs(x)
    mag = mag1 = mp.mpf(0)
    for j, cj in enumerate(c):
        mag += abs(cj) * ax ** j
        if j:
            mag1 += j * abs(cj) * ax ** (j - 1)
    return [p, d1, d2], mag, mag1


def _group_value(g, x):
    """([value, d/dx, d2/dx2], sum of |terms| of the value, of the first derivative) of A(x) + exp(-x^2/4) B(x)."""
    x = mp.mpf(x)
    (a, a1, a2), ma, ma1 = poly(g.A, x)
    (b, b1, b2), mb, mb1 = poly(g.B, x)
    e = mp.exp(-x * x / 4)
    v = a + e * b
    # d/dx [e B] = e (B' - x B / 2);  d2/dx2 [e B] = e (B'' - x B' + (x^2 / 4 - 1 / 2) B)
    d1 = a1 + e * (b1 - x * b / 2)
    d2 = a2 + e * (b2 - x * b1 + (x * x / 4 - mp.mpf(1) / 2) * b)
    return [v, d1, d2], ma + e * mb, ma1 + e * (mb1 + abs(x) * mb / 2)


def horner(coefs, x):
    """[p, p', p''] of the monomial coefficients `coefs` (doubles) at x, in mpmath (poly's values, without its sums; trailing zero
    coefficients are skipped)."""
    x = mp.mpf(x)
    p = d1 = d2 = mp.mpf(0)
    for cj in reversed(coefs[:degree(coefs) + 1]):
        d2 = d2 * x + 2 * d1
        d1 = d1 * x + p
        p = p * x + mp.mpf(float(cj))
    return [p, d1, d2]


def mags(coefs, x):
    """[sum |c_j x^j|, sum |j c_j x^(j-1)|, sum |j (j-1) c_j x^(j-2)|, |sum j (j-1) (j-2) c_j x^(j-3)|] as doubles: the sums of the
    absolute values of the terms of p, p', p'' (magnitudes: a bound's weights, never a reference value) and the size of p'''."""
    c = np.asarray(coefs, dtype=float)
    j = np.arange(len(c), dtype=float)
    ax, fx = abs(float(x)), float(x)
    pw = lambda r, b: np.where(j >= r, b ** np.maximum(j - r, 0.0), 0.0)      # noqa: E731
    return [float(np.sum(np.abs(c) * pw(0, ax))), float(np.sum(np.abs(c) * j * pw(1, ax))), float(np.sum(np.abs(c) * j * (j - 1) * pw(2, ax))),
            abs(float(np.sum(c * j * (j - 1) * (j - 2) * pw(3, fx))))]


def degree(coefs):
    """Index of the last nonzero coefficient (0 for an all-zero set): the Horner steps that can round."""
    nz = np.nonzero(np.asarray(coefs))[0]
    return int(nz[-1]) if len(nz) else 0


def group_terms(g, x):
    """A group f(x) = A(x) + E B(x), E = exp(-x^2/4), at x in full: dict(d=[f, f', f''] in mpmath (_group_value's), mag=[sums of
    |terms| of f, f', f''] (doubles; the second is the group's derivative magnitude), E, w=[|B|, |B' - x B / 2|,
    |B'' - x B' + (x^2/4 - 1/2) B|] (doubles: what an error of E is multiplied by in f, f', f'') and deg = (degree of B, of A))."""
    x = mp.mpf(float(x))
    a, a1, a2 = horner(g.A, x)
    b, b1, b2 = horner(g.B, x)
    e = mp.exp(-x * x / 4)
    parts = [b, b1 - x * b / 2, b2 - x * b1 + (x * x / 4 - mp.mpf(1) / 2) * b]
    ma, mb, ef, ax = mags(g.A, x), mags(g.B, x), float(e), abs(float(x))
    mag = [ma[0] + ef * mb[0], ma[1] + ef * (mb[1] + ax * mb[0] / 2), ma[2] + ef * (mb[2] + ax * mb[1] + (ax * ax / 4 + 0.5) * mb[0])]
    return dict(d=[a + e * parts[0], a1 + e * parts[1], a2 + e * parts[2]], mag=mag, E=e, w=[abs(float(v)) for v in parts],
                deg=(degree(g.B), degree(g.A)))


def monotone(comp, t, col=None):
    """The monotone part m(t) = own(t) + P_col(s) of a component at t (a double), from the stored doubles: dict(d=[m, m', m''] in
    mpmath, mag=[sums of |terms| of m, m', m''] (doubles), u, s, col, dP=[|P'|, |P''|, |P'''|] in the local coordinate (doubles, 0
    without a spline), own=group_terms of the own group or None).  col: the spline column to take (None: column_of's); a
    component read from the push records (s0 set) takes its local coordinate as the band kernels do, s = t sp_ds + s0[col] with
    s0 the stored double."""
    t = float(t)
    d, mag = [mp.mpf(0)] * 3, [0.0] * 3
    own = None
    if comp.own is not None:
        own = group_terms(comp.own, t)
        d, mag = list(own['d']), list(own['mag'])
    out = dict(u=None, s=None, col=None, dP=[0.0] * 3, own=own)
    if comp.nI > 0:
        c_own, u, _ = column_of(comp, t)
        col = c_own if col is None else int(col)
        if comp.s0 is None:
            s = 2 * (u - (col - 1)) - 1
        else:
            s = mp.mpf(t) * mp.mpf(comp.sp_ds) + mp.mpf(float(comp.s0[col]))
        p, p1, p2 = horner(comp.table[col], s)
        pm = mags(comp.table[col], s)
        ds = mp.mpf(comp.sp_ds)
        d = [d[0] + p, d[1] + p1 * ds, d[2] + p2 * ds * ds]
        mag = [mag[0] + pm[0], mag[1] + pm[1] * comp.sp_ds, mag[2] + pm[2] * comp.sp_ds * comp.sp_ds]
        out.update(u=u, s=s, col=col, dP=[abs(float(p1)), abs(float(p2)), pm[3]])
    out.update(d=d, mag=mag)
    return out


def read_push(tm, comps):
    """The push records of a banded map (include/ttm.h "push records"; csrc/ttm_uform.h: uform_scatter_push_records) read back from
    the fold buffer: (P [D + lag, stride], push) - push[k] is component k as the band kernels read it: c0 = record k's chain start
    [0] (the component's constants and its groups' A[0], summed by the builder), every group's B[0..DB] and A[1..DA] from its
    block (A[0] = 0: it is in the chain start), the own term's slope from [7], the spline table with the stored local-coordinate
    offsets s0 (padding slot 12 of the columns).  Coefficients beyond a class's degrees are not in a record: they read 0 here."""
    import dataclasses
    cm = tm._cm
    lag, ps, cls = int(cm.u_p_lag), int(cm.u_p_stride), int(cm.u_h_cls)
    assert lag > 0, 'the map has no push records'
    U, _ = u_section(tm)
    D = cm.D
    P = np.array(U[int(cm.u_p_off):int(cm.u_p_off) + (D + lag) * ps]).reshape(D + lag, ps)
    DB, DA = termtable.H_DB[cls], termtable.H_DA[cls]
    GP = DB + 1 + DA
    push = []
    for k, c in enumerate(comps):
        groups = []
        for g in c.groups:
            lg = c.kc - g.var
            assert 1 <= lg <= lag, 'a group outside the band'
            blk = P[k - lg + lag, termtable.P_HDR + (lg - 1) * GP:termtable.P_HDR + lg * GP]
            B, A = np.zeros(U_GHALF), np.zeros(U_GHALF)
            B[:DB + 1] = blk[:DB + 1]
            A[1:DA + 1] = blk[DB + 1:]
            groups.append(Group(g.var, g.flags, B, A))
        own = None
        if c.own is not None:
            A = np.zeros(U_GHALF)
            A[1] = P[k + lag, 7]
            own = Group(c.kc, UGF_POLY | (1 << 24), np.zeros(U_GHALF), A)
        push.append(dataclasses.replace(c, c0=float(P[k, 0]), groups=groups, own=own, s0=c.padding[:, 0].copy()))
    return P, push


def exact(comp, t, col=None, others=0.0):
    """S, dS/dt, d2S/dt2 of the component at x_kc = t (a double) from the stored doubles, with the sums of |terms|.

    col: the spline column to take (None: the exact evaluator's own, column_of); others: the value of every other column (a
    number) or {column: value}.  Returns dict(value, d1, d2, mag, mag1, u, s, col, spline=[P, P' sp_ds, P'' sp_ds^2],
    dP_ds, d2P_ds2): mag / mag1 are the sums of the absolute values of the terms of the value / of the first derivative."""
    with mp.workdps(DPS):
        t = float(t)
        v = mp.mpf(comp.c0)
        mag = abs(v)
        d1 = d2 = mag1 = mp.mpf(0)
        for g in comp.groups:
            x = others.get(g.var, 0.0) if isinstance(others, dict) else others
            gv, gm, _ = _group_value(g, float(x))
            v += gv[0]
            mag += gm
        if comp.own is not None:
            gv, gm, gm1 = _group_value(comp.own, t)
            v, d1, d2, mag, mag1 = v + gv[0], d1 + gv[1], d2 + gv[2], mag + gm, mag1 + gm1
        out = dict(u=None, s=None, col=None, spline=[mp.mpf(0)] * 3, dP_ds=mp.mpf(0), d2P_ds2=mp.mpf(0))
        if comp.nI > 0:
            c_own, u, _ = column_of(comp, t)
            col = c_own if col is None else int(col)
            s = 2 * (u - (col - 1)) - 1
            (p, p1, p2), pm, pm1 = poly(comp.table[col], s)
            ds = mp.mpf(comp.sp_ds)
            sp = [p, p1 * ds, p2 * ds * ds]
            v, d1, d2, mag, mag1 = v + sp[0], d1 + sp[1], d2 + sp[2], mag + pm, mag1 + pm1 * ds
            out.update(u=u, s=s, col=col, spline=sp, dP_ds=p1, d2P_ds2=p2)
        out.update(value=v, d1=d1, d2=d2, mag=mag, mag1=mag1)
        return out


def quotient(tm, T):
    """m''(t) / m'(t) of every component at the raw samples T (rows x D) in NumPy from the U section of the current coefficient
    vector: P''(s) sp_ds^2 / (P'(s) sp_ds + own1) - the log-determinant quotient of the score (tools/score_spline_error.py)."""
    comps = read(tm)
    q = np.zeros(T.shape)
    for k, c in enumerate(comps):
        own1 = c.own_linear_slope
        t = T[:, k]
        d1, d2 = np.full(t.shape, own1), np.zeros(t.shape)
        if c.nI > 0:
            u = t * c.sp_b + c.sp_a
            fl_ = np.floor(np.clip(u, -1.0, c.nI - 2.0))
            s_ = 2.0 * (u - fl_) - 1.0
            for n in range(len(t)):
                P = np.polynomial.Polynomial(c.table[int(fl_[n]) + 1])
                d1[n] += P.deriv(1)(s_[n]) * c.sp_ds
                d2[n] += P.deriv(2)(s_[n]) * c.sp_ds * c.sp_ds
        q[:, k] = d2 / d1
    return q
