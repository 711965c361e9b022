"""
The root searches of integrated-rectifier maps - ttm_inverse_bisect / ttm_inverse_newton (include/ttm.h), sample_bisect /
sample_newton of csrc/ttm_eval.h in the kernel families k_int_root, k_int_root_x and k_inverse_bisect / k_inverse_newton - held to a
per-row replay of the reference's search, on the host test double and on the device.

Reference.  replay_bisect(S, z, cap) restates TM:3842-3976 per sample in NumPy float64 for all rows at once (masks, no loop over
rows): bracket [-2, 2], ends swapped together with their values on a decreasing start, window shifts by 2 (hi - lo) to the side of
the sign while flo fhi > 0 (at most 2000), then midpoints (lo + hi) / 2 until not |fm| > 1e-9, at most 100 of them or `cap`.  S is
OracleMap.s of the component on the rows of the matrix THE KERNEL RETURNED with the own column replaced by the trial column, so a
disagreement in one component does not cascade into the next.  The replay is anchored to the oracle, not to the kernels: on the
goldens c2a_int and c3_int its last trial points for inv_Z[1:] are OracleMap.inverse_map's rows behind row 0 bit for bit
(test_the_replay_is_the_oracles_search; the oracle restates the reference's vectorised loop and is pinned by tests/golden/; row 0 is
the reference's loop-guard quirk, which the entry points leave to their caller).

tau.  The kernels' S and the oracle's differ in the last bits, so the two midpoint sequences can part only where a stop decision
|fm| > 1e-9 is within that difference of 1e-9 (a sign can flip only below it, where both stop).  A search (row, component) is
DECISIVE when margin = min over its replayed midpoints of | |fm| - 1e-9 | exceeds tau = 1e-12 (1 + |z|) and every replayed trial
point is finite.  The premise - |S_kernel - S_oracle| <= tau / 2 at the returned rows, S_kernel from ttm_forward - is checked by
every search test itself, on the host double and on the device (check_premise), and its largest ratio is recorded under
int_root_search/premise/...; tau = 1e-12 (1 + |z|) held on both.

Cap.  At most 5 % of the searches of a case may be indecisive; asserted on the replay alone, first at the target rows themselves
(test_the_cap_holds_on_the_replay_alone, no kernel involved) and again at the returned rows before the kernel's own columns are
looked at.

Inputs.  N = 257 (one block of 256 threads plus one row).  z[n, k] = OracleMap.s at the standardised training rows with the own
columns multiplied by scale[n % 8], so every target is reachable and the rows spread over 0 to 4 window shifts on both sides (the
histogram of replayed shifts must have rows at 0, 1, 2 and >= 3).  Scales and the replay-alone indecisive share on the CPU
(at the target rows):
    spiral3         (1, 1, 1, 2.5, 4, 8, 16, 40)    softplus 0.78 %, exponential 0.97 %, expneg 0.78 %,
                                                    explinearunit 0.78 %, squared 0.00 %
    spiral10        (1, 1, 1, 2.5, 4, 8, 16, 40)    softplus 0.58 %
    band5           (1, 1, 1, 2.5, 4, 8, 16, 40)    softplus 0.70 %, exponential 1.17 %
    special_cond    (1, 1, 1, 14, 8, 6, 12, 2.5)    softplus 2.08 %, explinearunit 2.85 %
special_cond is at or over the cap at the common scales (softplus 4.41 %, explinearunit 5.06 %: far targets whose |S| puts 1e-9
below double resolution), and where a column in front lies 15 or more deviations out its components are flat to 1e-8 per unit, so
that searches run 23 to 27 shifts away (with explinearunit from a scale of 8 on in most row classes n % 8).  Its scales were
narrowed per row class n % 8 until, for both rectifiers, the replay alone is under 5 % and no search needs more than 8 shifts
(asserted; most: 4): the far rows are the classes with scales 14 and 12.  The device gives the host double's figures.
What these inputs cannot reach: an integrated-rectifier component has dS/dx_k >= delta > 0, so S(-2) < S(2) on every finite row
and the swap of a decreasing start never fires (no replayed bracket of any case is swapped); that branch is held where it can
fire, on the separable push-form searches (tests/test_band_bisect.py).

Kernel families.  The host double follows the library's default plan whatever the options (monomial-form search); there
`special_cond` (special terms, a conditioning column) is the run of the generic search.  On the device
test_every_kernel_family_runs_the_same_search pins k_int_root, k_int_root_x (int_xprog = 2) and k_inverse_bisect / k_inverse_newton
(int_dense = 0) by name.  Newton steps use fast_div and the analytic derivative and are not replayable to the bit: the window phase
(the bisection's) gives their bracket exactly, the stopping rule their residual.  Every figure is printed before it is held.
"""
import numpy as np
import pytest

from tests.hostemu import emu
from tests.test_logdensity import RECTS, build
from tests.test_sample_logdensity import device_of, entry, last_kernel
from tests.util import load_case, make_oracle, options, record_parity

N = 257
THRESHOLD = 1e-9
CAP_SHARE = 0.05
SCALE = (1.0, 1.0, 1.0, 2.5, 4.0, 8.0, 16.0, 40.0)
SCALES = {'special_cond': (1.0, 1.0, 1.0, 14.0, 8.0, 6.0, 12.0, 2.5)}
CASES = [('spiral3', r) for r in RECTS] + [('spiral10', 'softplus'), ('band5', 'softplus'), ('band5', 'exponential'),
                                           ('special_cond', 'softplus'), ('special_cond', 'explinearunit')]
NO_ROW_AT_THE_LIMIT = ('spiral3', 'spiral10', 'band5')          # (Newton: no row of these may need 100 trial points)
POISON_ROWS = ((5, float('nan')), (130, float('inf')), (256, -float('inf')))


@pytest.fixture(params=[pytest.param('hostemu'), pytest.param('hip', marks=pytest.mark.gpu)])
def backend(request):
    if request.param == 'hostemu':
        with emu.install():
            yield 'hostemu'
    else:
        yield 'hip'


# ------------------------------------------------------------------------------------------ the reference

class Replay(dict):
    __getattr__ = dict.__getitem__


def replay_bisect(S, z, cap=None):
    """TM:3842-3976 per sample, all rows at once.  S(col, rows): map component at the trial points `col` of the rows `rows` (an index
    array); z: targets.  Per row: last (the last trial point), count (midpoints), shifts, lo / hi (the final bracket), win_lo /
    win_hi (the bracket after the window phase), margin (min over the midpoints of ||fm| - 1e-9|; inf without a midpoint), finite
    (every trial point finite)."""
    z = np.asarray(z, dtype=np.float64)
    n = len(z)
    rows = np.arange(n)
    lo, hi = np.full(n, -2.0), np.full(n, 2.0)
    with np.errstate(all='ignore'):
        flo, fhi = S(lo, rows) - z, S(hi, rows) - z
        last = hi.copy()
        finite = np.ones(n, dtype=bool)
        shifts = np.zeros(n, dtype=np.int64)

        def resort(idx):
            sw = idx[flo[idx] > fhi[idx]]
            flo[sw], fhi[sw] = fhi[sw], flo[sw]
            lo[sw], hi[sw] = hi[sw], lo[sw]
        resort(rows)
        shift = rows[flo * fhi > 0]
        guard = 0
        while len(shift) and guard < 2000:
            guard += 1
            resort(shift)
            diff = hi - lo
            pos, neg = shift[flo[shift] > 0], shift[flo[shift] < 0]
            hi[pos], fhi[pos] = lo[pos], flo[pos]
            lo[pos] = lo[pos] - diff[pos] * 2
            if len(pos):
                flo[pos] = S(lo[pos], pos) - z[pos]
            last[pos] = lo[pos]
            lo[neg], flo[neg] = hi[neg], fhi[neg]
            hi[neg] = hi[neg] + diff[neg] * 2
            if len(neg):
                fhi[neg] = S(hi[neg], neg) - z[neg]
            last[neg] = hi[neg]
            moved = np.concatenate((pos, neg))
            shifts[moved] += 1
            finite[moved] &= np.isfinite(last[moved])
            shift = shift[flo[shift] * fhi[shift] > 0]
        win_lo, win_hi = lo.copy(), hi.copy()
        count = np.zeros(n, dtype=np.int64)
        margin = np.full(n, np.inf)
        maxit = 100 if cap is None else min(int(cap), 100)
        active, it = rows, 0
        while len(active) and it < maxit:
            it += 1
            mid = (lo[active] + hi[active]) * 0.5
            last[active], count[active] = mid, it
            finite[active] &= np.isfinite(mid)
            fm = S(mid, active) - z[active]
            below, above = active[fm < 0], active[fm > 0]
            lo[below], hi[above] = mid[fm < 0], mid[fm > 0]
            margin[active] = np.minimum(margin[active], np.abs(np.abs(fm) - THRESHOLD))         # (NaN stays: never decisive)
            active = active[np.abs(fm) > THRESHOLD]
    return Replay(last=last, count=count, shifts=shifts, lo=lo, hi=hi, win_lo=win_lo, win_hi=win_hi, margin=margin, finite=finite)


def oracle_S(om, U, k):
    """S(col, rows) of component k on the rows of the standardised matrix U with the own column replaced by the trial column."""
    kc = om.skip_dimensions + k

    def S(col, rows):
        Xl = np.array(U[rows], dtype=np.float64, copy=True)
        Xl[:, kc] = col
        with np.errstate(all='ignore'):
            return om.s(Xl, k)
    return S


def tau_of(z):
    with np.errstate(all='ignore'):
        return 1e-12 * (1.0 + np.abs(z))


def decisive(rep, z):
    with np.errstate(all='ignore'):
        return (rep.margin > tau_of(z)) & rep.finite


def replay_all(om, U, z, cap=None):
    """The replay of every component at the rows U (own column of a component replaced by its trial points)."""
    return [replay_bisect(oracle_S(om, U, k), z[:, k], None if cap is None else cap[k]) for k in range(om.D)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize('name', ['c2a_int', 'c3_int'])
def test_the_replay_is_the_oracles_search(name):
    """The anchor: on the goldens, the replay of inv_Z[1:] with S from the oracle gives OracleMap.inverse_map's rows behind row 0
    bit for bit (the components in front are the oracle's own returned columns)."""
    npz, desc = load_case(name)
    om = make_oracle(name, npz, desc)
    Zin = np.array(npz['inv_Z'], dtype=float)
    assert om.skip_dimensions == 0 and Zin.shape[1] == om.D
    ref = om.inverse_map(Zin)
    U = np.zeros((len(Zin), om.D))
    for k in range(om.D):                                           # (inverse_map's loop, kept in standardised coordinates)
        U = om.vectorized_root_search_bisection(U, Zin[:, k], k)
    assert np.array_equal(bits(U * om.X_std + om.X_mean), bits(ref))
    counts = []
    for k in range(om.D):
        rep = replay_bisect(oracle_S(om, U[1:], k), Zin[1:, k])
        assert np.array_equal(bits(rep.last), bits(U[1:, k])), (name, k, int(np.sum(bits(rep.last) != bits(U[1:, k]))))
        counts.append(int(rep.count.max()))
    print('%s: %d rows, %d components, replay == OracleMap.inverse_map bit for bit; largest midpoint counts %s' % (name, len(Zin) - 1, om.D, counts))


# ------------------------------------------------------------------------------------------ inputs

_ORACLE, _MAPS, _RUNS = {}, {}, {}


def scale_of(name):
    return np.asarray(SCALES.get(name, SCALE), dtype=float)


def case(backend, name, rect):
    """(tm, om, E, U, z): the map of a backend (made once), the shared oracle, and the targets z[n, k] = OracleMap.s at the
    standardised training rows U with the own columns multiplied by scale[n % 8] (computed once, left unchanged)."""
    key = (backend, name, rect)
    if key not in _MAPS:
        tm, om, X, E = build(name, rect, alternate_root_finding=False, root_finder='reference', oracle=(name, rect) not in _ORACLE)
        if (name, rect) not in _ORACLE:
            U = (X[:N] - om.X_mean) / om.X_std
            U[:, E:] *= scale_of(name)[np.arange(N) % 8][:, None]
            with np.errstate(all='ignore'):
                z = np.column_stack([om.s(U.copy(), k) for k in range(om.D)])
            assert np.all(np.isfinite(z)), (name, rect)
            for a in (U, z):
                a.setflags(write=False)
            _ORACLE[(name, rect)] = (om, E, U, z)
        _MAPS[key] = tm
    return (_MAPS[key],) + _ORACLE[(name, rect)]


def oracle_case(name, rect):
    if (name, rect) not in _ORACLE:
        with emu.install():
            case('hostemu', name, rect)
    return _ORACLE[(name, rect)]


def shift_histogram(reps):
    sh = np.concatenate([r.shifts for r in reps])
    return [int(np.sum(sh == 0)), int(np.sum(sh == 1)), int(np.sum(sh == 2)), int(np.sum(sh >= 3))], int(sh.max())


@pytest.mark.parametrize('name,rect', CASES)
def test_the_cap_holds_on_the_replay_alone(name, rect):
    """No kernel: the replay at the target rows themselves.  At most 5 % of a case's searches are indecisive and the rows spread
    over 0, 1, 2 and >= 3 window shifts; `special_cond`, whose scales are its own, needs no more than 8."""
    om, E, U, z = oracle_case(name, rect)
    reps = replay_all(om, U, z)
    dec = np.column_stack([decisive(r, z[:, k]) for k, r in enumerate(reps)])
    hist, most = shift_histogram(reps)
    share = 1.0 - dec.mean()
    print('%s/%s: %d searches, indecisive %.2f %% (5 %%), shifts 0 / 1 / 2 / >= 3: %s, most %d, midpoints up to %d' % (
        name, rect, dec.size, 100 * share, hist, most, max(int(r.count.max()) for r in reps)))
    assert share <= CAP_SHARE
    assert min(hist) > 0
    if name == 'special_cond':
        assert most <= 8


# ------------------------------------------------------------------------------------------ the kernels

def load(tm, backend, E, U, z):
    """(Zs, Xs): the targets and the zeroed matrix the search writes into, conditioning columns in front."""
    import torch
    dev = device_of(backend)
    Zs, Xs = tm._cols(tm.D, N, zero=True), tm._cols(tm._cm.d_cols, N, zero=True)
    Zs[:, :N] = torch.from_numpy(np.ascontiguousarray(z.T)).to(dev)
    if E:
        Xs[:E, :N] = torch.from_numpy(np.ascontiguousarray(U[:, :E].T)).to(dev)
    return Zs, Xs


def returned(Xs):
    return np.ascontiguousarray(Xs[:, :N].cpu().numpy().T)


def run(backend, name, rect, newton, opts=(), kernel=None):
    """One whole call and N calls on one row each (made once per backend, case, method and options): the returned matrix U [N x d],
    the whole call's iters [D], every row's own counts [N x D], and the kernel's S at the returned rows [N x D].  The single-row
    calls must reproduce the whole call bit for bit."""
    key = (backend, name, rect, newton, tuple(opts), kernel)
    if key in _RUNS:
        return _RUNS[key]
    tm, om, E, U0, z = case(backend, name, rect)
    with options(tm._lib, **dict(opts)):
        Zs, Xs = load(tm, backend, E, U0, z)
        rc, iters = entry(tm, backend, Zs, Xs, N, newton, plain=True)
        assert rc == 0
        if kernel is not None:
            assert last_kernel(tm) == kernel
        _, Xr = load(tm, backend, E, U0, z)
        counts = np.zeros((N, tm.D), dtype=np.int64)
        for n in range(N):
            rc, it = entry(tm, backend, Zs, Xr, 1, newton, row0=n, plain=True)
            assert rc == 0
            counts[n] = it
        if kernel is not None:
            assert last_kernel(tm) == kernel
        U = returned(Xs)
        assert np.array_equal(bits(returned(Xr)), bits(U)), 'rows searched one by one differ from the whole call'
        Sk = np.ascontiguousarray(tm.forward_device(Xs, N)[:, :N].cpu().numpy().T)
    assert np.array_equal(bits(U[:, :E]), bits(U0[:, :E]))
    for a in (U, iters, counts, Sk):
        a.setflags(write=False)
    _RUNS[key] = (U, iters, counts, Sk)
    return _RUNS[key]


def label_of(backend, name, rect, method, opts):
    tag = ','.join('%s=%d' % kv for kv in opts)
    return '%s/%s/%s%s/%s' % (name, rect, method, '[%s]' % tag if tag else '', backend)


def record(backend, what, label, value, tol=None):
    if backend == 'hip':
        record_parity('int_root_search/%s/%s' % (what, label), value, tol)


def oracle_values(om, U):
    with np.errstate(all='ignore'):
        return np.column_stack([om.s(np.array(U, copy=True), k) for k in range(om.D)])


def check_premise(backend, label, Sk, So, z):
    """|S_kernel - S_oracle| <= tau / 2 at the returned rows: what tau rests on."""
    with np.errstate(all='ignore'):
        ratio = np.abs(Sk - So) / (0.5 * tau_of(z))
    fin = np.isfinite(So)
    worst = float(ratio[fin].max())
    print('%s: premise |S_kernel - S_oracle| / (tau / 2) = %.3e (1) on %d of %d searches' % (label, worst, int(fin.sum()), fin.size))
    record(backend, 'premise', label, worst, 1.0)
    assert np.array_equal(np.isfinite(Sk), fin)
    assert worst <= 1.0


def check_residual(backend, label, So, z, counts, own):
    """Every search that ended below 100 trial points ended on the stopping rule: |S_oracle(x) - z| <= 1e-9 + tau."""
    with np.errstate(all='ignore'):
        ratio = np.abs(So - z) / (THRESHOLD + tau_of(z))
    sel = (counts < 100) & own
    worst = float(ratio[sel].max()) if sel.any() else 0.0
    print('%s: largest |S_oracle(x) - z| / (1e-9 + tau) = %.4f (1) on %d searches below 100 trial points' % (label, worst, int(sel.sum())))
    record(backend, 'residual_over_bound', label, worst, 1.0)
    assert np.all(ratio[sel] <= 1.0)


def inside(x, a, b):
    return (x >= np.minimum(a, b)) & (x <= np.maximum(a, b))


def check_bisection(backend, name, rect, opts=(), kernel=None):
    tm, om, E, U0, z = case(backend, name, rect)
    label = label_of(backend, name, rect, 'bisect', opts)
    U, iters, counts, Sk = run(backend, name, rect, False, opts, kernel)
    D = om.D
    # the replay alone: decisive searches, the cap, the spread of the window shifts
    reps = replay_all(om, U, z)
    dec = np.column_stack([decisive(r, z[:, k]) for k, r in enumerate(reps)])
    hist, most = shift_histogram(reps)
    share = 1.0 - dec.mean()
    print('%s: %d searches, indecisive %.2f %% (5 %%), shifts 0 / 1 / 2 / >= 3: %s, most %d' % (label, dec.size, 100 * share, hist, most))
    record(backend, 'indecisive_share', label, share, CAP_SHARE)
    assert share <= CAP_SHARE
    assert min(hist) > 0
    So = oracle_values(om, U)
    check_premise(backend, label, Sk, So, z)
    # the kernel's columns
    own = U[:, E:]
    last = np.column_stack([r.last for r in reps])
    cnt = np.column_stack([r.count for r in reps])
    same = bits(own) == bits(last)
    print('%s: decisive %d, of them other bits %d, other counts %d; indecisive %d, of them the replay\'s bits %d; iters %s' % (
        label, int(dec.sum()), int(np.sum(dec & ~same)), int(np.sum(dec & (counts != cnt))), int(np.sum(~dec)), int(np.sum(~dec & same)), iters))
    assert np.array_equal(bits(own[dec]), bits(last[dec]))
    assert np.array_equal(counts[dec], cnt[dec])
    assert np.array_equal(iters, counts.max(axis=0))
    assert np.all(counts >= 1) and np.all(counts <= 100)
    # indecisive searches: inside the bracket of the window phase, and stopped by the rule
    wl, wh = np.column_stack([r.win_lo for r in reps]), np.column_stack([r.win_hi for r in reps])
    assert np.all(inside(own, wl, wh)[~dec])
    check_residual(backend, label, So, z, counts, np.ones_like(dec))
    # row 0 again under a cap
    with options(tm._lib, **dict(opts)):
        import torch
        Zs, Xc = load(tm, backend, E, U0, z)
        for capv in (np.zeros(D, dtype=np.int32), np.full(D, 3, dtype=np.int32), np.array(iters, dtype=np.int32)):
            cap = torch.from_numpy(capv).to(device_of(backend))
            rc, ic = entry(tm, backend, Zs, Xc, 1, False, cap=cap, plain=True)
            assert rc == 0
            if kernel is not None:
                assert last_kernel(tm) == kernel
            row = returned(Xc)[:1]
            rc_rep = replay_all(om, row, z[:1], cap=capv)
            d0 = np.array([bool(decisive(r, z[:1, k])[0]) for k, r in enumerate(rc_rep)])
            l0, c0 = np.array([r.last[0] for r in rc_rep]), np.array([r.count[0] for r in rc_rep])
            print('%s: row 0 under cap %s: iters %s, replay %s, decisive %s' % (label, capv, ic, c0, d0))
            assert np.all(ic <= capv)
            assert np.array_equal(bits(row[0, E:][d0]), bits(l0[d0])) and np.array_equal(ic[d0], c0[d0])
            assert np.all(inside(row[0, E:], np.array([r.win_lo[0] for r in rc_rep]), np.array([r.win_hi[0] for r in rc_rep]))[~d0])
    return counts


def check_newton(backend, name, rect, opts=(), kernel=None):
    tm, om, E, U0, z = case(backend, name, rect)
    label = label_of(backend, name, rect, 'newton', opts)
    U, iters, counts, Sk = run(backend, name, rect, True, opts, kernel)
    So = oracle_values(om, U)
    check_premise(backend, label, Sk, So, z)
    # the window phase is the bisection's: its bracket, replayed without a midpoint
    reps = replay_all(om, U, z, cap=np.zeros(om.D, dtype=np.int32))
    own = U[:, E:]
    wl, wh = np.column_stack([r.win_lo for r in reps]), np.column_stack([r.win_hi for r in reps])
    hist, most = shift_histogram(reps)
    out = ~inside(own, wl, wh)
    print('%s: shifts 0 / 1 / 2 / >= 3: %s, most %d; outside the bracket %d; iters %s, rows at 100: %d' % (
        label, hist, most, int(out.sum()), iters, int(np.sum(counts >= 100))))
    assert min(hist) > 0
    assert not out.any()
    check_residual(backend, label, So, z, counts, np.ones(own.shape, dtype=bool))
    if name in NO_ROW_AT_THE_LIMIT:
        assert counts.max() < 100
    assert np.array_equal(iters, counts.max(axis=0))
    assert np.all(counts >= 0) and np.all(counts <= 100)
    return counts


@pytest.mark.parametrize('name,rect', CASES)
def test_bisection_is_the_replayed_search(backend, name, rect):
    check_bisection(backend, name, rect)


@pytest.mark.parametrize('name,rect', CASES)
def test_newton_stays_in_the_replayed_bracket_and_ends_on_the_rule(backend, name, rect):
    newton = check_newton(backend, name, rect)
    bisect = run(backend, name, rect, False)[2]
    ratio = float(newton.sum()) / float(bisect.sum())
    print('%s/%s %s: trial points newton / bisection = %d / %d = %.3f' % (name, rect, backend, int(newton.sum()), int(bisect.sum()), ratio))
    record(backend, 'newton_over_bisection_counts', '%s/%s/%s' % (name, rect, backend), ratio)


# ------------------------------------------------------------------------------------------ every kernel family

@pytest.mark.gpu
@pytest.mark.parametrize('method', ['bisect', 'newton'])
def test_every_kernel_family_runs_the_same_search(method):
    """The device library's three kernel families by option, each named after every direct call (the host double follows the
    default plan whatever the options: there `special_cond` is the run of the generic search)."""
    families = [((), 'k_int_root<%s>'), ((('int_xprog', 2),), 'k_int_root_x<%s>'), ((('int_dense', 0),), 'k_inverse_%s')]
    for opts, kernel in families:
        kernel = kernel % method if '%s' in kernel else kernel
        (check_newton if method == 'newton' else check_bisection)('hip', 'spiral3', 'softplus', opts, kernel)


# ------------------------------------------------------------------------------------------ non-finite targets

def test_the_oracle_leaves_a_nan_target_at_the_first_midpoint():
    """The bisection half of the NaN contract against the oracle on the CPU: every comparison of the reference's loop is false on
    NaN, so the row keeps the first midpoint, 0.0, after one iteration - in the oracle and in the replay."""
    om, E, U, z = oracle_case('spiral3', 'softplus')
    zk = np.array(z[:, 0], copy=True)
    zk[5] = np.nan
    X = om.vectorized_root_search_bisection(np.array(U, copy=True), zk, 0)
    rep = replay_bisect(oracle_S(om, U, 0), zk)
    assert X[5, E] == 0.0 and rep.last[5] == 0.0 and rep.count[5] == 1 and rep.shifts[5] == 0
    assert not decisive(rep, zk)[5]
    assert np.array_equal(bits(X[1:, E]), bits(rep.last[1:]))


@pytest.mark.parametrize('method', ['bisect', 'newton'])
@pytest.mark.parametrize('name,rect', [('spiral3', 'softplus'), ('band5', 'exponential'), ('special_cond', 'softplus')])
def test_non_finite_targets_stay_in_their_row(backend, name, rect, method):
    """Two calls on copies of the targets, the second with z = NaN, +inf, -inf in rows 5, 130 and 256 of component D // 2.  Every
    other row, and the components in front of the poisoned one in those rows, have the same bits in both.  NaN: the bisection returns
    its first midpoint 0.0 after one iteration, Newton the start's hi, 2.0, with a count of 0.  Infinite targets: the call returns
    0 and iters <= 100."""
    tm, om, E, U0, z = case(backend, name, rect)
    newton = method == 'newton'
    D, kp = om.D, om.D // 2
    zp = np.array(z, copy=True)
    for n, v in POISON_ROWS:
        zp[n, kp] = v
    Zs, Xa = load(tm, backend, E, U0, z)
    Zp, Xb = load(tm, backend, E, U0, zp)
    rc_a, it_a = entry(tm, backend, Zs, Xa, N, newton, plain=True)
    rc_b, it_b = entry(tm, backend, Zp, Xb, N, newton, plain=True)
    assert rc_a == 0 and rc_b == 0
    A, B = returned(Xa), returned(Xb)
    assert np.array_equal(bits(A), bits(run(backend, name, rect, newton)[0]))
    rows = np.array([n for n, _ in POISON_ROWS])
    clean = np.ones(N, dtype=bool)
    clean[rows] = False
    print('%s/%s/%s %s: iters %s, poisoned %s; rows 5 / 130 / 256 of component %d: %s' % (name, rect, method, backend, it_a, it_b, kp, B[rows, E + kp]))
    assert np.array_equal(bits(A[clean]), bits(B[clean]))
    assert np.array_equal(bits(A[rows, :E + kp]), bits(B[rows, :E + kp]))
    assert np.all(it_b >= 0) and np.all(it_b <= 100)
    assert np.all(it_b[:kp] == it_a[:kp])
    # the NaN row alone, for its own count
    _, Xn = load(tm, backend, E, U0, zp)
    rc, it_n = entry(tm, backend, Zp, Xn, 1, newton, row0=5, plain=True)
    assert rc == 0
    got = returned(Xn)[5]
    assert np.array_equal(bits(got[:E + kp + 1]), bits(B[5, :E + kp + 1]))
    if newton:
        assert got[E + kp] == 2.0 and it_n[kp] == 0
    else:
        assert got[E + kp] == 0.0 and not np.signbit(got[E + kp]) and it_n[kp] == 1
