"""
Interval slopes in the resident-table images of k_band_inverse_ring (option band_slopes; csrc/ttm_band_image.h: the slope layout,
band_interval_slope, band_ring_plan; csrc/ttm_band.hip: template parameter SL of band_inverse_tile).  The kernel that builds a
table stores, per interval of the window, the slope the lookup used to form per row - the same device operations in the same
order - and the lookup reads it.  Nothing a row computes changes, so no bit of a result may move.

CPU: the plan is a function of sizes and the option; a stand-alone C++ program (tests/band_slope_gate.cpp) includes the headers
and prints it: which layout, the ring, the doubles per image (counted by hand beside the planner's), and the launch that
band_ring_launch - the function the host entry point calls - makes of it.

GPU: forward map and table inverse with band_slopes = 0 and then 1 in one process - a fresh coefficient vector per setting, so that
tables and images are built under it - through the harness of tests/test_row_ownership.py (canary-filled allocations, poisoned
pad rows): per setting the kernel's name, ownership of rows [0, N), independence of the pad rows and the oracle at 1e-11 (the bound
of tests/test_band_resident.py, on the same maps); between the settings rows [0, N) of X bit for bit.  The maps:

  c5     26 components of C5's shape: the refilled ring (G = 4), 24 slots without slopes, 12 with them;
  cls2   10 components of class 2, every table resident (G = 0): ten whole tables without slopes, ten windowed ones with them (the
         window differs between the settings - rows beyond it take the outlier path, which forms the slope per row);
  cls3   5 components of class 3 (G = 0): whole tables under both settings;
  own    tests/test_band_linear.py's 'mixed', seven components with linear own terms: whole tables under both settings;
  flat   5 components of C5's shape, one of them without its two edge terms: its monotone part is two saturating iRBF terms, so
         its table is FLAT over the first and the last quarter - tied entries at the table's start and inside the window.  Such a
         table is degenerate by the kernel's own rule (more tied entries in a bucket than the resident search compares), so every row
         of that component takes the outlier path; the other four take the slopes from the image.  (searchsorted-left never
         locates a tied interval except the first one, by clipping - include/ttm.h, THE TIE RULE - so no row can reach a tied
         interval's stored slope through the resident search; what IS reached is held here: the image build over tied entries, the
         degenerate header and the bucket index behind the slopes, and the rows of the rule.)  Which component: the first of 3, 2,
         1, 0 whose table the device reports sorted (an ulp of noise where a term saturates can make one unsorted).

The targets: standard normal, every 61st row scaled by 3 (outlier rows in every wave: a wave holds 128 consecutive rows of each
half of a tile), and from 2047 rows on rows placed by construction in component 0, whose target is z minus a constant:
  * on table nodes: z = S_0(y_i) by the library's forward map and its neighbours up to 3 ulp either way, so that the target
    falls on the node or immediately beside it on either side - at the nodes next to both ends of the window [240, 760) of the
    windowed plans, next to both ends of the whole table, and in the middle;
  * inside the first and the last interval of the window and of the whole table (midpoints of two such z);
  * far below and far above every table (z = -+50: clipped to the table's first / last entry);
  * on the flat table start ('flat'): targets far below the flat component's table are clipped onto its tied first entries - the
    first interval, of width 0, where the slope meets the 1e-300 floor: the result must be the first abscissa, -10, to the bit
    under both settings (THE TIE RULE; the oracle's interp1d gives NaN there).  Every other target below that table is clipped
    onto the flat start as well - a good part of all rows.  The flat component and all behind it have no bound against the
    oracle (the reason stands where `held` is set); the components in front of it keep 1e-11;
  * a NaN target in the last component (it reaches no other column; the oracle is held on every other entry, and the NaN itself
    must be a NaN under both settings).

test_image_slopes_are_the_one_function holds the image itself: the slopes read back from the device equal band_interval_slope of
the image's own xs (the table entry in front of the window for the first) and np.linspace's abscissae, bit for bit - evaluated on
the device by a few-line kernel (tests/band_slope_probe.hip, compiled with the library's flags and run as a process of its own).
For 'flat' the image must hold tied intervals, at the table's start among them, each with the finite slope of the floor.

test_z_through_lds_on_images_without_slopes: with band_slopes on by default a coefficient vector packed under band_zdma = 0 has
images with slopes, which ZD = 1 never takes; here the vector is packed under band_zdma = 1 - images without slopes, as the plan
of tests/band_slope_gate.cpp says - and ZD = 1 is held to ZD = 0 bit for bit on those images (tests/test_band_zdma.py's harness).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.hostemu import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'triangular_transport_toolbox_amd', 'csrc')

T_TABLE, NB, LDS_PER_CU = 1001, 1023, 160 * 1024           # the inverse tables of transport_map, the LDS of a CU of the MI355X
HDR, INDEX = 6, 256                                         # doubles of an image's header and of its bucket index (nb + 1 = 1024 uint16)


# ---------------------------------------------------------------------------
# CPU: the plan
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gate(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('band_slope') / 'band_slope_gate')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'band_slope_gate.cpp')],
                   check=True)

    def plan(ncomp, slopes=-1, zdma=0, N=1000000, cus=256, T=T_TABLE, lds=LDS_PER_CU):
        out = subprocess.run([exe] + [str(v) for v in (T, NB, ncomp, lds, N, cus, slopes, zdma)], check=True, capture_output=True,
                             text=True).stdout.replace('|', ' ').split()
        v = [int(x) for x in out]
        return dict(ok=v[0], slopes=v[1], R=v[2], G=v[3], W=v[4], w0=v[5], doubles=v[6], counted=v[7], lds=v[8],
                    launch=dict(zd=v[9], R=v[10], slopes=v[11], lds=v[12]))
    return plan


def _weven(W):
    return (W + 4 + 1) & ~1


def test_the_headline_geometry_takes_the_slopes_in_a_ring_of_twelve(gate):
    for ncomp in (40, 26, 25):
        off, on = gate(ncomp, slopes=0), gate(ncomp, slopes=1)
        assert (off['ok'], off['slopes'], off['R'], off['G'], off['W'], off['w0']) == (1, 0, 24, 4, 520, 240)
        assert (on['ok'], on['slopes'], on['R'], on['G'], on['W'], on['w0']) == (1, 1, 12, 4, 520, 240)
        assert off['doubles'] == HDR + 524 + INDEX == 786 and on['doubles'] == HDR + 2 * 524 + INDEX == 1310
        assert off['lds'] == 8 * (2 * 524 + 24 * 786) and on['lds'] == 8 * (2 * 524 + 12 * 1310) <= LDS_PER_CU
        assert on['launch'] == dict(zd=0, R=12, slopes=1, lds=on['lds'])


def test_resident_maps_stay_resident(gate):
    # ten components: whole tables without slopes, windowed ones with them - resident (G = 0) under both
    off, on = gate(10, slopes=0), gate(10, slopes=1)
    assert (off['slopes'], off['R'], off['G'], off['W'], off['w0']) == (0, 10, 0, 1001, 0)
    assert (on['slopes'], on['R'], on['G'], on['W'], on['w0']) == (1, 10, 0, 520, 240)
    # five and seven: whole tables with their slopes fit
    for ncomp in (5, 7):
        on = gate(ncomp, slopes=1)
        assert (on['slopes'], on['R'], on['G'], on['W'], on['doubles']) == (1, ncomp, 0, 1001, HDR + 2 * 1006 + INDEX)
    # twenty (up to twenty-four) fit without slopes and do not with them: OFF, today's plan to the byte
    for ncomp in (15, 20, 24):
        off, on = gate(ncomp, slopes=0), gate(ncomp, slopes=1)
        assert on == off and (on['slopes'], on['R'], on['G'], on['doubles']) == (0, ncomp, 0, 786)


def test_no_plan_today_no_plan_with_slopes(gate):
    # 64 KB of LDS: eight slots of today's images - no ring, whatever the option
    for slopes in (-1, 0, 1):
        assert gate(40, slopes=slopes, lds=64 * 1024)['ok'] == 0
    # 128 KB: today's ring has 16 slots; with slopes eleven would be left - fewer than 3 G: OFF
    off, on = gate(40, slopes=0, lds=128 * 1024), gate(40, slopes=1, lds=128 * 1024)
    assert on == off and (on['ok'], on['slopes'], on['R'], on['G']) == (1, 0, 16, 4)


def test_the_option_and_zd(gate):
    for ncomp in (40, 10, 5):
        assert gate(ncomp, slopes=0)['slopes'] == 0 and gate(ncomp, slopes=1)['slopes'] == 1
        assert gate(ncomp, slopes=-1) in (gate(ncomp, slopes=0), gate(ncomp, slopes=1))
    # ZD = 1 never beside images with slopes
    for ncomp, N, cus in ((40, 1000000, 256), (26, 8192, 1), (8, 8192, 1), (5, 8192, 1)):
        on = gate(ncomp, slopes=1, zdma=1, N=N, cus=cus)
        assert on['slopes'] == 1 and on['launch']['zd'] == 0 and on['launch']['slopes'] == 1
    assert gate(26, slopes=0, zdma=1, N=8192, cus=1)['launch'] == dict(zd=1, R=12, slopes=0, lds=8 * (2 * 524 + 12 * 786) + 65536)


def test_doubles_per_image_are_header_window_slopes_index(gate):
    for T in (64, 257, 1001, 2048):
        for ncomp in (5, 10, 20, 26, 40):
            for slopes in (0, 1):
                for lds in (LDS_PER_CU, 128 * 1024, 64 * 1024):
                    p = gate(ncomp, slopes=slopes, T=T, lds=lds)
                    if not p['ok']:
                        continue
                    assert p['doubles'] == p['counted'] == HDR + (2 if p['slopes'] else 1) * _weven(p['W']) + INDEX, (T, ncomp, slopes, lds, p)
                    assert p['doubles'] % 2 == 0 and p['lds'] == 8 * (2 * _weven(p['W']) + p['R'] * p['doubles']) <= lds
                    assert p['G'] == 0 and p['R'] == ncomp or p['G'] == 4 and p['R'] >= 12 and p['R'] % 4 == 0
                    assert p['G'] == 0 or p['doubles'] <= 2048                          # (a refill: one 1 KB piece per wave, 16 waves)


def test_the_option_exists_in_the_host_double():
    with emu.install():
        emu._lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        try:
            for v in (-1, 0, 1):
                assert emu._lib.ttm_set_option(b'band_slopes', v) == 0
            assert emu._lib.ttm_set_option(b'band_slope', 0) != 0
        finally:
            emu._lib.ttm_reset_options()


# ---------------------------------------------------------------------------
# GPU: the slopes change no bit
# ---------------------------------------------------------------------------
NS = (1, 33, 2047, 4096, 4097, 8195)
NMAX = max(NS)
NODES = (1, 2, 3, 240, 241, 242, 243, 500, 501, 756, 757, 758, 759, 997, 998, 999)    # both ends of [240, 760) and of [0, 1001), the middle
INSIDE = ((1, 2), (241, 242), (242, 243), (757, 758), (758, 759), (998, 999))       # first / last intervals: midpoints of two nodes' z
ULPS = (-3, -2, -1, 0, 1, 2, 3)


def _flatten_one(tm, om):
    """Takes the edge terms (LET, RET: the first and the last monotone coefficient) from one component of both maps, so that its
    table is flat where its iRBF terms saturate; returns the component: the first of 3, 2, 1, 0 whose table the device reports
    sorted and whose first two entries are tied."""
    for k in (3, 2, 1, 0):
        keep = tm.coeffs_mon[k].copy()
        for m in (tm, om):
            m.coeffs_mon[k][0] = 0.0
            m.coeffs_mon[k][-1] = 0.0
        tm._pack_memo = None
        coef = tm._pack_coeffs()
        tm._inverse_table(coef, 0, tm.D, None, None, 0)     # (tables only)
        tm._sync_stream()
        entry = next(iter(coef._ttm_tables.values()))
        row = entry[0].cpu().numpy().reshape(tm.D, T_TABLE)[k]
        if entry[4] and row[0] == row[1] and (np.diff(row[240:760]) == 0).any():
            tm._pack_memo = None
            return k
        for m in (tm, om):
            m.coeffs_mon[k] = keep.copy()
    raise AssertionError('no component of the map has a sorted table with a flat start')


@functools.lru_cache(maxsize=2)
def _map(kind):
    """(tm, om, X) trained on NMAX rows (the cases evaluate the first N of them, as tests/test_row_ownership.py does)."""
    if kind == 'own':
        from tests.test_band_linear import _build
        tm, om, X, _ = _build('mixed', n=NMAX)
        assert tm.D == 7
    else:
        from tests.test_band import _ring_map
        D, shape, scale, cls = {'c5': (26, (3, 1, 2), 0.3, 1), 'cls2': (10, (5, 3, 2), 0.04, 2), 'cls3': (5, (7, 6, 2), 0.04, 3),
                                'flat': (5, (3, 1, 2), 0.3, 1)}[kind]
        tm, om, X, _ = _ring_map(D, n=NMAX, shape=shape, nm_scale=scale)
        assert tm._cm.u_h_cls == cls
        if kind == 'flat':
            tm._flat_k = _flatten_one(tm, om)
    assert tm._cm.u_p_lag == 2
    return tm, om, X


@functools.lru_cache(maxsize=4)
def _node_z(kind):
    """z = S_0(y_i) of component 0 at the table's abscissae y_i, i in NODES, by the library's forward map."""
    tm, _, _ = _map(kind)
    tm._ensure_pts(T_TABLE, 10)
    n = len(NODES)
    Xs = tm._cols(tm._cm.d_cols, n, zero=True)
    Xs[0, :n] = tm._to_dev(np.ascontiguousarray(tm._pts[list(NODES)]))
    Z = tm.forward_device(Xs, n)
    tm._sync_stream()
    return dict(zip(NODES, Z[0, :n].cpu().numpy().tolist()))


@functools.lru_cache(maxsize=32)
def _targets(kind, N):
    """(Zin, rows whose last column is NaN, rows clipped onto the flat start of component tm._flat_k, the oracle's inverse of Zin
    with 0 in place of the NaN) - once per map and size"""
    tm, om, _ = _map(kind)
    D = tm.D
    flat_rows = np.zeros(0, dtype=int)
    Z = np.random.default_rng(23 + N).standard_normal((N, D))
    Z[::61] *= 3.0                                          # (outlier rows in every wave)
    nan_rows = np.zeros(0, dtype=int)
    if N >= 2047:
        zn = _node_z(kind)
        col = []
        for i in NODES:
            base = np.float64(zn[i])
            for u in ULPS:
                v = base
                for _ in range(abs(u)):
                    v = np.nextafter(v, np.inf if u > 0 else -np.inf)
                col.append(v)
        col += [0.5 * (zn[a] + zn[b]) for a, b in INSIDE]
        col += [-50.0, 50.0]
        rows = 7 + 13 * np.arange(len(col))                 # (spread over the waves of the first tile's first half; never a multiple of 61 twice in a row)
        assert rows.max() < 2047
        Z[rows, 0] = col
        nan_rows = np.array([5, 1029, 2046])
        Z[nan_rows, D - 1] = np.nan
        if kind == 'flat':
            flat_rows = np.array([9, 70, 1033, 2040])       # (70: also one of the wave's scaled rows' neighbours; four waves)
            Z[flat_rows, tm._flat_k] = [-50.0, -1e3, -50.0, -7.5]
    with np.errstate(all='ignore'):                         # (interp1d's inf * 0 on the flat start)
        Xo = om.inverse_map(np.where(np.isnan(Z), 0.0, Z))   # (a NaN target reaches its own entry only)
    Xo.setflags(write=False)                                # (shared among the cases: left unchanged)
    return Z, nan_rows, flat_rows, Xo


def _both_settings(kind, N, cus, resident, ttm_opt):
    from tests.test_row_ownership import Buf, Case, _band_on, run_guarded
    from tests.util import relerr
    tm, om, X = _map(kind)
    _band_on(ttm_opt, cus=cus, ring=1)
    ttm_opt('band_resident', resident)
    ttm_opt('band_zdma', 0)
    case = Case(tm, om, X, 0, N)
    Zin, nan_rows, flat_rows, Xo = _targets(kind, N)
    held = np.ones(Zin.shape, dtype=bool)                   # entries held to the oracle
    isnan = np.zeros(Zin.shape, dtype=bool)
    isnan[nan_rows, case.D - 1] = True
    held[isnan] = False
    ruled = np.zeros(Zin.shape, dtype=bool)                 # entries of the flat component the oracle answers with interp1d's NaN
    if kind == 'flat':
        # every target below the flat component's table is clipped onto its tied first entries: the oracle has NaN there and in the
        # columns behind it, the library the first abscissa (THE TIE RULE) - a good part of the rows, the range of two iRBF terms is short
        ruled[:, tm._flat_k] = np.isnan(Xo[:, tm._flat_k])
        assert ruled[flat_rows, tm._flat_k].all() and (N < 2047 or ruled.sum() > len(flat_rows))
        # No bound against the oracle for the flat component and all behind it: the two tables come from two erf implementations
        # and differ in their last bits, and a table's inverse amplifies that by 0.02 / (x_hi - x_lo) - without limit where the table
        # flattens (the first of the tied last entries is grid point 737 in one table and 736 in the other: 3.5e-3).  They are held
        # to the rule, to finiteness and to each other under the two settings; the components in front of it to the oracle at 1e-11.
        held[:, tm._flat_k:] = False

    def launch(t):
        tm.inverse_device(t['Z'], N, X=t['X'], table=True)
        return {}

    def check(out, red):
        got = case._raw(out['X'])
        assert np.isnan(got[isnan]).all() and np.isfinite(got[~isnan]).all()
        if kind == 'flat':
            # THE TIE RULE: a target clipped onto a flat start returns the first abscissa, -10 in standardised coordinates
            assert (out['X'].T[ruled] == -10.0).all(), out['X'].T[ruled][:8]
        err = relerr(got[held], Xo[held])
        print('%s N=%d cus=%d resident=%d: table inverse against the oracle %.3e' % (kind, N, cus, resident, err))
        assert err < 1e-11, ('table inverse', err)

    got = {}
    for setting in (0, 1):
        ttm_opt('band_slopes', setting)
        tm._pack_memo = None                                # (a fresh coefficient vector: tables and images under this setting)
        fwd = case.forward('k_band_forward', 'alt', tol_z=1e-11)
        bufs = {'Z': Buf('in', case.D, Zin.T), 'X': Buf('inout', case.d, case.Xs, n_in=case.E)}
        inv = run_guarded(tm, N, bufs, launch, 'k_band_inverse_ring', 'alt', check=check)
        assert fwd['kernel'] == 'k_band_forward' and inv['kernel'] == 'k_band_inverse_ring'
        # the images follow the setting: doubles per image as the plan of tests/band_slope_gate.cpp counts them
        img = next(iter(tm._pack_coeffs()._ttm_tables.values()))[5]
        per = img.numel() // case.D
        assert per == int(tm._lib.ttm_inverse_table_image_doubles(tm._pp, 0, case.D, T_TABLE, NB))
        W = {('c5', 0): 520, ('c5', 1): 520, ('cls2', 0): 1001, ('cls2', 1): 520}.get((kind, setting), 1001)
        assert per == HDR + (1 + setting) * _weven(W) + INDEX, (kind, setting, per)
        got[setting] = (fwd['out']['Z'], inv['out']['X'])
    for a, b, what in zip(got[0], got[1], ('Z', 'X')):
        assert a.shape == b.shape and a.shape[1] == N
        differ = int((a.view(np.int64) != b.view(np.int64)).sum())
        assert differ == 0, '%s: %d entries of %s differ between band_slopes = 0 and 1' % (kind, differ, what)


@pytest.mark.gpu
@pytest.mark.parametrize('resident,cus', [(0, 1), (3, 2), (3, 1), (0, 2)])
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('kind', ['c5', 'cls2', 'cls3', 'own', 'flat'])
def test_slopes_from_the_image_change_no_bit(kind, N, resident, cus, ttm_opt):
    _both_settings(kind, N, cus, resident, ttm_opt)


@pytest.mark.gpu
def test_the_option_exists_in_the_device_library(ttm_opt):
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    for v in (-1, 0, 1):
        assert lib.ttm_set_option(b'band_slopes', v) == 0
    assert lib.ttm_set_option(b'band_slope', 0) != 0
    ttm_opt('band_slopes', -1)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['c5', 'own', 'flat'])
def test_image_slopes_are_the_one_function(kind, ttm_opt, tmp_path):
    """c5: windowed images (the first window entry's x_lo is the table entry in front of the window); own: whole tables (entry 0 has
    no interval below it: 0)."""
    from triangular_transport_toolbox_amd import build as ttm_build
    from tests.test_row_ownership import _band_on
    tm, _, _ = _map(kind)
    _band_on(ttm_opt, ring=1)
    ttm_opt('band_slopes', 1)
    tm._pack_memo = None
    coef = tm._pack_coeffs()
    tm._inverse_table(coef, 0, tm.D, None, None, 0)         # (tables only)
    tm._sync_stream()
    entry = next(iter(coef._ttm_tables.values()))
    tab, img = entry[0].cpu().numpy().reshape(tm.D, T_TABLE), entry[5].cpu().numpy().reshape(tm.D, -1)
    W = 520 if kind == 'c5' else 1001
    w0, We = (T_TABLE - W) // 2, _weven(W)
    assert img.shape[1] == HDR + 2 * We + INDEX
    xs, sl = img[:, HDR:HDR + We], img[:, HDR + We:HDR + 2 * We]
    assert np.array_equal(xs[:, :W], tab[:, w0:w0 + W]) and np.isinf(xs[:, W:]).all()
    y = tm._pts                                             # np.linspace: the abscissae a lookup computes as i * step + y0, to the bit
    i0 = 1 if w0 == 0 else 0                                # (window entries with an interval below them: [i0, W))
    x_hi, x_lo = xs[:, i0:W], np.concatenate((tab[:, w0 + i0 - 1:w0 + i0], xs[:, i0:W - 1]), axis=1)
    y_hi, y_lo = np.broadcast_to(y[w0 + i0:w0 + W], x_hi.shape), np.broadcast_to(y[w0 + i0 - 1:w0 + W - 1], x_hi.shape)
    quad = np.ascontiguousarray(np.stack((x_lo, x_hi, y_lo, y_hi), axis=-1).reshape(-1, 4))
    # band_interval_slope on the device: a few-line kernel with the library's flags, a process of its own
    exe, fin, fout = str(tmp_path / 'band_slope_probe'), str(tmp_path / 'in.f64'), str(tmp_path / 'out.f64')
    flags = [f for f in ttm_build.FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.run([ttm_build.hipcc_path()] + flags + ['-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'band_slope_probe.hip')], check=True)
    quad.tofile(fin)
    subprocess.run([exe, fin, fout], check=True, timeout=120)
    want = np.fromfile(fout, dtype=np.float64).reshape(x_hi.shape)
    assert np.isfinite(want).all() and (want > 0).all()
    got = sl[:, i0:W]
    differ = int((got.view(np.int64) != want.view(np.int64)).sum())
    assert differ == 0, '%d of %d slopes differ from band_interval_slope of the image\'s own entries' % (differ, got.size)
    # no interval: 0 (entry 0 of a whole table, the sentinels)
    assert (sl[:, :i0] == 0).all() and (sl[:, W:] == 0).all()
    # a tied interval meets the floor: (y_hi - y_lo) * rcp(1e-300)
    tied = x_hi == x_lo
    print('%s: %d slopes, %d of tied intervals' % (kind, got.size, int(tied.sum())))
    assert (got[tied] > 1e290).all() and np.isfinite(got[tied]).all()
    if kind == 'flat':
        k = tm._flat_k
        # tied entries at the table's start and inside the window [240, 760) of the windowed plans, each with the slope of the floor
        assert tab[k, 0] == tab[k, 1] and tied[k, 0] and tied[k, 239:759].any() and int(tied[k].sum()) > 100, int(tied[k].sum())
        step = (y[1] - y[0])
        assert (got[k][tied[k]] >= 0.5 * step * 1e300).all() and (got[k][tied[k]] <= 2.0 * step * 1e300).all()
        # ... and the table is degenerate by the kernel's rule: header int32 {entries per bucket at most, 0}, {degenerate, 0}
        hdr = img[k, 4:6].view(np.int32)
        assert hdr[0] > 4 and hdr[2] == 1, hdr


@pytest.mark.gpu
@pytest.mark.parametrize('kind,N,cus,scaled', [('c5', 8195, 1, True), ('c5', 4097, 2, False), ('cls2_8', 8192, 1, False), ('own', 12288, 2, False)])
def test_z_through_lds_on_images_without_slopes(kind, N, cus, scaled, ttm_opt):
    from tests import test_band_zdma as zd

    def zin(case):
        Z = np.random.default_rng(11 + case.N).standard_normal((case.N, case.D))
        Z[::61] *= 3.0
        return Z
    # band_zdma = 1 first: the vector is packed and its images are built under it, then ZD = 0 on the same images
    zd._both_settings(kind, N, cus, ttm_opt, zin=zin if scaled else None, settings=(1, 0))
    tm = zd._map(kind)[0]
    img = next(iter(tm._pack_coeffs()._ttm_tables.values()))[5]
    W = 520 if kind == 'c5' else 1001
    assert img.numel() // tm.D == HDR + _weven(W) + INDEX      # (no slopes: the images ZD = 1 takes)
