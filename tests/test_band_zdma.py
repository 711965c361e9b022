"""
The cut of k_band_forward / k_band_inverse_ring launches into whole tiles (option band_full_tiles), Z through LDS, two
columns deep, on the full tiles of k_band_inverse_ring (template parameter ZD, option band_zdma) and the slots of its refilled
ring (option band_ring_slots) - csrc/ttm_band_policy.h, csrc/ttm_band_image.h (the ring beside the two column buffers),
csrc/ttm_band.hip.  None changes what a row computes: only which workgroup owns it, by which path its z arrives and how far
ahead the tables are copied, so no bit of a result may move.

CPU: the planner is a function of sizes; a stand-alone C++ program (tests/band_cut_gate.cpp) includes the two headers and prints
the cut, the resident rows of that cut, the ring that is left beside the column buffers and - from band_ring_launch, the function
the host entry point itself calls - ZD and the ring of the launch.

GPU: forward map and table inverse with band_zdma = 0 and then 1 in one process under band_resident = 3 and band_full_tiles = 1,
through the harness of tests/test_row_ownership.py (canary-filled allocations, poisoned pad rows), as tests/test_band_resident.py
does: per setting the kernel's name, ownership of rows [0, N), independence of the pad rows, the oracle at 1e-11; between the
settings rows [0, N) of Z and X bit for bit.  The sizes: 4096, 8192 and 12288 rows are one, two and three full tiles (band_cus = 1:
in one workgroup, the trailing requests of a tile followed by the next tile's first two columns; band_cus = 2: 8192 rows are one full
tile each under the whole-tile cut), 4097 and 8195 put a partial tile - ZD = 0's code inside the ZD = 1 kernel - behind them;
1, 33 and 2047 rows have no full tile and the planner declines ZD = 1.  The launch names are the same for every instantiation, so
which one a launch took is held on the CPU side: band_cut_gate prints band_ring_launch (csrc/ttm_band_image.h), the one function
ttm_band::inverse plans its ring launch with, for these very sizes.  The maps:

  c5      26 components of C5's shape: the refilled ring (G = 4), 24 slots without the column buffers and 12 beside them;
  cls2    10 components of class 2, every table resident (G = 0): ten whole tables do not fit beside the column buffers, so the
          planner declines ZD = 1 here at every size - the launch must be the one of band_zdma = 0;
  cls2_8  8 components of class 2 (G = 0): they fit, ZD = 1 runs without a refill;
  own     tests/test_band_linear.py's 'mixed' (seven components).

The harness's targets scale the first N / 50 rows by 3.5 (the first waves of a workgroup take the outlier path);
test_outlier_rows_in_every_wave scales every 61st row by 3 instead, so that every wave has ordinary loads - table rows, tmin /
tmax - among its DMA requests and between a request and its counted wait.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'triangular_transport_toolbox_amd', 'csrc')

T_TABLE, NB, LDS_PER_CU = 1001, 1023, 160 * 1024           # the inverse tables of transport_map, the LDS of a CU of the MI355X


# ---------------------------------------------------------------------------
# CPU: the planner
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gate(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('band_cut') / 'band_cut_gate')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'band_cut_gate.cpp')],
                   check=True)

    def cut(N, cus=256, option=-1):
        out = subprocess.run([exe, 'cut', str(N), str(cus), str(option)], check=True, capture_output=True, text=True).stdout.split()
        return dict(rows=int(out[0]), grid=int(out[1]), rule=int(out[2]), resident_rows=int(out[3]))

    def ring(ncomp, N, cus, full_tiles=1, resident=3, zdma=1, slots=0, T=T_TABLE, lds=LDS_PER_CU):
        out = subprocess.run([exe, 'ring'] + [str(v) for v in (T, NB, ncomp, lds, N, cus, full_tiles, resident, zdma, slots)], check=True,
                             capture_output=True, text=True).stdout.replace('|', ' ').split()
        v = [int(x) for x in out]
        return dict(plain=dict(ok=v[0], R=v[1], G=v[2], lds=v[3]), beside=dict(ok=v[4], R=v[5], G=v[6], lds=v[7]), zd=v[8],
                    launch=dict(R=v[9], lds=v[10]))
    return type('Gate', (), dict(cut=staticmethod(cut), ring=staticmethod(ring)))


def _todays(N, cus=256):
    rows = ((N + cus - 1) // cus + 31) // 32 * 32
    return rows, (N + rows - 1) // rows


def test_cut_of_the_headline_shape_and_its_neighbours(gate):
    # 1e6 rows: 245 workgroups of 4096 rows, 244 of them a full tile, the last 576 rows
    got = gate.cut(1000000)
    assert (got['rows'], got['grid'], got['rule']) == (4096, 245, 1)
    assert got['resident_rows'] == 244 * 2048 + 576
    # 5e5 rows: 123 whole tiles would leave more than 1 / 16 of 256 CUs idle (123 < 240): today's cut
    assert _todays(500000) == (1984, 253)
    got = gate.cut(500000)
    assert (got['rows'], got['grid'], got['rule']) == (1984, 253, 0)
    # 256 whole tiles to the row; one row more needs a 257th workgroup: today's cut
    got = gate.cut(1048576)
    assert (got['rows'], got['grid'], got['rule']) == (4096, 256, 1)
    got = gate.cut(1048577)
    assert (got['rows'], got['grid'], got['rule']) == _todays(1048577) + (0,) == (4128, 255, 0)
    # the lower bound: 240 tiles are taken, 239 are not
    assert gate.cut(240 * 4096)['rule'] == 1 and gate.cut(239 * 4096)['rule'] == 0 and gate.cut(239 * 4096 + 1)['rule'] == 1


def test_cut_obeys_the_option(gate):
    assert (gate.cut(1000000, option=0)['rows'], gate.cut(1000000, option=0)['grid']) == _todays(1000000) == (3936, 255)
    assert gate.cut(1000000, option=0)['resident_rows'] == 254 * 2048 + 256
    got = gate.cut(500000, option=1)                       # forced: wherever whole tiles give every CU at most one chunk
    assert (got['rows'], got['grid'], got['rule']) == (4096, 123, 1)
    got = gate.cut(1048577, option=1)                      # ... which 257 tiles do not
    assert (got['rows'], got['grid'], got['rule']) == (4128, 255, 0)
    # the sizes of the GPU cases: band_cus = 1 / 2
    for N, cus, want in ((4096, 1, (4096, 1, 1)), (4097, 1, (4128, 1, 0)), (4097, 2, (4096, 2, 1)), (8192, 1, (8192, 1, 0)),
                         (8192, 2, (4096, 2, 1)), (8195, 2, (4128, 2, 0)), (12288, 1, (12288, 1, 0)), (12288, 2, (6144, 2, 0)),
                         (1, 1, (4096, 1, 1)), (2047, 2, (4096, 1, 1))):
        got = gate.cut(N, cus, 1)
        assert (got['rows'], got['grid'], got['rule']) == want, (N, cus, got)


def test_ring_beside_the_column_buffers(gate):
    # C5's geometry, 26 components (as the 40 of the headline): 24 windowed images, 12 beside the 64 KB of column buffers
    for ncomp in (26, 40):
        got = gate.ring(ncomp, 1000000, 256, full_tiles=-1, resident=-1, zdma=1)
        assert got['plain']['ok'] == 1 and (got['plain']['R'], got['plain']['G']) == (24, 4)
        assert got['beside']['ok'] == 1 and (got['beside']['R'], got['beside']['G']) == (12, 4)
        # (a window of 520 entries: 524 pairs {E_i, y_i}, images of 786 doubles)
        assert got['plain']['lds'] == 8 * (2 * 524 + 24 * 786) and got['beside']['lds'] == 8 * (2 * 524 + 12 * 786) + 65536 <= LDS_PER_CU
    # every table resident: eight whole tables fit beside the buffers, ten do not
    assert gate.ring(8, 8192, 1)['beside'] == dict(ok=1, R=8, G=0, lds=gate.ring(8, 8192, 1)['plain']['lds'] + 65536)
    assert gate.ring(10, 8192, 1)['plain']['ok'] == 1 and gate.ring(10, 8192, 1)['beside']['ok'] == 0 and gate.ring(10, 8192, 1)['zd'] == 0
    # less LDS: fewer than 3 G slots would be left
    assert gate.ring(26, 8192, 1, lds=128 * 1024)['plain']['ok'] == 1 and gate.ring(26, 8192, 1, lds=128 * 1024)['zd'] == 0


def test_zd_needs_a_full_tile_the_policy_and_the_option(gate):
    for N, cus, want in ((4096, 1, 1), (4097, 1, 1), (4097, 2, 1), (8195, 2, 1), (12288, 2, 1), (1, 1, 0), (33, 2, 0), (2047, 1, 0), (4095, 1, 0)):
        assert gate.ring(26, N, cus)['zd'] == want, (N, cus)
    assert gate.ring(26, 8192, 1, zdma=0)['zd'] == 0
    assert gate.ring(26, 8192, 1, resident=0)['zd'] == 0 and gate.ring(26, 8192, 1, resident=1)['zd'] == 0
    assert gate.ring(26, 8192, 1, resident=2)['zd'] == 1
    # auto: off - not a gain by the log's rule (OPTLOG round 15)
    for N in (1000000, 500000, 1300000):
        assert gate.ring(40, N, 256, full_tiles=-1, resident=-1, zdma=-1, slots=-1)['zd'] == 0


def test_slots_of_the_refilled_ring(gate):
    whole = 8 * (2 * 524 + 24 * 786)
    # auto: as many as fit (12 slots did not gain by the log's rule: OPTLOG round 15)
    for N, full_tiles in ((1000000, -1), (1000000, 0), (1300000, -1)):
        assert gate.ring(40, N, 256, full_tiles=full_tiles, resident=-1, zdma=-1, slots=-1)['launch'] == dict(R=24, lds=whole)
    assert gate.ring(40, 1000000, 256, full_tiles=-1, resident=-1, zdma=-1, slots=12)['launch'] == dict(R=12, lds=8 * (2 * 524 + 12 * 786))
    # the option: 0 as many as fit, a cap in whole groups of four and never below 3 G
    assert gate.ring(40, 1000000, 256, full_tiles=-1, resident=-1, zdma=-1, slots=0)['launch']['R'] == 24
    for slots, want in ((12, 12), (16, 16), (18, 16), (5, 12), (24, 24), (40, 24)):
        assert gate.ring(26, 8192, 1, zdma=0, slots=slots)['launch']['R'] == want, slots
    # ZD = 1 beside a cap: the smaller of the two
    assert gate.ring(26, 8192, 1, zdma=1, slots=16)['launch'] == dict(R=12, lds=8 * (2 * 524 + 12 * 786) + 65536)
    # a cap never asks for more than fits: with 128 KB of LDS nine slots are left beside the column buffers - declined, whatever the cap -
    # and the launch stays inside the LDS
    small = gate.ring(26, 8192, 1, zdma=1, slots=4, lds=128 * 1024)
    assert small['beside']['ok'] == 0 and small['zd'] == 0 and small['launch'] == dict(R=12, lds=8 * (2 * 524 + 12 * 786))
    # a ring without refill keeps every component
    assert gate.ring(10, 8192, 1, zdma=0, slots=12)['launch']['R'] == 10 and gate.ring(8, 8192, 1, zdma=1, slots=4)['launch']['R'] == 8


# ---------------------------------------------------------------------------
# GPU: neither the cut nor the path of z changes a bit
# ---------------------------------------------------------------------------
NS = (1, 33, 2047, 4096, 4097, 8192, 8195, 12288)
NMAX = max(NS)


@functools.lru_cache(maxsize=2)
def _map(kind):
    """(tm, om, X) trained on NMAX rows (the cases evaluate the first N of them, as tests/test_row_ownership.py does)."""
    if kind == 'own':
        from tests.test_band_linear import _build
        tm, om, X, _ = _build('mixed', n=NMAX)
        assert tm.D == 7
    else:
        from tests.test_band import _ring_map
        D, shape, scale, cls = {'c5': (26, (3, 1, 2), 0.3, 1), 'cls2': (10, (5, 3, 2), 0.04, 2), 'cls2_8': (8, (5, 3, 2), 0.04, 2)}[kind]
        tm, om, X, _ = _ring_map(D, n=NMAX, shape=shape, nm_scale=scale)
        assert tm._cm.u_h_cls == cls
    assert tm._cm.u_p_lag == 2
    return tm, om, X


def _both_settings(kind, N, cus, ttm_opt, zin=None, option='band_zdma', settings=(0, 1)):
    from tests.test_row_ownership import Case, _band_on
    tm, om, X = _map(kind)
    _band_on(ttm_opt, cus=cus, ring=1)
    ttm_opt('band_resident', 3)
    ttm_opt('band_full_tiles', 1)
    tm._pack_memo = None                                    # (a fresh coefficient vector: tables and images under these options)
    case = Case(tm, om, X, 0, N)
    if zin is not None:
        case.__dict__['Zin'] = zin(case)                    # (in place of the cached property)
    got = {}
    for setting in settings:
        ttm_opt(option, setting)
        # (run_guarded: the name, ownership, independence of the pad rows, the oracle)
        fwd = case.forward('k_band_forward', 'alt', tol_z=1e-11)
        inv = case.inverse_table('k_band_inverse_ring', 'alt', tol=1e-11)
        assert fwd['kernel'] == 'k_band_forward' and inv['kernel'] == 'k_band_inverse_ring'
        got[setting] = (fwd['out']['Z'], inv['out']['X'])
    for other in settings[1:]:
        for a, b, what in zip(got[settings[0]], got[other], ('Z', 'X')):
            assert a.shape == b.shape and a.shape[1] == N
            differ = int((a.view(np.int64) != b.view(np.int64)).sum())
            assert differ == 0, '%s: %d entries of %s differ between %s = %d and %d' % (kind, differ, what, option, settings[0], other)


@pytest.mark.gpu
@pytest.mark.parametrize('cus', [1, 2])
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('kind', ['c5', 'cls2', 'cls2_8', 'own'])
def test_z_through_lds_changes_no_bit(kind, N, cus, ttm_opt):
    _both_settings(kind, N, cus, ttm_opt)


@pytest.mark.gpu
@pytest.mark.parametrize('cus', [1, 2])
def test_outlier_rows_in_every_wave(cus, ttm_opt):
    def zin(case):
        Z = np.random.default_rng(11 + case.N).standard_normal((case.N, case.D))
        Z[::61] *= 3.0                                      # (a wave holds 128 consecutive rows of each half: two or three of these)
        return Z
    _both_settings('c5', 8195, cus, ttm_opt, zin=zin)


@pytest.mark.gpu
@pytest.mark.parametrize('N,cus', [(4097, 2), (8195, 1)])
def test_slots_of_the_ring_change_no_bit(N, cus, ttm_opt):
    """The refilled ring (26 components) with as many slots as fit (24), 12 and 16 of them, ZD = 0."""
    ttm_opt('band_zdma', 0)
    _both_settings('c5', N, cus, ttm_opt, option='band_ring_slots', settings=(0, 12, 16))


@pytest.mark.gpu
def test_the_options_exist_in_the_device_library(ttm_opt):
    import ctypes
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    for name in (b'band_full_tiles', b'band_zdma', b'band_ring_slots'):
        for v in (0, 1):
            assert lib.ttm_set_option(name, v) == 0
    assert lib.ttm_set_option(b'band_zdmas', 0) != 0
    ttm_opt('band_full_tiles', -1); ttm_opt('band_zdma', -1); ttm_opt('band_ring_slots', -1)
