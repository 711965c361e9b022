"""
The cache policy of the long band kernels' column streams (csrc/ttm_band_policy.h; template parameter POL of k_band_forward and
k_band_inverse_ring, option band_resident): with POL = 1 only pair slot 0 of every tile of Z - rows [0, 2048) of a tile of
4096 - is stored and loaded plainly, X, X' and the other half of Z move with non-temporal accesses.  Only cache-policy bits of
the instructions differ, so the policy must not change one bit of a result.

CPU: the gate is a function of sizes; a stand-alone C++ program (tests/band_policy_gate.cpp) includes the header and prints
its decision.  The option exists in the library and in the host test double.

GPU: forward map and table inverse with band_resident = 0 and then 3 in one process, through the harness of
tests/test_row_ownership.py (canary-filled allocations, poisoned pad rows): per setting the kernel's name, ownership of rows
[0, N), independence of the pad rows and the oracle at the owning tests' tolerance (1e-11: tests/test_band.py,
tests/test_band_linear.py); between the settings rows [0, N) of Z and X bit for bit.  u_loader = band_fwd = band_inv = 1 pass
the size gate at these N; band_cus = 1 / 2 give a chunk several tiles and a partial last one (one workgroup: 8195 rows are two
full tiles and three rows; two workgroups: chunks of 4128 rows - a full tile and 32 rows - and 4067).  The maps:

  c5     26 components of C5's shape (class 1, lag 2): more than the 24 slots of a ring, so the refilled ring (G = 4) - C5's own;
  cls2   10 components of class 2 (orders 5 / 3), cls3: 5 of class 3 (orders 7 / 6) - every table resident (G = 0).  Not 26: the
         oracle sums a component's offsets in another order, which these degrees amplify along the inversions in a row
         (tests/test_band.py holds 26 of them to 1e-10 and 5 to 1e-11 for that reason).  Class 3 with ten components is beyond
         1e-11 as well, whatever the policy: 1.1e-11 at N = 2047 under band_resident = 0 - the parent's kernel;
  own    tests/test_band_linear.py's 'mixed': seven components, spline only / linear only / both (OWN = true).

test_refilled_ring_of_the_higher_classes adds the G = 4 instantiations of classes 2 and 3 (26 components, the maps of
tests/test_band.py::test_ring_inverse_of_the_higher_degree_classes) at one size - names, ownership, pad rows and the bits between
the settings, WITHOUT a bound against the oracle: 26 inversions of degree 7 in a row amplify the oracle's other summation order
beyond the owning test's 1e-10 on this harness's rows whatever the policy (class 3 under band_resident = 0, the parent's kernel:
1.0004e-10 with the harness's targets, 1.43e-10 with 30 rows scaled by 3); how these kernels agree with the oracle is the owning
test's subject, on its own map.
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


# ---------------------------------------------------------------------------
# CPU: the gate
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gate(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('band_policy') / 'band_policy_gate')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'band_policy_gate.cpp')],
                   check=True)

    def run(N, ncomp, option, rows=0):
        out = subprocess.run([exe, str(N), str(ncomp), str(option), str(rows)], check=True, capture_output=True, text=True).stdout.split()
        return dict(decision=int(out[0]), resident_rows=int(out[1]), rows=int(out[2]))
    return run


def _resident_rows(N, rows, tile=4096, half=2048):
    """min(half, rows of the tile) over every tile of every chunk, counted tile by tile."""
    total = 0
    for c0 in range(0, N, rows):
        c1 = min(c0 + rows, N)
        for t0 in range(c0, c1, tile):
            total += min(half, min(t0 + tile, c1) - t0)
    return total


def test_gate_takes_the_headline_shape(gate):
    got = gate(1000000, 40, -1, 3936)
    assert got['decision'] == 3
    # 254 chunks of 3936 rows and one of 256: 52 % of Z, 166.5 MB
    assert got['resident_rows'] == 254 * 2048 + 256 == _resident_rows(1000000, 3936)
    assert gate(1000000, 40, -1)['rows'] == 3936                             # (what the planner cuts for 256 CUs)


def test_gate_declines_what_fits_the_cache_and_what_is_too_large_to_keep(gate):
    # the pair's three buffers are 63 MB: plain accesses already hit
    assert gate(65536, 40, -1)['decision'] == 0
    # Z fits (160 MB), the pair does not (480 MB): measured, no gain (csrc/ttm_band_policy.h)
    assert gate(500000, 40, -1)['decision'] == 0
    # the half would be about 350 MB
    big = gate(2100003, 40, -1)
    assert big['decision'] == 0
    assert big['resident_rows'] == _resident_rows(2100003, big['rows']) and big['resident_rows'] * 8 * 40 > 330e6
    # the measured sizes on either side of the upper bound: a half of 0.93 caches is kept, one of 1.25 caches is not
    assert gate(1300000, 40, -1) == dict(decision=3, resident_rows=_resident_rows(1300000, 5088), rows=5088)
    assert gate(1600000, 40, -1)['decision'] == 0
    # ... and right at the bounds, 64 components.  Z at the cache's size to the byte fits; one row more and it does not (chunks
    # of 4096 rows: half of the rows in pair slot 0)
    llc = 256 << 20
    n_fit = llc // (8 * 64)
    assert n_fit * 8 * 64 == llc and n_fit % 4096 == 0
    assert gate(n_fit, 64, -1, 4096)['decision'] == 0
    assert gate(n_fit + 1, 64, -1, 4096) == dict(decision=3, resident_rows=n_fit // 2 + 1, rows=4096)
    # chunks of half a tile - every row in pair slot 0: a half of n_fit rows fills the cache to the byte and is kept
    assert gate(n_fit, 64, -1, 2048)['decision'] == 0                        # (... but that is all of Z, which then fits)
    assert gate(2 * n_fit - 2048, 64, -1, 4096)['decision'] == 3 and gate(2 * n_fit, 64, -1, 4096) == dict(decision=3, resident_rows=n_fit, rows=4096)
    assert gate(2 * n_fit + 1, 64, -1, 4096)['decision'] == 0


def test_gate_counts_the_resident_rows_from_the_tile_geometry(gate):
    for N, rows in ((1, 32), (2047, 2048), (2049, 4128), (4097, 4128), (8195, 8224), (8195, 4128), (1000000, 3936), (1300000, 5088),
                    (1600000, 6272), (12289, 12320)):
        assert gate(N, 40, -1, rows)['resident_rows'] == _resident_rows(N, rows), (N, rows)


def test_gate_obeys_the_option(gate):
    assert gate(1000000, 40, 0, 3936)['decision'] == 0
    for option in (1, 2, 3):
        assert gate(33, 40, option)['decision'] == option                    # forced, whatever the size
        assert gate(1000000, 40, option, 3936)['decision'] == option
    assert gate(33, 40, -1)['decision'] == 0


def test_band_resident_is_an_option_of_the_host_double():
    with emu.install():
        emu._lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        try:
            for v in (0, 1, 2, 3, -1):
                assert emu._lib.ttm_set_option(b'band_resident', v) == 0
            assert emu._lib.ttm_set_option(b'band_residents', 0) != 0
        finally:
            emu._lib.ttm_reset_options()


@pytest.mark.gpu
def test_band_resident_is_an_option_of_the_device_library(ttm_opt):
    from triangular_transport_toolbox_amd import _capi
    lib = _capi.load()
    lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
    for v in (0, 1, 2, 3):
        assert lib.ttm_set_option(b'band_resident', v) == 0
    assert lib.ttm_set_option(b'band_residents', 0) != 0
    ttm_opt('band_resident', -1)


# ---------------------------------------------------------------------------
# GPU: the policy changes no bit
# ---------------------------------------------------------------------------
NS = (1, 2, 33, 2047, 2049, 4097, 8195)
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
        D, shape, scale, cls = {'c5': (26, (3, 1, 2), 0.3, 1), 'cls2': (10, (5, 3, 2), 0.04, 2), 'cls3': (5, (7, 6, 2), 0.04, 3),
                                'cls2_26': (26, (5, 3, 2), 0.04, 2), 'cls3_26': (26, (7, 6, 2), 0.04, 3)}[kind]
        tm, om, X, _ = _ring_map(D, n=NMAX, shape=shape, nm_scale=scale)
        assert tm._cm.u_h_cls == cls
    assert tm._cm.u_p_lag == 2
    return tm, om, X


def _both_settings(kind, N, cus, ttm_opt, tol=1e-11):
    from tests.test_row_ownership import Case, _band_on
    tm, om, X = _map(kind)
    _band_on(ttm_opt, cus=cus, ring=1)
    tm._pack_memo = None                                    # (a fresh coefficient vector: tables and images under these options)
    case = Case(tm, om, X, 0, N)
    got = {}
    for setting in (0, 3):
        ttm_opt('band_resident', setting)
        # (run_guarded: the name, ownership, independence of the pad rows, the oracle)
        fwd = case.forward('k_band_forward', 'alt', tol_z=tol)
        inv = case.inverse_table('k_band_inverse_ring', 'alt', tol=tol)
        assert fwd['kernel'] == 'k_band_forward' and inv['kernel'] == 'k_band_inverse_ring'
        got[setting] = (fwd['out']['Z'], inv['out']['X'])
    for a, b, what in zip(got[0], got[3], ('Z', 'X')):
        assert a.shape == b.shape and a.shape[1] == N
        differ = int((a.view(np.int64) != b.view(np.int64)).sum())
        assert differ == 0, '%s: %d entries of %s differ between band_resident = 0 and 3' % (kind, differ, what)


@pytest.mark.gpu
@pytest.mark.parametrize('cus', [1, 2])
@pytest.mark.parametrize('N', NS)
@pytest.mark.parametrize('kind', ['c5', 'cls2', 'cls3', 'own'])
def test_the_policy_changes_no_bit(kind, N, cus, ttm_opt):
    _both_settings(kind, N, cus, ttm_opt)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['cls2_26', 'cls3_26'])
def test_refilled_ring_of_the_higher_classes(kind, ttm_opt):
    _both_settings(kind, 4097, 2, ttm_opt, tol=float('inf'))               # (no bound against the oracle: module docstring)
