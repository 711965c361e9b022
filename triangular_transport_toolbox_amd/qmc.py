"""Host tables of the quasi-Monte Carlo reference draws (ttm_sobol_normal_fill, include/ttm.h): per column the 30 direction
numbers of a Sobol' dimension, optionally under Matousek's linear matrix scramble, and a 30-bit digital shift.

The plain direction numbers are torch's (torch.quasirandom.SobolEngine.sobolstate: the Joe-Kuo table built into torch, read on
the CPU, nothing is fetched); torch's limit of 21201 dimensions is this module's.  Row c of the tables is Sobol' dimension c.

Scrambling (S. Joe, F. Y. Kuo 2008 for the numbers; J. Matousek, "On the L2-discrepancy for anchored boxes", 1998, for the
scramble): per column c a 30 x 30 lower-triangular matrix L_c over GF(2) with unit diagonal - row i is output bit i, counted
from the most significant of the 30 - and a 30-bit shift, both from np.random.default_rng([seed, draw, c]).  The scrambled
direction number is L_c times the plain one, bits as GF(2) vectors, so the scrambled point of a row is L_c times its plain
point, XOR the shift: every column stays stratified, every projection keeps its net property, and each point is uniform.
Column c's tables are a function of (seed, draw, c) alone - not of col0 or ncols.  That independence is the contract; the
generator's bit stream is not.
"""
import collections
import functools

import numpy as np

BITS = 30
MAX_COLUMNS = 21201          # torch.quasirandom.SobolEngine.MAXDIM
MAX_ROWS = 1 << BITS         # the sequence has 30 index bits: row0 + N <= 2^30
SEQUENCES = ('random', 'sobol')

_DEVICE_KEPT = 8
_device = collections.OrderedDict()


@functools.lru_cache(maxsize=8)
def _plain(dimensions):
    """torch's direction numbers of the first `dimensions` Sobol' dimensions as a (dimensions, 30) uint32 array: [c][b] is XORed
    into the point when bit b of the row's Gray code is set."""
    from torch.quasirandom import SobolEngine
    state = SobolEngine(dimensions, scramble=False).sobolstate.numpy()
    assert state.shape == (dimensions, BITS) and state.min() >= 0 and state.max() < MAX_ROWS
    return np.ascontiguousarray(state.astype(np.uint32))


def _parity(x):
    x = x ^ (x >> np.uint32(16))
    x = x ^ (x >> np.uint32(8))
    x = x ^ (x >> np.uint32(4))
    x = x ^ (x >> np.uint32(2))
    x = x ^ (x >> np.uint32(1))
    return x & np.uint32(1)


_POS = (BITS - 1 - np.arange(BITS)).astype(np.uint32)                              # output bit i from the top is integer bit _POS[i]
_DIAG = (np.uint32(1) << _POS)                                                      # the unit diagonal of row i
_ABOVE = np.array([((MAX_ROWS - 1) >> (int(p) + 1)) << (int(p) + 1) for p in _POS], dtype=np.uint32)   # the input bits 0 .. i - 1 from the top
_CHUNK = 1024                                                                       # columns scrambled at once (30 x 30 words each)


def _scramble(seed, draw, col0, plain):
    """(L_c times the 30 plain direction numbers, the shift) of the columns col0 .. col0 + len(plain) - 1.  Only the generators
    are made column by column; the 30 rows of every matrix meet the 30 direction numbers of its column in one array operation."""
    ncols = len(plain)
    words = np.empty((ncols, BITS + 1), dtype=np.uint32)
    for j in range(ncols):
        words[j] = np.random.default_rng([seed, draw, col0 + j]).integers(0, MAX_ROWS, size=BITS + 1, dtype=np.uint32)
    dirs = np.empty((ncols, BITS), dtype=np.uint32)
    for lo in range(0, ncols, _CHUNK):
        rows = (words[lo:lo + _CHUNK, :BITS] & _ABOVE) | _DIAG                      # [c, i]: row i of L_c, random left of the diagonal
        bits = _parity(rows[:, :, None] & plain[lo:lo + _CHUNK, None, :])           # [c, i, b]: output bit i of direction number b
        dirs[lo:lo + _CHUNK] = np.bitwise_or.reduce(bits << _POS[None, :, None], axis=1)
    return dirs, words[:, BITS].copy()


def tables(seed, draw, col0, ncols, scramble=True):
    """(dirs, shift) of the Sobol' dimensions col0 .. col0 + ncols - 1: dirs uint32 (ncols, 30), shift uint32 (ncols,).
    scramble False: torch's plain direction numbers and a zero shift - seed and draw have no effect, and the point of a row,
    (q + 0.5) 2^-30, is torch's unscrambled point + 2^-31.  scramble True: column c under the matrix and the shift of
    (seed, draw, c)."""
    col0, ncols = int(col0), int(ncols)
    if col0 < 0 or ncols < 1:
        raise ValueError('col0 must be at least 0 and ncols at least 1')
    if col0 + ncols > MAX_COLUMNS:
        raise ValueError('Sobol\' direction numbers exist for %d columns, not for %d' % (MAX_COLUMNS, col0 + ncols))
    plain = _plain(col0 + ncols)[col0:]
    if not scramble:
        return plain.copy(), np.zeros(ncols, dtype=np.uint32)
    seed, draw = int(seed) % 2 ** 64, int(draw)
    if draw < 0:
        raise ValueError('draw must be at least 0')
    return _scramble(seed, draw, col0, plain)


def device_tables(seed, draw, col0, ncols, scramble, device):
    """tables(...) as two int32 tensors (the words are below 2^30) on `device`, views of ONE upload, kept for the most recent few
    keys: a repeated (seed, draw) launches the fill and nothing else.  A new draw - every call with draw=None, every replicate of
    an error bar - builds and uploads its tables first: host work of 10 to 40 us per column depending on the host, nearly all of it the column's generator (tools/qmc_bench.py times it)."""
    import torch
    key = (int(seed) % 2 ** 64 if scramble else 0, int(draw) if scramble else 0, int(col0), int(ncols), bool(scramble), str(device))
    hit = _device.get(key)
    if hit is None:
        dirs, shift = tables(key[0], key[1], col0, ncols, scramble)
        both = torch.from_numpy(np.concatenate((dirs.ravel(), shift)).view(np.int32)).to(device)
        hit = (both[:dirs.size], both[dirs.size:])
        _device[key] = hit
        while len(_device) > _DEVICE_KEPT:
            _device.popitem(last=False)
    else:
        _device.move_to_end(key)
    return hit
