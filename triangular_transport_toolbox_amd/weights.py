"""Host side of the fixed-point importance weights (include/ttm.h: ttm_weight_scan, ttm_resample): the
constants of the contract and what is derived from the four-word summary.  The arithmetic on the rows is the library's."""
import math

import numpy as np

TILE = 1024                       # rows per scan tile (csrc/ttm_resample.h: RS_TILE)
PASS = 256                        # tiles per pass of the tile-sum scan (RS_PASS)
MAX_ROWS = 2 ** 30
SCHEMES = {'systematic': 0, 'stratified': 1, 'multinomial': 2}


def weight_bits(N):
    """K = min(40, 62 - ceil(log2 N)): the weights are multiples of 2^-K of the largest."""
    return min(40, 62 - (int(N) - 1).bit_length())


def work_words(N):
    """8-byte words of the workspace of ttm_weight_scan (TTM_WEIGHT_SCAN_WORK_WORDS)."""
    return 4 * ((int(N) + TILE - 1) // TILE)


def s2_depth(N):
    """Largest depth of the summation tree of S2 (include/ttm.h): its relative error is below (depth + 2) 2^-53."""
    tiles = (int(N) + TILE - 1) // TILE
    return 18 + (tiles + PASS - 1) // PASS


def lost_mass_bound(N):
    """Upper bound of the share of the total weight that the truncation to multiples of 2^-K drops: N 2^-K."""
    return int(N) * 2.0 ** -weight_bits(N)


def scheme_id(scheme):
    if scheme not in SCHEMES:
        raise ValueError('scheme must be one of %s, not %r' % (', '.join(repr(s) for s in SCHEMES), scheme))
    return SCHEMES[scheme]


class Weights:
    """What ttm_weight_scan left on the device: cum (N words, an int64 tensor: T <= 2^62), the summary (4 words) and, if asked
    for, q; K and N.  `summary()` reads the four words (one small copy, the only host synchronisation)."""

    def __init__(self, cum, words, N, K, q=None):
        self.cum, self.words, self.N, self.K, self.q = cum, words, int(N), int(K), q
        self._host = None

    def summary(self):
        if self._host is None:
            w = self.words.cpu().numpy()
            i = w.view(np.int64)
            self._host = {'max': float(w[0]), 'T': int(i[1]), 'S2': float(w[2]), 'n_bad': int(i[3])}
        return self._host

    def importance_summary(self):
        return importance_summary(self.summary(), self.N, self.K)


def importance_summary(s, N, K):
    """ess = (T / 2^K)^2 / S2, log_mean_weight = m + log T - K log 2 - log N (the log of the evidence estimate when
    logw = log p - log q), max = m, n_bad.  ValueError for bad entries or no valid weight."""
    if s['n_bad'] > 0:
        raise ValueError('%d of the %d log-weights are NaN or +inf' % (s['n_bad'], N))
    if s['T'] == 0:
        raise ValueError('no log-weight is finite: the total weight is 0')
    t = s['T'] / 2.0 ** K                 # (exact up to the rounding of T to 53 bits)
    return {'ess': t * t / s['S2'], 'log_mean_weight': s['max'] + math.log(s['T']) - K * math.log(2.0) - math.log(N),
            'max': s['max'], 'n_bad': 0}
