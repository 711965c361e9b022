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


TEMPER_MAX = 64                   # candidates of one ttm_temper_scan (csrc/ttm_smc.h: TS_CMAX)


def temper_work_words(N, C):
    """8-byte words of the workspace of ttm_temper_scan (TTM_TEMPER_SCAN_WORK_WORDS)."""
    return 4 + (2 + 2 * int(C)) * ((int(N) + TILE - 1) // TILE)


def summary_of_words(w):
    """The four words of a ttm_weight_summary (a NumPy vector of 4 doubles) as a dict."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    i = w.view(np.int64)
    return {'max': float(w[0]), 'T': int(i[1]), 'S2': float(w[2]), 'n_bad': int(i[3])}


def temper_ess(words, N, K):
    """The effective sample size of every candidate of a ttm_temper_scan from its C x 4 summary words (NumPy), by the formula
    of importance_summary: (T / 2^K)^2 / S2; 0.0 for a candidate without a positive weight.  ValueError for bad entries."""
    out = []
    for row in np.asarray(words, dtype=np.float64).reshape(-1, 4):
        s = summary_of_words(row)
        out.append(importance_summary(s, N, K)['ess'] if s['T'] > 0 or s['n_bad'] > 0 else 0.0)
    return out


def temper_search(ess_of, span, target, C=64, rounds=3):
    """The next step delta in (0, span] of the tempering exponent: the largest candidate of a C-ary search whose effective sample
    size is still at least `target`.  ess_of(deltas) returns the ESS of every candidate of a list (one ttm_temper_scan and one
    small read-back); span = 1 - beta.
    Round 1: the candidates span * c / C, c = 1 .. C, the last one span itself; if that one passes (ESS >= target) the result is
    span.  Otherwise c* = the number of LEADING candidates that pass - a prefix, not a maximum: ESS(delta) does not increase
    (d log ESS / d delta = 2 (E_delta[l] - E_2delta[l]) <= 0) and a rounding that reorders two values must not move the result
    past a failing candidate.  Rounds 2 .. rounds: [lo, hi] = [candidate c* (or 0), candidate c* + 1] is cut into C equal parts and
    the C - 1 interior points are tried by the same rule.  Result: lo if positive, else the smallest positive candidate tried -
    progress is made even when no delta satisfies the target (fewer than `target` positive weights, say).
    A deterministic function of the ESS values alone; resolution span / C^rounds (span / 262144 by default)."""
    span, C, rounds = float(span), int(C), int(rounds)
    if not span > 0.0 or not 2 <= C <= TEMPER_MAX or rounds < 1:
        raise ValueError('span must be positive, C in [2, %d] and rounds at least 1' % TEMPER_MAX)
    cand = [span * c / C for c in range(1, C)] + [span]
    lo, hi, smallest = 0.0, span, None
    for r in range(rounds):
        if r > 0:
            cand = [x for x in (lo + (hi - lo) * c / C for c in range(1, C)) if lo < x < hi]
            if not cand:
                break
        ess = list(ess_of(cand))
        if len(ess) != len(cand):
            raise ValueError('ess_of must return one value per candidate')
        if r == 0 and ess[-1] >= target:
            return span
        smallest = cand[0] if smallest is None else min(smallest, cand[0])
        k = 0
        while k < len(cand) and ess[k] >= target:
            k += 1
        if k > 0:
            lo = cand[k - 1]
        if k < len(cand):
            hi = cand[k]
    return lo if lo > 0.0 else smallest


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
            self._host = summary_of_words(self.words.cpu().numpy())
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
