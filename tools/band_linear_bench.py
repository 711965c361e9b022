"""Time the device-resident entry points on LONG banded separable maps whose monotone parts carry a linear own term.

    python tools/band_linear_bench.py [--root TREE] [--label NAME] [--commit ID] [--out FILE.json] [--launches 100] [--rounds 10] [--rows N]

Shapes: d = 40, band 2, N = 1e6 samples of specs.sample_mixture (the C5 ensemble), nonmonotone terms of C5, and as monotone
part  (a) `linear`: [[k]] alone - the order-1 transport filter;  (b) `linear_irbf`: [k] + two iRBF - example 05's
parameterisation.  Coefficients are drawn from a fixed seed (monotone 0.2 + 0.5 U, decaying nonmonotone), the same in
every tree.
Steps, alternated round by round within the one process after a warm-up of every step and a second of busy chip (the chip
holds its clock only while it is kept busy: bench.py):
  forward   ttm_forward, Z                          density   ttm_forward, Z + log-determinant + sum of squares
  logdet    ttm_forward, log-determinant alone      sumsq     ttm_forward, sum of squares alone (the two passes of the pullback density)
  table     ttm_inverse_table on tables built beforehand                newton    ttm_inverse_newton
HIP events around every batch of launches; per step the median over the rounds of the mean launch time and the spread (min,
max over the rounds), the kernel that ran (ttm_last_kernel) and the share of the HBM roof on the algorithmic bytes.
--root: the repository tree whose package is timed (a build of another commit in a second directory: run the tool once per
tree, one process each, in the same GPU visit and compare the files).
"""
import ctypes

import numpy as np

import benchlib

D, BAND, N = 40, 2, 1000000


def spec(which):
    non = []
    for k in range(D):
        nm = [[]]
        for j in range(max(0, k - BAND), k):
            nm += [[j], [j, j, 'HF'], [j, j, j, 'HF']]
        non.append(nm)
    mon = [[[k]] + (['iRBF %d' % k] * 2 if which == 'linear_irbf' else []) for k in range(D)]
    return mon, non


def build(which, X):
    """The map `which` on the ensemble X with its coefficients of the fixed seed (tools/score_bench.py times the same map)."""
    from triangular_transport_toolbox_amd.transport_map import transport_map
    mon, non = spec(which)
    tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, monotonicity='separable monotonicity')
    rng = np.random.default_rng(7)
    for k in range(D):
        tm.coeffs_mon[k] = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
        tm.coeffs_nonmon[k] = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
    return tm


def main():
    ap = benchlib.parser(__doc__, 100)
    ap.add_argument('--maps', default='linear,linear_irbf')
    args = ap.parse_args()
    bench, res = benchlib.start(args, 'launches_per_step')
    import torch
    from triangular_transport_toolbox_amd import specs
    res['maps'] = {}
    X = specs.sample_mixture(args.rows or N, d=D)
    for which in args.maps.split(','):
        tm = build(which, X)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        n, d = tm._N, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Z = tm._cols(D, n)
        tm.forward_device(tm._Xs, n, coef=coef, Z=Z)
        Zd = tm._cols(D, n)
        Xinv = tm._cols(d, n, zero=True)
        ld, ss = tm._empty(n), tm._empty(n)
        iters = tm._zeros(D, dtype=torch.int32)

        def newton():
            lib.ttm_inverse_newton(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z), Z.shape[1], tm._ptr(Xinv),
                                   Xinv.shape[1], n, ctypes.c_void_p(iters.data_ptr()), tm._stream())

        steps = [('forward', None, lambda: tm.forward_device(tm._Xs, n, coef=coef, Z=Zd)),
                 ('density', None, lambda: tm.forward_device(tm._Xs, n, coef=coef, Z=Zd, logdet=ld, sumsq=ss)),
                 ('logdet', None, lambda: tm.density_device(tm._Xs, n, coef=coef, logdet=ld)),
                 ('sumsq', None, lambda: tm.density_device(tm._Xs, n, coef=coef, sumsq=ss)),
                 ('table', None, lambda: tm.inverse_device(Z, n, coef=coef, X=Xinv, table=True)),
                 ('newton', None, newton)]
        cols = {'forward': 2 * D, 'density': 2 * D + 2, 'logdet': D + 1, 'sumsq': D + 1, 'table': 2 * D, 'newton': 2 * D}

        def after(name, v):                              # the step's algorithmic bytes, round trip and trial points of the warm-up launches
            v['algorithmic_gbytes'] = 8.0 * cols[name] * n / 1e9
            if name in ('table', 'newton'):
                v['round_trip_max'] = float((Xinv[:, :n] - tm._Xs[:, :n]).abs().max().item())
            if name == 'newton':
                v['trial_points_max_per_component'] = iters.cpu().numpy().tolist()

        info = benchlib.warm_up(steps, None, 3, kernel, after)
        benchlib.keep_busy(steps[0][2], 20)
        benchlib.time_rounds(steps, info, None, args.rounds, benchlib.per_round(args), settle=2)
        for v in info.values():
            benchlib.summarise(v, v['algorithmic_gbytes'], bench.HBM_PEAK_GBS)
        res['maps'][which] = {'N': n, 'D': D, 'u_p_lag': int(tm._cm.u_p_lag), 'u_h_cls': int(tm._cm.u_h_cls), 'u_h_ng': int(tm._cm.u_h_ng),
                              'steps': info}
        benchlib.report(which, info)
        del tm, Z, Zd, Xinv
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
