"""Time the Newton root search of the banded separable maps on the device-resident entry point (inverse_device).

    python tools/newton_bench.py [--root TREE] [--label NAME] [--commit ID] [--out FILE.json] [--launches 200] [--rounds 10] [--rows N]

Workloads: C5 N = 1e6, C2b N = 1e6, C3 N = 5e5 (bench.py's maps and coefficient fixtures).  Versions, alternated round by
round within the one process after a warm-up of every shape (the chip holds its clock only while it is kept busy: bench.py):
  newton   root_finder='newton' as the library plans it (k_band_newton / k_band_few_newton: with the bisection kernels
           instantiations of one template per shape, k_band_search / k_band_few_search)
  generic  the same call with option band_newton = 0 (k_inverse_newton) - left out where the library does not know the option
  table    the table inverse of the same build (k_band_inverse_ring / k_band_few_inverse), tables built beforehand
HIP events around every batch of launches; per version the median over the rounds of the mean launch time and the spread
(min, max over the rounds).  --root: the repository tree whose package is timed (a build of another commit in a second
directory: run the tool once per tree in the same GPU visit and compare the files).
Also reported: trial points (per-component maxima, as `iters` returns them), the share of the HBM roof on the algorithmic
bytes 8 (2 D + E) N and of the fp64 vector peak on 2 x 34 flops per trial point (22 FMA of the spline and its derivative,
the column, the Newton step), with the per-component maxima standing in for the mean number of trial points: an upper bound.
"""
import ctypes

import numpy as np

import benchlib

FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    args = benchlib.parser(__doc__, 200, 'C5,C2b,C3').parse_args()
    bench, res = benchlib.start(args)
    import torch
    res['workloads'] = {}
    for wl in args.workloads.split(','):
        tm, X, cfg = bench.build_map(wl, 0, n_override=args.rows or None, root_finder='newton', alternate_root_finding=False)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Z = tm._cols(D, N)
        tm.forward_device(tm._Xs, N, coef=coef, Z=Z)
        Xinv = tm._cols(d, N, zero=True)
        pin = benchlib.option(lib, 'band_newton', probe=True)
        iters = tm._zeros(D, dtype=torch.int32)

        def newton():
            # (the entry point itself, as _inverse_bisect calls it, with one counter: no host read-back between launches)
            lib.ttm_inverse_newton(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z), Z.shape[1], tm._ptr(Xinv),
                                   Xinv.shape[1], N, ctypes.c_void_p(iters.data_ptr()), tm._stream())

        def table():
            tm.inverse_device(Z, N, coef=coef, X=Xinv, table=True)

        def after(name, v):                              # round trip and trial points of the warm-up; the counter back to 0 for the next version
            v['round_trip_max'] = float((Xinv[:, :N] - tm._Xs[:, :N]).abs().max().item())
            if name != 'table':
                v['trial_points_max_per_component'] = iters.cpu().numpy().tolist()
            iters.zero_()

        versions = [('newton', -1, newton)] + ([('generic', 0, newton)] if pin else []) + [('table', -1, table)]
        info = benchlib.warm_up(versions, pin, 3, kernel, after)
        benchlib.keep_busy(versions[0][2], 20)
        benchlib.time_rounds(versions, info, pin, args.rounds, benchlib.per_round(args), settle=2)
        E = int(tm.skip_dimensions)
        gbytes = 8.0 * (2 * D + E) * N / 1e9
        for v in info.values():
            benchlib.summarise(v, gbytes, bench.HBM_PEAK_GBS)
            if 'trial_points_max_per_component' in v:
                tp = float(np.sum(v['trial_points_max_per_component']))
                v['fp64_frac_upper_bound'] = 2.0 * 34.0 * tp * N / (v['ms'] * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS
        out = {'N': N, 'D': D, 'algorithmic_gbytes': gbytes, 'versions': info}
        if 'generic' in info:
            out['newton_over_generic'] = info['generic']['ms'] / info['newton']['ms']
        out['newton_over_table_time'] = info['newton']['ms'] / info['table']['ms']
        res['workloads'][wl] = out
        benchlib.report(wl, info)
        del tm, Z, Xinv
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
