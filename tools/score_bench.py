"""Time the score of the pullback density (ttm_score) on the device-resident entry point (score_device).

    python tools/score_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out FILE.json] [--launches 200] [--rounds 10] [--workloads C5,linear_irbf,C2b,C3]

Workloads: C5 (d = 40, N = 1e6), C2b (N = 1e6), C3 (N = 5e5) - bench.py's maps and coefficient fixtures - and `linear_irbf`, the
long map with linear own terms of tools/band_linear_bench.py (d = 40, band 2, [k] + two iRBF, N = 1e6).  Versions, alternated
round by round within the one process after a warm-up of every version and a second of busy chip (the chip holds its clock only
while it is kept busy: bench.py):
  band      ttm_score as the library plans it (k_band_score), with g_scale and ld_affine - the raw-coordinate score of
            evaluate_pullback_score: two spline gathers per row and column
  band_std  the same without them - the score in standardised coordinates: one gather
  generic   option band_score = 0 (k_score_u, one row per thread), with g_scale and ld_affine
  forward   ttm_forward on the same sample buffer, Z into the score's output buffer (k_band_forward / k_band_few): the
            byte-equivalent yardstick - the score reads the same columns once and writes D columns once
HIP events around every batch of launches; per version the median over the rounds of the mean launch time and the spread (min,
max over the rounds), the kernel that ran (ttm_last_kernel) and the share of the HBM roof on the algorithmic bytes 8 N (d + D).
"""
import numpy as np

import band_linear_bench as blb
import benchlib


def build(bench, wl, rows):
    if wl != 'linear_irbf':
        tm, X, cfg = bench.build_map(wl, 0, n_override=rows or None)
        return tm
    from triangular_transport_toolbox_amd import specs
    return blb.build('linear_irbf', specs.sample_mixture(rows or blb.N, d=blb.D))


def main():
    args = benchlib.parser(__doc__, 200, 'C5,linear_irbf,C2b,C3').parse_args()
    bench, res = benchlib.start(args)
    res['workloads'] = {}
    for wl in args.workloads.split(','):
        tm = build(bench, wl, args.rows)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        pin = benchlib.option(lib, 'band_score')
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        E = d - D
        coef = tm._pack_coeffs()
        std = np.asarray(tm.X_std, dtype=float)[E:E + D]
        mean = np.asarray(tm.X_mean, dtype=float)[E:E + D]
        gs = tm._to_dev(np.ascontiguousarray(1.0 / std))
        af = tm._to_dev(np.ascontiguousarray(np.column_stack((std, mean))))
        G = tm._cols(D, N)

        def score_raw():
            tm.score_device(tm._Xs, N, coef=coef, G=G, g_scale=gs, ld_affine=af)

        def score_std():
            tm.score_device(tm._Xs, N, coef=coef, G=G)

        def forward():
            tm.forward_device(tm._Xs, N, coef=coef, Z=G)

        ref = {}

        def after(name, v):                              # the versions against each other
            if name == 'band':
                ref['band'] = G[:, :N].clone()
            elif name == 'generic':
                v['max_rel_diff_to_band'] = float(((G[:, :N] - ref['band']).abs() / (1.0 + ref['band'].abs())).max().item())

        versions = [('band', -1, score_raw), ('band_std', -1, score_std), ('generic', 0, score_raw), ('forward', -1, forward)]
        info = benchlib.warm_up(versions, pin, 3, kernel, after)
        ref.clear()
        benchlib.keep_busy(versions[0][2], 20)
        benchlib.time_rounds(versions, info, pin, args.rounds, benchlib.per_round(args), settle=2)
        gbytes = 8.0 * (d + D) * N / 1e9
        for v in info.values():
            benchlib.summarise(v, gbytes, bench.HBM_PEAK_GBS)
        out = {'N': N, 'D': D, 'd': d, 'algorithmic_gbytes': gbytes, 'versions': info,
               'band_over_forward_time': info['band']['ms'] / info['forward']['ms'],
               'generic_over_band_time': info['generic']['ms'] / info['band']['ms']}
        res['workloads'][wl] = out
        benchlib.report(wl, info)
        del tm, G
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
