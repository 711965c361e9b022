"""Time the quasi-Monte Carlo reference draws (ttm_sobol_normal_fill) beside the counter-based ones (ttm_normal_fill), and measure what they buy.

    python tools/qmc_bench.py [--root TREE] [--label NAME] [--commit ID] [--out profiles/qmc_bench.json] [--launches 200] [--rounds 10]
                              [--workloads C5,C2b] [--rows N] [--error-rows 4096,16384,65536] [--error-draws 32] [--truth-rows 1048576]

Workloads: C5 (40 columns, N = 1e6) and C2b (2 columns, N = 1e6) - bench.py's maps and coefficient fixtures.  Versions, alternated
round by round within the one process after a warm-up of every version and a second of busy chip (the chip holds its clock only
while it is kept busy: bench.py), all on the same buffers:
  philox                reference_device: one launch of k_normal_fill
  sobol                 reference_device(sequence='sobol'): one launch of k_sobol_normal_fill, the tables resident
  sobol_fresh           the same with a NEW draw number on every launch - what draw=None and the replicates of an error bar do: the
                        tables of the draw are built on the host (qmc.tables) and uploaded before the launch; the Philox fill has no
                        such cost, a new draw there is another counter word
  sample_device_random  fill + the map's configured inverse
  sample_device_sobol   the same with the Sobol' fill, one draw, the tables resident
  sample_device_sobol_fresh  the same with a new draw on every launch
HIP events around every batch of launches; per version the median over the rounds of the mean launch time, the spread (min, max over
the rounds) and the kernel that ran (ttm_last_kernel); for the two fills the bytes written (8 N D) over the time beside the
6.29 TB/s copy peak.  The events bracket the stream, so the host work of a fresh draw shows as the time the device waits for it;
`tables_host_ms` is that work alone (wall clock around qmc.tables, median of 20 draws), `sample_fresh_draw_ms` the host call
sample(N) with a new draw every time, for both sequences.

What the points buy (--error-rows, '' to skip): C5 with root_finder='newton' (the table inverse's 9e-5 interpolation error would
floor the comparison).  Two functionals of the raw-coordinate sample x (N x 40): `mean` = the mean over rows and columns of x,
`second_moment` = the mean over rows and columns of x^2.  Per N and sequence the root-mean-square, over --error-draws draws, of the
estimate's difference from the truth; the truth is the mean of 8 scrambled Sobol' estimates at --truth-rows rows (draws that the
error draws do not use), whose own standard error is reported beside it.  Reported, not gated.
"""
import itertools
import json
import statistics
import time

import numpy as np

import benchlib

TRUTH_DRAWS = 8


def functionals(tm, X, N, std, mean):
    x = X[:, :N] * std[:, None] + mean[:, None]
    return float(x.mean().item()), float((x * x).mean().item())


def error_study(bench, args, torch):
    rows = [int(n) for n in args.error_rows.split(',') if n]
    tm, _, _ = bench.build_map('C5', 0, n_override=65536)
    tm.alternate_root_finding, tm.root_finder = False, 'newton'
    std, mean = tm._to_dev(np.asarray(tm.X_std, dtype=float)), tm._to_dev(np.asarray(tm.X_mean, dtype=float))
    names = ('mean', 'second_moment')
    truth = np.array([functionals(tm, tm.sample_device(args.truth_rows, seed=7, draw=10 ** 6 + r, sequence='sobol'), args.truth_rows, std, mean)
                      for r in range(TRUTH_DRAWS)])
    res = {'map': 'C5, root_finder newton', 'draws': args.error_draws, 'truth_rows': args.truth_rows, 'truth_draws': TRUTH_DRAWS,
           'truth': dict(zip(names, truth.mean(axis=0).tolist())),
           'truth_standard_error': dict(zip(names, (truth.std(axis=0, ddof=1) / np.sqrt(TRUTH_DRAWS)).tolist())), 'rmse': {}}
    for N in rows:
        res['rmse'][str(N)] = {}
        for seq in ('random', 'sobol'):
            est = np.array([functionals(tm, tm.sample_device(N, seed=7, draw=r, sequence=seq), N, std, mean) for r in range(args.error_draws)])
            rmse = np.sqrt(((est - truth.mean(axis=0)) ** 2).mean(axis=0))
            res['rmse'][str(N)][seq] = dict(zip(names, rmse.tolist()))
        r, s = res['rmse'][str(N)]['random'], res['rmse'][str(N)]['sobol']
        res['rmse'][str(N)]['random_over_sobol'] = {k: r[k] / s[k] for k in names}
        print('rmse N = %d' % N, json.dumps(res['rmse'][str(N)]), flush=True)
    return res


def main():
    ap = benchlib.parser(__doc__, 200, 'C5,C2b')
    ap.add_argument('--error-rows', default='4096,16384,65536')
    ap.add_argument('--error-draws', type=int, default=32)
    ap.add_argument('--truth-rows', type=int, default=1 << 20)
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('qmc_bench: no GPU - nothing is timed without one')
    res.update({'copy_peak_GBs': bench.COPY_PEAK_GBS, 'workloads': {}})
    for wl in [w for w in args.workloads.split(',') if w]:
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        kernel = benchlib.bind(tm._lib)
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        Z = tm._cols(D, N)
        X = tm._cols(d, N, zero=True)

        def philox():
            tm.reference_device(N, seed=1, draw=0, out=Z)

        def sobol():
            tm.reference_device(N, seed=1, draw=0, out=Z, sequence='sobol')

        def sample_device_random():
            tm.sample_device(N, seed=1, draw=0, X=X, Z=Z)

        def sample_device_sobol():
            tm.sample_device(N, seed=1, draw=0, X=X, Z=Z, sequence='sobol')

        fresh = itertools.count(1000)

        def sobol_fresh():
            tm.reference_device(N, seed=1, draw=next(fresh), out=Z, sequence='sobol')

        def sample_device_sobol_fresh():
            tm.sample_device(N, seed=1, draw=next(fresh), X=X, Z=Z, sequence='sobol')

        versions = [('philox', None, philox), ('sobol', None, sobol), ('sobol_fresh', None, sobol_fresh),
                    ('sample_device_random', None, sample_device_random), ('sample_device_sobol', None, sample_device_sobol),
                    ('sample_device_sobol_fresh', None, sample_device_sobol_fresh)]

        def after(name, v):
            if name in ('philox', 'sobol', 'sobol_fresh'):
                z = Z[:, :N]
                v['mean'], v['variance'] = float(z.mean().item()), float(z.var().item())

        info = benchlib.warm_up(versions, None, 2, kernel, after)
        benchlib.keep_busy(philox, 20)
        benchlib.time_rounds(versions, info, None, args.rounds, benchlib.per_round(args), settle=1)
        for v in info.values():
            benchlib.summarise(v)
        gbytes = 8.0 * N * D / 1e9
        for name in ('philox', 'sobol', 'sobol_fresh'):
            v = info[name]
            v['written_gbytes'] = gbytes
            v['written_GBs'] = gbytes / (v['ms'] * 1e-3)
            v['copy_peak_frac'] = v['written_GBs'] / bench.COPY_PEAK_GBS
        from triangular_transport_toolbox_amd import qmc
        host = []
        for _ in range(20):
            t0 = time.perf_counter()
            qmc.tables(1, next(fresh), 0, D)
            host.append((time.perf_counter() - t0) * 1e3)
        # the host boundary: sample() with a new draw on every call, wall clock around calls that end in a synchronise, median of 7
        calls = {}
        for seq in ('random', 'sobol'):
            tm.sample(N, seed=1, draw=next(fresh), sequence=seq)
            ts = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tm.sample(N, seed=1, draw=next(fresh), sequence=seq)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            calls[seq] = float(statistics.median(ts))
        t = {k: v['ms'] for k, v in info.items()}
        res['workloads'][wl] = {'N': N, 'D': D, 'd': d, 'versions': info, 'tables_host_ms': float(statistics.median(host)),
                                'sample_fresh_draw_ms': calls,
                                'sobol_over_philox_time': t['sobol'] / t['philox'],
                                'sobol_fresh_over_philox_time': t['sobol_fresh'] / t['philox'],
                                'sample_device_sobol_over_random_time': t['sample_device_sobol'] / t['sample_device_random'],
                                'sample_device_sobol_fresh_over_random_time': t['sample_device_sobol_fresh'] / t['sample_device_random']}
        benchlib.report(wl, info)
        del tm, Z, X
    if args.error_rows:
        res['error'] = error_study(bench, args, torch)
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
