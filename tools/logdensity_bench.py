"""Time the log-density and score of integrated-rectifier maps (ttm_logdensity) on the device-resident entry point.

    python tools/logdensity_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out profiles/logdensity_bench.json] [--launches 40] [--rounds 10]
                                     [--workloads C2a,C5int]

Workloads: C2a (spiral, d = 2, Q = 25, N = 1e6) and C5int (d = 40, band 2, Q = 25, N = 2e5) - bench.py's maps and coefficient
fixtures.  Versions, alternated round by round within the one process after a warm-up of every version and a second of busy chip
(the chip holds its clock only while it is kept busy: bench.py):
  logdensity        one ttm_logdensity launch: log p and the D score columns, with g_scale (k_logdensity_int)
  logp_only         the same launch without the score buffer: what the adjoint walk costs on top of the density
  forward           ttm_forward with logdet + sumsq on the same buffers as the library plans it (the dense / X-program kernels of
                    csrc/ttm_int.hip): what one evaluation of the density costs a user today
  forward_generic   the same with option int_dense = 0: the generic k_forward, the like-for-like table interpreter
HIP events around every batch of launches; per version the median over the rounds of the mean launch time and the spread (min,
max over the rounds) and the kernel that ran (ttm_last_kernel).  Derived: the ratios of `logdensity` to the two forward figures,
and the (1 + 2 D) forward passes central finite differences of the density would cost for the same score, over `logdensity`.
"""
import numpy as np

import benchlib


def main():
    args = benchlib.parser(__doc__, 40, 'C2a,C5int').parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('logdensity_bench: no GPU - nothing is timed without one')
    res['workloads'] = {}
    for wl in args.workloads.split(','):
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        pin = benchlib.option(lib, 'int_dense')
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        E = d - D
        coef = tm._pack_coeffs()
        std = np.asarray(tm.X_std, dtype=float)[E:E + D]
        gs = tm._to_dev(np.ascontiguousarray(1.0 / std))
        sg = tm._to_dev(np.ascontiguousarray(std))
        G = tm._cols(D, N)
        lp, ld, ss = tm._empty(N), tm._empty(N), tm._empty(N)

        def logdensity():
            tm.logdensity_device(tm._Xs, N, coef=coef, logp=lp, G=G, g_scale=gs)

        def logp_only():
            tm.logdensity_device(tm._Xs, N, coef=coef, logp=lp, g_scale=gs)

        def forward():
            tm.density_device(tm._Xs, N, coef=coef, logdet=ld, sigma=sg, sumsq=ss)

        def after(name, v):                              # the density against the forward map's
            if name.startswith('forward'):
                ref = -0.5 * ss + ld
                fin = torch.isfinite(ref)
                v['max_rel_diff_of_logp'] = float(((lp - ref).abs() / (1.0 + ref.abs()))[fin].max().item())

        versions = [('logdensity', -1, logdensity), ('logp_only', -1, logp_only), ('forward', -1, forward), ('forward_generic', 0, forward)]
        info = benchlib.warm_up(versions, pin, 2, kernel, after)
        benchlib.keep_busy(versions[0][2], 4)
        benchlib.time_rounds(versions, info, pin, args.rounds, benchlib.per_round(args), settle=1)
        for v in info.values():
            benchlib.summarise(v)
        t = {k: v['ms'] for k, v in info.items()}
        out = {'N': N, 'D': D, 'd': d, 'Q': int(tm._qx_d.numel()), 'versions': info,
               'logdensity_over_forward_time': t['logdensity'] / t['forward'],
               'logdensity_over_forward_generic_time': t['logdensity'] / t['forward_generic'],
               'logp_only_over_forward_generic_time': t['logp_only'] / t['forward_generic'],
               'finite_difference_passes': 1 + 2 * D,
               'finite_difference_step_ms': (1 + 2 * D) * t['forward'],
               'finite_difference_step_generic_ms': (1 + 2 * D) * t['forward_generic'],
               'finite_differences_over_logdensity_time': (1 + 2 * D) * t['forward'] / t['logdensity'],
               'finite_differences_generic_over_logdensity_time': (1 + 2 * D) * t['forward_generic'] / t['logdensity']}
        res['workloads'][wl] = out
        benchlib.report(wl, info)
        del tm, G
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
