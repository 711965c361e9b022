"""Time draws with their log-density from integrated-rectifier maps: the fused root search (ttm_inverse_logdensity) against the
plain search and against what a caller ran before it existed, the plain search followed by ttm_logdensity on the result.

    python tools/sample_logdensity_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out profiles/sample_logdensity_bench.json]
                                            [--launches 40] [--rounds 10] [--workloads C2a,C5int] [--methods newton,reference]

Workloads: C2a (spiral, d = 2, Q = 25, N = 1e6) and C5int (d = 40, band 2, Q = 25, N = 2e5) - bench.py's maps and coefficient
fixtures; the reference draws are reference_device(N, seed 0, draw 0).  Methods: newton (ttm_inverse_newton) and reference
(ttm_inverse_bisect without a cap), every row of the ensemble in one launch.  Versions, alternated round by round within the one
process after a warm-up of every version and a second of busy chip (the chip holds its clock only while it is kept busy: bench.py):
  fused      one ttm_inverse_logdensity launch: X and logq, with g_scale
  plain      the plain search on the same buffers: X alone
  two_pass   plain, then logdensity_device(X) for log p alone (k_logdensity_int): X and log p the way a caller got them before
A tree under --root whose library has no ttm_inverse_logdensity (an older commit) is timed on plain and two_pass alone: that is
how `plain` of two commits is compared, the tool run on both trees in turn.
HIP events around every batch of launches; per version the median over the rounds of the mean launch time and the spread (min,
max over the rounds) and the kernel that ran last (ttm_last_kernel).  Derived: fused / plain, fused / two_pass, and whether the fused
median lies below the two-pass median by more than the larger of the two versions' min-to-max ranges.  After the warm-up the fused
X is compared bitwise with the plain X, and logq with two_pass's log p (|a - b| / (1 + |b|) over the finite rows).
"""
import ctypes

import numpy as np

import benchlib


def main():
    ap = benchlib.parser(__doc__, 40, 'C2a,C5int')
    ap.add_argument('--methods', default='newton,reference')
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sample_logdensity_bench: no GPU - nothing is timed without one')
    from triangular_transport_toolbox_amd import _capi
    res['workloads'] = {}
    for wl in args.workloads.split(','):
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        has_fused = hasattr(lib, 'ttm_inverse_logdensity')
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        E = d - D
        coef = tm._pack_coeffs()
        fold = coef._ttm_fold
        gs = tm._to_dev(np.ascontiguousarray(1.0 / np.asarray(tm.X_std, dtype=float)[E:E + D]))
        Z = tm.reference_device(N, seed=0, draw=0)
        X, Xf = tm._cols(d, N, zero=True), tm._cols(d, N, zero=True)
        if E:
            X[:E, :N].copy_(tm._Xs[:E, :N])
            Xf[:E, :N].copy_(tm._Xs[:E, :N])
        lq, lp = tm._empty(N), tm._empty(N)
        iters = tm._zeros(D, dtype=torch.int32)
        it_p = ctypes.c_void_p(iters.data_ptr())
        head = (tm._pp, tm._ptr(coef), tm._ptr(fold), 0, D, tm._ptr(Z), Z.shape[1])
        out = {'N': N, 'D': D, 'd': d, 'Q': int(tm._qx_d.numel()), 'methods': {}}
        for method in args.methods.split(','):
            newton = {'newton': 1, 'reference': 0}[method]

            def plain():
                if newton:
                    _capi.check(lib.ttm_inverse_newton(*head, tm._ptr(X), X.shape[1], N, it_p, tm._stream()))
                else:
                    _capi.check(lib.ttm_inverse_bisect(*head, tm._ptr(X), X.shape[1], N, it_p, None, tm._stream()))

            def two_pass():
                plain()
                tm.logdensity_device(X, N, coef=coef, logp=lp, g_scale=gs)

            def fused():
                _capi.check(lib.ttm_inverse_logdensity(*head, tm._ptr(Xf), Xf.shape[1], N, newton, it_p, None, tm._ptr(lq), tm._ptr(gs), tm._stream()))

            def after(name, v):
                if name == 'two_pass' and has_fused:             # (fused has run: versions are warmed up in order)
                    fin = torch.isfinite(lp[:N]) & torch.isfinite(lq[:N])
                    v['fused_x_equals_plain_x'] = bool(torch.equal(X[E:, :N], Xf[E:, :N]))
                    v['max_rel_diff_of_logq_to_two_pass'] = float(((lq[:N] - lp[:N]).abs() / (1.0 + lp[:N].abs()))[fin].max().item())
                    v['rows_compared'] = int(fin.sum().item())

            versions = ([('fused', None, fused)] if has_fused else []) + [('plain', None, plain), ('two_pass', None, two_pass)]
            info = benchlib.warm_up(versions, None, 2, kernel, after)
            benchlib.keep_busy(plain, 4)
            benchlib.time_rounds(versions, info, None, args.rounds, benchlib.per_round(args), settle=1)
            for v in info.values():
                benchlib.summarise(v)
            m = {'versions': info, 'trial_points_max_per_component': int(iters.max().item())}
            if has_fused:
                f, p, t = info['fused'], info['plain'], info['two_pass']
                m['fused_over_plain_time'] = f['ms'] / p['ms']
                m['fused_over_two_pass_time'] = f['ms'] / t['ms']
                m['fused_below_two_pass_by_more_than_the_spread'] = bool(
                    t['ms'] - f['ms'] > max(f['ms_max'] - f['ms_min'], t['ms_max'] - t['ms_min']))
            out['methods'][method] = m
            benchlib.report('%s %s' % (wl, method), info)
            iters.zero_()
        res['workloads'][wl] = out
        del tm, X, Xf, Z
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
