"""Time the reference's bisection of the banded separable maps on the device-resident entry point (inverse_device with
alternate_root_finding=False: the launch on rows 1.., then the replay of sample 0 with the cap, no host read between them).

    python tools/bisect_bench.py [--root TREE] [--label NAME] [--commit ID] [--out FILE.json] [--launches 50] [--rounds 10] [--rows N]

Workloads: C5 N = 1e6, C2b N = 1e6, C3 N = 5e5 (bench.py's maps and coefficient fixtures).  Versions, alternated round by
round within the one process after a warm-up of every shape (the chip holds its clock only while it is kept busy: bench.py):
  bisect   as the library plans it (k_band_bisect / k_band_few_bisect where the build has them, else k_inverse_bisect; with the Newton
           kernels instantiations of one template per shape, k_band_search / k_band_few_search)
  generic  the same call with option band_bisect = 0 (k_inverse_bisect) - left out where the library does not know the option
  newton   ttm_inverse_newton of the same build (k_band_newton / k_band_few_newton)
  table    the table inverse of the same build (k_band_inverse_ring / k_band_few_inverse), tables built beforehand
HIP events around every batch of launches; per version the median over the rounds of the mean call time and the spread
(min, max over the rounds).  --root: the repository tree whose package is timed (a build of another commit in a second
directory: run the tool once per tree in the same GPU visit and compare the files).
Also reported: midpoints (per-component maxima, as `iters` returns them), the kernel the launch on rows 1.. took, and - where
the option exists - the share of entries of rows 1.. that are bit-identical under band_bisect = -1 and 0.
"""
import ctypes

import benchlib


def main():
    args = benchlib.parser(__doc__, 50, 'C5,C2b,C3').parse_args()
    bench, res = benchlib.start(args)
    import torch
    res['workloads'] = {}
    for wl in args.workloads.split(','):
        tm, X, cfg = bench.build_map(wl, 0, n_override=args.rows or None, alternate_root_finding=False)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Z = tm._cols(D, N)
        tm.forward_device(tm._Xs, N, coef=coef, Z=Z)
        Xinv = tm._cols(d, N, zero=True)
        pin = benchlib.option(lib, 'band_bisect', probe=True)
        iters = tm._zeros(D, dtype=torch.int32)

        def bisect():
            tm.inverse_device(Z, N, coef=coef, X=Xinv, table=False)

        def rows_from_1():
            # (the first launch of _inverse_bisect by itself: its kernel by name, its counter)
            iters.zero_()
            lib.ttm_inverse_bisect(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z, 1), Z.shape[1], tm._ptr(Xinv, 1),
                                   Xinv.shape[1], N - 1, ctypes.c_void_p(iters.data_ptr()), None, tm._stream())
            torch.cuda.synchronize()
            return kernel(), iters.cpu().numpy().tolist()

        def newton():
            lib.ttm_inverse_newton(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z), Z.shape[1], tm._ptr(Xinv),
                                   Xinv.shape[1], N, ctypes.c_void_p(iters.data_ptr()), tm._stream())

        def table():
            tm.inverse_device(Z, N, coef=coef, X=Xinv, table=True)

        kept = {}

        def after(name, v):                              # errors; for the bisection the kernel and midpoints of its launch on rows 1..
            v['round_trip_max_rows_1_on'] = float((Xinv[:, 1:N] - tm._Xs[:, 1:N]).abs().max().item())
            if name in ('bisect', 'generic'):
                kept[name] = Xinv[:, 1:N].clone()
                v['kernel'], v['midpoints_max_per_component'] = rows_from_1()

        versions = [('bisect', -1, bisect)] + ([('generic', 0, bisect)] if pin else []) + [('newton', -1, newton), ('table', -1, table)]
        info = benchlib.warm_up(versions, pin, 2, kernel, after)
        if 'generic' in kept:
            same = float((kept['bisect'] == kept['generic']).double().mean().item())
            info['bisect']['share_bit_identical_to_generic'] = same
            info['bisect']['max_abs_difference_to_generic'] = float((kept['bisect'] - kept['generic']).abs().max().item())
        kept.clear()
        benchlib.keep_busy(versions[0][2], 5)
        benchlib.time_rounds(versions, info, pin, args.rounds, benchlib.per_round(args), settle=1)
        for v in info.values():
            benchlib.summarise(v)
        out = {'N': N, 'D': D, 'versions': info}
        if 'generic' in info:
            out['generic_over_bisect'] = info['generic']['ms'] / info['bisect']['ms']
        out['bisect_over_newton'] = info['bisect']['ms'] / info['newton']['ms']
        out['bisect_over_table'] = info['bisect']['ms'] / info['table']['ms']
        res['workloads'][wl] = out
        benchlib.report(wl, info)
        for name in ('bisect', 'generic'):               # (in the file the bisection's kernel goes by what it is: that of rows 1..)
            if name in info:
                info[name]['kernel_rows_1_on'] = info[name].pop('kernel')
        del tm, Z, Xinv
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
