"""Time the Newton root search of the banded separable maps on the device-resident entry point (inverse_device).

    python tools/newton_bench.py [--root TREE] [--label NAME] [--commit ID] [--out FILE.json] [--launches 200] [--rounds 10]

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
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--workloads', default='C5,C2b,C3')
    ap.add_argument('--commit', default='', help='what to record as the commit when the tree is not a git checkout')
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import bench
    res = {'label': args.label, 'launches_per_version': args.launches, 'rounds': args.rounds, 'workloads': {}}
    try:
        res['commit'] = subprocess.run(['git', '-C', root, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        res['commit'] = ''
    res['commit'] = res['commit'] or args.commit
    per = max(1, args.launches // args.rounds)
    for wl in args.workloads.split(','):
        tm, X, cfg = bench.build_map(wl, 0, root_finder='newton', alternate_root_finding=False)
        lib = tm._lib
        lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        lib.ttm_last_kernel.restype = ctypes.c_char_p
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Z = tm._cols(D, N)
        tm.forward_device(tm._Xs, N, coef=coef, Z=Z)
        Xinv = tm._cols(d, N, zero=True)
        has_opt = lib.ttm_set_option(b'band_newton', -1) == 0
        iters = tm._zeros(D, dtype=torch.int32)

        def newton():
            # (the entry point itself, as _inverse_bisect calls it, with one counter: no host read-back between launches)
            lib.ttm_inverse_newton(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z), Z.shape[1], tm._ptr(Xinv),
                                   Xinv.shape[1], N, ctypes.c_void_p(iters.data_ptr()), tm._stream())

        def table():
            tm.inverse_device(Z, N, coef=coef, X=Xinv, table=True)

        versions = [('newton', -1, newton)] + ([('generic', 0, newton)] if has_opt else []) + [('table', -1, table)]
        info = {}
        for name, opt, fn in versions:                   # warm-up of every shape (tables, first launches), kernel names, errors
            if has_opt:
                lib.ttm_set_option(b'band_newton', opt)
            iters.zero_()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            err = float((Xinv[:, :N] - tm._Xs[:, :N]).abs().max().item())
            info[name] = {'kernel': lib.ttm_last_kernel().decode(), 'round_trip_max': err, 'ms_rounds': []}
            if name != 'table':
                info[name]['trial_points_max_per_component'] = iters.cpu().numpy().tolist()
        t_busy = 0.0
        while t_busy < 1000.0:                           # keep the chip busy for a second before anything is timed
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                versions[0][2]()
            b.record()
            torch.cuda.synchronize()
            t_busy += a.elapsed_time(b)
        for _ in range(args.rounds):
            for name, opt, fn in versions:
                if has_opt:
                    lib.ttm_set_option(b'band_newton', opt)
                for _ in range(2):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per):
                    fn()
                b.record()
                torch.cuda.synchronize()
                info[name]['ms_rounds'].append(a.elapsed_time(b) / per)
        if has_opt:
            lib.ttm_set_option(b'band_newton', -1)
        E = int(tm.skip_dimensions)
        gbytes = 8.0 * (2 * D + E) * N / 1e9
        for name, v in info.items():
            r = np.array(v['ms_rounds'])
            v['ms'] = float(np.median(r))
            v['ms_min'], v['ms_max'] = float(r.min()), float(r.max())
            v['spread_rel'] = float((r.max() - r.min()) / np.median(r))
            v['hbm_frac_on_algorithmic_bytes'] = gbytes / (v['ms'] * 1e-3) / bench.HBM_PEAK_GBS
            if 'trial_points_max_per_component' in v:
                tp = float(np.sum(v['trial_points_max_per_component']))
                v['fp64_frac_upper_bound'] = 2.0 * 34.0 * tp * N / (v['ms'] * 1e-3) / 1e12 / FP64_VECTOR_PEAK_TFLOPS
        out = {'N': N, 'D': D, 'algorithmic_gbytes': gbytes, 'versions': info}
        if 'generic' in info:
            out['newton_over_generic'] = info['generic']['ms'] / info['newton']['ms']
        out['newton_over_table_time'] = info['newton']['ms'] / info['table']['ms']
        res['workloads'][wl] = out
        print(wl, json.dumps({k: (v['kernel'], round(v['ms'], 4), round(v['ms_min'], 4), round(v['ms_max'], 4)) for k, v in info.items()}), flush=True)
        del tm, Z, Xinv
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
