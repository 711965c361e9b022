"""Time the reference's bisection of the banded separable maps on the device-resident entry point (inverse_device with
alternate_root_finding=False: the launch on rows 1.., then the replay of sample 0 with the cap, no host read between them).

    python tools/bisect_bench.py [--root TREE] [--label NAME] [--commit ID] [--out FILE.json] [--launches 50] [--rounds 10]

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
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--launches', type=int, default=50)
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
    res['commit'] = args.commit or res['commit']
    per = max(1, args.launches // args.rounds)
    for wl in args.workloads.split(','):
        tm, X, cfg = bench.build_map(wl, 0, alternate_root_finding=False)
        lib = tm._lib
        lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        lib.ttm_last_kernel.restype = ctypes.c_char_p
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Z = tm._cols(D, N)
        tm.forward_device(tm._Xs, N, coef=coef, Z=Z)
        Xinv = tm._cols(d, N, zero=True)
        has_opt = lib.ttm_set_option(b'band_bisect', -1) == 0
        iters = tm._zeros(D, dtype=torch.int32)

        def bisect():
            tm.inverse_device(Z, N, coef=coef, X=Xinv, table=False)

        def rows_from_1():
            # (the first launch of _inverse_bisect by itself: its kernel by name, its counter)
            iters.zero_()
            lib.ttm_inverse_bisect(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z, 1), Z.shape[1], tm._ptr(Xinv, 1),
                                   Xinv.shape[1], N - 1, ctypes.c_void_p(iters.data_ptr()), None, tm._stream())
            torch.cuda.synchronize()
            return lib.ttm_last_kernel().decode(), iters.cpu().numpy().tolist()

        def newton():
            lib.ttm_inverse_newton(tm._pp, tm._ptr(coef), tm._ptr(coef._ttm_fold), 0, D, tm._ptr(Z), Z.shape[1], tm._ptr(Xinv),
                                   Xinv.shape[1], N, ctypes.c_void_p(iters.data_ptr()), tm._stream())

        def table():
            tm.inverse_device(Z, N, coef=coef, X=Xinv, table=True)

        versions = [('bisect', -1, bisect)] + ([('generic', 0, bisect)] if has_opt else []) + [('newton', -1, newton), ('table', -1, table)]
        info, kept = {}, {}
        for name, opt, fn in versions:                   # warm-up of every shape (tables, first launches), kernel names, errors
            if has_opt:
                lib.ttm_set_option(b'band_bisect', opt)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            err = float((Xinv[:, 1:N] - tm._Xs[:, 1:N]).abs().max().item())
            info[name] = {'round_trip_max_rows_1_on': err, 'ms_rounds': []}
            if fn is bisect:
                kept[name] = Xinv[:, 1:N].clone()
                info[name]['kernel_rows_1_on'], info[name]['midpoints_max_per_component'] = rows_from_1()
            else:
                info[name]['kernel'] = lib.ttm_last_kernel().decode()
        if 'generic' in kept:
            same = float((kept['bisect'] == kept['generic']).double().mean().item())
            info['bisect']['share_bit_identical_to_generic'] = same
            info['bisect']['max_abs_difference_to_generic'] = float((kept['bisect'] - kept['generic']).abs().max().item())
        kept.clear()
        t_busy = 0.0
        while t_busy < 1000.0:                           # keep the chip busy for a second before anything is timed
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                versions[0][2]()
            b.record()
            torch.cuda.synchronize()
            t_busy += a.elapsed_time(b)
        for _ in range(args.rounds):
            for name, opt, fn in versions:
                if has_opt:
                    lib.ttm_set_option(b'band_bisect', opt)
                fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per):
                    fn()
                b.record()
                torch.cuda.synchronize()
                info[name]['ms_rounds'].append(a.elapsed_time(b) / per)
        if has_opt:
            lib.ttm_set_option(b'band_bisect', -1)
        for name, v in info.items():
            r = np.array(v['ms_rounds'])
            v['ms'] = float(np.median(r))
            v['ms_min'], v['ms_max'] = float(r.min()), float(r.max())
            v['spread_rel'] = float((r.max() - r.min()) / np.median(r))
        out = {'N': N, 'D': D, 'versions': info}
        if 'generic' in info:
            out['generic_over_bisect'] = info['generic']['ms'] / info['bisect']['ms']
        out['bisect_over_newton'] = info['bisect']['ms'] / info['newton']['ms']
        out['bisect_over_table'] = info['bisect']['ms'] / info['table']['ms']
        res['workloads'][wl] = out
        print(wl, json.dumps({k: (v.get('kernel_rows_1_on', v.get('kernel')), round(v['ms'], 4), round(v['ms_min'], 4), round(v['ms_max'], 4))
                              for k, v in info.items()}), flush=True)
        del tm, Z, Xinv
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
