"""Time the device-resident entry points on LONG banded separable maps whose monotone parts carry a linear own term.

    python tools/band_linear_bench.py [--root TREE] [--label NAME] [--commit ID] [--out FILE.json] [--launches 100] [--rounds 10]

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
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--launches', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--maps', default='linear,linear_irbf')
    ap.add_argument('--rows', type=int, default=N)
    ap.add_argument('--commit', default='', help='what to record as the commit when the tree is not a git checkout')
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch
    import bench
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    res = {'label': args.label, 'launches_per_step': args.launches, 'rounds': args.rounds, 'maps': {}}
    try:
        res['commit'] = subprocess.run(['git', '-C', root, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        res['commit'] = ''
    res['commit'] = args.commit or res['commit']
    per = max(1, args.launches // args.rounds)
    X = specs.sample_mixture(args.rows, d=D)
    for which in args.maps.split(','):
        mon, non = spec(which)
        tm = transport_map(X=X, monotone=mon, nonmonotone=non, verbose=False, monotonicity='separable monotonicity')
        rng = np.random.default_rng(7)
        for k in range(D):
            tm.coeffs_mon[k] = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
            tm.coeffs_nonmon[k] = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
        lib = tm._lib
        lib.ttm_last_kernel.restype = ctypes.c_char_p
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

        steps = [('forward', lambda: tm.forward_device(tm._Xs, n, coef=coef, Z=Zd), 2 * D),
                 ('density', lambda: tm.forward_device(tm._Xs, n, coef=coef, Z=Zd, logdet=ld, sumsq=ss), 2 * D + 2),
                 ('logdet', lambda: tm.density_device(tm._Xs, n, coef=coef, logdet=ld), D + 1),
                 ('sumsq', lambda: tm.density_device(tm._Xs, n, coef=coef, sumsq=ss), D + 1),
                 ('table', lambda: tm.inverse_device(Z, n, coef=coef, X=Xinv, table=True), 2 * D),
                 ('newton', newton, 2 * D)]
        info = {}
        for name, fn, cols in steps:                     # warm-up of every step (tables, first launches), kernel names, errors
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            info[name] = {'kernel': lib.ttm_last_kernel().decode(), 'ms_rounds': [], 'algorithmic_gbytes': 8.0 * cols * n / 1e9}
            if name in ('table', 'newton'):
                info[name]['round_trip_max'] = float((Xinv[:, :n] - tm._Xs[:, :n]).abs().max().item())
            if name == 'newton':
                info[name]['trial_points_max_per_component'] = iters.cpu().numpy().tolist()
        t_busy = 0.0
        while t_busy < 1000.0:                           # keep the chip busy for a second before anything is timed
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                steps[0][1]()
            b.record()
            torch.cuda.synchronize()
            t_busy += a.elapsed_time(b)
        for _ in range(args.rounds):
            for name, fn, cols in steps:
                for _ in range(2):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per):
                    fn()
                b.record()
                torch.cuda.synchronize()
                info[name]['ms_rounds'].append(a.elapsed_time(b) / per)
        for name, v in info.items():
            r = np.array(v['ms_rounds'])
            v['ms'] = float(np.median(r))
            v['ms_min'], v['ms_max'] = float(r.min()), float(r.max())
            v['spread_rel'] = float((r.max() - r.min()) / np.median(r))
            v['hbm_frac_on_algorithmic_bytes'] = v['algorithmic_gbytes'] / (v['ms'] * 1e-3) / bench.HBM_PEAK_GBS
        res['maps'][which] = {'N': n, 'D': D, 'u_p_lag': int(tm._cm.u_p_lag), 'u_h_cls': int(tm._cm.u_h_cls), 'u_h_ng': int(tm._cm.u_h_ng),
                              'steps': info}
        print(which, json.dumps({k: (v['kernel'], round(v['ms'], 4), round(v['ms_min'], 4), round(v['ms_max'], 4)) for k, v in info.items()}), flush=True)
        del tm, Z, Zd, Xinv
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
