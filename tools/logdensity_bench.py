"""Time the log-density and score of integrated-rectifier maps (ttm_logdensity) on the device-resident entry point.

    python tools/logdensity_bench.py [--label NAME] [--commit ID] [--out profiles/logdensity_bench.json] [--launches 40] [--rounds 10]
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
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--workloads', default='C2a,C5int')
    ap.add_argument('--rows', type=int, default=0, help='rows instead of the workload\'s own N (rehearsals)')
    ap.add_argument('--commit', default='', help='what to record as the commit when the tree is not a git checkout')
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import bench
    if not torch.cuda.is_available():
        raise SystemExit('logdensity_bench: no GPU - nothing is timed without one')
    res = {'label': args.label, 'launches_per_version': args.launches, 'rounds': args.rounds, 'workloads': {}}
    try:
        res['commit'] = subprocess.run(['git', '-C', root, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        res['commit'] = ''
    res['commit'] = res['commit'] or args.commit
    per = max(1, args.launches // args.rounds)
    for wl in args.workloads.split(','):
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib = tm._lib
        lib.ttm_last_kernel.restype = ctypes.c_char_p
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

        versions = [('logdensity', -1, logdensity), ('logp_only', -1, logp_only), ('forward', -1, forward), ('forward_generic', 0, forward)]
        info = {}
        for name, opt, fn in versions:                   # warm-up of every version, kernel names, the density against the forward map's
            lib.ttm_set_option(b'int_dense', opt)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            info[name] = {'kernel': lib.ttm_last_kernel().decode(), 'ms_rounds': []}
            if name.startswith('forward'):
                ref = -0.5 * ss + ld
                fin = torch.isfinite(ref)
                info[name]['max_rel_diff_of_logp'] = float(((lp - ref).abs() / (1.0 + ref.abs()))[fin].max().item())
        t_busy = 0.0
        while t_busy < 1000.0:                           # keep the chip busy for a second before anything is timed
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(4):
                versions[0][2]()
            b.record()
            torch.cuda.synchronize()
            t_busy += a.elapsed_time(b)
        for _ in range(args.rounds):
            for name, opt, fn in versions:
                lib.ttm_set_option(b'int_dense', opt)
                fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per):
                    fn()
                b.record()
                torch.cuda.synchronize()
                info[name]['ms_rounds'].append(a.elapsed_time(b) / per)
        lib.ttm_set_option(b'int_dense', -1)
        for name, v in info.items():
            r = np.array(v['ms_rounds'])
            v['ms'] = float(np.median(r))
            v['ms_min'], v['ms_max'] = float(r.min()), float(r.max())
            v['spread_rel'] = float((r.max() - r.min()) / np.median(r))
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
        print(wl, json.dumps({k: (v['kernel'], round(v['ms'], 4), round(v['ms_min'], 4), round(v['ms_max'], 4)) for k, v in info.items()}), flush=True)
        del tm, G
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or '.', exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
