"""Time the score of the pullback density (ttm_score) on the device-resident entry point (score_device).

    python tools/score_bench.py [--label NAME] [--commit ID] [--out FILE.json] [--launches 200] [--rounds 10] [--workloads C5,linear_irbf,C2b,C3]

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
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np


def build(bench, wl):
    if wl != 'linear_irbf':
        tm, X, cfg = bench.build_map(wl, 0)
        return tm
    from tools import band_linear_bench as blb
    from triangular_transport_toolbox_amd import specs
    from triangular_transport_toolbox_amd.transport_map import transport_map
    mon, non = blb.spec('linear_irbf')
    tm = transport_map(X=specs.sample_mixture(blb.N, d=blb.D), monotone=mon, nonmonotone=non, verbose=False,
                       monotonicity='separable monotonicity')
    rng = np.random.default_rng(7)
    for k in range(blb.D):
        tm.coeffs_mon[k] = 0.2 + 0.5 * rng.random(len(tm.coeffs_mon[k]))
        tm.coeffs_nonmon[k] = 0.3 * rng.standard_normal(len(tm.coeffs_nonmon[k])) / (1 + np.arange(len(tm.coeffs_nonmon[k])))
    return tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--workloads', default='C5,linear_irbf,C2b,C3')
    ap.add_argument('--commit', default='', help='what to record as the commit when the tree is not a git checkout')
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
        tm = build(bench, wl)
        lib = tm._lib
        lib.ttm_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int32]
        lib.ttm_last_kernel.restype = ctypes.c_char_p
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

        versions = [('band', -1, score_raw), ('band_std', -1, score_std), ('generic', 0, score_raw), ('forward', -1, forward)]
        info = {}
        ref = None
        for name, opt, fn in versions:                   # warm-up of every version, kernel names, the versions against each other
            lib.ttm_set_option(b'band_score', opt)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            info[name] = {'kernel': lib.ttm_last_kernel().decode(), 'ms_rounds': []}
            if name == 'band':
                ref = G[:, :N].clone()
            elif name == 'generic':
                info[name]['max_rel_diff_to_band'] = float(((G[:, :N] - ref).abs() / (1.0 + ref.abs())).max().item())
        del ref
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
                lib.ttm_set_option(b'band_score', opt)
                for _ in range(2):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(per):
                    fn()
                b.record()
                torch.cuda.synchronize()
                info[name]['ms_rounds'].append(a.elapsed_time(b) / per)
        lib.ttm_set_option(b'band_score', -1)
        gbytes = 8.0 * (d + D) * N / 1e9
        for name, v in info.items():
            r = np.array(v['ms_rounds'])
            v['ms'] = float(np.median(r))
            v['ms_min'], v['ms_max'] = float(r.min()), float(r.max())
            v['spread_rel'] = float((r.max() - r.min()) / np.median(r))
            v['hbm_frac_on_algorithmic_bytes'] = gbytes / (v['ms'] * 1e-3) / bench.HBM_PEAK_GBS
        out = {'N': N, 'D': D, 'd': d, 'algorithmic_gbytes': gbytes, 'versions': info,
               'band_over_forward_time': info['band']['ms'] / info['forward']['ms'],
               'generic_over_band_time': info['generic']['ms'] / info['band']['ms']}
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
