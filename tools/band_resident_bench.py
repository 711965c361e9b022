"""Time the two launches of the headline step (bench.py, C5: k_band_forward then k_band_inverse_ring) under the cache policies of
option band_resident (csrc/ttm_band_policy.h), in ONE process.

    python tools/band_resident_bench.py [--out FILE.json] [--steps 40] [--rounds 6] [--n 1000000] [--sweep 500000,1000000,1300000,1600000]

At --n: band_resident = 0, 1, 2, 3 (plain | forward only | inverse only | both), alternated round by round after the chip has
been kept busy for a second (it holds its clock only under load: bench.py).  A round of a setting is 3 untimed steps - the cache
still holds what the previous setting left - then --steps steps with HIP events in front of the forward launch, between the two
and behind the inverse, so the table shows which half of the policy earns what in which launch.  Per setting: the median over
the rounds of the mean forward, inverse and step time, and the rounds' min-max.
--sweep: at each N the settings 0, 3 and -1 (auto: the gate), the same way - where does keeping half of Z stop paying?
The map, its coefficients and the buffers are bench.py's (build_map; Z and X' persist from step to step, as there).
"""
import argparse
import os
import sys

import numpy as np

import benchlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--sweep', default='500000,1000000,1300000,1600000')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import bench

    def run(N, settings):
        tm, X, cfg = bench.build_map('C5', 0, n_override=N)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Xs, Z, Xinv = tm._Xs, tm._cols(D, N), tm._cols(d, N, zero=True)

        def step():
            tm.forward_device(Xs, N, coef=coef, Z=Z)
            tm.inverse_device(Z, N, coef=coef, X=Xinv)

        info = {}
        ref = None
        for s in settings:                                   # first launches, kernel names, the same bits under every setting
            assert lib.ttm_set_option(b'band_resident', s) == 0
            tm.forward_device(Xs, N, coef=coef, Z=Z)
            torch.cuda.synchronize()
            kf = kernel()
            tm.inverse_device(Z, N, coef=coef, X=Xinv)
            torch.cuda.synchronize()
            info[s] = {'kernels': [kf, kernel()], 'fwd': [], 'inv': [], 'step': []}
            if ref is None:
                ref = (Z.clone(), Xinv.clone())
            info[s]['bit_identical_to_first_setting'] = bool(torch.equal(Z.view(torch.int64), ref[0].view(torch.int64)) and
                                                            torch.equal(Xinv.view(torch.int64), ref[1].view(torch.int64)))
        ref = None
        benchlib.keep_busy(step, 50)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
        for _ in range(args.rounds):
            for s in settings:
                lib.ttm_set_option(b'band_resident', s)
                for _ in range(3):
                    step()
                for a, b, c in ev:
                    a.record()
                    tm.forward_device(Xs, N, coef=coef, Z=Z)
                    b.record()
                    tm.inverse_device(Z, N, coef=coef, X=Xinv)
                    c.record()
                torch.cuda.synchronize()
                info[s]['fwd'].append(float(np.mean([a.elapsed_time(b) for a, b, c in ev])))
                info[s]['inv'].append(float(np.mean([b.elapsed_time(c) for a, b, c in ev])))
                info[s]['step'].append(float(ev[0][0].elapsed_time(ev[-1][2]) / len(ev)))
        lib.ttm_set_option(b'band_resident', -1)
        out = {}
        for s, v in info.items():
            o = {'kernels': v['kernels'], 'bit_identical_to_first_setting': v['bit_identical_to_first_setting']}
            for key in ('fwd', 'inv', 'step'):
                r = np.array(v[key])
                o[key + '_ms'] = {'median': float(np.median(r)), 'min': float(r.min()), 'max': float(r.max()), 'rounds': v[key]}
            out[str(s)] = o
            print('N = %d band_resident = %2d  %s' % (N, s, '  '.join('%s %.4f (%.4f-%.4f)' % (k, o[k + '_ms']['median'], o[k + '_ms']['min'],
                                                                                              o[k + '_ms']['max']) for k in ('fwd', 'inv', 'step'))),
                  flush=True)
        del tm, Z, Xinv, Xs
        torch.cuda.empty_cache()
        return {'N': N, 'D': D, 'settings': out}

    res = {'steps_per_round': args.steps, 'rounds': args.rounds, 'halves': run(args.n, (0, 1, 2, 3)), 'sweep': []}
    for n in [int(v) for v in args.sweep.split(',') if v]:
        res['sweep'].append(run(n, (0, 3, -1)))
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
