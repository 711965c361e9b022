"""Time the two launches of the headline step (bench.py, C5: k_band_forward then k_band_inverse_ring) with and without the interval
slopes in the resident-table images (option band_slopes; csrc/ttm_band_image.h), in ONE process.

    python tools/band_slopes_bench.py [--out FILE.json] [--steps 100] [--rounds 10] [--n 1000000]

The settings, alternated round by round after the chip has been kept busy (tools/benchlib.py's method, as tools/band_zdma_bench.py):

    off      band_slopes = 0, band_ring_slots = 0      today's images, 24 slots at C5
    off12    band_slopes = 0, band_ring_slots = 12     today's images in the 12 slots the slopes leave: the smaller ring alone
    on       band_slopes = 1, band_ring_slots = 0      images with slopes, 12 slots at C5
    auto     every option at -1: what a plain run takes

A coefficient vector's images follow the value of band_slopes they were built under, so every setting has a packed vector of its
own, its tables built under that setting before anything is timed.  A round of a setting is 3 untimed steps, then --steps steps
with HIP events in front of the forward launch, between the two and behind the inverse.  Per setting: the median over the rounds
of the mean forward, inverse and step time, and the rounds' min-max.
"""
import argparse
import os
import sys

import numpy as np

import benchlib

SETTINGS = (('off', 0, 0), ('off12', 0, 12), ('on', 1, 0), ('auto', -1, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--n', type=int, default=1000000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import bench

    tm, X, cfg = bench.build_map('C5', 0, n_override=args.n)
    lib = tm._lib
    kernel = benchlib.bind(lib)
    N, D, d = tm._N, tm.D, tm._cm.d_cols
    Xs, Z, Xinv = tm._Xs, tm._cols(D, N), tm._cols(d, N, zero=True)

    def opt(name, v):
        assert lib.ttm_set_option(name, v) == 0

    def choose(s):
        opt(b'band_slopes', s[1])
        opt(b'band_ring_slots', s[2])

    coefs, info = {}, {}
    ref = None
    for s in SETTINGS:                                       # a vector per setting, its tables, the kernel names, the same bits under every setting
        choose(s)
        tm._pack_memo = None
        coefs[s[0]] = tm._pack_coeffs()
        tm.forward_device(Xs, N, coef=coefs[s[0]], Z=Z)
        torch.cuda.synchronize()
        kf = kernel()
        tm.inverse_device(Z, N, coef=coefs[s[0]], X=Xinv)
        torch.cuda.synchronize()
        img = next(iter(coefs[s[0]]._ttm_tables.values()))[5]
        info[s[0]] = {'kernels': [kf, kernel()], 'image_doubles': int(img.numel() // D), 'fwd': [], 'inv': [], 'step': []}
        if ref is None:
            ref = (Z.clone(), Xinv.clone())
        info[s[0]]['bit_identical_to_first_setting'] = bool(torch.equal(Z.view(torch.int64), ref[0].view(torch.int64)) and
                                                           torch.equal(Xinv.view(torch.int64), ref[1].view(torch.int64)))
    ref = None

    def step(s):
        tm.forward_device(Xs, N, coef=coefs[s[0]], Z=Z)
        tm.inverse_device(Z, N, coef=coefs[s[0]], X=Xinv)

    choose(SETTINGS[0])
    benchlib.keep_busy(lambda: step(SETTINGS[0]), 50)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    for _ in range(args.rounds):
        for s in SETTINGS:
            choose(s)
            c = coefs[s[0]]
            for _ in range(3):
                step(s)
            for a, b, e in ev:
                a.record()
                tm.forward_device(Xs, N, coef=c, Z=Z)
                b.record()
                tm.inverse_device(Z, N, coef=c, X=Xinv)
                e.record()
            torch.cuda.synchronize()
            info[s[0]]['fwd'].append(float(np.mean([a.elapsed_time(b) for a, b, e in ev])))
            info[s[0]]['inv'].append(float(np.mean([b.elapsed_time(e) for a, b, e in ev])))
            info[s[0]]['step'].append(float(ev[0][0].elapsed_time(ev[-1][2]) / len(ev)))
    choose(SETTINGS[-1])
    out = {}
    for name, v in info.items():
        o = {'kernels': v['kernels'], 'image_doubles': v['image_doubles'], 'bit_identical_to_first_setting': v['bit_identical_to_first_setting']}
        for key in ('fwd', 'inv', 'step'):
            r = np.array(v[key])
            o[key + '_ms'] = {'median': float(np.median(r)), 'min': float(r.min()), 'max': float(r.max()), 'rounds': v[key]}
        out[name] = o
        print('N = %d %-6s image %4d doubles  %s  bits %s' % (N, name, o['image_doubles'],
                                                              '  '.join('%s %.4f (%.4f-%.4f)' % (k, o[k + '_ms']['median'], o[k + '_ms']['min'],
                                                                                                   o[k + '_ms']['max']) for k in ('fwd', 'inv', 'step')),
                                                              'same' if o['bit_identical_to_first_setting'] else 'DIFFER'), flush=True)
    benchlib.finish({'N': N, 'D': D, 'steps_per_round': args.steps, 'rounds': args.rounds, 'settings': out}, args.out)


if __name__ == '__main__':
    main()
