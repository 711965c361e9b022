"""Time the two launches of the headline step (bench.py, C5: k_band_forward then k_band_inverse_ring) under the whole-tile cut
(option band_full_tiles), with Z through LDS on full tiles (option band_zdma) and with fewer slots in the inverse's ring (option
band_ring_slots; csrc/ttm_band_policy.h), in ONE process.

    python tools/band_zdma_bench.py [--out FILE.json] [--steps 40] [--rounds 6] [--n 1000000]

The settings, alternated round by round after the chip has been kept busy (tools/benchlib.py's method, as
tools/band_resident_bench.py):

    today    band_full_tiles = 0, band_zdma = 0, band_ring_slots = 0     N / #CUs rows per workgroup (no full tile at 1e6 rows), 24 slots
    today12  ... band_ring_slots = 12                                      today's cut, a ring of 12 slots
    cut      band_full_tiles = 1, band_zdma = 0, band_ring_slots = 0      245 workgroups of 4096 rows
    ring16   ... band_ring_slots = 16
    ring12   ... band_ring_slots = 12                                      ZD = 0 with the 12 slots ZD = 1 leaves the ring
    zdma     band_full_tiles = 1, band_zdma = 1, band_ring_slots = 0      Z through LDS (12 slots beside the column buffers)
    auto     every option at -1: what a plain run takes

A round of a setting is 3 untimed steps, then --steps steps with HIP events in front of the forward launch, between the two and
behind the inverse.  Per setting: the median over the rounds of the mean forward, inverse and step time, and the rounds' min-max.
"""
import argparse
import os
import sys

import numpy as np

import benchlib

SETTINGS = (('today', 0, 0, 0), ('today12', 0, 0, 12), ('cut', 1, 0, 0), ('ring16', 1, 0, 16), ('ring12', 1, 0, 12), ('zdma', 1, 1, 0),
            ('auto', -1, -1, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out', default='')
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--n', type=int, default=1000000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import bench

    tm, X, cfg = bench.build_map('C5', 0, n_override=args.n)
    lib = tm._lib
    kernel = benchlib.bind(lib)
    N, D, d = tm._N, tm.D, tm._cm.d_cols
    coef = tm._pack_coeffs()
    Xs, Z, Xinv = tm._Xs, tm._cols(D, N), tm._cols(d, N, zero=True)

    def opt(name, v):
        assert lib.ttm_set_option(name, v) == 0

    def forward(s):
        tm.forward_device(Xs, N, coef=coef, Z=Z)

    def inverse(s):
        tm.inverse_device(Z, N, coef=coef, X=Xinv)

    def choose(s):
        opt(b'band_full_tiles', s[1])
        opt(b'band_zdma', s[2])
        opt(b'band_ring_slots', s[3])

    info = {}
    ref = None
    for s in SETTINGS:                                       # first launches, kernel names, the same bits under every setting
        choose(s)
        forward(s)
        torch.cuda.synchronize()
        kf = kernel()
        inverse(s)
        torch.cuda.synchronize()
        info[s[0]] = {'kernels': [kf, kernel()], 'fwd': [], 'inv': [], 'step': []}
        if ref is None:
            ref = (Z.clone(), Xinv.clone())
        info[s[0]]['bit_identical_to_first_setting'] = bool(torch.equal(Z.view(torch.int64), ref[0].view(torch.int64)) and
                                                           torch.equal(Xinv.view(torch.int64), ref[1].view(torch.int64)))
    ref = None
    benchlib.keep_busy(lambda: (forward(SETTINGS[0]), inverse(SETTINGS[0])), 50)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.steps)]
    for _ in range(args.rounds):
        for s in SETTINGS:
            choose(s)
            for _ in range(3):
                forward(s)
                inverse(s)
            for a, b, c in ev:
                a.record()
                forward(s)
                b.record()
                inverse(s)
                c.record()
            torch.cuda.synchronize()
            info[s[0]]['fwd'].append(float(np.mean([a.elapsed_time(b) for a, b, c in ev])))
            info[s[0]]['inv'].append(float(np.mean([b.elapsed_time(c) for a, b, c in ev])))
            info[s[0]]['step'].append(float(ev[0][0].elapsed_time(ev[-1][2]) / len(ev)))
    choose(SETTINGS[-1])
    out = {}
    for name, v in info.items():
        o = {'kernels': v['kernels'], 'bit_identical_to_first_setting': v['bit_identical_to_first_setting']}
        for key in ('fwd', 'inv', 'step'):
            r = np.array(v[key])
            o[key + '_ms'] = {'median': float(np.median(r)), 'min': float(r.min()), 'max': float(r.max()), 'rounds': v[key]}
        out[name] = o
        print('N = %d %-8s %s  bits %s' % (N, name, '  '.join('%s %.4f (%.4f-%.4f)' % (k, o[k + '_ms']['median'], o[k + '_ms']['min'],
                                                                                        o[k + '_ms']['max']) for k in ('fwd', 'inv', 'step')),
                                         'same' if o['bit_identical_to_first_setting'] else 'DIFFER'), flush=True)
    benchlib.finish({'N': N, 'D': D, 'steps_per_round': args.steps, 'rounds': args.rounds, 'settings': out}, args.out)


if __name__ == '__main__':
    main()
