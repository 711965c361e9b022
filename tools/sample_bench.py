"""Time sampling from a fitted map: the reference-draw fill (ttm_normal_fill), sample_device beside inverse_device, sample() beside inverse_map().

    python tools/sample_bench.py [--root TREE] [--label NAME] [--commit ID] [--out profiles/sample_bench.json] [--launches 200] [--rounds 10]
                                 [--workloads C5,C2b,C5int] [--rows N]

Workloads: C5 (d = 40, N = 1e6), C2b (d = 2, N = 1e6) and C5int (d = 40, integrated rectifier, N = 2e5: the reference's bisection
with its sample-0 replay) - bench.py's maps and coefficient fixtures.  Device versions, alternated round by round within the one
process after a warm-up of every version and a second of busy chip (the chip holds its clock only while it is kept busy: bench.py):
  fill            reference_device into a resident buffer: one launch of k_normal_fill
  fill_odd        the same window shifted by one row (row0 = 1): every pair goes out as two 8-byte stores
  inverse_device  the map's configured inverse on the pre-filled Z - what the parent of this feature offers, the yardstick
  sample_device   fill + inverse, Z and X resident
HIP events around every batch of launches; per version the median over the rounds of the mean launch time and the spread (min,
max over the rounds) and the kernel that ran (ttm_last_kernel).  For the fill: the bytes it writes (8 N D) over its time beside the
6.29 TB/s copy peak, and its fp64 rate beside the 78.6 TFLOP/s vector peak - FLOP_PER_PAIR operations per pair and column, counted
in the kernel's ISA on the path a deviate takes (below).
Host versions (wall clock around calls that end in a synchronise, median of --host-reps):
  sample          sample(N): N x D NumPy array out, nothing in
  inverse_map     inverse_map(Z) on a host Z of the same size: the same array out, Z over PCIe first
"""
import json
import time

import numpy as np

import benchlib

# fp64 operations per row pair and column of k_normal_fill, counted in the ISA hipcc emits for gfx950 on the path every deviate
# takes (the small-argument branch of sincos: 0 < t < 2 pi): 134 v_*_f64 instructions, 39 of them fused multiply-adds counted
# twice - 2 conversions of the uniforms aside, log, sqrt, the argument reduction and the two polynomial kernels.  The ten Philox
# rounds beside them are 190 integer instructions (two 32 x 32 -> 64 multiplies per round) that no fp64 rate accounts for.
FLOP_PER_PAIR = 134 + 39


def main():
    ap = benchlib.parser(__doc__, 200, 'C5,C2b,C5int')
    ap.add_argument('--host-reps', type=int, default=7)
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('sample_bench: no GPU - nothing is timed without one')
    res.update({'flop_per_pair': FLOP_PER_PAIR, 'copy_peak_GBs': bench.COPY_PEAK_GBS, 'fp64_peak_TFLOPs': bench.FP64_PEAK_TFLOPS, 'workloads': {}})
    for wl in args.workloads.split(','):
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        kernel = benchlib.bind(tm._lib)
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        coef = tm._pack_coeffs()
        Z, Zodd = tm._cols(D, N), tm._cols(D, N + 2)
        X = tm._cols(d, N, zero=True)
        tm.reference_device(N, seed=1, draw=0, out=Z)

        def fill():
            tm.reference_device(N, seed=1, draw=0, out=Z)

        def fill_odd():
            tm.reference_device(N, seed=1, draw=0, row0=1, out=Zodd)

        def inverse_device():
            tm.inverse_device(Z, N, coef=coef, X=X)

        def sample_device():
            tm.sample_device(N, seed=1, draw=0, X=X, Z=Z)

        versions = [('fill', None, fill), ('fill_odd', None, fill_odd), ('inverse_device', None, inverse_device),
                    ('sample_device', None, sample_device)]
        slow = tm.monotonicity.lower() != 'separable monotonicity'              # (a bisection of 2e5 x 40 roots: tens of ms)
        per = {name: max(1, (args.launches // (20 if slow and name.endswith('device') else 1)) // args.rounds) for name, _, _ in versions}

        def after(name, v):
            v['launches_per_round'] = per[name]

        info = benchlib.warm_up(versions, None, 2, kernel, after)
        Xa = X[:, :N].clone()
        sample_device()
        torch.cuda.synchronize()
        info['sample_device']['equals_inverse_device_of_the_fill'] = bool(torch.equal(Xa, X[:, :N]))
        del Xa
        benchlib.keep_busy(fill, 20)
        benchlib.time_rounds(versions, info, None, args.rounds, per, settle=1)
        for v in info.values():
            benchlib.summarise(v)
        gbytes = 8.0 * N * D / 1e9
        gflop = FLOP_PER_PAIR * 0.5 * N * D / 1e9
        for name in ('fill', 'fill_odd'):
            v = info[name]
            v['written_gbytes'] = gbytes
            v['written_GBs'] = gbytes / (v['ms'] * 1e-3)
            v['copy_peak_frac'] = v['written_GBs'] / bench.COPY_PEAK_GBS
            v['counted_fp64_TFLOPs'] = gflop / (v['ms'] * 1e-3) / 1e3
            v['fp64_peak_frac'] = v['counted_fp64_TFLOPs'] / bench.FP64_PEAK_TFLOPS
        del Z, Zodd, X
        # the host boundary: sample() beside inverse_map() on a host Z of the same size
        Zhost = np.random.default_rng(3).standard_normal((N, D))
        host = {}
        for name, fn in (('sample', lambda: tm.sample(N, seed=1, draw=0)), ('inverse_map', lambda: tm.inverse_map(Zhost))):
            fn()
            ts = []
            for _ in range(args.host_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                assert out.shape == (N, D)
            h = {'ms_rounds': ts}
            benchlib.summarise(h)
            host[name] = {k: h[k] for k in ('ms', 'ms_min', 'ms_max')}
        t = {k: v['ms'] for k, v in info.items()}
        res['workloads'][wl] = {'N': N, 'D': D, 'd': d, 'device': info, 'host': host,
                                'fill_over_inverse_device_time': t['fill'] / t['inverse_device'],
                                'sample_device_over_inverse_device_time': t['sample_device'] / t['inverse_device'],
                                'sample_over_inverse_map_time': host['sample']['ms'] / host['inverse_map']['ms']}
        benchlib.report(wl, info, json.dumps({k: round(v['ms'], 3) for k, v in host.items()}))
        del tm
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
