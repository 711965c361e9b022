"""Time importance weights and resampling on the device (ttm_weight_scan, ttm_resample) against the torch composition a caller had
before them, and sample_importance against sample(logdensity=True) with NumPy resampling on the host.

    python tools/resample_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out profiles/resample_bench.json]
                                   [--launches 100] [--rounds 10] [--workloads C5,C2b] [--calls 3]

Workloads: C5 (40 columns) and C2b (2 columns), N = M = 1e6 - bench.py's maps and coefficient fixtures.  The matrix that is
resampled is the map's own draw sample_device(N, seed 0, draw 0, logq) in standardised coordinates, the log-weights are those of
the standard normal target against it.  Versions, alternated round by round within the one process after a warm-up of every
version and a second of busy chip (the chip holds its clock only while it is kept busy: bench.py):
  scan                 ttm_weight_scan as the library plans it (phase C forms exp again), cum alone
  scan_reread          option wscan_reread = 1 (phase C rereads the q that phase A parked in cum)
  resample_<scheme>    ttm_resample with the ancestors written as well, for systematic, stratified and multinomial
  pair_<scheme>        scan, then resample_<scheme>
  torch_weights        m = max, w = exp(logw - m), cum = cumsum(w) in float64
  torch_resample_<s>   thresholds from torch.rand on the device, searchsorted(cum, t, right=True), index_select along the rows
  torch_pair_<scheme>  the two
The torch versions run on the same buffers in the same session and reuse their outputs (out=) where torch lets them.
HIP events around every batch of launches; per version the median over the rounds of the mean launch time with min and max, and the
share of the 6.29 TB/s copy peak on the algorithmic bytes: scan 8 N read + 8 N written; resample 16 M ncols + 4 M (ancestors) +
8 N (cum, read at least once by the ordered schemes; the multinomial search touches more).
sample_importance (C5 only, wall clock around whole calls, --calls of each, alternated): `device` is
sample_importance(N, target, target_on_device=True), `host` is sample(N, logdensity=True), the target in NumPy, exp / cumsum /
searchsorted / take on the host.
"""
import time

import numpy as np

import benchlib

SCHEMES = ['systematic', 'stratified', 'multinomial']


class WallClock:
    def __init__(self, torch):
        self.torch = torch

    def sync(self):
        self.torch.cuda.synchronize()

    def start(self):
        self.sync()
        self.t = time.perf_counter()

    def stop(self):
        self.sync()
        return (time.perf_counter() - self.t) * 1e3


def main():
    ap = benchlib.parser(__doc__, 100, 'C5,C2b')
    ap.add_argument('--calls', type=int, default=3)
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('resample_bench: no GPU - nothing is timed without one')
    from triangular_transport_toolbox_amd import _capi, weights
    res['workloads'] = {}
    res['copy_peak_gbs'] = bench.COPY_PEAK_GBS
    for wl in args.workloads.split(','):
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        pin = benchlib.option(lib, 'wscan_reread')
        N, D = tm._N, tm.D
        M = N
        Xs, logq = tm.sample_device(N, seed=0, draw=0, logq=True)
        X = Xs[-D:].contiguous()
        ld = X.shape[1]
        logw = (-0.5 * (X[:, :N] * X[:, :N]).sum(dim=0) - logq[:N]).contiguous()
        cum = tm._empty(N, dtype=torch.int64)
        words, work = tm._empty(4), tm._empty(weights.work_words(N))
        Y = tm._cols(D, M)
        idx = tm._empty(M, dtype=torch.int32)
        st = tm._stream()

        def scan():
            _capi.check(lib.ttm_weight_scan(tm._ptr(logw), N, tm._ptr(cum), None, tm._ptr(words), tm._ptr(work), st))

        def resample(sid):
            def fn():
                _capi.check(lib.ttm_resample(tm._ptr(cum), N, M, sid, 0, 0, tm._ptr(X), ld, D, tm._ptr(Y), Y.shape[1], tm._ptr(idx), st))
            return fn

        def pair(sid):
            r = resample(sid)

            def fn():
                scan()
                r()
            return fn

        w, cumf = torch.empty_like(logw), torch.empty_like(logw)
        thr, u = torch.empty(M, dtype=torch.float64, device=X.device), torch.empty(M, dtype=torch.float64, device=X.device)
        steps = torch.arange(M, dtype=torch.float64, device=X.device)
        tidx = torch.empty(M, dtype=torch.int64, device=X.device)
        Yt = torch.empty((D, M), dtype=torch.float64, device=X.device)

        def torch_weights():
            torch.sub(logw, logw.max(), out=w)
            torch.exp(w, out=w)
            torch.cumsum(w, 0, out=cumf)

        def torch_resample(sid):
            def fn():
                if sid == 0:
                    torch.add(steps, torch.rand(1, dtype=torch.float64, device=X.device), out=thr)
                    thr.mul_(cumf[-1] / M)
                elif sid == 1:
                    torch.rand(M, dtype=torch.float64, device=X.device, out=u)
                    torch.add(steps, u, out=thr)
                    thr.mul_(cumf[-1] / M)
                else:
                    torch.rand(M, dtype=torch.float64, device=X.device, out=thr)
                    thr.mul_(cumf[-1])
                torch.searchsorted(cumf, thr, right=True, out=tidx)
                tidx.clamp_(max=N - 1)
                torch.index_select(X, 1, tidx, out=Yt)
            return fn

        def torch_pair(sid):
            r = torch_resample(sid)

            def fn():
                torch_weights()
                r()
            return fn

        versions = [('scan', -1, scan), ('scan_reread', 1, scan), ('torch_weights', None, torch_weights)]
        for sid, name in enumerate(SCHEMES):
            versions += [('resample_' + name, None, resample(sid)), ('pair_' + name, None, pair(sid)),
                         ('torch_resample_' + name, None, torch_resample(sid)), ('torch_pair_' + name, None, torch_pair(sid))]
        info = benchlib.warm_up(versions, pin, 3, kernel)
        s = weights.Weights(cum, words, N, weights.weight_bits(N)).importance_summary()
        benchlib.keep_busy(scan, 50)
        benchlib.time_rounds(versions, info, pin, args.rounds, benchlib.per_round(args), settle=2)
        gb_scan = 16.0 * N / 1e9
        gb_res = (16.0 * M * D + 4.0 * M + 8.0 * N) / 1e9
        for name, v in info.items():
            gb = gb_scan if ('scan' in name or 'weights' in name) else gb_res + (gb_scan if 'pair' in name else 0.0)
            benchlib.summarise(v, gb, bench.COPY_PEAK_GBS)
            v['copy_peak_frac_on_algorithmic_bytes'] = v.pop('hbm_frac_on_algorithmic_bytes')
            v['algorithmic_gbytes'] = gb
            if name.startswith('torch'):
                v['kernel'] = 'torch'
        out = {'N': N, 'M': M, 'ncols': D, 'ess': s['ess'], 'log_mean_weight': s['log_mean_weight'], 'versions': info,
               'reread_over_recompute_time': info['scan_reread']['ms'] / info['scan']['ms'],
               'scan_over_torch_weights_time': info['scan']['ms'] / info['torch_weights']['ms']}
        for name in SCHEMES:
            out['resample_over_torch_time_' + name] = info['resample_' + name]['ms'] / info['torch_resample_' + name]['ms']
            out['pair_over_torch_time_' + name] = info['pair_' + name]['ms'] / info['torch_pair_' + name]['ms']
        benchlib.report(wl, info)

        if wl == 'C5':
            sd, mu = np.asarray(tm.X_std, dtype=float), np.asarray(tm.X_mean, dtype=float)
            sd_t, mu_t = tm._to_dev(sd)[:, None], tm._to_dev(mu)[:, None]

            def target(x):
                z = (x - mu) / sd
                return -0.5 * (z * z).sum(axis=1)

            def target_dev(x):
                z = (x - mu_t) / sd_t
                return -0.5 * (z * z).sum(dim=0)

            def device_call():
                tm.sample_importance(N, target_dev, seed=0, draw=0, target_on_device=True)

            def host_call():
                x, lq = tm.sample(N, seed=0, draw=0, logdensity=True)
                lw = target(x) - lq
                c = np.cumsum(np.exp(lw - lw.max()))
                t = (np.arange(N) + np.random.random()) * (c[-1] / N)
                return x[np.minimum(np.searchsorted(c, t, side='right'), N - 1)]

            wall = WallClock(torch)
            calls = [('device', None, device_call), ('host', None, host_call)]
            cinfo = benchlib.warm_up(calls, None, 1, kernel, clock=wall)
            benchlib.time_rounds(calls, cinfo, None, args.calls, 1, settle=0, clock=wall)
            for v in cinfo.values():
                benchlib.summarise(v)
            out['sample_importance'] = {'calls': cinfo, 'device_over_host_time': cinfo['device']['ms'] / cinfo['host']['ms']}
            benchlib.report(wl + ' sample_importance (wall clock)', cinfo)
        res['workloads'][wl] = out
        del tm, X, Xs, Y, Yt
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
