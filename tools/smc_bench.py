"""Time the two device pieces of tempered sequential Monte Carlo - the temperature search's scan (ttm_temper_scan: k_temper_sums,
k_temper_finish) and the tempered Metropolis-Hastings step (ttm_mh_step_tempered, k_mh_step) - beside what they replace, and
whole runs of smc_device.

    python tools/smc_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out profiles/smc_bench.json]
                              [--launches 50] [--rounds 10] [--workloads C5,C2b] [--particles 100000] [--calls 3]
                              [--smc-workloads C5,C5newton,C2b] [--shift 0.3] [--scale 0.8]

Scan (N = 1e6 log-weights, standard normal times 3; --rows for rehearsals).  Versions, alternated round by round within the one
process after a warm-up of every version and a second of busy chip (bench.py), for C = 1, 8, 64 candidates:
  temper_C      one ttm_temper_scan of C candidates (four launches)
  scan_xC       C calls of ttm_weight_scan (five launches each) on a pre-multiplied vector - the same vector every time, so the
                C x N products that the composition would also have to form and hold are NOT charged to it
  torch_C       the effective sample sizes from torch ops on the same buffer: per chunk of at most 8 candidates the outer product,
                logsumexp of it and of twice it (a chunk is a 64 MB temporary at N = 1e6)
HIP events around every batch; per version the median over the rounds of the mean call time with min and max, and the share of
the 6.29 TB/s copy peak on the algorithmic bytes (16 N: logw is read by the maximum and by the sums; the tile words are small).
Step (the maps of bench.py, C5: 40 columns, C2b: 2 columns, N = 1e6 rows; buffers as tools/mcmc_bench.py): mh_step is ttm_mh_step
in fused mode (decide and propose, rho = 0.7), mh_step_tempered the same call at beta = 0.5 - one kernel, one more multiply.
Runs (wall clock around whole calls of smc_device, --calls of each, alternated): --particles particles towards
N(X_mean + shift X_std, diag((scale X_std)^2)) evaluated on the device, ess_target 0.5, two moves per stage at rho = 0.5, for C5
with the table inverse, C5 with the Newton inverse and C2b; reported as ms per stage with the number of stages, the log-evidence
and the mean acceptance rate.
"""
import time

import numpy as np

import benchlib

RHO = 0.7
BETA = 0.5
CANDIDATES = (1, 8, 64)
TORCH_CHUNK = 8


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
    ap = benchlib.parser(__doc__, 50, 'C5,C2b')
    ap.add_argument('--particles', type=int, default=100000)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--smc-workloads', default='C5,C5newton,C2b')
    ap.add_argument('--shift', type=float, default=0.3)
    ap.add_argument('--scale', type=float, default=0.8)
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import ctypes
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('smc_bench: no GPU - nothing is timed without one')
    from triangular_transport_toolbox_amd import _capi, weights
    res['copy_peak_gbs'] = bench.COPY_PEAK_GBS

    # the scan
    tm, _, _ = bench.build_map('C2b', 0, n_override=args.rows or None)
    lib, st = tm._lib, tm._stream()
    kernel = benchlib.bind(lib)
    N = tm._N
    logw = (3.0 * tm.reference_device(N, seed=2, draw=0, ncols=1)[0, :N]).contiguous()
    pre = (0.37 * logw).contiguous()
    cum, words = tm._empty(N, dtype=torch.int64), tm._empty(4)
    swork = tm._empty(weights.work_words(N))
    versions, per, n = [], {}, benchlib.per_round(args)          # (calls per timed batch: fewer of the versions that are C calls in one)
    for C in CANDIDATES:
        deltas = np.ascontiguousarray(np.arange(1, C + 1, dtype=np.float64) / C)
        d_dev = tm._to_dev(deltas)
        out, twork = tm._empty(C, 4), tm._empty(weights.temper_work_words(N, C))

        def temper(deltas=deltas, C=C, out=out, twork=twork):
            _capi.check(lib.ttm_temper_scan(tm._ptr(logw), N, ctypes.c_void_p(deltas.ctypes.data), C, tm._ptr(out), tm._ptr(twork), st))

        def scans(C=C):
            for _ in range(C):
                _capi.check(lib.ttm_weight_scan(tm._ptr(pre), N, tm._ptr(cum), None, tm._ptr(words), tm._ptr(swork), st))

        def torch_ess(d_dev=d_dev, C=C):
            ess = []
            for c0 in range(0, C, TORCH_CHUNK):
                v = d_dev[c0:c0 + TORCH_CHUNK, None] * logw[None, :]
                ess.append(torch.exp(2.0 * torch.logsumexp(v, dim=1) - torch.logsumexp(2.0 * v, dim=1)))
            return torch.cat(ess)

        versions += [('temper_%d' % C, None, temper), ('scan_x%d' % C, None, scans), ('torch_%d' % C, None, torch_ess)]
        per.update({'temper_%d' % C: n, 'scan_x%d' % C: max(1, n // C), 'torch_%d' % C: max(1, n // C)})
    info = benchlib.warm_up(versions, None, 2, kernel)
    # the two device paths agree on the effective sample sizes (the torch composition has no fixed-point truncation: 1e-5)
    K = weights.weight_bits(N)
    d8 = np.arange(1, 9, dtype=np.float64) / 8
    ours = np.array(weights.temper_ess(tm.temper_device(logw, N, d8).cpu().numpy(), N, K))
    v = tm._to_dev(d8)[:, None] * logw[None, :]
    theirs = torch.exp(2.0 * torch.logsumexp(v, dim=1) - torch.logsumexp(2.0 * v, dim=1)).cpu().numpy()
    res['scan_ess_rel_diff_vs_torch'] = float(np.max(np.abs(ours - theirs) / theirs))
    del v
    benchlib.keep_busy(versions[0][2], 50)
    benchlib.time_rounds(versions, info, None, args.rounds, per, settle=1)
    for name, v in info.items():
        benchlib.summarise(v, 16.0 * N / 1e9, bench.COPY_PEAK_GBS)
        v['copy_peak_frac_on_algorithmic_bytes'] = v.pop('hbm_frac_on_algorithmic_bytes')
        if name.startswith('torch'):
            v['kernel'] = 'torch'
    res['scan'] = {'N': N, 'versions': info,
                   'temper_over_scans_time': {str(C): info['temper_%d' % C]['ms'] / info['scan_x%d' % C]['ms'] for C in CANDIDATES},
                   'temper_over_torch_time': {str(C): info['temper_%d' % C]['ms'] / info['torch_%d' % C]['ms'] for C in CANDIDATES}}
    benchlib.report('scan', info, 'ESS against torch %.2e' % res['scan_ess_rel_diff_vs_torch'])
    del tm, logw, pre, cum

    # the step
    res['workloads'] = {}
    for wl in [w for w in args.workloads.split(',') if w]:
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib, st = tm._lib, tm._stream()
        kernel = benchlib.bind(lib)
        N, D = tm._N, tm.D
        Zc, Xc, Zp, Xp = (tm.reference_device(N, seed=1, draw=k) for k in range(4))
        Zn = tm._cols(D, N)
        ld = Zc.shape[1]
        lc = tm.reference_device(N, seed=2, draw=0, ncols=1)[0, :N].contiguous()
        lp = (lc + 1.5 * tm.reference_device(N, seed=2, draw=1, ncols=1)[0, :N] - 0.8).contiguous()
        lo = tm._empty(N)
        n_acc, n_bad = tm._zeros(N, dtype=torch.int32), tm._zeros(N, dtype=torch.int32)

        def plain():
            _capi.check(lib.ttm_mh_step(tm._ptr(Zc), ld, tm._ptr(Xc), ld, tm._ptr(lc), tm._ptr(lo), tm._ptr(Zp), ld, tm._ptr(Xp), ld, tm._ptr(lp),
                                        tm._ptr(Zn), ld, RHO, None, ld, tm._ptr(n_acc), tm._ptr(n_bad), N, D, 0, 0, 1, 2, 0, st))

        def tempered():
            _capi.check(lib.ttm_mh_step_tempered(tm._ptr(Zc), ld, tm._ptr(Xc), ld, tm._ptr(lc), tm._ptr(lo), tm._ptr(Zp), ld, tm._ptr(Xp), ld, tm._ptr(lp),
                                                 tm._ptr(Zn), ld, RHO, BETA, None, ld, tm._ptr(n_acc), tm._ptr(n_bad), N, D, 0, 0, 1, 2, 0, st))

        versions = [('mh_step', None, plain), ('mh_step_tempered', None, tempered)]
        info = benchlib.warm_up(versions, None, 3, kernel)
        shares = {}
        for name, _, fn in versions:
            n_acc.zero_()
            fn()
            shares[name] = float(n_acc.sum().item()) / N
        benchlib.keep_busy(plain, 50)
        benchlib.time_rounds(versions, info, None, args.rounds, benchlib.per_round(args), settle=2)
        for name, v in info.items():
            a = shares[name]
            gb = (24 + 8 * a + D * (32 * a + 8 * (1 - a) + 8)) * N / 1e9
            benchlib.summarise(v, gb, bench.COPY_PEAK_GBS)
            v['copy_peak_frac_on_algorithmic_bytes'] = v.pop('hbm_frac_on_algorithmic_bytes')
            v['accepted_share'] = a
        res['workloads'][wl] = {'N': N, 'ncols': D, 'rho': RHO, 'beta': BETA, 'versions': info,
                                'tempered_over_plain_time': info['mh_step_tempered']['ms'] / info['mh_step']['ms']}
        benchlib.report(wl, info, 'accepted %.3f / %.3f' % (shares['mh_step'], shares['mh_step_tempered']))
        del tm, Zc, Xc, Zp, Xp, Zn

    # whole runs
    wall = WallClock(torch)
    res['smc'] = {'particles': args.particles, 'ess_target': 0.5, 'moves': 2, 'rho': 0.5, 'shift': args.shift, 'scale': args.scale, 'cases': {}}
    calls, meta = [], {}
    for case in [c for c in args.smc_workloads.split(',') if c]:
        wl = case.replace('newton', '')
        tm, _, _ = bench.build_map(wl, 0, n_override=args.particles)
        if case.endswith('newton'):
            tm.alternate_root_finding, tm.root_finder = False, 'newton'
        mean, sd = np.asarray(tm.X_mean, dtype=float)[-tm.D:], np.asarray(tm.X_std, dtype=float)[-tm.D:]
        mu, s = tm._to_dev(mean + args.shift * sd)[:, None], tm._to_dev(args.scale * sd)[:, None]
        norm = -float(np.sum(np.log(args.scale * sd))) - 0.5 * tm.D * float(np.log(2.0 * np.pi))

        def target(raw, mu=mu, s=s, norm=norm):
            z = (raw - mu) / s
            return norm - 0.5 * (z * z).sum(dim=0)

        def run(tm=tm, target=target, case=case):
            _, meta[case] = tm.smc_device(target, args.particles, ess_target=0.5, moves=2, rho=0.5, max_stages=400, seed=0, draw=0)

        calls.append((case, None, run))
        kernel = benchlib.bind(tm._lib)
    if calls:
        cinfo = benchlib.warm_up(calls, None, 1, kernel, clock=wall)
        benchlib.time_rounds(calls, cinfo, None, args.calls, 1, settle=0, clock=wall)
        for case, v in cinfo.items():
            benchlib.summarise(v)
            m = meta[case]
            v['stages'] = m['stages']
            v['ms_per_stage'] = v['ms'] / m['stages']
            v['log_evidence'] = m['log_evidence']
            v['accept_rate'] = float(np.mean(m['accept_rate']))
            v['min_stage_ess_over_n'] = min(m['ess']) / args.particles
        res['smc']['cases'] = cinfo
        benchlib.report('smc (wall clock, ms per run)', cinfo, ' '.join('%s: %d stages' % (c, v['stages']) for c, v in cinfo.items()))
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
