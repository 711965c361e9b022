"""Time the Metropolis-Hastings step in reference space (ttm_mh_step, k_mh_step) beside the reference-draw fill it contains and
against the torch composition of the same step, and whole chains (mcmc_device) in steps per second.

    python tools/mcmc_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out profiles/mcmc_bench.json]
                               [--launches 100] [--rounds 10] [--workloads C5,C2b] [--chains 100000] [--steps 20] [--calls 3]

Workloads: C5 (40 columns) and C2b (2 columns), N = 1e6 rows - bench.py's maps.  The state and the proposal are standard normal
matrices, the log-weights are drawn so that about half the rows accept (the accepted share is recorded).  Versions, alternated
round by round within the one process after a warm-up of every version and a second of busy chip (bench.py):
  mh_step       ttm_mh_step in fused mode: decide the step (rho = 0.7) and propose the next one, counts written
  mh_accept     the accept phase alone
  mh_propose    the propose phase alone
  normal_fill   ttm_normal_fill of the same shape alone: the deviates the propose phase contains
  torch_step    the same step from torch ops on the same buffers: rand, log, sub, compare, where (into the state) per state
                tensor, the counts, randn, mul, add - outputs reused (out=) where torch lets them
HIP events around every batch of launches; per version the median over the rounds of the mean launch time with min and max, and the
share of the 6.29 TB/s copy peak on the algorithmic bytes.  With a the accepted share and c the columns, per row: fused 24 + 8 a
(log-weights in and out, counts) + c (32 a + 8 (1 - a) + 8) (an accepted row reads the proposal's z and x and writes both, a
rejected row reads z; every row writes the next proposal); accept alone 24 + 8 a + 32 a c; propose alone 16 c; fill 8 c.
These are the bytes the step needs, not what a version moves: k_mh_step loads the proposal's z and x of every row whatever the
decision, and the torch composition (charged the same bytes, though it has no handling of bad or -inf weights and no n_bad) reads
and writes whole tensors.  The shares are therefore a common yardstick, not achieved bandwidths.
Chains (wall clock around whole calls of mcmc_device, --calls of each, alternated): --chains chains of --steps steps at rho = 0.7
towards N(X_mean, diag(X_std^2)) evaluated on the device, for C5 with the table inverse, C5 with the Newton inverse and C2a
(integrated rectifier, the search that carries log q out); reported as steps per second with the acceptance rate.
"""
import time

import numpy as np

import benchlib

RHO = 0.7


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
    ap.add_argument('--chains', type=int, default=100000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--chain-workloads', default='C5,C5newton,C2a')
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('mcmc_bench: no GPU - nothing is timed without one')
    from triangular_transport_toolbox_amd import _capi
    res['workloads'] = {}
    res['copy_peak_gbs'] = bench.COPY_PEAK_GBS
    for wl in [w for w in args.workloads.split(',') if w]:
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        N, D = tm._N, tm.D
        st = tm._stream()
        Zc, Xc, Zp, Xp = (tm.reference_device(N, seed=1, draw=k) for k in range(4))
        Zn = tm._cols(D, N)
        ld = Zc.shape[1]
        lc = tm.reference_device(N, seed=2, draw=0, ncols=1)[0, :N].contiguous()
        lp = (lc + 1.5 * tm.reference_device(N, seed=2, draw=1, ncols=1)[0, :N] - 0.8).contiguous()
        lo = tm._empty(N)
        n_acc, n_bad = tm._zeros(N, dtype=torch.int32), tm._zeros(N, dtype=torch.int32)
        s = float(np.sqrt((1.0 - RHO) * (1.0 + RHO)))

        def mh(accept, propose):
            def fn():
                _capi.check(lib.ttm_mh_step(tm._ptr(Zc), ld, tm._ptr(Xc), ld, tm._ptr(lc), tm._ptr(lo), tm._ptr(Zp) if accept else None, ld,
                                            tm._ptr(Xp) if accept else None, ld, tm._ptr(lp) if accept else None, tm._ptr(Zn) if propose else None,
                                            ld, RHO, None, ld, tm._ptr(n_acc), tm._ptr(n_bad), N, D, 0, 0, 1, 2, 0, st))
            return fn

        def fill():
            _capi.check(lib.ttm_normal_fill(tm._ptr(Zn), ld, N, D, 0, 0, 2, 0, st))

        u, diff = torch.empty_like(lc), torch.empty_like(lc)
        acc = torch.empty(N, dtype=torch.bool, device=lc.device)
        cnt = torch.zeros(N, dtype=torch.int32, device=lc.device)
        Zcv, Xcv, Zpv, Xpv, Znv = Zc[:, :N], Xc[:, :N], Zp[:, :N], Xp[:, :N], Zn[:, :N]

        def torch_step():
            torch.rand(N, dtype=torch.float64, device=lc.device, out=u)
            torch.log(u, out=u)
            torch.sub(lp, lc, out=diff)
            torch.lt(u, diff, out=acc)
            torch.where(acc, Zpv, Zcv, out=Zcv)
            torch.where(acc, Xpv, Xcv, out=Xcv)
            torch.where(acc, lp, lc, out=lo)
            cnt.add_(acc)
            torch.randn(Znv.shape, dtype=torch.float64, device=lc.device, out=Znv)
            Znv.mul_(s)
            Znv.add_(Zcv, alpha=RHO)

        versions = [('mh_step', None, mh(True, True)), ('mh_accept', None, mh(True, False)), ('mh_propose', None, mh(False, True)),
                    ('normal_fill', None, fill), ('torch_step', None, torch_step)]
        info = benchlib.warm_up(versions, None, 3, kernel)
        n_acc.zero_()
        mh(True, False)()
        a = float(n_acc.sum().item()) / N
        benchlib.keep_busy(fill, 50)
        benchlib.time_rounds(versions, info, None, args.rounds, benchlib.per_round(args), settle=2)
        per_row = {'mh_step': 24 + 8 * a + D * (32 * a + 8 * (1 - a) + 8), 'mh_accept': 24 + 8 * a + 32 * a * D, 'mh_propose': 16 * D,
                   'normal_fill': 8 * D}
        per_row['torch_step'] = per_row['mh_step']
        for name, v in info.items():
            gb = per_row[name] * N / 1e9
            benchlib.summarise(v, gb, bench.COPY_PEAK_GBS)
            v['copy_peak_frac_on_algorithmic_bytes'] = v.pop('hbm_frac_on_algorithmic_bytes')
            v['algorithmic_gbytes'] = gb
            if name.startswith('torch'):
                v['kernel'] = 'torch'
        res['workloads'][wl] = {'N': N, 'ncols': D, 'rho': RHO, 'accepted_share': a, 'versions': info,
                                'step_over_torch_time': info['mh_step']['ms'] / info['torch_step']['ms'],
                                'step_over_fill_time': info['mh_step']['ms'] / info['normal_fill']['ms']}
        benchlib.report(wl, info, 'accepted %.3f' % a)
        del tm, Zc, Xc, Zp, Xp, Zn

    # whole chains
    wall = WallClock(torch)
    res['chains'] = {'chains': args.chains, 'steps': args.steps, 'rho': RHO, 'cases': {}}
    calls, meta = [], {}
    for case in [c for c in args.chain_workloads.split(',') if c]:
        wl = case.replace('newton', '')
        tm, _, _ = bench.build_map(wl, 0, n_override=args.chains)
        if case.endswith('newton'):
            tm.alternate_root_finding, tm.root_finder = False, 'newton'
        mu, sd = tm._to_dev(np.asarray(tm.X_mean, dtype=float))[-tm.D:, None], tm._to_dev(np.asarray(tm.X_std, dtype=float))[-tm.D:, None]

        def target(raw, mu=mu, sd=sd):
            z = (raw - mu) / sd
            return -0.5 * (z * z).sum(dim=0)

        def run(tm=tm, target=target, case=case):
            _, state = tm.mcmc_device(target, args.chains, args.steps, rho=RHO, seed=0, draw=0)
            meta[case] = state

        calls.append((case, None, run))
        kernel = benchlib.bind(tm._lib)
    if calls:
        cinfo = benchlib.warm_up(calls, None, 1, kernel, clock=wall)
        benchlib.time_rounds(calls, cinfo, None, args.calls, 1, settle=0, clock=wall)
        for case, v in cinfo.items():
            benchlib.summarise(v)
            v['steps_per_second'] = args.steps / (v['ms'] * 1e-3)
            v['ms_per_step'] = v['ms'] / args.steps
            v['accept_rate'] = float(meta[case]['n_acc'].sum().item()) / (args.chains * args.steps)
        res['chains']['cases'] = cinfo
        benchlib.report('chains (wall clock, ms per call of %d steps)' % args.steps, cinfo)
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
