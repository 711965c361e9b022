"""Time the device pieces of the Langevin moves - the gradient's pull through the map (ttm_pull_gradient, k_pull_gradient_u), the
correction of the acceptance ratio (ttm_langevin_corr, k_langevin_corr) and the step with drift (ttm_mh_step_langevin,
k_mh_step<drift>) - beside their nearest neighbours, and whole chains with and without the gradient.

    python tools/langevin_bench.py [--root TREE] [--rows N] [--label NAME] [--commit ID] [--out profiles/langevin_bench.json]
                                   [--launches 100] [--rounds 10] [--workloads C5,C2b] [--chain-workloads C5,C2b]
                                   [--chains 100000] [--steps 20] [--calls 3] [--rhos 0.5,0.7,0.9]

Workloads: C5 (40 columns) and C2b (2 columns), N = 1e6 rows - bench.py's maps, on their own standardised samples.  Versions,
alternated round by round within the one process after a warm-up of every version and a second of busy chip (bench.py):
  pull_gradient      ttm_pull_gradient over the whole map, out of place, with g_scale and the log-determinant term
  score_u            ttm_score forced onto k_score_u (option band_score = 0): the like-for-like kernel, one row per thread
  score_band         ttm_score as the library plans it (k_band_score for banded maps)
  langevin_corr      ttm_langevin_corr of the same shape
  mh_step_langevin   ttm_mh_step_langevin in fused mode (decide with the correction, take W, propose with drift), rho = 0.7
  mh_step_tempered   ttm_mh_step_tempered in fused mode on the same buffers
HIP events around every batch of launches; per version the median over the rounds of the mean launch time with min and max, and
the share of the 6.29 TB/s copy peak on the algorithmic bytes: pull and score (d + 2 ncols) 8 N and (d + ncols) 8 N, the
correction 4 ncols 8 N + 8 N, the steps as tools/mcmc_bench.py charges ttm_mh_step (the step with drift: 16 a ncols + 8 ncols
+ 8 more per row for W and the correction, a the accepted share).
Chains (wall clock around whole calls of mcmc_device, --calls of each, alternated): --chains chains of --steps steps towards
N(X_mean, diag(X_std^2)) evaluated on the device (the target of tools/mcmc_bench.py), without and with its gradient, at every
rho of --rhos; per case ms per step, the acceptance rate and the mean squared jump in z per step, sum_j (z_j(t + 1) - z_j(t))^2
averaged over chains and steps (from an untimed run continued step by step: the same chain, bit for bit).
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
    ap.add_argument('--chain-workloads', default='C5,C2b')
    ap.add_argument('--rhos', default='0.5,0.7,0.9')
    args = ap.parse_args()
    bench, res = benchlib.start(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('langevin_bench: no GPU - nothing is timed without one')
    from triangular_transport_toolbox_amd import _capi
    res['workloads'] = {}
    res['copy_peak_gbs'] = bench.COPY_PEAK_GBS
    for wl in [w for w in args.workloads.split(',') if w]:
        tm, _, _ = bench.build_map(wl, 0, n_override=args.rows or None)
        lib = tm._lib
        kernel = benchlib.bind(lib)
        pin = benchlib.option(lib, 'band_score')
        N, D, d = tm._N, tm.D, tm._cm.d_cols
        st, p = tm._stream(), tm._ptr
        coef = tm._pack_coeffs()
        fold = coef._ttm_fold
        Xs = tm._Xs
        ldx = Xs.shape[1]
        G, Zc, Xc, Zp, Xp, Wc, Wp = (tm.reference_device(N, seed=1, draw=k) for k in range(7))
        W, Zn = tm._cols(D, N), tm._cols(D, N)
        ld = G.shape[1]
        sigma = tm._to_dev(np.asarray(tm.X_std, dtype=float)[d - D:])
        inv_sigma = tm._inv_std(d - D, d)
        affine = tm._to_dev(np.ascontiguousarray(np.column_stack((np.asarray(tm.X_std, dtype=float)[d - D:], np.asarray(tm.X_mean, dtype=float)[d - D:]))))
        lc = tm.reference_device(N, seed=2, draw=0, ncols=1)[0, :N].contiguous()
        lp = (lc + 1.5 * tm.reference_device(N, seed=2, draw=1, ncols=1)[0, :N] - 0.8).contiguous()
        lo, corr = tm._empty(N), tm._empty(N)
        n_acc, n_bad = tm._zeros(N, dtype=torch.int32), tm._zeros(N, dtype=torch.int32)
        kappa = 1.0 - RHO

        def pull():
            _capi.check(lib.ttm_pull_gradient(tm._pp, p(coef), p(fold), 0, D, p(Xs), ldx, N, p(G), ld, p(sigma), 1, p(W), ld, st))

        def score():
            _capi.check(lib.ttm_score(tm._pp, p(coef), p(fold), p(Xs), ldx, N, p(W), ld, p(inv_sigma), p(affine), st))

        def corr_fn():
            _capi.check(lib.ttm_langevin_corr(p(Zc), ld, p(Wc), ld, p(Zp), ld, p(Wp), ld, RHO, kappa, N, D, p(corr), st))

        def step_langevin():
            _capi.check(lib.ttm_mh_step_langevin(p(Zc), ld, p(Xc), ld, p(lc), p(lo), p(Zp), ld, p(Xp), ld, p(lp), p(Zn), ld, RHO, 1.0, None, ld, p(n_acc),
                                                 p(n_bad), N, D, 0, 0, 1, 2, 0, p(Wc), ld, p(Wp), ld, p(corr), kappa, st))

        def step_tempered():
            _capi.check(lib.ttm_mh_step_tempered(p(Zc), ld, p(Xc), ld, p(lc), p(lo), p(Zp), ld, p(Xp), ld, p(lp), p(Zn), ld, RHO, 1.0, None, ld, p(n_acc),
                                                 p(n_bad), N, D, 0, 0, 1, 2, 0, st))

        corr_fn()
        corr.mul_(0.05)                                  # (corrections of a few tenths: about half the rows still accept)
        versions = [('pull_gradient', None, pull), ('score_u', 0, score), ('score_band', None, score), ('langevin_corr', None, corr_fn),
                    ('mh_step_langevin', None, step_langevin), ('mh_step_tempered', None, step_tempered)]
        info = benchlib.warm_up(versions, pin, 3, kernel)
        corr_fn()
        corr.mul_(0.05)
        n_acc.zero_()
        step_langevin()
        a = float(n_acc.sum().item()) / N
        benchlib.keep_busy(pull, 50)
        # (the correction is rewritten by its own version in every round: the steps then decide on whatever it left, which moves
        # the accepted share, not the bytes a step loads - k_mh_step loads both rows of every matrix whatever is decided)
        benchlib.time_rounds(versions, info, pin, args.rounds, benchlib.per_round(args), settle=2)
        step_bytes = 24 + 8 * a + D * (32 * a + 8 * (1 - a) + 8)
        per_row = {'pull_gradient': 8 * (d + 2 * D), 'score_u': 8 * (d + D), 'score_band': 8 * (d + D), 'langevin_corr': 32 * D + 8,
                   'mh_step_langevin': step_bytes + 16 * a * D + 8 * D + 8, 'mh_step_tempered': step_bytes}
        for name, v in info.items():
            gb = per_row[name] * N / 1e9
            benchlib.summarise(v, gb, bench.COPY_PEAK_GBS)
            v['copy_peak_frac_on_algorithmic_bytes'] = v.pop('hbm_frac_on_algorithmic_bytes')
            v['algorithmic_gbytes'] = gb
        res['workloads'][wl] = {'N': N, 'ncols': D, 'rho': RHO, 'accepted_share': a, 'versions': info,
                                'pull_over_score_u_time': info['pull_gradient']['ms'] / info['score_u']['ms'],
                                'langevin_over_tempered_step_time': info['mh_step_langevin']['ms'] / info['mh_step_tempered']['ms']}
        benchlib.report(wl, info, 'accepted %.3f' % a)
        del tm, G, Zc, Xc, Zp, Xp, Wc, Wp, W, Zn

    # whole chains
    wall = WallClock(torch)
    rhos = [float(r) for r in args.rhos.split(',') if r]
    res['chains'] = {'chains': args.chains, 'steps': args.steps, 'rhos': rhos, 'cases': {}}
    for wl in [c for c in args.chain_workloads.split(',') if c]:
        tm, _, _ = bench.build_map(wl, 0, n_override=args.chains)
        kernel = benchlib.bind(tm._lib)
        mu, sd = tm._to_dev(np.asarray(tm.X_mean, dtype=float))[-tm.D:, None], tm._to_dev(np.asarray(tm.X_std, dtype=float))[-tm.D:, None]

        def target(raw, mu=mu, sd=sd):
            z = (raw - mu) / sd
            return -0.5 * (z * z).sum(dim=0)

        def grad(raw, mu=mu, sd=sd):
            return -(raw - mu) / (sd * sd)

        res['chains']['cases'][wl] = {}
        for rho in rhos:
            meta = {}

            def run(kind, rho=rho):
                def fn():
                    _, meta[kind] = tm.mcmc_device(target, args.chains, args.steps, rho=rho, seed=0, draw=0,
                                                   grad_log_target_pdf=grad if kind == 'langevin' else None)
                return fn
            calls = [('plain', None, run('plain')), ('langevin', None, run('langevin'))]
            cinfo = benchlib.warm_up(calls, None, 1, kernel, clock=wall)
            benchlib.time_rounds(calls, cinfo, None, args.calls, 1, settle=0, clock=wall)
            for kind, v in cinfo.items():
                benchlib.summarise(v)
                v['ms_per_step'] = v['ms'] / args.steps
                v['accept_rate'] = float(meta[kind]['n_acc'].sum().item()) / (args.chains * args.steps)
                # the jumps in z: the same chain continued step by step (untimed)
                g = grad if kind == 'langevin' else None
                _, state = tm.mcmc_device(target, args.chains, 1, rho=rho, seed=0, draw=0, grad_log_target_pdf=g)
                total = 0.0
                for _ in range(args.steps - 1):
                    before = state['Z'][:, :args.chains].clone()
                    _, state = tm.mcmc_device(target, args.chains, 1, rho=rho, init=state, grad_log_target_pdf=g)
                    total += float(((state['Z'][:, :args.chains] - before) ** 2).sum().item())
                v['msj'] = total / (args.chains * max(1, args.steps - 1))
            res['chains']['cases'][wl]['%g' % rho] = cinfo
            benchlib.report('%s chains rho %g (wall clock, ms per call of %d steps)' % (wl, rho, args.steps), cinfo,
                            'acceptance %.3f / %.3f, msj %.4f / %.4f' % (cinfo['plain']['accept_rate'], cinfo['langevin']['accept_rate'],
                                                                        cinfo['plain']['msj'], cinfo['langevin']['msj']))
        del tm
    benchlib.finish(res, args.out)


if __name__ == '__main__':
    main()
