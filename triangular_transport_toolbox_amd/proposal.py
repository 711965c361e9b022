"""The fitted map as a proposal: what sample(logdensity=True), sample_importance, the chains of mcmc_device
and the particles of smc_device share, and the Metropolis-Hastings move loop of the last two.  A new sampler starts from here;
the arithmetic on the rows is the library's and the map's (transport_map._inverse_logq)."""
import numpy as np

from . import _capi


class Proposal:
    """The map `tm` restricted to the components k0 .. D - 1 given the columns in front, for N rows.  Xs: the (d, ldp) device
    matrix the inverse writes into, the standardised conditioning columns in front - its own columns c0 .. d - 1 are scratch;
    coef, table: the packed coefficients and the configured table-or-search choice; g_scale: 1 / sigma of the own columns (None:
    standardised coordinates); const: the (D - k0)/2 log 2 pi that _inverse_logq leaves out."""

    def __init__(self, tm, N, k0, Xs=None, density=True):
        """Xs: a caller's contiguous (d, even width >= N) device matrix (mcmc_device has the contract); None: nothing in front.
        density False: no g_scale is uploaded - for a caller that only conditions, adapts a target or exports."""
        import torch
        d = tm._cm.d_cols
        if Xs is None:
            Xs = tm._cols(d, N, zero=True)
        if (not isinstance(Xs, torch.Tensor) or Xs.dim() != 2 or Xs.shape[0] != d or Xs.shape[1] < N or Xs.shape[1] & 1
                or Xs.dtype != torch.float64 or Xs.device.type != tm._dev.type or not Xs.is_contiguous()):
            raise ValueError('Xs must be a contiguous (%d, even width >= %d) matrix of doubles on the device' % (d, N))
        self.tm, self.N, self.k0, self.d, self.ncols = tm, N, k0, d, tm.D - k0
        self.c0 = d - self.ncols                         # (column of component k0)
        self.Xs, self.ldp = Xs, Xs.shape[1]              # (any such width: a sampler's state has its own leading dimension)
        self.coef = tm._pack_coeffs()
        self.table = tm._table_inverse
        self.const = 0.5 * self.ncols * np.log(2 * np.pi)
        if density:                                      # (here, before the caller queues work: the copy waits for the stream)
            self.g_scale = tm._inv_std(self.c0, d)

    @classmethod
    def from_star(cls, tm, N, X_star, one_point_only=False, density=True):
        """The conditioning shapes of sample(): those of inverse_map, or ONE point of shape (E,) / (1, E) spread over the N rows on
        the device.  one_point_only: a point per row is refused (resampling moves particles between rows)."""
        k0, E, cols = tm._conditioning(X_star)
        one_point = cols is not None and (cols.ndim == 1 or cols.shape[0] == 1)
        if one_point_only and cols is not None and not one_point:
            raise ValueError('X_star must be one conditioning point for all particles')
        return cls(tm, N, k0, tm._conditioned_cols(cols, E, N, one_point=one_point), density)

    def inverse_logq(self, Zs, logq):
        """Xs = S^-1(Zs) by the configured inverse, logq (N doubles on the device) = the log-density of those rows without const."""
        self.tm._inverse_logq(self.coef, self.k0, self.tm.D, Zs, self.Xs, self.N, self.table, logq, self.g_scale)

    def raw(self, first):
        """The raw coordinates of the columns first .. d - 1 of Xs, a (d - first, N) device tensor: what a target is given."""
        tm = self.tm
        x = self.Xs[first:self.d, :self.N]
        if tm.standardize_samples:                       # (what ttm_export computes: x * sd + mean, two roundings)
            x = x * tm._std_d[first:self.d, None] + tm._mean_d[first:self.d, None]
        return x

    def weigh(self, target, logq, first=None):
        """log p - log q of the rows in Xs, a contiguous device vector: the device-convention `target` at the raw columns
        first .. d - 1 (default: the own columns), logq as inverse_logq fills it."""
        import torch
        N = self.N
        logp = target(self.raw(self.c0 if first is None else first))
        if not isinstance(logp, torch.Tensor) or logp.numel() != N:
            raise ValueError('log_target_pdf must return a tensor of %d values' % N)
        return (logp.reshape(N).to(device=self.tm._dev, dtype=torch.float64) - (logq[:N] - self.const)).contiguous()

    def host_target(self, log_target_pdf):
        """A NumPy-convention target (N x ncols rows in, N values out) as a device-convention one."""
        N, to_dev = self.N, self.tm._to_dev

        def target(raw):
            logp = np.asarray(log_target_pdf(np.ascontiguousarray(raw.cpu().numpy().T)), dtype=float).reshape(-1)
            if logp.shape[0] != N:
                raise ValueError('log_target_pdf must return %d values' % N)
            return to_dev(logp)
        return target

    def host_gradient(self, grad_log_target_pdf):
        """A NumPy-convention gradient (N x ncols rows in, N x ncols out) as a device-convention one ((ncols, N) in and out)."""
        N, ncols, to_dev = self.N, self.ncols, self.tm._to_dev

        def grad(raw):
            g = np.asarray(grad_log_target_pdf(np.ascontiguousarray(raw.cpu().numpy().T)), dtype=float)
            if g.shape != (N, ncols):
                raise ValueError('grad_log_target_pdf must return a %d x %d array' % (N, ncols))
            return to_dev(np.ascontiguousarray(g.T))
        return grad

    @staticmethod
    def autograd_gradient(target):
        """The gradient of a device-convention target by torch.autograd.grad: one more evaluation of the target per call."""
        import torch

        def grad(raw):
            with torch.enable_grad():
                x = raw.detach().clone().requires_grad_(True)
                (g,) = torch.autograd.grad(target(x).sum(), x)
            return g
        return grad

    def pull(self, grad, W):
        """W (ncols, ld) = the gradient of the log of the pulled-back target density with respect to z at the rows in Xs: the
        device-convention `grad` at the raw own columns, then ttm_pull_gradient over [k0, D) in place, with sigma of the own
        columns as g_scale and the log-determinant term."""
        import torch
        tm, N = self.tm, self.N
        g = grad(self.raw(self.c0))
        if not isinstance(g, torch.Tensor) or tuple(g.shape) != (self.ncols, N):
            raise ValueError('grad_log_target_pdf must return a (%d, %d) tensor' % (self.ncols, N))
        W[:, :N].copy_(g)
        sigma = tm._ptr(tm._std_d, self.c0) if tm.standardize_samples else None
        _capi.check(tm._lib.ttm_pull_gradient(tm._pp, tm._ptr(self.coef), tm._ptr(self.coef._ttm_fold), self.k0, tm.D, tm._ptr(self.Xs), self.ldp, N,
                                              tm._ptr(W), W.shape[1], sigma, 1, tm._ptr(W), W.shape[1], tm._stream()))

    def export_own(self, cols, out):
        """The standardised own columns `cols` (column-major, (ncols, ld)) as raw rows into `out` (N x ncols, row-major): ttm_export."""
        tm = self.tm
        mean = tm._ptr(tm._mean_d, self.c0) if tm.standardize_samples else None
        sd = tm._ptr(tm._std_d, self.c0) if tm.standardize_samples else None
        _capi.check(tm._lib.ttm_export(tm._ptr(cols), cols.shape[1], self.N, 0, self.ncols, mean, sd, tm._ptr(out), tm._stream()))

    def moves(self, target, n, Zcur, Xcur, lw, Zp, n_acc, n_bad, logq, rho, beta, seed64, draw, row0=0, record=None, grad=None, Wcur=None, Wp=None,
              corr=None):
        """n Metropolis-Hastings moves of the state (Zcur, Xcur: (ncols, ld), updated in place) at the exponent beta (1.0: the plain
        step): n + 1 launches of ttm_mh_step_tempered - the first proposes, each later one decides move t and proposes move t + 1,
        the last decides - and between two of them the inverse with its log-density and the target.  lw: two vectors of N doubles,
        lw[0] the current log-weights, written by turns; Zp: two (ncols, ld) matrices for the proposals; logq: N doubles of
        scratch.  Move t takes draw + t for its innovations and accept uniforms.  record(t): the (ncols, ld) matrix that receives
        the own columns after move t, or None.  Returns the vector of lw that holds the log-weights afterwards; n = 0: nothing.
        grad (a device-convention gradient of the target): Langevin moves, ttm_mh_step_langevin with kappa = (1 - rho) beta -
        Wcur: the state's pulled gradient ((ncols, ld), updated in place), Wp: a matrix for the proposal's, corr: N doubles of
        scratch; between two launches the inverse with its log-density, the target, the pull (pull) and ttm_langevin_corr.
        Without grad: the calls above and nothing else."""
        tm, N, k0, ncols, ld = self.tm, self.N, self.k0, self.ncols, Zcur.shape[1]
        ptr, step, st = tm._ptr, tm._lib.ttm_mh_step_tempered, tm._stream()
        xprop = ptr(self.Xs, self.c0 * self.ldp)         # (where the inverse leaves the proposal's own columns)
        kappa = (1.0 - rho) * beta
        drift = () if grad is None else (ptr(Wcur), ld, ptr(Wp), ld)
        if grad is not None:
            step = tm._lib.ttm_mh_step_langevin
        lw, lwp = list(lw), None
        for t in range(n + 1 if n else 0):
            accept, propose = t >= 1, t < n
            rec = record(t) if record is not None else None
            zn = Zp[t & 1] if propose else None
            _capi.check(step(ptr(Zcur), ld, ptr(Xcur), ld, ptr(lw[0]), ptr(lw[1]) if accept else None,
                             ptr(Zp[(t - 1) & 1]) if accept else None, ld, xprop if accept else None, self.ldp,
                             ptr(lwp) if accept else None, ptr(zn), ld, rho, beta, ptr(rec), ld, ptr(n_acc), ptr(n_bad), N, ncols, k0,
                             seed64, draw + t if accept else 0, draw + t + 1 if propose else 0, row0,
                             *(drift + ((ptr(corr) if accept else None, kappa) if drift else ()) + (st,))))
            if accept:
                lw.reverse()
            if propose:
                self.inverse_logq(zn, logq)
                lwp = self.weigh(target, logq)
                if grad is not None:
                    self.pull(grad, Wp)
                    _capi.check(tm._lib.ttm_langevin_corr(ptr(Zcur), ld, ptr(Wcur), ld, ptr(zn), ld, ptr(Wp), ld, rho, kappa, N, ncols, ptr(corr), st))
        return lw[0]
