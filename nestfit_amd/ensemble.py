"""Ensemble MCMC at a fixed component count: the affine-invariant stretch move of Goodman & Weare (2010) in
the unit cube, where the prior is flat by construction, around the engine's likelihood batch -- posteriors with real error
bars under every prior kind, model and likelihood option, without an evidence.

`run_twin` is the numpy twin of the device sampler (csrc/nfa_ensemble.h, contract: csrc/nfa_ensemble_plan.h): one state
record (`EnsState`, fields named like `EnsDev`'s) and one function per stage of the device -- `_create` (nfa_ensemble_create),
`_propose` (ens_propose_kernel), `_accept` (the likelihood batch and ens_accept_kernel), `_trace` (ens_trace_kernel), `_keep`
(ens_keep_kernel) -- with the same arithmetic and the same random numbers (`nested._uniform`), so the same arguments give
the same run.  `summarize` is the twin of ens_summary_kernel, `pdf_counts` of ens_hist_kernel (equal to the bit) and
`covariance_of` of ens_cov_kernel (the same formula summed in another order).  `sample_pixels` and `sample_cube` drive the
device; the products of a chain -- marginal histograms, parameter covariances, moments of the model spectra --
are reduced there, so the chain need not leave it."""
import ctypes as C
import math
import types

import numpy as np

from . import _ffi
from .nested import LOG_ZERO, _U64, _uniform

# csrc/nfa_ensemble_plan.h (tests/test_ensemble_cpu.py compares them with the header's)
ENS_TAG = 1 << 61
MAX_WALKERS, MAX_Q, MAX_SORT, A_MAX = 512, 8, 8192, 16.0
MAX_BINS = 1024


class EnsState(types.SimpleNamespace):
    """What a run of the twin holds, under `EnsDev`'s names: P, W, D, DT, fmap, pix; the walkers u[P, W, D], theta[P, W, DT],
    lnL[P, W]; a half-step's rows, row_lnL, y, inside; counts[P, 3] (accepted, outside, evaluated).  Beside them what only
    the host has: loglike, chunk, margin."""


class TwinResult(types.SimpleNamespace):
    """`run_twin`'s outputs: u[P, W, ndim] (0.5 where not sampled), theta, lnL: the walkers as they stand; chain_theta[P,
    n_keep, W, ndim], chain_lnL[P, n_keep, W]; trace[P, n_steps, D + 1]; accepted, outside, evaluated [P]; margin; `state`,
    to continue from."""


def check_arguments(n_walkers, n_sampled, n_steps, n_burn, thin, a):
    """ens_check_walkers and ens_check_run of the plan header, for the twin: the device says the same in its own words."""
    if not 2 <= n_walkers <= MAX_WALKERS or n_walkers % 2:
        raise ValueError('n_walkers must be even and in 2 .. 512')
    if n_walkers // 2 < n_sampled + 1:
        raise ValueError('half the walkers must number the sampled dimensions + 1 at least')
    if not 1.0 < a <= A_MAX:
        raise ValueError('the stretch scale a must lie in (1, 16]')
    if thin < 1 or n_steps < 1 or not 0 <= n_burn < n_steps or (n_steps - n_burn) // thin < 1:
        raise ValueError('thin >= 1, 0 <= n_burn < n_steps and (n_steps - n_burn) / thin >= 1 are required')


def n_keep_of(n_steps, n_burn, thin):
    return (n_steps - n_burn) // thin


def keeps(step, n_burn, thin):
    """Whether the state after step `step` (from 1) is kept."""
    return step > n_burn and (step - n_burn) % thin == 0


def _evaluate(S, pix, T):
    """Raw lnL of rows T of cube pixels pix, `chunk` rows a call.  T comes back as theta."""
    out = np.empty(T.shape[0])
    for b in range(0, T.shape[0], S.chunk):
        out[b:b + S.chunk] = S.loglike(pix[b:b + S.chunk], T[b:b + S.chunk])
    return out


def _expand(S, u):
    T = np.full(u.shape[:-1] + (S.DT,), 0.5)
    T[..., S.fmap] = u
    return T


def _create(loglike, ndim, pix, n_walkers, u0, free_mask, chunk):
    """nfa_ensemble_create: the start rows evaluated once."""
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    P, W = pix.size, int(n_walkers)
    fmap = np.arange(ndim) if free_mask is None else np.flatnonzero(np.asarray(free_mask))
    u0 = np.asarray(u0, dtype=np.float64).reshape(P, W, ndim)
    S = EnsState(P=P, W=W, D=int(fmap.size), DT=int(ndim), fmap=fmap, pix=pix, loglike=loglike, chunk=chunk, margin=np.inf)
    S.u = u0[:, :, fmap].copy()
    if not ((S.u > 0.0) & (S.u < 1.0)).all():
        raise ValueError('u0 must lie inside (0, 1) at every sampled slot')
    T = _expand(S, S.u).reshape(P * W, ndim)
    S.lnL = _evaluate(S, np.repeat(pix, W), T).reshape(P, W)
    S.theta = T.reshape(P, W, ndim)
    S.counts = np.zeros((P, 3), dtype=np.int64)
    return S


def _uniforms(S, seed, step, h, k):
    """r_0, r_1, r_2 [P, W/2] of the walkers k in half-step h of step `step`."""
    tag = _U64(ENS_TAG + 2 * step + h)
    p = S.pix.astype(_U64)[:, None]
    return [_uniform(seed, p, tag, (3 * k + i).astype(_U64)[None, :]) for i in range(3)]


def _stretch(a, r1):
    t = (a - 1.0) * r1 + 1.0
    return t * t / a


def _propose(S, seed, step, h, a):
    """ens_propose_kernel: y, inside and the batch rows of the moving half."""
    half = S.W // 2
    k = h * half + np.arange(half)
    r0, r1, _ = _uniforms(S, seed, step, h, k)
    j = (1 - h) * half + np.minimum(np.floor(r0 * half).astype(np.int64), half - 1)
    z = _stretch(a, r1)
    uk = S.u[:, k, :]
    uj = np.take_along_axis(S.u, j[:, :, None], axis=1)
    S.y = uj + z[:, :, None] * (uk - uj)
    S.inside = ((S.y > 0.0) & (S.y < 1.0)).all(axis=2)
    S.rows = _expand(S, np.where(S.inside[:, :, None], S.y, uk))


def _accept(S, seed, step, h, a):
    """The likelihood of the rows, then ens_accept_kernel."""
    half = S.W // 2
    k = h * half + np.arange(half)
    _, r1, r2 = _uniforms(S, seed, step, h, k)
    z = _stretch(a, r1)
    T = S.rows.reshape(S.P * half, S.DT)
    Ly = _evaluate(S, np.repeat(S.pix, half), T).reshape(S.P, half)
    T = T.reshape(S.P, half, S.DT)
    Lk = S.lnL[:, k]
    live = S.inside & np.isfinite(Ly)
    with np.errstate(invalid='ignore', over='ignore'):
        rhs = float(S.D - 1) * np.log(z) + (Ly - Lk)
        lr = np.log(r2)
        acc = live & (lr < rhs)
        if live.any():
            S.margin = min(S.margin, float(np.abs(lr - rhs)[live].min()))
    pp, mm = np.nonzero(acc)
    S.u[pp, k[mm]] = S.y[pp, mm]
    S.theta[pp, k[mm]] = T[pp, mm]
    S.lnL[pp, k[mm]] = Ly[pp, mm]
    S.counts[:, 0] += acc.sum(axis=1)
    S.counts[:, 1] += (~S.inside).sum(axis=1)
    S.counts[:, 2] += half


def _wave_mean(x):
    """The mean over the last axis (W <= 512 walkers) as one wave forms it: lane l adds walkers l, l + 64, ... in order, then a
    butterfly over the lanes at distances 32, 16, .. 1."""
    W = x.shape[-1]
    v = np.zeros(x.shape[:-1] + (64,))
    for b in range(0, W, 64):
        n = min(64, W - b)
        v[..., :n] = v[..., :n] + x[..., b:b + n]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0] / float(W)


def _trace(S):
    """ens_trace_kernel: [P, D + 1], the walkers' mean of every sampled u and of lnL."""
    return np.concatenate([_wave_mean(np.moveaxis(S.u, 1, 2)), _wave_mean(S.lnL)[:, None]], axis=1)


def run_twin(loglike, ndim, n_pix, n_walkers, u0, n_steps, n_burn=0, thin=1, a=2.0, seed=1, free_mask=None, log_zero=LOG_ZERO,
             pix=None, state=None, chunk=1 << 18):
    """The device's run on the host: `loglike(pix, T)` returns lnL of the unit-cube rows T[B, ndim] of cube pixels pix[B]
    and leaves theta in T.  pix: the cube pixel of each of the n_pix pixels (None: 0 .. n_pix - 1); it is in the random
    stream.  state: a `TwinResult.state` to continue from (u0 is then not read); the steps count from 1 again, so a
    continuation takes another seed.  Returns a `TwinResult`."""
    pix = np.arange(n_pix, dtype=np.int32) if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
    assert pix.shape == (n_pix,)
    seed = _U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    n_sampled = state.D if state is not None else ndim if free_mask is None else int(np.count_nonzero(free_mask))
    check_arguments(int(n_walkers), n_sampled, n_steps, n_burn, thin, a)
    S = _create(loglike, ndim, pix, n_walkers, u0, free_mask, chunk) if state is None else state
    n_keep = n_keep_of(n_steps, n_burn, thin)
    S.counts[:] = 0
    S.margin = np.inf
    S.lnL = np.where(np.isfinite(S.lnL), S.lnL, log_zero)
    chain_theta, chain_lnL = np.empty((S.P, n_keep, S.W, S.DT)), np.empty((S.P, n_keep, S.W))
    trace = np.empty((S.P, n_steps, S.D + 1))
    for step in range(1, n_steps + 1):
        for h in (0, 1):
            _propose(S, seed, step, h, a)
            _accept(S, seed, step, h, a)
        trace[:, step - 1] = _trace(S)
        if keeps(step, n_burn, thin):                           # ens_keep_kernel
            slot = (step - n_burn) // thin - 1
            chain_theta[:, slot], chain_lnL[:, slot] = S.theta, S.lnL
    return TwinResult(u=_expand(S, S.u), theta=S.theta.copy(), lnL=S.lnL.copy(), chain_theta=chain_theta, chain_lnL=chain_lnL,
                      trace=trace, accepted=S.counts[:, 0].copy(), outside=S.counts[:, 1].copy(), evaluated=S.counts[:, 2].copy(),
                      margin=S.margin, state=S)


# ---- the summary's twin and the autocorrelation time ----------------------------------------------------------------
def quantile(sorted_samples, q):
    """The device's quantile of an ascending array along its last axis: s[i] + (s[i + 1] - s[i]) g with h = (N - 1) q,
    i = floor(h), g = h - i."""
    s = np.asarray(sorted_samples, dtype=np.float64)
    N = s.shape[-1]
    h = float(N - 1) * float(q)
    i = int(h)
    g = h - float(i)
    i1 = min(i + 1, N - 1)
    return s[..., i] + (s[..., i1] - s[..., i]) * g


def summarize(chain_theta, chain_lnL, levels=()):
    """ens_summary_kernel in numpy, on chain_theta[P, n_keep, W, ndim] and chain_lnL[P, n_keep, W]: (mean, std, best, best_lnL,
    quantiles) = [P, ndim], [P, ndim], [P, ndim], [P], [P, ndim, len(levels)].  best and the quantiles are the device's to the
    bit; the moments are the same expressions summed in another order."""
    P, n_keep, W, ndim = chain_theta.shape
    X, L = chain_theta.reshape(P, n_keep * W, ndim), chain_lnL.reshape(P, n_keep * W)
    row = np.argmax(L, axis=1)                                  # the first of the largest
    best = X[np.arange(P), row]
    d = X - best[:, None, :]
    m = d.mean(axis=1)
    var = (d * d).mean(axis=1) - m * m
    srt = np.sort(X, axis=1)
    quant = np.stack([quantile(np.moveaxis(srt, 1, 2), q) for q in levels], axis=2) if len(levels) else np.empty((P, ndim, 0))
    return best + m, np.sqrt(np.maximum(var, 0.0)), best, L[np.arange(P), row], quant


def pdf_counts(chain_theta, edges):
    """ens_hist_kernel in numpy, on chain_theta[P, n_keep, W, ndim] and edges[ndim, n_bins + 1]: (counts int64[P, ndim, n_bins],
    outside int64[P, ndim]) -- `np.histogram(x, bins=edges[c])[0]` of every (pixel, column), and the samples it left out (a NaN,
    an x beyond the edges)."""
    P, n_keep, W, ndim = chain_theta.shape
    edges = np.asarray(edges, dtype=np.float64)
    if edges.ndim != 2 or edges.shape[0] != ndim or edges.shape[1] < 2:
        raise ValueError('edges must be [ndim, n_bins + 1]')
    X = chain_theta.reshape(P, n_keep * W, ndim)
    counts = np.empty((P, ndim, edges.shape[1] - 1), dtype=np.int64)
    for p in range(P):
        for c in range(ndim):
            counts[p, c] = np.histogram(X[p, :, c], bins=edges[c])[0]
    return counts, n_keep * W - counts.sum(axis=2)


def covariance_of(chain_theta, chain_lnL, dtype=np.float64):
    """ens_cov_kernel's formula in numpy, computed in `dtype`: cov[P, ndim, ndim] of chain_theta[P, n_keep, W, ndim] about every
    pixel's best row (the first of largest chain_lnL[P, n_keep, W]): with d the differences from that row, S_ab / N - (S_a / N)
    (S_b / N), the diagonal not below 0 -- a population covariance of differences, for the reason DESIGN 4.21 gives."""
    P, n_keep, W, ndim = chain_theta.shape
    N = n_keep * W
    X, L = chain_theta.reshape(P, N, ndim).astype(dtype), chain_lnL.reshape(P, N)
    row = np.argmax(np.where(np.isnan(L), -np.inf, L), axis=1)
    d = X - X[np.arange(P), row][:, None, :]
    m = d.sum(axis=1) / dtype(N)
    cov = np.einsum('pia,pib->pab', d, d) / dtype(N) - m[:, :, None] * m[:, None, :]
    k = np.arange(ndim)
    cov[:, k, k] = np.maximum(cov[:, k, k], 0)
    return cov


def bin_edges(utrans, ncomp, n_bins):
    """edges[ndim, n_bins + 1] for `histogram`: per column of a theta row (the chain's layout, `lsq.prior_box`'s)
    `np.linspace(lower, upper, n_bins + 1)` over the box of the priors.  A column whose box is a point (a constant parameter)
    gets the box of width 1 around it: edges have to increase."""
    from .lsq import prior_box
    lower, upper = prior_box(utrans, ncomp)
    point = ~(upper > lower)
    lower, upper = np.where(point, lower - 0.5, lower), np.where(point, upper + 0.5, upper)
    return np.ascontiguousarray(np.linspace(lower, upper, int(n_bins) + 1, axis=1))


def autocorr_time(x, c=5.0):
    """Integrated autocorrelation time of the series x[n] (in its steps) by Sokal's windowed estimator: tau(M) = 1 + 2
    sum_{t=1..M} rho_t at the smallest M with M >= c tau(M); NaN for a constant series."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    x = x - x.mean()
    if n < 2 or not np.any(x):
        return np.nan
    size = 1 << (2 * n - 1).bit_length()
    f = np.fft.rfft(x, size)
    acf = np.fft.irfft(f * np.conjugate(f), size)[:n]
    rho = acf / acf[0]
    taus = 2.0 * np.cumsum(rho) - 1.0
    ok = np.arange(n) >= c * taus
    M = int(np.argmax(ok)) if ok.any() else n - 1
    return float(taus[M])


# ---- the device ------------------------------------------------------------------------------------------------------
class _Handle:
    """An nfa_ensemble and the runner it uses."""

    def __init__(self, runner, pix, n_walkers, free_mask, u0):
        lib = _ffi.engine()
        self.runner = runner                                     # (the runner outlives its ensemble)
        h = C.c_void_p()
        _ffi.check(lib.nfa_ensemble_create(C.byref(h), runner._run.handle, None if pix is None else pix.ctypes.data_as(_ffi._ip),
                                           u0.shape[0], int(n_walkers), None if free_mask is None else free_mask.ctypes.data_as(_ffi._ip),
                                           _ffi.dptr(u0)))
        self.handle = h

    def close(self):
        if getattr(self, 'handle', None) is not None:
            _ffi.load().nfa_ensemble_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceEnsemble:
    """The C calls of an ensemble on arrays: `run`, `counts`, `state`, `trace`, `chain`, `summary`, and the products of the
    chain `histogram`, `covariance`, `moments`.  pix: int32[P] cube pixels, or None for the pixel of a one-pixel runner (then
    P = 1); u0[P, W, ndim]."""

    def __init__(self, runner, pix, n_walkers, u0, free_mask=None):
        self.ndim, self.W = int(runner.ndim), int(n_walkers)
        self.pix = None if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
        self.P = 1 if pix is None else int(self.pix.size)
        fm = None if free_mask is None else np.ascontiguousarray(free_mask, dtype=np.int32)
        if fm is not None and fm.shape != (self.ndim,):
            raise ValueError('free_mask must hold one flag per unit-cube slot')
        self.D = self.ndim if fm is None else int(np.count_nonzero(fm))
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        if u0.shape != (self.P, self.W, self.ndim):
            raise ValueError('the start must be [n_pix, n_walkers, ndim]')
        self.n_spec, self.n_chan_tot = int(runner.n_spec), int(runner._ss.chan_tot)
        self._h = _Handle(runner, self.pix, n_walkers, fm, u0)
        self.n_steps = self.n_keep = 0

    def close(self):
        self._h.close()

    def run(self, n_steps, n_burn=0, thin=1, a=2.0, seed=1, log_zero=LOG_ZERO):
        _ffi.check(_ffi.load().nfa_ensemble_run(self._h.handle, int(n_steps), int(n_burn), int(thin), float(a),
                                                C.c_int64(int(seed) & 0xFFFFFFFFFFFFFFFF).value, float(log_zero)))
        self.n_steps, self.n_keep = int(n_steps), n_keep_of(int(n_steps), int(n_burn), int(thin))

    def counts(self):
        out = [np.empty(self.P, dtype=np.int64) for _ in range(3)]
        _ffi.check(_ffi.load().nfa_ensemble_counts(self._h.handle, *[o.ctypes.data_as(_ffi._lp) for o in out]))
        return tuple(out)

    def state(self):
        u, theta, lnL = np.empty((self.P, self.W, self.ndim)), np.empty((self.P, self.W, self.ndim)), np.empty((self.P, self.W))
        _ffi.check(_ffi.load().nfa_ensemble_state(self._h.handle, _ffi.dptr(u), _ffi.dptr(theta), _ffi.dptr(lnL)))
        return u, theta, lnL

    def trace(self):
        out = np.empty((self.P, self.n_steps, self.D + 1))
        _ffi.check(_ffi.load().nfa_ensemble_trace(self._h.handle, _ffi.dptr(out)))
        return out

    def chain(self):
        theta, lnL = np.empty((self.P, self.n_keep, self.W, self.ndim)), np.empty((self.P, self.n_keep, self.W))
        _ffi.check(_ffi.load().nfa_ensemble_chain(self._h.handle, _ffi.dptr(theta), _ffi.dptr(lnL)))
        return theta, lnL

    def summary(self, levels=()):
        """(mean, std, best, best_lnL, quantiles) as `summarize` returns them, reduced on the device."""
        levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        nq = int(levels.size)
        summ, best = np.empty((self.P, self.ndim, 2)), np.empty((self.P, self.ndim + 1))
        quant = np.empty((self.P, self.ndim, nq))
        _ffi.check(_ffi.load().nfa_ensemble_summary(self._h.handle, _ffi.dptr(levels) if nq else None, nq, _ffi.dptr(summ),
                                                    _ffi.dptr(best), _ffi.dptr(quant) if nq else None))
        return summ[:, :, 0].copy(), summ[:, :, 1].copy(), best[:, :self.ndim].copy(), best[:, self.ndim].copy(), quant

    def histogram(self, edges):
        """(counts int64[P, ndim, n_bins], outside int64[P, ndim]) of the chain on edges[ndim, n_bins + 1], as `pdf_counts`
        returns them, counted on the device."""
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        if edges.ndim != 2 or edges.shape[0] != self.ndim:
            raise ValueError('edges must be [ndim, n_bins + 1]')
        n_bins = edges.shape[1] - 1
        counts, outside = np.empty((self.P, self.ndim, max(n_bins, 0)), dtype=np.int64), np.empty((self.P, self.ndim), dtype=np.int64)
        _ffi.check(_ffi.load().nfa_ensemble_histogram(self._h.handle, _ffi.dptr(edges), n_bins, counts.ctypes.data_as(_ffi._lp),
                                                      outside.ctypes.data_as(_ffi._lp)))
        return counts, outside

    def covariance(self):
        """cov[P, ndim, ndim] of the chain about every pixel's best row, as `covariance_of` defines it, summed on the device."""
        cov = np.empty((self.P, self.ndim, self.ndim))
        _ffi.check(_ffi.load().nfa_ensemble_covariance(self._h.handle, _ffi.dptr(cov)))
        return cov

    def moments(self, chunk_rows=None, want_spectra=True):
        """The `PosteriorMoments` of the runner's `predict_moments` over every pixel's kept samples with equal weights, one
        segment per pixel, bit for bit -- from the chain where it lies."""
        from .moments import PosteriorMoments
        mean = np.empty((self.P, self.n_chan_tot)) if want_spectra else None
        std = np.empty((self.P, self.n_chan_tot)) if want_spectra else None
        smean, sstd = np.empty((self.P, self.n_spec, 2)), np.empty((self.P, self.n_spec, 2))
        opt = lambda a: None if a is None else _ffi.dptr(a)
        _ffi.check(_ffi.load().nfa_ensemble_moments(self._h.handle, 0 if chunk_rows is None else int(chunk_rows), opt(mean), opt(std),
                                                    _ffi.dptr(smean), _ffi.dptr(sstd)))
        return PosteriorMoments(mean, std, smean[:, :, 0].copy(), sstd[:, :, 0].copy(), smean[:, :, 1].copy(), sstd[:, :, 1].copy())


class EnsembleResult(types.SimpleNamespace):
    """`sample_pixels`' outputs, one row per pixel: mean, std, best [P, ndim], best_lnL [P], quantiles [P, ndim, len(levels)],
    levels; acceptance (accepted / proposed), outside (the share of proposals outside the unit cube), n_evals [P]; tau, n_eff
    [P, D] per sampled dimension; trace [P, n_steps, D + 1]; with `keep_chain` theta [P, n_keep, W, ndim] and lnL [P, n_keep,
    W].  The products asked for, None otherwise: pdf_counts int64[P, ndim, n_bins], pdf_outside int64[P, ndim], pdf_bins [ndim,
    n_bins] (the bins' centres), cov [P, ndim, ndim], model (a `PosteriorMoments` of one row per pixel)."""

    def chain(self):
        """(theta, lnL) of the kept samples: the fetched copy, or fetched now from the device."""
        if getattr(self, 'theta', None) is not None:
            return self.theta, self.lnL
        if self._ensemble is None:
            raise ValueError('the chain was not kept and the ensemble is closed')
        return self._ensemble.chain()

    def moments(self, runner, chunk_rows=None, want_spectra=True):
        """`predict_moments` over every pixel's kept samples with equal weights: a `PosteriorMoments` record, one segment per
        pixel.  While the ensemble is open the chain is reduced where it lies (`DeviceEnsemble.moments`); with only a fetched
        chain left its rows go through the host.  The same bits either way."""
        from . import _calls
        if self._ensemble is not None:
            return self._ensemble.moments(chunk_rows, want_spectra)
        theta, _ = self.chain()
        P, n_keep, W, ndim = theta.shape
        rows = theta.reshape(P * n_keep * W, ndim)
        offsets = np.arange(P + 1, dtype=np.int64) * (n_keep * W)
        return _calls._predict_moments(runner._run.handle, self.pix, offsets, _calls.parameter_rows(runner, rows), None, chunk_rows,
                                       want_spectra, int(runner._ss.chan_tot), int(runner.n_spec))

    def close(self):
        """Frees the ensemble on the device (the chain with it)."""
        if self._ensemble is not None:
            self._ensemble.close()
            self._ensemble = None


def starts(runner, pix, n_walkers, n_init=2048, seed=0):
    """u0[P, n_walkers, ndim]: per pixel the `n_walkers` prior draws of highest lnL among `n_init`, ties by draw index, as
    unit-cube rows (`lsq.best_draws`, the scoring `lsq.fit_cube` starts from)."""
    from .lsq import best_draws
    return best_draws(runner, pix, int(n_init), int(n_walkers), np.random.default_rng(seed), unit=True)


def default_thin(n_steps, n_walkers):
    return max(1, math.ceil(n_steps / 2 / (MAX_SORT // n_walkers)))


def sample_pixels(runner, pix, n_walkers=64, n_steps=2000, n_burn=None, thin=None, a=2.0, seed=1, start=None, free_mask=None,
                  levels=(0.16, 0.5, 0.84), keep_chain=False, log_zero=LOG_ZERO, n_init=2048, par_bins=None, covariance=False,
                  moments=False, utrans=None):
    """The posterior of the cube pixels `pix` of a `CubeRunner` (None: the pixel of a one-pixel runner) by `n_steps` steps of
    `n_walkers` walkers each on the device: an `EnsembleResult`.  n_burn None: half the steps; thin None: so that the kept
    samples of a pixel number 8192 at most, what the quantiles sort.  start: u0[P, n_walkers, ndim] in (0, 1), None:
    `starts(runner, pix, n_walkers, n_init, seed)`.  free_mask: the sampled unit-cube slots (None: all; `utrans.free_mask(ncomp)`
    leaves out the slots of constant and duplicated parameters).  par_bins: edges[ndim, n_bins + 1] of the marginal histograms
    (an int with `utrans=`: `bin_edges(utrans, runner.ncomp, par_bins)`); covariance, moments: the parameter covariances and
    the moments of the model spectra.  The three are reduced on the device before the result is handed back, so they outlive
    `close()`.  The argument checks are the engine's (`EngineError`)."""
    n_steps = int(n_steps)
    if par_bins is not None and np.ndim(par_bins) == 0:
        if utrans is None:
            raise ValueError('a number of bins needs utrans= for the edges')
        par_bins = bin_edges(utrans, runner.ncomp, int(par_bins))
    n_burn = n_steps // 2 if n_burn is None else int(n_burn)
    thin = default_thin(n_steps, int(n_walkers)) if thin is None else int(thin)
    pix = None if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
    u0 = starts(runner, pix, n_walkers, n_init, seed) if start is None else start
    ens = DeviceEnsemble(runner, pix, n_walkers, u0, free_mask)
    try:
        ens.run(n_steps, n_burn, thin, a, seed, log_zero)
        accepted, outside, evaluated = ens.counts()
        trace = ens.trace()
        mean, std, best, best_lnL, quant = ens.summary(levels)
        theta, lnL = ens.chain() if keep_chain else (None, None)
        pdf, pdf_out, pdf_bins = None, None, None
        if par_bins is not None:
            edges = np.ascontiguousarray(par_bins, dtype=np.float64)
            pdf, pdf_out = ens.histogram(edges)
            pdf_bins = 0.5 * (edges[:, :-1] + edges[:, 1:])
        cov = ens.covariance() if covariance else None
        model = ens.moments() if moments else None
    except Exception:
        ens.close()
        raise
    proposed = float(n_steps * int(n_walkers))
    tau = np.array([[autocorr_time(trace[p, n_burn:, d]) for d in range(ens.D)] for p in range(ens.P)])
    with np.errstate(divide='ignore', invalid='ignore'):
        n_eff = int(n_walkers) * (n_steps - n_burn) / tau
    return EnsembleResult(mean=mean, std=std, best=best, best_lnL=best_lnL, quantiles=quant, levels=tuple(levels),
                          acceptance=accepted / proposed, outside=outside / proposed, n_evals=evaluated, tau=tau, n_eff=n_eff,
                          trace=trace, theta=theta, lnL=lnL, pix=pix, n_steps=n_steps, n_burn=n_burn, thin=thin, pdf_counts=pdf,
                          pdf_outside=pdf_out, pdf_bins=pdf_bins, cov=cov, model=model, _ensemble=ens)


MAP_FIELDS = ('mean', 'std', 'best', 'best_lnL', 'quantiles', 'acceptance', 'outside', 'n_evals', 'tau', 'n_eff')


def pixel_groups(n_pix, bytes_per_pixel, memory_budget):
    """The cut of n_pix pixels into consecutive groups whose ensembles fit `memory_budget` bytes: [(first, end), ...]."""
    per = max(1, int(memory_budget) // max(1, int(bytes_per_pixel)))
    return [(a, min(n_pix, a + per)) for a in range(0, n_pix, per)]


def sample_cube(stack, utrans, runner_cls, ncomp, runner_kwargs=None, memory_budget=2 << 30, par_bins=None, covariance=False,
                moments=False, **kw):
    """`sample_pixels` over every good pixel of a `CubeStack` with `ncomp` components: a namespace of maps (lat, lon) of
    every field of the result -- mean, std, best [ndim, lat, lon], best_lnL, acceptance, outside, n_evals [lat, lon],
    quantiles [ndim, n_levels, lat, lon], tau, n_eff [D, lat, lon] -- NaN where a pixel is not good (n_evals: -1).  The runner
    With par_bins (edges[ndim, n_bins + 1], or an int: `bin_edges(utrans, ncomp, par_bins)`) pdf_counts [ndim, n_bins, lat, lon]
    and pdf_outside [ndim, lat, lon] (int64, -1 where a pixel is not good) and pdf_bins [ndim, n_bins]; with covariance cov [ndim,
    ndim, lat, lon]; with moments spec_mean, spec_std [chan_tot, lat, lon] and peak_mean, peak_std, total_mean, total_std
    [n_spec, lat, lon].  The runner is built as `CubeFitter` builds it; the pixels go in groups whose device bytes
    (nfa_ensemble_bytes: state, chain and trace; with moments nfa_ensemble_moments_bytes too) fit `memory_budget`.  A pixel's run does not depend on its group: the cube pixel is in the random stream, and
    the starts are drawn for all pixels before the cut.  kw: `sample_pixels`' keywords."""
    from .fitter import CubeFitter
    fitter = CubeFitter(stack, utrans, runner_cls, runner_kwargs=runner_kwargs)
    kwargs = fitter.runner_kwargs if fitter.species is None else dict(fitter.runner_kwargs, species=fitter.species, fill=fitter.fill)
    runner, lon, lat = stack.to_device(utrans, ncomp=ncomp, model=fitter.model_id, **kwargs)
    n_pix, ndim = runner.n_pix, runner.ndim
    W, n_steps = int(kw.get('n_walkers', 64)), int(kw.get('n_steps', 2000))
    n_burn = n_steps // 2 if kw.get('n_burn') is None else int(kw['n_burn'])
    thin = default_thin(n_steps, W) if kw.get('thin') is None else int(kw['thin'])
    fm = kw.get('free_mask')
    D = ndim if fm is None else int(np.count_nonzero(fm))
    all_pix = np.arange(n_pix, dtype=np.int32)
    start = kw.pop('start', None)
    if start is None:
        start = starts(runner, all_pix, W, kw.get('n_init', 2048), kw.get('seed', 1))
    per_pixel = _ffi.load().nfa_ensemble_bytes(1, W, ndim, D, n_steps, max(0, n_keep_of(n_steps, n_burn, thin)))
    if moments:
        per_pixel += _ffi.load().nfa_ensemble_moments_bytes(1, runner.n_chan_tot, runner.n_spec)
    if par_bins is not None and np.ndim(par_bins) == 0:
        par_bins = bin_edges(utrans, ncomp, int(par_bins))
    groups = pixel_groups(n_pix, per_pixel, memory_budget)
    parts = []
    for first, end in groups:
        res = sample_pixels(runner, all_pix[first:end], start=start[first:end], par_bins=par_bins, covariance=covariance,
                            moments=moments, **kw)
        res.close()
        parts.append(res)
    n_lon, n_lat = stack.spatial_shape
    maps = types.SimpleNamespace(n_groups=len(groups), levels=parts[0].levels if parts else ())
    for name in MAP_FIELDS:
        val = np.concatenate([getattr(part, name) for part in parts], axis=0)
        if name == 'n_evals':
            full = np.full((n_lat, n_lon), -1, dtype=np.int64)
        else:
            full = np.full(val.shape[1:] + (n_lat, n_lon), np.nan)
        full[..., lat, lon] = np.moveaxis(val, 0, -1)
        setattr(maps, name, full)
    products = {}
    if par_bins is not None:
        products.update(pdf_counts=[part.pdf_counts for part in parts], pdf_outside=[part.pdf_outside for part in parts])
        maps.pdf_bins = parts[0].pdf_bins if parts else None
    if covariance:
        products['cov'] = [part.cov for part in parts]
    if moments:
        for name, field in (('spec_mean', 'mean'), ('spec_std', 'std'), ('peak_mean',) * 2, ('peak_std',) * 2, ('total_mean',) * 2,
                            ('total_std',) * 2):
            products[name] = [getattr(part.model, field) for part in parts]
    for name, vals in products.items():
        val = np.concatenate(vals, axis=0)
        full = np.full(val.shape[1:] + (n_lat, n_lon), -1 if val.dtype == np.int64 else np.nan, dtype=val.dtype)
        full[..., lat, lon] = np.moveaxis(val, 0, -1)
        setattr(maps, name, full)
    return maps
