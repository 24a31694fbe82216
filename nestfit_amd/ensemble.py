"""Ensemble MCMC at a fixed component count: the affine-invariant stretch move of Goodman & Weare (2010) in
the unit cube, where the prior is flat by construction, around the engine's likelihood batch -- posteriors with real error
bars under every prior kind, model and likelihood option; without an evidence unless the ensemble is tempered.

`run_twin` is the numpy twin of the device sampler (csrc/nfa_ensemble.h, contract: csrc/nfa_ensemble_plan.h): one state
record (`EnsState`, fields named like `EnsDev`'s) and one function per stage of the device -- `_create` (nfa_ensemble_create),
`_propose` (ens_propose_kernel), `_accept` (the likelihood batch and ens_accept_kernel), `_trace` (ens_trace_kernel), `_keep`
(ens_keep_kernel) -- with the same arithmetic and the same random numbers (`nested._uniform`), so the same arguments give
the same run.  `summarize` is the twin of ens_summary_kernel, `pdf_counts` of ens_hist_kernel (equal to the bit) and
`covariance_of` of ens_cov_kernel (the same formula summed in another order).  `sample_pixels` and `sample_cube` drive the
device; the products of a chain -- marginal histograms, parameter covariances, moments of the model spectra --
are reduced there, so the chain need not leave it.

Tempered ensembles: with `betas=` (`ladder`) a pixel carries T ensembles at inverse temperatures 1 = beta_0 > ..
>= 0, each moving against L^beta, neighbours exchanging walkers (`_swap`, ens_swap_kernel).  The cold chain then crosses
between separated modes, and the kept lnL of the rungs give the evidence by stepping stones (`evidence_of`, the twin of
ens_evidence_kernel); `compare_ncomp` applies the fitter's rule to such evidences."""
import ctypes as C
import math
import types
import warnings

import numpy as np

from . import _ffi
from .nested import LOG_ZERO, _U64, _uniform

# csrc/nfa_ensemble_plan.h (tests/test_ensemble_cpu.py compares them with the header's)
ENS_TAG = 1 << 61
MAX_WALKERS, MAX_Q, MAX_SORT, A_MAX = 512, 8, 8192, 16.0
MAX_BINS = 1024
# a tempered ensemble (tests/test_ensemble_tempered_cpu.py compares these with the header's)
MAX_TEMPS, MAX_BLOCKS, RUNG_SHIFT = 32, 16, 48
ENS_SWAP_TAG = ENS_TAG + (1 << 60)


class EnsState(types.SimpleNamespace):
    """What a run of the twin holds, under `EnsDev`'s names: P, W, D, DT, fmap, pix; the walkers u[P, W, D], theta[P, W, DT],
    lnL[P, W]; a half-step's rows, row_lnL, y, inside; counts[P, 3] (accepted, outside, evaluated).  P counts units: unit p is
    rung p % T of pixel p // T (untempered: T = 1, a unit is a pixel); betas[T], swaps[n_pix, T - 1, 2] (accepted, proposed).
    Beside them what only the host has: loglike, chunk, margin, swap_margin, n_pix, rung[P], beta[P]."""


class TwinResult(types.SimpleNamespace):
    """`run_twin`'s outputs: u[P, W, ndim] (0.5 where not sampled), theta, lnL: the walkers as they stand; chain_theta[P,
    n_keep, W, ndim], chain_lnL[P, n_keep, W]; trace[P, n_steps, D + 1]; accepted, outside, evaluated [P]; margin; `state`,
    to continue from.  Of a tempered run these describe the cold chain (rung 0), and beside them stand rung_u, rung_theta
    [P, T, W, ndim], rung_lnL_state [P, T, W]; rung_lnL [P, T, n_keep, W]; rung_trace [P, T, n_steps, D + 1]; rung_accepted,
    rung_outside, rung_evaluated [P, T]; swaps_accepted, swaps_proposed [P, T - 1]; swap_margin, the smallest |log r - rhs| over
    the swap decisions (`margin` is the moves')."""


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


def check_betas(betas):
    """ens_check_betas of the plan header, for the twin."""
    b = np.asarray(betas, dtype=np.float64)
    if b.ndim != 1 or not 2 <= b.size <= MAX_TEMPS:
        raise ValueError('a tempered ensemble takes 2 .. 32 rungs')
    if not np.isfinite(b).all() or b[0] != 1.0 or not (np.diff(b) < 0).all() or b[-1] < 0:
        raise ValueError('betas must be finite, start at 1, decrease strictly and end at 0 or above')
    return b


def ladder(n_temps, beta_min=1e-4):
    """betas[n_temps]: geometric from 1 to `beta_min` over n_temps - 1 rungs, then 0 (where Z = 1: the prior of the unit cube)."""
    b = np.concatenate([np.geomspace(1.0, float(beta_min), int(n_temps) - 1), [0.0]])
    b[0] = 1.0
    return b


def _create(loglike, ndim, pix, n_walkers, u0, free_mask, chunk, betas=None):
    """nfa_ensemble_create (betas: nfa_ensemble_create_tempered): the start rows evaluated once.  u0[n_pix, W, ndim] goes to
    every rung; [n_pix, T, W, ndim] is taken as it is."""
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    n_pix, W = pix.size, int(n_walkers)
    betas = None if betas is None else check_betas(betas)
    T = 1 if betas is None else int(betas.size)
    P = n_pix * T
    fmap = np.arange(ndim) if free_mask is None else np.flatnonzero(np.asarray(free_mask))
    u0 = np.asarray(u0, dtype=np.float64)
    if u0.size == n_pix * W * ndim:
        u0 = np.repeat(u0.reshape(n_pix, 1, W, ndim), T, axis=1)
    u0 = u0.reshape(P, W, ndim)
    pix = np.repeat(pix, T)
    S = EnsState(P=P, W=W, D=int(fmap.size), DT=int(ndim), fmap=fmap, pix=pix, loglike=loglike, chunk=chunk, margin=np.inf,
                 T=T, n_pix=n_pix, betas=betas, rung=np.tile(np.arange(T), n_pix), swap_margin=np.inf)
    S.beta = np.ones(P) if betas is None else np.tile(betas, n_pix)
    S.swaps = np.zeros((n_pix, T - 1, 2), dtype=np.int64)
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
    tag = np.array([ENS_TAG + (int(t) << RUNG_SHIFT) + 2 * step + h for t in S.rung], dtype=_U64)[:, None]
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
        rhs = float(S.D - 1) * np.log(z) + S.beta[:, None] * (Ly - Lk)      # (beta = 1 multiplies exactly)
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


def swap_parity(sweep):
    return sweep & 1


def _swap(S, seed, step, sweep):
    """ens_swap_kernel: sweep `sweep` (from 0 in every run), after the half-steps of step `step`."""
    n_pix, T, W = S.n_pix, S.T, S.W
    u, theta, lnL = S.u.reshape(n_pix, T, W, S.D), S.theta.reshape(n_pix, T, W, S.DT), S.lnL.reshape(n_pix, T, W)
    assert np.shares_memory(u, S.u) and np.shares_memory(theta, S.theta) and np.shares_memory(lnL, S.lnL)
    p = S.pix[::T].astype(_U64)[:, None]
    k = np.arange(W).astype(_U64)[None, :]
    for t in range(swap_parity(sweep), T - 1, 2):
        r = _uniform(seed, p, _U64(ENS_SWAP_TAG + (t << RUNG_SHIFT) + step), k)
        rhs = (S.betas[t] - S.betas[t + 1]) * (lnL[:, t + 1] - lnL[:, t])
        lr = np.log(r)
        acc = lr < rhs
        S.swap_margin = min(S.swap_margin, float(np.abs(lr - rhs).min()))
        for x in (u, theta, lnL):
            a, b = x[:, t][acc].copy(), x[:, t + 1][acc].copy()
            x[:, t][acc], x[:, t + 1][acc] = b, a
        S.swaps[:, t, 0] += acc.sum(axis=1)
        S.swaps[:, t, 1] += W


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
             pix=None, state=None, chunk=1 << 18, betas=None, swap_every=1):
    """The device's run on the host: `loglike(pix, T)` returns lnL of the unit-cube rows T[B, ndim] of cube pixels pix[B]
    and leaves theta in T.  pix: the cube pixel of each of the n_pix pixels (None: 0 .. n_pix - 1); it is in the random
    stream.  state: a `TwinResult.state` to continue from (u0 is then not read); the steps count from 1 again, so a
    continuation takes another seed.  betas: the ladder of a tempered run (`ladder`), swap_every: a swap sweep after every so many
    steps, 0: never; a state brings its own of both, as the device's ensemble does.  Returns a `TwinResult`."""
    pix = np.arange(n_pix, dtype=np.int32) if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
    assert pix.shape == (n_pix,)
    seed = _U64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    n_sampled = state.D if state is not None else ndim if free_mask is None else int(np.count_nonzero(free_mask))
    check_arguments(int(n_walkers), n_sampled, n_steps, n_burn, thin, a)
    if int(swap_every) < 0:
        raise ValueError('swap_every must be 0 (never) or a number of steps')
    S = _create(loglike, ndim, pix, n_walkers, u0, free_mask, chunk, betas) if state is None else state
    if state is None:
        S.swap_every = int(swap_every)
    n_keep = n_keep_of(n_steps, n_burn, thin)
    T, NP = S.T, S.n_pix
    S.counts[:] = 0
    S.swaps[:] = 0
    S.margin = S.swap_margin = np.inf
    S.lnL = np.where(np.isfinite(S.lnL), S.lnL, log_zero)
    chain_theta, rung_lnL = np.empty((NP, n_keep, S.W, S.DT)), np.empty((NP, T, n_keep, S.W))
    trace = np.empty((S.P, n_steps, S.D + 1))
    sweep = 0
    for step in range(1, n_steps + 1):
        for h in (0, 1):
            _propose(S, seed, step, h, a)
            _accept(S, seed, step, h, a)
        if T > 1 and S.swap_every > 0 and step % S.swap_every == 0:
            _swap(S, seed, step, sweep)
            sweep += 1
        trace[:, step - 1] = _trace(S)
        if keeps(step, n_burn, thin):                           # ens_keep_kernel: theta of rung 0, lnL of every rung
            slot = (step - n_burn) // thin - 1
            chain_theta[:, slot], rung_lnL[:, :, slot] = S.theta[::T], S.lnL.reshape(NP, T, S.W)
    per = lambda x: x.reshape((NP, T) + x.shape[1:])           # noqa: E731 (units -> pixel, rung)
    u, counts, rung_trace = per(_expand(S, S.u)), per(S.counts), per(trace)
    return TwinResult(u=u[:, 0].copy(), theta=per(S.theta)[:, 0].copy(), lnL=per(S.lnL)[:, 0].copy(), chain_theta=chain_theta,
                      chain_lnL=rung_lnL[:, 0].copy(), trace=rung_trace[:, 0].copy(), accepted=counts[:, 0, 0].copy(),
                      outside=counts[:, 0, 1].copy(), evaluated=counts[:, 0, 2].copy(), margin=S.margin, state=S,
                      rung_u=u, rung_theta=per(S.theta).copy(), rung_lnL_state=per(S.lnL).copy(), rung_lnL=rung_lnL, rung_trace=rung_trace,
                      rung_accepted=counts[:, :, 0].copy(), rung_outside=counts[:, :, 1].copy(), rung_evaluated=counts[:, :, 2].copy(),
                      swaps_accepted=S.swaps[:, :, 0].copy(), swaps_proposed=S.swaps[:, :, 1].copy(), swap_margin=S.swap_margin)


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


class Evidence(types.SimpleNamespace):
    """`evidence_of`'s outputs: sets[P, T, B + 1, 3] = (mean, var, r) of every (pixel, rung, set) as nfa_ensemble_evidence
    lays them out (set 0: all kept steps; sets 1 .. B: the blocks); lnZ [P], the stepping-stone evidence sum_t r[t, set 0]; lnZ_err
    [P], the standard deviation (divisor B - 1) of the B block values of sum_t r over sqrt(B), NaN for B = 1; lnZ_ti [P], the
    trapezoid of the rungs' mean lnL over beta -- a diagnostic of the ladder, not an estimate to use; mean_lnL [P, T]."""


def evidence_sets(rung_lnL, betas, n_blocks=8, dtype=np.float64):
    """ens_evidence_kernel's formulas in numpy, computed in `dtype`, on rung_lnL[P, T, n_keep, W]: sets[P, T, B + 1, 3].  Block
    sets hold floor(n_keep / B) kept steps each; the remainder of n_keep / B is in set 0 only."""
    x = np.asarray(rung_lnL)
    P, T, n_keep, W = x.shape
    B = int(n_blocks)
    if not 1 <= B <= MAX_BLOCKS or B > n_keep:
        raise ValueError('an evidence takes 1 .. 16 blocks and no more than kept steps')
    b = np.asarray(betas, dtype=np.float64).astype(dtype)
    delta = np.concatenate([[dtype(0)], b[:-1] - b[1:]]).astype(dtype)[None, :, None]
    out = np.empty((P, T, B + 1, 3), dtype=dtype)
    blk = n_keep // B
    for j in range(B + 1):
        first, steps = (0, n_keep) if j == 0 else ((j - 1) * blk, blk)
        v = x[:, :, first:first + steps].reshape(P, T, steps * W).astype(dtype)
        n = dtype(steps * W)
        d = v - v[:, :, :1]
        mean = d.sum(axis=2) / n
        out[:, :, j, 0] = v[:, :, 0] + mean
        out[:, :, j, 1] = np.maximum((d * d).sum(axis=2) / n - mean * mean, 0)
        M = v.max(axis=2, keepdims=True)
        out[:, :, j, 2] = delta[:, :, 0] * M[:, :, 0] + np.log(np.exp(delta * (v - M)).sum(axis=2) / n)
        out[:, 0, j, 2] = 0
    return out


def evidence_from(sets, betas):
    """The `Evidence` of sets[P, T, B + 1, 3] (`evidence_sets`, or the device's) on the ladder betas[T]."""
    sets = np.asarray(sets)
    b = np.asarray(betas, dtype=np.float64)
    B = sets.shape[2] - 1
    total = sets[:, :, :, 2].sum(axis=1)                        # [P, B + 1]: sum over the rungs
    lnZ = total[:, 0].astype(np.float64)
    if b[-1] != 0.0:
        warnings.warn('the ladder does not end at beta = 0, where Z = 1: the stepping stones give no evidence', RuntimeWarning, stacklevel=2)
        lnZ = np.full(lnZ.shape, np.nan)
    lnZ_err = (total[:, 1:].astype(np.float64).std(axis=1, ddof=1) / math.sqrt(B)) if B > 1 else np.full(lnZ.shape, np.nan)
    mean = sets[:, :, 0, 0].astype(np.float64)
    lnZ_ti = (0.5 * (mean[:, :-1] + mean[:, 1:]) * (b[:-1] - b[1:])[None, :]).sum(axis=1)
    return Evidence(sets=sets, lnZ=lnZ, lnZ_err=lnZ_err, lnZ_ti=lnZ_ti, mean_lnL=mean)


def evidence_of(rung_lnL, betas, n_blocks=8, dtype=np.float64):
    """The twin of nfa_ensemble_evidence and what follows from it: an `Evidence` of rung_lnL[P, T, n_keep, W] on betas[T]."""
    return evidence_from(evidence_sets(rung_lnL, betas, n_blocks, dtype), betas)


def nbest_of(lnZ, lnZ_thresh=11):
    """`CubeFitter`'s rule on evidences lnZ[K + 1, ...] (lnZ[0]: no component, the runner's null_lnZ): a pixel advances from
    n - 1 to n components while lnZ[n] - lnZ[n - 1] >= lnZ_thresh, and stops at its first failure (a NaN fails).  int64[...]."""
    lnZ = np.asarray(lnZ, dtype=np.float64)
    nbest = np.zeros(lnZ.shape[1:], dtype=np.int64)
    for n in range(1, lnZ.shape[0]):
        with np.errstate(invalid='ignore'):
            nbest[(nbest == n - 1) & (lnZ[n] - lnZ[n - 1] >= lnZ_thresh)] = n
    return nbest


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

    def __init__(self, runner, pix, n_walkers, free_mask, u0, betas=None, swap_every=1):
        lib = _ffi.engine()
        self.runner = runner                                     # (the runner outlives its ensemble)
        h = C.c_void_p()
        ipix = None if pix is None else pix.ctypes.data_as(_ffi._ip)
        mask = None if free_mask is None else free_mask.ctypes.data_as(_ffi._ip)
        if betas is None:
            _ffi.check(lib.nfa_ensemble_create(C.byref(h), runner._run.handle, ipix, u0.shape[0], int(n_walkers), mask, _ffi.dptr(u0)))
        else:
            _ffi.check(lib.nfa_ensemble_create_tempered(C.byref(h), runner._run.handle, ipix, u0.shape[0], int(n_walkers), _ffi.dptr(betas),
                                                        int(betas.size), int(swap_every), mask, _ffi.dptr(u0)))
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
    P = 1); u0[P, W, ndim].  betas[T]: a tempered ensemble with a swap sweep every `swap_every` steps (0: never);
    u0[P, W, ndim] then goes to every rung and [P, T, W, ndim] is taken as it is; the calls above describe its cold chain, and
    `rung_counts`, `rung_state`, `rung_trace`, `rung_lnL` and `evidence` every rung.  The ladder is checked by the engine."""

    def __init__(self, runner, pix, n_walkers, u0, free_mask=None, betas=None, swap_every=1):
        self.ndim, self.W = int(runner.ndim), int(n_walkers)
        self.betas = None if betas is None else np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        self.T = 1 if betas is None else int(self.betas.size)
        self.pix = None if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
        self.P = 1 if pix is None else int(self.pix.size)
        fm = None if free_mask is None else np.ascontiguousarray(free_mask, dtype=np.int32)
        if fm is not None and fm.shape != (self.ndim,):
            raise ValueError('free_mask must hold one flag per unit-cube slot')
        self.D = self.ndim if fm is None else int(np.count_nonzero(fm))
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        if betas is not None and u0.shape == (self.P, self.W, self.ndim):
            u0 = np.ascontiguousarray(np.repeat(u0[:, None], self.T, axis=1))
        if u0.shape != ((self.P, self.W, self.ndim) if betas is None else (self.P, self.T, self.W, self.ndim)):
            raise ValueError('the start must be [n_pix, n_walkers, ndim], or [n_pix, n_temps, n_walkers, ndim] of a tempered ensemble')
        self.n_spec, self.n_chan_tot = int(runner.n_spec), int(runner._ss.chan_tot)
        self._h = _Handle(runner, self.pix, n_walkers, fm, u0, self.betas, swap_every)
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

    def rung_counts(self):
        """(accepted, outside, evaluated) int64[P, T] and (swaps accepted, swaps proposed) int64[P, T - 1] of the last run."""
        out = [np.empty((self.P, self.T), dtype=np.int64) for _ in range(3)] + [np.empty((self.P, max(self.T - 1, 0)), dtype=np.int64) for _ in range(2)]
        _ffi.check(_ffi.load().nfa_ensemble_rung_counts(self._h.handle, *[o.ctypes.data_as(_ffi._lp) for o in out]))
        return tuple(out)

    def rung_state(self):
        """(u, theta [P, T, W, ndim], lnL [P, T, W]) of every rung as it stands; u is a start."""
        shape = (self.P, self.T, self.W)
        u, theta, lnL = np.empty(shape + (self.ndim,)), np.empty(shape + (self.ndim,)), np.empty(shape)
        _ffi.check(_ffi.load().nfa_ensemble_rung_state(self._h.handle, _ffi.dptr(u), _ffi.dptr(theta), _ffi.dptr(lnL)))
        return u, theta, lnL

    def rung_trace(self):
        out = np.empty((self.P, self.T, self.n_steps, self.D + 1))
        _ffi.check(_ffi.load().nfa_ensemble_rung_trace(self._h.handle, _ffi.dptr(out)))
        return out

    def rung_lnL(self):
        """The kept lnL of every rung, [P, T, n_keep, W]."""
        out = np.empty((self.P, self.T, self.n_keep, self.W))
        _ffi.check(_ffi.load().nfa_ensemble_rung_lnl(self._h.handle, _ffi.dptr(out)))
        return out

    def evidence(self, n_blocks=8):
        """The `Evidence` of the last run, its sets[P, T, n_blocks + 1, 3] reduced on the device (`evidence_of` is the twin)."""
        n_blocks = int(n_blocks)
        sets = np.empty((self.P, self.T, max(n_blocks, 0) + 1, 3))
        _ffi.check(_ffi.load().nfa_ensemble_evidence(self._h.handle, n_blocks, _ffi.dptr(sets)))
        return evidence_from(sets, self.betas)

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
                  moments=False, utrans=None, betas=None, swap_every=1, n_blocks=8):
    """The posterior of the cube pixels `pix` of a `CubeRunner` (None: the pixel of a one-pixel runner) by `n_steps` steps of
    `n_walkers` walkers each on the device: an `EnsembleResult`.  n_burn None: half the steps; thin None: so that the kept
    samples of a pixel number 8192 at most, what the quantiles sort.  start: u0[P, n_walkers, ndim] in (0, 1), None:
    `starts(runner, pix, n_walkers, n_init, seed)`.  free_mask: the sampled unit-cube slots (None: all; `utrans.free_mask(ncomp)`
    leaves out the slots of constant and duplicated parameters).  par_bins: edges[ndim, n_bins + 1] of the marginal histograms
    (an int with `utrans=`: `bin_edges(utrans, runner.ncomp, par_bins)`); covariance, moments: the parameter covariances and
    the moments of the model spectra.  The three are reduced on the device before the result is handed back, so they outlive
    `close()`.  betas[T] (`ladder`): a tempered ensemble of T rungs per pixel with a swap sweep every `swap_every` steps (DESIGN
    4.26): a start [P, n_walkers, ndim] is given to every rung, [P, T, n_walkers, ndim] taken as it is; every field above then
    describes the cold chain, and the result gains lnZ, lnZ_err (batch means over `n_blocks` blocks of the kept steps), lnZ_ti
    [P], mean_lnL, rung_acceptance [P, T] and swap_rate [P, T - 1] (None without betas).  The argument checks are the engine's
    (`EngineError`)."""
    n_steps = int(n_steps)
    if par_bins is not None and np.ndim(par_bins) == 0:
        if utrans is None:
            raise ValueError('a number of bins needs utrans= for the edges')
        par_bins = bin_edges(utrans, runner.ncomp, int(par_bins))
    n_burn = n_steps // 2 if n_burn is None else int(n_burn)
    thin = default_thin(n_steps, int(n_walkers)) if thin is None else int(thin)
    pix = None if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
    u0 = starts(runner, pix, n_walkers, n_init, seed) if start is None else start
    ens = DeviceEnsemble(runner, pix, n_walkers, u0, free_mask, betas, swap_every)
    tempered = dict(lnZ=None, lnZ_err=None, lnZ_ti=None, mean_lnL=None, swap_rate=None, rung_acceptance=None)
    try:
        ens.run(n_steps, n_burn, thin, a, seed, log_zero)
        if betas is not None:
            ev = ens.evidence(n_blocks)
            r_acc, _, _, s_acc, s_prop = ens.rung_counts()
            with np.errstate(divide='ignore', invalid='ignore'):
                tempered = dict(lnZ=ev.lnZ, lnZ_err=ev.lnZ_err, lnZ_ti=ev.lnZ_ti, mean_lnL=ev.mean_lnL, swap_rate=s_acc / s_prop,
                                rung_acceptance=r_acc / float(n_steps * int(n_walkers)))
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
                          pdf_outside=pdf_out, pdf_bins=pdf_bins, cov=cov, model=model, _ensemble=ens, **tempered)


MAP_FIELDS = ('mean', 'std', 'best', 'best_lnL', 'quantiles', 'acceptance', 'outside', 'n_evals', 'tau', 'n_eff')
TEMPERED_FIELDS = ('lnZ', 'lnZ_err', 'lnZ_ti', 'mean_lnL', 'swap_rate', 'rung_acceptance')


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
    the starts are drawn for all pixels before the cut.  kw: `sample_pixels`' keywords; with betas= (a tempered ensemble, cut by
    nfa_ensemble_tempered_bytes) the maps lnZ, lnZ_err, lnZ_ti [lat, lon], mean_lnL, rung_acceptance [T, lat, lon] and swap_rate
    [T - 1, lat, lon] too."""
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
    betas = kw.get('betas')
    if betas is None:
        per_pixel = _ffi.load().nfa_ensemble_bytes(1, W, ndim, D, n_steps, max(0, n_keep_of(n_steps, n_burn, thin)))
    else:
        per_pixel = _ffi.load().nfa_ensemble_tempered_bytes(1, W, int(np.size(betas)), ndim, D, n_steps, max(0, n_keep_of(n_steps, n_burn, thin)))
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
    for name in MAP_FIELDS + (TEMPERED_FIELDS if betas is not None else ()):
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


def compare_ncomp(stack, utrans, runner_cls, ncomp_max=2, lnZ_thresh=11, betas=None, **kw):
    """The evidences of 1 .. `ncomp_max` components for every good pixel of a `CubeStack` by tempered ensembles (`sample_cube`
    with betas=, None: `ladder(16)`), and the component count `CubeFitter`'s rule takes from them (`nbest_of`): a namespace of
    maps lnZ, lnZ_err [ncomp_max + 1, lat, lon] (row 0: the runner's null_lnZ, error 0; NaN where a pixel is not good) and nbest
    int64[lat, lon] (-1 where a pixel is not good).  Every pixel is sampled at every count; nothing is written to a store.  kw:
    `sample_cube`'s keywords."""
    betas = ladder(16) if betas is None else betas
    maps = [sample_cube(stack, utrans, runner_cls, n, betas=betas, **kw) for n in range(1, int(ncomp_max) + 1)]
    from .fitter import CubeFitter
    fitter = CubeFitter(stack, utrans, runner_cls, runner_kwargs=kw.get('runner_kwargs'))
    kwargs = fitter.runner_kwargs if fitter.species is None else dict(fitter.runner_kwargs, species=fitter.species, fill=fitter.fill)
    runner, lon, lat = stack.to_device(utrans, ncomp=1, model=fitter.model_id, **kwargs)
    null = np.full(maps[0].lnZ.shape, np.nan)
    null[lat, lon] = runner.null_lnZ
    lnZ = np.stack([null] + [m.lnZ for m in maps])
    lnZ_err = np.stack([np.where(np.isnan(null), np.nan, 0.0)] + [m.lnZ_err for m in maps])
    nbest = nbest_of(lnZ, lnZ_thresh)
    nbest[np.isnan(null)] = -1
    return types.SimpleNamespace(lnZ=lnZ, lnZ_err=lnZ_err, nbest=nbest)
