"""Least-squares fits: the normal equations of a damped Gauss-Newton step, and a Levenberg-Marquardt driver
that fits every pixel of a cube in lock-step.

A point is one (pixel, theta).  With p(theta) the model spectrum `predict_batch` returns for it, the probes of parameter k
are theta+ = theta + step_k e_k and theta- = theta - step_k e_k, clipped into [lower_k, upper_k] where those are given, and

    J_k = (p(theta+) - p(theta-)) / (theta+_k - theta-_k)        (0 for a fixed parameter: theta+_k == theta-_k)

With r = data - p(theta) and W the channels' inverse variances (0: a masked channel, left out whatever it holds)

    chi2 = sum W r^2,    grad_k = sum W J_k r = -1/2 d chi2 / d theta_k,    curv_kl = sum W J_k J_l

-- the entries of one augmented Gram matrix [J r]^T W [J r].  `nfa_runner_normal_equations` (csrc/nfa_lsq.h) forms them on
the device from spectra that never leave it (`DeviceBackend`); `normal_equations_from_spectra` is the same arithmetic in
numpy on spectra the caller has (`PredictBackend`: `predict_batch` to the host; `FunctionBackend`: any Python model).

The step of the finite difference is 1e-3 of the prior range and must not be made much smaller: the models narrow the
optical depth to float on its way into the exponential, so a spectrum is a staircase at the 1e-7 relative level (DESIGN
5), and a difference over a tiny step measures the staircase."""
from collections import namedtuple

import numpy as np

NormalEquations = namedtuple('NormalEquations', 'chi2 grad curv')
NormalEquations.__doc__ = """chi2 [B]; grad [B, ndim] = J^T W r; curv [B, ndim, ndim] = J^T W J (None where not asked for)."""
LsqResult = namedtuple('LsqResult', 'theta chi2 cov n_iter status')
LsqResult.__doc__ = """theta [B, ndim]; chi2 [B]; cov [B, ndim, ndim], the pseudo-inverse of J^T W J over the free parameters at
theta (zeros in the rows and columns of fixed or pinned ones); n_iter [B]; status [B]: 'converged', 'max_iter', 'stalled' or
'invalid' (a chi2 that is not finite at the start)."""
CubeFit = namedtuple('CubeFit', 'params errors chi2 status lnL')
CubeFit.__doc__ = """Maps of a `fit_cube`: params, errors [ndim, n_lat, n_lon] (the 1-sigma errors sqrt(diag cov)); chi2,
status, lnL [n_lat, n_lon].  NaN (status '') in a pixel that was not fitted."""

STEP_FRACTION = 1e-3               # of the prior range: the default step of the central difference
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-12, 1e12


def probe_rows(theta, step, lower=None, upper=None):
    """(rows [B, 1 + 2 ndim, ndim], inv_dtheta [B, ndim]): per point the base row, then theta+ and theta- of parameter 0,
    of parameter 1, ...; inv_dtheta = 1 / (theta+_k - theta-_k), 0 for a fixed parameter.  The rows and the numbers
    `lsq_probe_kernel` writes on the device."""
    theta = np.asarray(theta, dtype=np.float64)
    B, n = theta.shape
    step = np.asarray(step, dtype=np.float64)
    lo = np.full(n, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64)
    hi = np.full(n, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
    plus, minus = np.minimum(np.maximum(theta + step, lo), hi), np.minimum(np.maximum(theta - step, lo), hi)
    rows = np.repeat(theta[:, None, :], 1 + 2 * n, axis=1)
    k = np.arange(n)
    rows[:, 1 + 2 * k, k] = plus
    rows[:, 2 + 2 * k, k] = minus
    with np.errstate(divide='ignore'):
        inv = np.where(plus == minus, 0.0, 1.0 / (plus - minus))
    return rows, inv


def normal_equations_from_spectra(spec_rows, inv_dtheta, data, weight):
    """`NormalEquations` of B points from their model spectra: spec_rows [B, R, n_chan] in the order of `probe_rows` (R = 1 +
    2 ndim, or R = 1: chi2 alone, grad and curv None), inv_dtheta [B, ndim], data [B, n_chan], weight [B, n_chan] >= 0.  A
    channel of weight 0 is left out; a model value that is not finite at a channel of positive weight makes the point's
    outputs NaN.  Computed in the dtype of `spec_rows` (float64 unless the caller hands longdouble)."""
    spec_rows = np.asarray(spec_rows)
    dt = np.longdouble if spec_rows.dtype == np.longdouble else np.float64
    spec_rows = spec_rows.astype(dt, copy=False)
    B, R, _ = spec_rows.shape
    n = (R - 1) // 2
    data, weight = np.asarray(data).astype(dt, copy=False), np.asarray(weight).astype(dt, copy=False)
    keep = weight > 0
    with np.errstate(invalid='ignore', over='ignore'):
        T = np.zeros((B, n + 1, spec_rows.shape[2]), dtype=dt)
        T[:, n] = np.where(keep, data - spec_rows[:, 0], 0)
        bad = np.any(keep & ~np.isfinite(spec_rows[:, 0]), axis=1)
        if n:
            inv = np.asarray(inv_dtheta).astype(dt, copy=False)
            J = (spec_rows[:, 1::2] - spec_rows[:, 2::2]) * inv[:, :, None]
            live = keep[:, None, :] & (inv != 0)[:, :, None]
            T[:, :n] = np.where(live, J, 0)
            bad |= np.any(live & ~np.isfinite(J), axis=(1, 2))
        G = np.einsum('bkc,blc->bkl', np.where(keep, weight, 0)[:, None, :] * T, T)
        G = np.triu(G) + np.swapaxes(np.triu(G, 1), 1, 2)    # entry (k, l), k <= l, is (w T_k) T_l; both triangles hold it
    G[bad] = np.nan
    if R == 1:
        return NormalEquations(G[:, 0, 0].copy(), None, None)
    return NormalEquations(G[:, n, n].copy(), G[:, :n, n].copy(), G[:, :n, :n].copy())


def channel_weights(runner, pix, dtype=np.float64):
    """(data, weight), [B, n_chan_tot] each, of a `CubeRunner`'s pixels pix[B] as the device holds them: for a scalar noise
    weight = 1 / sigma^2; for a noise per channel chan_w / sigma_ref^2 with sigma_ref the smallest finite sigma of the
    (pixel, spectrum) and chan_w = (sigma_ref / sigma)^2 in float64, 0 at a masked channel.  The factors are formed in float64
    as the engine forms them and multiplied in `dtype`."""
    pix = np.asarray(pix, dtype=np.int64)
    data = np.asarray(runner._data, dtype=np.float64)[pix]
    noise = np.asarray(runner._noise, dtype=np.float64)[pix]
    off = runner._ss.offsets
    weight = np.empty(data.shape, dtype=dtype)
    for k in range(runner.n_spec):
        sl = slice(off[k], off[k + 1])
        if runner._ss.per_channel:
            sigma = noise[:, sl]
            ref = np.min(np.where(np.isfinite(sigma), sigma, np.inf), axis=1, keepdims=True)
            ratio = ref / sigma
            weight[:, sl] = (ratio * ratio).astype(dtype) * (1.0 / (ref * ref)).astype(dtype)
        else:
            weight[:, sl] = (1.0 / (noise[:, k] * noise[:, k])).astype(dtype)[:, None]
    return data, weight


class FunctionBackend:
    """The normal equations over any Python model: predict_fn(pix[B], theta[B, ndim]) -> spectra [B, n_chan]; data and
    weight [n_pix, n_chan]."""

    def __init__(self, predict_fn, data, weight):
        self.predict_fn = predict_fn
        self.data, self.weight = np.asarray(data, dtype=np.float64), np.asarray(weight, dtype=np.float64)

    def _spectra(self, pix, rows):
        B, R, n = rows.shape
        spec = np.asarray(self.predict_fn(np.repeat(pix, R), rows.reshape(B * R, n)))
        return spec.reshape(B, R, -1)

    def _points(self, pix):
        return self.data[pix], self.weight[pix]

    def normal_equations(self, pix, theta, step, lower=None, upper=None):
        pix = np.asarray(pix, dtype=np.int64)
        rows, inv = probe_rows(theta, step, lower, upper)
        return normal_equations_from_spectra(self._spectra(pix, rows), inv, *self._points(pix))

    def chi_squared(self, pix, theta):
        pix = np.asarray(pix, dtype=np.int64)
        theta = np.asarray(theta, dtype=np.float64)
        return normal_equations_from_spectra(self._spectra(pix, theta[:, None, :]), None, *self._points(pix)).chi2


class PredictBackend(FunctionBackend):
    """The normal equations through `CubeRunner.predict_batch`: the spectra of the probe rows come to the host and numpy
    reduces them.  What `DeviceBackend` is measured and tested against."""

    def __init__(self, runner):
        self.runner = runner
        self.predict_fn = lambda pix, theta: runner.predict_batch(pix, theta)[0]

    def _points(self, pix):
        return channel_weights(self.runner, pix)


class DeviceBackend:
    """The normal equations on the device (`CubeRunner.normal_equations`, `CubeRunner.chi_squared`)."""

    def __init__(self, runner, chunk_rows=None):
        self.runner, self.chunk_rows = runner, chunk_rows

    def normal_equations(self, pix, theta, step, lower=None, upper=None):
        return self.runner.normal_equations(pix, theta, step, lower, upper, chunk_rows=self.chunk_rows)

    def chi_squared(self, pix, theta):
        return self.runner.chi_squared(pix, theta)


def prior_box(utrans, ncomp, n=4096, seed=0):
    """(lower, upper), [ndim] each: the smallest and the largest value every parameter takes in `n` prior draws through
    `utrans.transform` -- the box of every prior, the placement priors included, whose parameters depend on one another."""
    rng = np.random.default_rng(seed)
    U = rng.uniform(size=(n, utrans.n_param * ncomp))
    if hasattr(utrans, 'transform_batch'):
        utrans.transform_batch(U, ncomp)
    else:
        for row in U:
            utrans.transform(row, ncomp)
    return U.min(axis=0), U.max(axis=0)


def best_draws(runner, pix, n_draws, n_best, rng, unit=False):
    """Per pixel of `pix`, the `n_best` prior draws of highest lnL among `n_draws`, ties by draw index: [len(pix), n_best,
    ndim], the physical parameters, or (`unit`) the unit-cube rows they came from.  The draws are scored with
    `loglikelihood_batch` in blocks of pixels; `pix` None: the pixel of a one-pixel runner."""
    one = pix is None
    pix = np.zeros(1, dtype=np.int32) if one else np.ascontiguousarray(pix, dtype=np.int32)
    n_pix, ndim = pix.size, runner.ndim
    out = np.empty((n_pix, n_best, ndim))
    block = max(1, (1 << 22) // (n_draws * ndim))            # pixels scored per call: 32 MB of draws
    for a in range(0, n_pix, block):
        b = min(n_pix, a + block)
        U = rng.uniform(size=((b - a) * n_draws, ndim))
        kept = U.copy() if unit else U
        lnl = runner.loglikelihood_batch(U) if one else runner.loglikelihood_batch(np.repeat(pix[a:b], n_draws), U)      # U becomes theta
        lnl = np.where(np.isfinite(lnl), lnl, -np.inf).reshape(b - a, n_draws)
        best = np.argsort(-lnl, axis=1, kind='stable')[:, :n_best]
        out[a:b] = kept.reshape(b - a, n_draws, ndim)[np.arange(b - a)[:, None], best]
    return out


def _free(theta, grad, curv, lower, upper):
    """The parameters a step may move: a positive curvature, and not at a bound with the gradient pointing outward."""
    diag = np.diagonal(curv, axis1=1, axis2=2)
    return (diag > 0) & ~((theta <= lower) & (grad < 0)) & ~((theta >= upper) & (grad > 0))


def _masked(curv, free):
    return np.where(free[:, :, None] & free[:, None, :], curv, 0.0)


def fit_pixels(backend, pix, theta0, lower, upper, step=None, max_iter=50, xtol=1e-3, ftol=1e-6):
    """Levenberg-Marquardt over the points (pix[B], theta0[B, ndim]) in lock-step, inside the box [lower, upper]: an
    `LsqResult`.  Per iteration: one normal-equations call on the points whose last step was accepted; a batched solve of
    (A + lambda diag A) delta = g over the free parameters (A_kk > 0, and not at a bound with g_k pointing outward); one
    chi2-only call on the trial points clip(theta + delta).  A step is accepted where chi2 fell (lambda / 10, floor 1e-12)
    and refused otherwise (lambda * 10; above 1e12 the point has 'stalled').  A point has 'converged' at an accepted step
    with max_k |delta_k| / sqrt(C_kk) < xtol or a fall of chi2 below ftol (chi2 is in natural units: an absolute test), C
    the pseudo-inverse of A over the free parameters.  step: of the central difference, default 1e-3 (upper - lower)."""
    pix = np.asarray(pix, dtype=np.int64)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    theta = np.clip(np.array(theta0, dtype=np.float64, ndmin=2), lower, upper)
    B, n = theta.shape
    if pix.shape != (B,):
        raise ValueError('one pixel index per row of theta0 is required')
    step = STEP_FRACTION * (upper - lower) if step is None else np.array(step, dtype=np.float64)
    step = np.where(upper > lower, step, 1.0)                # a parameter without a range is fixed: any step, clipped away
    chi2 = np.full(B, np.nan)
    grad, curv = np.zeros((B, n)), np.zeros((B, n, n))
    lam = np.full(B, LAMBDA0)
    n_iter = np.zeros(B, dtype=np.int64)
    status = np.full(B, 'max_iter', dtype='<U9')
    stale = np.ones(B, dtype=bool)                           # the normal equations are not those of theta
    active = np.ones(B, dtype=bool)

    def refresh(sel):
        ne = backend.normal_equations(pix[sel], theta[sel], step, lower, upper)
        chi2[sel], grad[sel], curv[sel] = ne.chi2, ne.grad, ne.curv
        stale[sel] = False

    for it in range(max_iter + 1):
        sel = np.flatnonzero(active & stale)
        if sel.size:
            refresh(sel)
        if it == 0:
            invalid = ~np.isfinite(chi2)
            status[invalid] = 'invalid'
            active &= ~invalid
        # (a point whose equations went non-finite after an accepted step cannot be stepped further)
        broken = active & ~(np.isfinite(grad).all(axis=1) & np.isfinite(curv).all(axis=(1, 2)))
        status[broken] = 'stalled'
        active &= ~broken
        act = np.flatnonzero(active)
        if act.size == 0 or it == max_iter:
            break
        free = _free(theta[act], grad[act], curv[act], lower, upper)
        nothing = ~free.any(axis=1)                          # every parameter fixed or pinned: the point is where it can be
        A = _masked(curv[act], free)
        diag = np.diagonal(A, axis1=1, axis2=2)
        M = A + lam[act, None, None] * (np.eye(n) * diag[:, None, :]) + np.eye(n) * (~free)[:, None, :]
        g = np.where(free, grad[act], 0.0)
        try:
            delta = np.linalg.solve(M, g[:, :, None])[:, :, 0]
        except np.linalg.LinAlgError:
            delta = np.einsum('bkl,bl->bk', np.linalg.pinv(M, hermitian=True), g)
        trial = np.clip(theta[act] + delta, lower, upper)
        chi2_t = backend.chi_squared(pix[act], trial)
        n_iter[act] += 1
        fell = (chi2_t < chi2[act]) & ~nothing
        with np.errstate(divide='ignore', invalid='ignore'):
            C = np.linalg.pinv(A, hermitian=True)
            sig = np.sqrt(np.diagonal(C, axis1=1, axis2=2))
            small = np.nanmax(np.where(free & (sig > 0), np.abs(delta) / sig, 0.0), axis=1) < xtol
        drop = chi2[act] - chi2_t
        done = (fell & (small | (drop < ftol))) | nothing
        ok = act[fell]
        theta[ok], chi2[ok] = trial[fell], chi2_t[fell]
        stale[ok] = True
        lam[ok] = np.maximum(lam[ok] / 10.0, LAMBDA_MIN)
        no = act[~fell & ~nothing]
        lam[no] *= 10.0
        status[act[done]] = 'converged'
        active[act[done]] = False
        gone = no[lam[no] > LAMBDA_MAX]
        status[gone] = 'stalled'
        active[gone] = False
    # the covariance at the returned theta, lambda = 0
    valid = status != 'invalid'
    sel = np.flatnonzero(valid & stale)
    if sel.size:
        saved = chi2[sel].copy()
        refresh(sel)
        chi2[sel] = saved                                    # (the same number: chi_squared and normal_equations agree to the bit)
    cov = np.zeros((B, n, n))
    good = np.flatnonzero(valid & np.isfinite(grad).all(axis=1) & np.isfinite(curv).all(axis=(1, 2)))
    if good.size:
        free = _free(theta[good], grad[good], curv[good], lower, upper)
        cov[good] = _masked(np.linalg.pinv(_masked(curv[good], free), hermitian=True), free)
    cov[valid & ~np.isin(np.arange(B), good)] = np.nan
    return LsqResult(theta, chi2, cov, n_iter, status)


def fit_cube(stack, utrans, runner_cls, ncomp=1, n_draws=2048, n_starts=4, runner_kwargs=None, seed=0, **fit_kw):
    """Least-squares fit of every good pixel of a `CubeStack` with `ncomp` components: a `CubeFit` of maps.  The runner is
    built as `CubeFitter` builds it; `n_draws` prior draws per pixel are scored with `loglikelihood_batch`, `fit_pixels`
    starts from the best `n_starts` of every pixel and the lowest chi2 is kept.  lnL is the likelihood of the result
    through `predict_batch`, comparable to a nested run's `max_loglike`.  fit_kw: `fit_pixels`' keywords."""
    from .fitter import CubeFitter
    fitter = CubeFitter(stack, utrans, runner_cls, runner_kwargs=runner_kwargs)
    kwargs = fitter.runner_kwargs if fitter.species is None else dict(fitter.runner_kwargs, species=fitter.species, fill=fitter.fill)
    runner, lon, lat = stack.to_device(utrans, ncomp=ncomp, model=fitter.model_id, **kwargs)
    n_pix, ndim = runner.n_pix, runner.ndim
    n_starts = min(int(n_starts), int(n_draws))
    lower, upper = prior_box(utrans, ncomp, seed=seed)
    starts = best_draws(runner, np.arange(n_pix, dtype=np.int32), n_draws, n_starts, np.random.default_rng(seed))
    lower, upper = np.minimum(lower, starts.min(axis=(0, 1))), np.maximum(upper, starts.max(axis=(0, 1)))
    pix = np.repeat(np.arange(n_pix), n_starts)
    res = fit_pixels(DeviceBackend(runner), pix, starts.reshape(n_pix * n_starts, ndim), lower, upper, **fit_kw)
    chi2 = np.where(np.isfinite(res.chi2) & (res.status != 'invalid'), res.chi2, np.inf).reshape(n_pix, n_starts)
    row = np.arange(n_pix) * n_starts + np.argmin(chi2, axis=1)
    theta = res.theta[row]
    _, lnl = runner.predict_batch(np.arange(n_pix, dtype=np.int32), theta, want_spectra=False)
    n_lon, n_lat = stack.spatial_shape
    params, errors = np.full((ndim, n_lat, n_lon), np.nan), np.full((ndim, n_lat, n_lon), np.nan)
    chi2_map, lnl_map = np.full((n_lat, n_lon), np.nan), np.full((n_lat, n_lon), np.nan)
    status = np.full((n_lat, n_lon), '', dtype='<U9')
    params[:, lat, lon] = theta.T
    with np.errstate(invalid='ignore'):
        errors[:, lat, lon] = np.sqrt(np.diagonal(res.cov[row], axis1=1, axis2=2)).T
    chi2_map[lat, lon], lnl_map[lat, lon], status[lat, lon] = res.chi2[row], lnl, res.status[row]
    return CubeFit(params, errors, chi2_map, status, lnl_map)
