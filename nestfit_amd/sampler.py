"""Built-in batched nested sampler: the stand-in for MultiNest when
``libmultinest`` is not available, built so that the GPU sees batches.

The reference drives one serial MultiNest instance per pixel
(``run_multinest``, nestfit/core/core.pyx:727-823; pixel loop nestfit/main.py:452-469), one
likelihood per callback.  Here every pixel of a cube is a nested-sampling run of its own, but all
runs advance in lock-step: each round proposes candidates per active pixel -- uniform in the
bounding ellipsoid(s) of its live points (MultiNest's ellipsoidal rejection sampling, Feroz et al. 2009;
up to four ellipsoids around clusters of live points where at most six dimensions are sampled),
or, where that has become hopeless, one
differential-evolution Metropolis step of each of 64 walkers inside the likelihood constraint --
all candidates of all pixels go to the device in ONE likelihood batch, and every pixel scans its
candidates in order: each one above the pixel's current threshold
replaces its worst live point (Skilling 2006 bookkeeping).  The outputs follow what the
reference's ``mn_dump`` stores (core.pyx:627-687): posterior rows ``[theta..., -2 lnL, weight]``,
``param_constr`` rows 2, 3 = best-fit and MAP, global lnZ and its error, max log-likelihood.

Two implementations of one algorithm: `run_nested` (numpy, any likelihood callable: `nestfit_amd.nested`, the twin, one
state and the stages `_begin`, `_refit`, `_propose`, `_update_reject`, `_walk_step`, `_replace`, `_chunk_kr` named after
the device's) and `run_nested_device` here (state and per-round logic on the GPU, csrc/nfa_sampler.h); they share
their conventions (`nested._conventions`) and a counter-based random stream, so the same seed gives the same run.
This module drives the device sampler and holds the reference-shaped front end: `Dumper`, `run_multinest`, `fit_pixels`.

This is not MultiNest: the random streams differ and the decomposition into ellipsoids is a simpler one
(principal-axis cuts kept by a volume test; none above six sampled dimensions, where constrained walks take
over), so evidences agree with a MultiNest run only within their sampling error.  What can be checked
bit-for-bit is the likelihood it is fed (tests drive the same sampler with the CPU oracle).
"""
import ctypes as C
import time

import numpy as np

from . import _ffi
from .nested import _NS_ME, LOG_ZERO, PRECISION, NestedResult, _conventions, default_cap_iter, resolve_precision, run_nested  # noqa: F401


def _assemble_packed(nlive, n_iter, n_evals, off, table, tol, stats):
    """`_assemble` for tables the device has laid out and weighted (nfa_sampler_posterior_packed): rows off[p] .. off[p + 1]
    of `table` are pixel p's dead points followed by its live points, columns theta, -2 lnL, weight; `stats` holds what
    the device has formed of them (evidence, information, moments: `NestedResult.from_stats`)."""
    results = []
    for p in range(len(n_iter)):
        nl = int(nlive[p])
        r = NestedResult.from_stats(table[off[p]:off[p + 1]], stats[p], nl, n_evals[p], n_iter[p])
        if tol is not None:
            remain = stats[p, 4] - n_iter[p] / nl
            # (the live rows' -2 lnL: all equal = a plateau, a finished run -- `nested._plateau`)
            live = table[off[p + 1] - nl:off[p + 1], -2]
            r.truncated = bool(not (np.logaddexp(stats[p, 1], remain) - stats[p, 1] < tol) and not live.max() == live.min())
        results.append(r)
    return results


def run_nested_device(runner, pix, nlive=400, tol=0.5, efr=0.3, seed=-1, maxiter=int(1e6), n_cand=None,
                      upd_frac=0.1, log_zero=LOG_ZERO, cap_iter=None, check_every=32, batch_target=262144,
                      enlarge=1.5, method='auto', n_steps=None, free_mask=None, progress=None, time_limit=None,
                      ellipsoids=None, frames=None, margin=None, shear=None, pairs=None, precision=None):
    """The same algorithm with its whole state on the GPU (``nfa_sampler_*``): pixels `pix` of a
    `CubeRunner` (or pixel 0 of a single-pixel runner) in lock-step rounds, no per-round host
    work.  Options as `run_nested`; `cap_iter` defaults to min(maxiter, 60 nlive).  `progress`
    (callable(n_active, rounds)) is called about once a second; after `time_limit` seconds the
    pixels still running are stopped where they are (their results are then lower bounds)."""
    lib = _ffi.engine()
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    P, ndim = int(pix.size), int(runner.ndim)
    assert tol > 0 and maxiter >= 0
    fm = None if free_mask is None else np.ascontiguousarray(free_mask, dtype=np.int32)
    assert fm is None or fm.shape == (ndim,)
    # the conventions of the twin (live points one number, or one per pixel: nfa_sampler_set_pixel_nlive, one lock-step
    # group all the same)
    cv = _conventions(P, ndim, nlive, efr, n_cand, upd_frac, seed, method, n_steps, fm, precision, margin, pairs, shear)
    nl, margin, pairs, shear = cv.nl, cv.margin, cv.pairs, cv.shear
    # dead-point slots: the device allocates them, so at least one, and a given cap_iter as it is (the twin keeps lists
    # and clips to maxiter: nested._begin)
    capp = np.array([int(cap_iter) if cap_iter else int(max(1, min(maxiter, default_cap_iter(int(n))))) for n in nl], dtype=np.int64)
    h = C.c_void_p()
    _ffi.check(lib.nfa_sampler_create(C.byref(h), runner._run.handle, pix.ctypes.data_as(_ffi._ip), P,
                                      cv.nlive, cv.K, int(batch_target), int(capp.max()),
                                      None if fm is None else fm.ctypes.data_as(_ffi._ip)))
    try:
        if ellipsoids:
            _ffi.check(lib.nfa_sampler_set_ellipsoids(h, int(ellipsoids)))
        if frames is not None or margin is not None:
            _ffi.check(lib.nfa_sampler_set_boxes(h, -2 if frames is None else int(frames), 0.0 if margin is None else float(margin)))
        if shear is not None:
            _ffi.check(lib.nfa_sampler_set_shear(h, float(shear)))
        if pairs is not None:
            _ffi.check(lib.nfa_sampler_set_pairs(h, float(pairs)))
        if (nl != nl[0]).any():
            nl32, upd32 = nl.astype(np.int32), cv.updp.astype(np.int32)
            _ffi.check(lib.nfa_sampler_set_pixel_nlive(h, nl32.ctypes.data_as(_ffi._ip), capp.ctypes.data_as(_ffi._lp),
                                                       upd32.ctypes.data_as(_ffi._ip)))
        _ffi.check(lib.nfa_sampler_begin(h, float(tol), float(efr), cv.seed, int(maxiter), int(cv.updp.max()), float(log_zero),
                                         int(check_every), float(enlarge), cv.method, cv.n_steps))
        n_active = C.c_int64(P)
        t0 = time.perf_counter()
        t_created = t0
        chunks = 16
        while True:
            t1 = time.perf_counter()
            _ffi.check(lib.nfa_sampler_advance(h, chunks, C.byref(n_active)))
            if n_active.value == 0:
                break
            dt = time.perf_counter() - t1
            chunks = int(min(4096, max(1, chunks * (1.0 / max(dt, 1e-3)))))     # about a second per call
            if progress is not None:
                progress(int(n_active.value), None)
                if hasattr(progress, 'counts'):                                  # (debugging aid: the counters, chunk by chunk)
                    ni, ne, rr = np.empty(P, dtype=np.int64), np.empty(P, dtype=np.int64), C.c_int64()
                    _ffi.check(lib.nfa_sampler_counts(h, ni.ctypes.data_as(_ffi._lp), ne.ctypes.data_as(_ffi._lp), C.byref(rr)))
                    chunks = progress.counts(ni, ne, int(rr.value)) or chunks
            if time_limit is not None and time.perf_counter() - t0 > time_limit:
                break
        t_rounds = time.perf_counter()
        n_iter = np.empty(P, dtype=np.int64)
        n_evals = np.empty(P, dtype=np.int64)
        rounds = C.c_int64()
        _ffi.check(lib.nfa_sampler_counts(h, n_iter.ctypes.data_as(_ffi._lp), n_evals.ctypes.data_as(_ffi._lp),
                                          C.byref(rounds)))
        # every pixel's table of posterior samples, laid out by the device (dead points, then live points; theta, -2 lnL,
        # ln(prior mass x likelihood)): one copy, and a pixel's table is a view into it
        n_dead = np.minimum(n_iter, capp)
        off = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(n_dead + nl, out=off[1:])
        live_off = -n_iter / nl - np.log(nl)
        table = np.empty((int(off[-1]), ndim + 2))
        stats = np.empty((P, 6 + 4 * ndim))
        _ffi.check(lib.nfa_sampler_posterior_packed(h, off.ctypes.data_as(_ffi._lp), _ffi.dptr(live_off), _ffi.dptr(table), _ffi.dptr(stats)))
    finally:
        lib.nfa_sampler_destroy(h)
    t_read = time.perf_counter()
    res = _assemble_packed(nl, n_iter, n_evals, off, table, tol, stats)
    for r in res:
        r.rounds = int(rounds.value)
    # where the call's time went (seconds): the rounds on the device, the read-back of live and dead points, the assembly of
    # the results on the host
    res[0].timings = {'rounds': t_rounds - t_created, 'read_back': t_read - t_rounds, 'assemble': time.perf_counter() - t_read}
    return res


# ---------------------------------------------------------------------------
#  reference-shaped front end: Dumper + run_multinest (core.pyx:564-823)
# ---------------------------------------------------------------------------
class MemoryGroup:
    """Minimal stand-in for an ``h5py.Group`` (attrs + datasets) when h5py is absent."""

    class _File:
        def flush(self):
            pass

    def __init__(self):
        self.attrs = {}
        self.datasets = {}
        self.file = MemoryGroup._File()

    def create_dataset(self, name, data=None):
        self.datasets[name] = np.array(data)
        return self.datasets[name]

    def __getitem__(self, name):
        return self.datasets[name]


# What a finished run leaves in its store group (docs/store_spec.rst:77-96; the reference's writer is
# mn_dump, core.pyx:627-687).  Every entry: name in the store <- function of (runner, result, dumper).
def information_criteria(n_chan, n_par, lnL):
    """(BIC, AIC, AICc) of a model with `n_par` parameters on `n_chan` channels at log-likelihood lnL."""
    n, k = float(n_chan), float(n_par)
    aic = 2.0 * k - 2.0 * lnL
    return np.log(n) * k - 2.0 * lnL, aic, aic + (2.0 * k * k + 2.0 * k) / (n - k - 1.0)


def _criteria(prefix, which_lnL):
    names = (prefix + 'BIC', prefix + 'AIC', prefix + 'AICc')

    def make(k):
        return lambda run, res, dmp: information_criteria(run.n_chan_tot, run.n_params, which_lnL(run, res))[k]
    return tuple((name, make(k)) for k, name in enumerate(names))


RUN_ATTRIBUTES = (
    ('ncomp', lambda run, res, dmp: run.ncomp),
    ('null_lnZ', lambda run, res, dmp: run.null_lnZ),
    ('n_chan_tot', lambda run, res, dmp: run.n_chan_tot),
    ('n_samples', lambda run, res, dmp: res.n_samples),
    ('n_live', lambda run, res, dmp: res.n_live),
    ('n_params', lambda run, res, dmp: res.n_params),
    ('global_lnZ', lambda run, res, dmp: res.lnZ),
    ('global_lnZ_err', lambda run, res, dmp: res.lnZ_err),
    ('max_loglike', lambda run, res, dmp: res.max_loglike),
    ('marg_cols', lambda run, res, dmp: dmp.marginal_cols),
    ('marg_quantiles', lambda run, res, dmp: dmp.quantiles),
) + _criteria('', lambda run, res: res.max_loglike) + _criteria('null_', lambda run, res: run.null_lnZ) + (
    ('truncated', lambda run, res, dmp: bool(getattr(res, 'truncated', False))),     # not in the reference: see NestedResult
)
RUN_DATASETS = (
    ('posteriors', lambda run, res, dmp: res.posterior.astype('float32')),           # (n_samples, n_params + 2)
    ('marginals', lambda run, res, dmp: dmp.calc_marginals(res.posterior)),          # (n_quantiles, n_params)
    ('bestfit_params', lambda run, res, dmp: res.param_constr[2]),
    ('map_params', lambda run, res, dmp: res.param_constr[3]),
)


def marginal_quantile_table():
    """(column names, quantiles) of the `marginals` dataset: extremes and percentiles, then the 1 / 2 / 3
    sigma credible intervals.  The reference stores the normal tail areas truncated to nine significant
    digits below and eight decimals above the median (its marg_quantiles attribute): reproduced here from
    the normal distribution, not typed in."""
    from scipy.stats import norm
    percent = (1, 10, 25, 50, 75, 90, 99)
    names = ['min'] + [f'p{q:02d}' for q in percent] + ['max']
    quant = [0.0] + [q / 100 for q in percent] + [1.0]
    for k in (1, 2, 3):
        names += [f'{k}s_lo', f'{k}s_hi']
        quant += [float(f'{norm.cdf(-k):.8e}'), float(f'{norm.cdf(k):.8f}')]
    return names, np.array(quant)


class Dumper:
    """Writer of one run's outputs into a store group (an h5py group, a `store.Group` or a
    `MemoryGroup`), with the reference's entry points (core.pyx:564-612)."""

    def __init__(self, group, no_dump=False):
        self.group, self.no_dump = group, no_dump
        self.n_calls, self.n_samples = 0, -1
        self.marginal_cols, self.quantiles = marginal_quantile_table()

    def calc_marginals(self, posteriors):
        """Quantiles of every parameter column (the two trailing columns are -2 lnL and the weights):
        `np.quantile(columns, quantiles, axis=0)` of the reference's Dumper (core.pyx:596-598), bit for bit, from
        one sort of the columns and numpy's own interpolation rule (a + (b - a) t, from the upper side for
        t >= 1/2) -- a map has tens of thousands of runs and the general routine costs six times as much per run."""
        n_par = posteriors.shape[1] - 2
        a = np.asarray(posteriors[:, :n_par], dtype=np.float64)
        n = a.shape[0]
        if n == 0 or np.isnan(a).any():
            return np.quantile(a, self.quantiles, axis=0)
        q = np.asarray(self.quantiles, dtype=np.float64)
        s = np.sort(a, axis=0)
        virtual = (n - 1) * q
        below = np.floor(virtual).astype(np.intp)
        above = np.minimum(below + 1, n - 1)
        t = (virtual - below)[:, None]
        lo, hi = s[below], s[above]
        step = hi - lo
        out = lo + step * t
        upper = (t >= 0.5)[:, 0]
        out[upper] = hi[upper] - step[upper] * (1 - t[upper])
        return out

    def flush(self):
        self.group.file.flush()

    def append_attributes(self, **attributes):
        self.group.attrs.update(attributes)

    def append_datasets(self, **datasets):
        for name in datasets:
            self.group.create_dataset(name, data=datasets[name])

    def dump(self, runner, res):
        """The final call of the sampler's dump callback: evidence into the runner, everything of
        RUN_ATTRIBUTES / RUN_DATASETS into the group."""
        self.n_calls += 1
        self.n_samples = res.n_samples
        runner.run_lnZ = res.lnZ
        if self.no_dump:
            return
        self.append_attributes(**{name: get(runner, res, self) for name, get in RUN_ATTRIBUTES})
        self.append_datasets(**{name: get(runner, res, self) for name, get in RUN_DATASETS})


def run_multinest(runner, dumper, IS=False, mmodal=True, ceff=False, nlive=400, tol=0.5, efr=0.3,
                  nClsPar=None, maxModes=100, updInt=10, Ztol=-1e90, root='results', seed=-1,
                  pWrap=None, fb=False, resume=False, initMPI=False, outfile=False, logZero=-1e100,
                  maxiter=int(1e6), precision=None):
    """Signature of the reference's ``run_multinest`` (core.pyx:727-823) on the built-in sampler,
    for one runner (one pixel).  `mmodal` / `maxModes`: clusters of live points get bounding ellipsoids of
    their own (at most min(maxModes, 4), and only where at most six dimensions are sampled; mmodal = False: one
    ellipsoid); the evidence is the global one either way (the reference's dumper stores no per-mode values).
    Options that concern importance sampling, constant efficiency, the clustering parameters or MultiNest's output
    files are accepted and ignored; the argument checks are the reference's.  `precision` (not MultiNest's): the
    built-in sampler's named setting, `PRECISION`."""
    assert runner.ndim > 0
    assert nlive > 0
    assert tol > 0
    assert 0 < efr <= 1
    assert maxModes > 0
    assert updInt > 0
    assert Ztol is not None and np.isfinite(Ztol)
    assert logZero is not None and np.isfinite(logZero)
    assert maxiter >= 0
    if nClsPar is None:
        nClsPar = runner.n_params
    if nClsPar > runner.n_params:
        raise ValueError('Number of clustering parameters must be less than total.')

    utrans = getattr(runner, 'utrans', None)
    free_mask = utrans.free_mask(runner.ncomp) if hasattr(utrans, 'free_mask') else None
    ellipsoids = min(int(maxModes), _NS_ME) if mmodal else 1
    if hasattr(runner, '_run'):          # engine runner: the whole run stays on the device
        res = run_nested_device(runner, np.zeros(1, dtype=np.int32), nlive=nlive, tol=tol, efr=efr, seed=seed,
                                maxiter=maxiter, log_zero=logZero, free_mask=free_mask, ellipsoids=ellipsoids, precision=precision)[0]
    else:                                # any object with loglikelihood_batch(U): the numpy twin
        def loglike(pix, U):
            return runner.loglikelihood_batch(U)

        res = run_nested(loglike, runner.ndim, 1, nlive=nlive, tol=tol, efr=efr, seed=seed,
                         maxiter=maxiter, log_zero=logZero, free_mask=free_mask, ellipsoids=ellipsoids, precision=precision)[0]
    dumper.dump(runner, res)
    return res


def fit_pixels(cube_runner, pix, nlive=400, tol=0.5, efr=0.3, seed=-1, maxiter=int(1e6), device=True,
               **kwargs):
    """All pixels `pix` of a `CubeRunner` in one lock-step run; returns a list of NestedResult.
    device=True keeps the sampler state on the GPU (`run_nested_device`); device=False runs the
    host twin and sends only the likelihood batches to the GPU."""
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    if 'free_mask' not in kwargs and getattr(cube_runner, 'utrans', None) is not None:
        kwargs['free_mask'] = cube_runner.utrans.free_mask(cube_runner.ncomp)   # dummies are not sampled
    if device:
        return run_nested_device(cube_runner, pix, nlive=nlive, tol=tol, efr=efr, seed=seed,
                                 maxiter=maxiter, **kwargs)

    def loglike(k, U):
        return cube_runner.loglikelihood_batch(pix[k], U)

    return run_nested(loglike, cube_runner.ndim, pix.size, nlive=nlive, tol=tol, efr=efr, seed=seed,
                      maxiter=maxiter, **kwargs)
