"""Everything a device run hands back besides lnZ and the table: the statistics `ns_finish_kernel` forms of a pixel's
table (`NestedResult.from_stats`: information, largest lnL of all and of the live points, dead-only lnZ, weight sum,
moments, best-fit and MAP rows, the arg-max tie rule) and the read-back entry points nobody called (`nfa_sampler_run`,
`nfa_sampler_dead`, `nfa_sampler_dead_packed`, `nfa_sampler_live`, `nfa_sampler_posterior_packed` without `stats`).

The reference is `reference_result`: `np.longdouble` arithmetic on a pixel's RAW table (last column still ln(prior mass x
likelihood), as `nfa_sampler_posterior_packed` gives it with stats = NULL).  The kernel's table with weights and its
statistics are compared against it, never the other way round.  The tolerance is not typed in: the numpy double path
(`nested._assemble` -> `NestedResult`) is measured against the same reference on the same tables and the device gets four
times its error, with a floor of 1e-13 of the quantity's scale -- 256 threads sum in another order, not worse.  Scales:
the quantity's own size; for H, |H| + |lnZ| (H = sum w (L - lnZ) moves by whatever rounding lnZ carries); for a
mean, sum w |t|.

Measured on an MI355X, worst over the cases below, device / numpy, in units of the scale: weights 1.6e-14 / 1.6e-14 and
weight sum and mean the same (all three carry lnZ's rounding, 1e-16 of |lnZ| ~ 150, as a common factor); lnZ 1.2e-16 / 1.2e-16;
dead lnZ 9.4e-17 / 9.4e-17; H 1.5e-15 / 1.5e-15; std 2.2e-12 / 2.2e-12 at vsys = 1e4 km/s and below 2e-14 on both sides
in every other case but one: 'buffer full', 9.4e-13 / 2.4e-13.  There one live point of pixel 1 carries all the weight but
4e-16, the spread is 5e-9 about a mean of 14.5, and what is left of it after the mean has been rounded to a double is
(ulp(mean))^2 / variance ~ 1e-12 on either side: 3.99 times numpy's, inside the rule by rounding luck, not by margin.
Everywhere else the device is within 1.05 of numpy's error (the two lnZ errors are equal to three digits in every case)."""
import contextlib
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest

from nestfit_amd import _ffi, nested, sampler
from nestfit_amd.synth import CKMS, NU0
from test_sibling_models import _simple_priors

pytestmark = pytest.mark.gpu

N_CHAN, NOISE, TOL, EFR = 128, 0.15, 0.5, 0.3
FLOOR = 1e-13
# The reference and numpy's double path are two correct implementations and must agree as such: the worst-conditioned
# number of these cases is the velocity spread at vsys = 1e4 km/s (|mean| / sigma up to 1e6: 2^-53 x 1e6 = 1.1e-10), all
# else is a sum of fewer than 2000 terms of one sign, or moves with lnZ's rounding (|lnZ| < 1e3: 1e-13).  Without this the
# four-times rule could not see a wrong reference: both sides would be equally far from it.
NUMPY_CEILING = 1e-10


# ---------------------------------------------------------------------------- the reference
def reference_result(table_with_ln_weights, n_dead, nlive, n_iter, tol):
    """What a result holds, from a pixel's raw table [n_dead dead rows, then nlive live rows; theta, -2 lnL, ln(prior mass
    x likelihood)], in np.longdouble.  `mean` is sum w t and `var` sum w (t - mean)^2 (the weights add up to one to
    rounding, and nothing divides by their sum: `NestedResult`); `ibest` / `imap` are the FIRST rows of the largest lnL and
    of the largest weight; `truncated` as `nested._assemble` has it (not on a plateau, `nested._plateau`)."""
    ld = np.longdouble
    raw = np.asarray(table_with_ln_weights)
    L = -0.5 * raw[:, -2]                                   # (exact in doubles)
    lw, th = raw[:, -1].astype(ld), raw[:, :-2].astype(ld)

    def lse(x):
        if x.size == 0:
            return ld(-np.inf)
        m = x.max()
        return m if not np.isfinite(m) else m + np.log(np.exp(x - m).sum())
    lnz_dead, lnz_live = lse(lw[:n_dead]), lse(lw[n_dead:])
    lnz = lnz_live if lnz_dead == -np.inf else np.logaddexp(lnz_dead, lnz_live)
    w = np.exp(lw - lnz)
    pos = w > 0
    r = types.SimpleNamespace(lnZ=lnz, lnZ_dead=lnz_dead, weights=w, wsum=w.sum(), max_L=L.max(), max_live_L=L[n_dead:].max())
    r.H = (w[pos] * (L[pos].astype(ld) - lnz)).sum()
    r.H_scale = abs(r.H) + abs(lnz)
    r.mean = (w[:, None] * th).sum(axis=0)
    r.mean_scale = (w[:, None] * np.abs(th)).sum(axis=0)
    r.var = (w[:, None] * (th - r.mean) ** 2).sum(axis=0)
    r.ibest, r.imap = int(np.argmax(L)), int(np.argmax(raw[:, -1]))         # (np.argmax: the first among equals)
    live_L = L[n_dead:]
    remain = ld(r.max_live_L) - ld(n_iter) / ld(nlive)
    met = lnz_dead != -np.inf and (np.logaddexp(lnz_dead, remain) - lnz_dead < tol)
    r.truncated = bool(not met and not live_L.max() == live_L.min())
    return r


def _rel(got, ref, scale):
    """Largest |got - ref| in units of `scale` (a scale of zero: the absolute error, which must then be zero itself)."""
    got, ref, scale = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble), np.abs(np.asarray(scale, dtype=np.longdouble))
    same = (got == ref)                                                         # (-inf = -inf: no error)
    with np.errstate(invalid='ignore'):
        err = np.where(same, 0.0, np.abs(got - ref) / np.where(scale > 0, scale, 1.0))
    return float(np.max(err))


def _errors(ref, lnZ, lnZ_dead, H, weights, mean, std):
    """The seven compared quantities of one pixel against the reference, each in units of its scale."""
    rstd = np.sqrt(ref.var)
    return {'weights': _rel(weights, ref.weights, ref.weights.max()), 'lnZ': _rel(lnZ, ref.lnZ, ref.lnZ),
            'dead lnZ': _rel(lnZ_dead, ref.lnZ_dead, ref.lnZ_dead if np.isfinite(ref.lnZ_dead) else 1.0),
            'H': _rel(H, ref.H, ref.H_scale), 'weight sum': _rel(np.asarray(weights).sum(), ref.wsum, 1.0),
            'mean': _rel(mean, ref.mean, ref.mean_scale), 'std': _rel(std, rstd, rstd)}


def _numpy_path(raw, dead_lnw, n_dead, nlive, n_iter, tol):
    """The host's double-precision result of the same table: `nested._assemble` (and through it `NestedResult`), fed the
    dead points' own ln w and the live rows; its dead-only lnZ by `_assemble`'s log_sum_exp, restated."""
    ndim = raw.shape[1] - 2
    L = -0.5 * raw[:, -2]
    dead = [(raw[:n_dead, :ndim], L[:n_dead], dead_lnw)]
    res = nested._assemble(ndim, np.array([nlive]), np.array([n_iter]), np.array([0]), dead, [raw[n_dead:, :ndim]], [L[n_dead:]], tol)[0]
    lw = dead_lnw + L[:n_dead]
    res.lnZ_dead = -np.inf if n_dead == 0 else float(lw.max() + math.log(np.exp(lw - lw.max()).sum()))
    return res


def check_tables(data, reference=reference_result, report=print):
    """The pure-numpy part of a case: `data` holds what came off the device (raw tables, tables with weights, statistics,
    the dead points' ln w, offsets, counts), `reference` the helper to hold it against.  Returns the worst errors
    (device, numpy) per quantity."""
    ndim = data.raw.shape[1] - 2
    worst_dev, worst_np = {}, {}
    for p in range(len(data.n_iter)):
        a, b, nl = int(data.off[p]), int(data.off[p + 1]), int(data.nl[p])
        n_dead = b - a - nl
        raw, tab, st = data.raw[a:b], data.weighted[a:b], data.stats[p]
        ref = reference(raw, n_dead, nl, int(data.n_iter[p]), data.tol)
        dev = nested.NestedResult.from_stats(tab, st, nl, int(data.n_evals[p]), int(data.n_iter[p]))
        # bit for bit: the largest lnL of all and of the live points, the rows of the first arg-maxima, everything but the weights
        assert st[3] == ref.max_L and st[4] == ref.max_live_L, (p, st[3], ref.max_L, st[4], ref.max_live_L)
        assert np.array_equal(dev.param_constr[2], raw[ref.ibest, :ndim]), (p, 'best-fit row', ref.ibest)
        assert np.array_equal(dev.param_constr[3], raw[ref.imap, :ndim]), (p, 'MAP row', ref.imap)
        assert np.array_equal(tab[:, :-1], raw[:, :-1])
        assert bool(data.truncated[p]) == ref.truncated, (p, data.truncated[p], ref.truncated)
        host = _numpy_path(raw, data.dead_lnw[p], n_dead, nl, int(data.n_iter[p]), data.tol)
        assert host.truncated == ref.truncated
        e_dev = _errors(ref, st[0], st[1], st[2], tab[:, -1], dev.param_constr[0], dev.param_constr[1])
        e_np = _errors(ref, host.lnZ, host.lnZ_dead, host.information, host.posterior[:, -1], host.param_constr[0], host.param_constr[1])
        for k in e_dev:
            worst_dev[k], worst_np[k] = max(worst_dev.get(k, 0.0), e_dev[k]), max(worst_np.get(k, 0.0), e_np[k])
    for k in worst_dev:
        report(f'    {data.name:>12s} {k:>10s}: device {worst_dev[k]:.2e}, numpy {worst_np[k]:.2e} (of the scale)')
    for k in worst_dev:
        assert worst_np[k] <= NUMPY_CEILING, (data.name, k, 'numpy against the reference', worst_np[k])
        assert worst_dev[k] <= max(4.0 * worst_np[k], FLOOR), (data.name, k, worst_dev[k], worst_np[k])
    return worst_dev, worst_np


# ---------------------------------------------------------------------------- device runs kept open
@contextlib.contextmanager
def device_run(cube, pix, nlive, seed, tol=TOL, efr=EFR, maxiter=int(1e6), cap_iter=None, one_call=False, time_limit=20.0):
    """A device run as `sampler.run_nested_device` makes it (same conventions, same calls), its handle still open:
    `one_call` = through nfa_sampler_run (method 1, 10 nd steps, enlarge 1.5) instead of begin + advance."""
    import time
    lib = _ffi.engine()
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    P, ndim = int(pix.size), int(cube.ndim)
    fm = np.ascontiguousarray(cube.utrans.free_mask(cube.ncomp), dtype=np.int32)
    cv = nested._conventions(P, ndim, nlive, efr, None, 0.1, seed, 'auto', None, fm, None, None, None, None)
    capp = np.array([int(cap_iter) if cap_iter else int(max(1, min(maxiter, nested.default_cap_iter(int(n))))) for n in cv.nl], dtype=np.int64)
    h = C.c_void_p()
    _ffi.check(lib.nfa_sampler_create(C.byref(h), cube._run.handle, pix.ctypes.data_as(_ffi._ip), P, cv.nlive, cv.K, 262144,
                                      int(capp.max()), fm.ctypes.data_as(_ffi._ip)))
    try:
        if (cv.nl != cv.nl[0]).any():
            nl32, upd32 = cv.nl.astype(np.int32), cv.updp.astype(np.int32)
            _ffi.check(lib.nfa_sampler_set_pixel_nlive(h, nl32.ctypes.data_as(_ffi._ip), capp.ctypes.data_as(_ffi._lp), upd32.ctypes.data_as(_ffi._ip)))
        if one_call:
            _ffi.check(lib.nfa_sampler_run(h, float(tol), float(efr), cv.seed, int(maxiter), int(cv.updp.max()), nested.LOG_ZERO, 32))
        else:
            _ffi.check(lib.nfa_sampler_begin(h, float(tol), float(efr), cv.seed, int(maxiter), int(cv.updp.max()), nested.LOG_ZERO, 32,
                                             1.5, cv.method, cv.n_steps))
            n_active, t0 = C.c_int64(P), time.perf_counter()
            while True:
                _ffi.check(lib.nfa_sampler_advance(h, 16, C.byref(n_active)))
                if n_active.value == 0:
                    break
                assert time.perf_counter() - t0 < time_limit, 'the device run did not end'
        run = types.SimpleNamespace(lib=lib, h=h, P=P, ndim=ndim, nl=cv.nl, nlive=cv.nlive, capp=capp, tol=tol)
        run.n_iter, run.n_evals = np.empty(P, dtype=np.int64), np.empty(P, dtype=np.int64)
        _ffi.check(lib.nfa_sampler_counts(h, run.n_iter.ctypes.data_as(_ffi._lp), run.n_evals.ctypes.data_as(_ffi._lp), None))
        run.n_dead = np.minimum(run.n_iter, capp)
        run.off = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(run.n_dead + cv.nl, out=run.off[1:])
        run.live_off = -run.n_iter / cv.nl - np.log(cv.nl)
        yield run
    finally:
        lib.nfa_sampler_destroy(h)


def posterior_tables(run, with_stats):
    """nfa_sampler_posterior_packed: the raw tables (stats = NULL), or the tables with weights and the statistics."""
    table = np.full((int(run.off[-1]), run.ndim + 2), np.nan)
    stats = np.full((run.P, 6 + 4 * run.ndim), np.nan) if with_stats else None
    _ffi.check(run.lib.nfa_sampler_posterior_packed(run.h, run.off.ctypes.data_as(_ffi._lp), _ffi.dptr(run.live_off), _ffi.dptr(table),
                                                    _ffi.dptr(stats) if with_stats else None))
    return table, stats


def dead_points(run, p, n):
    theta, lnL, lnw = np.full((n, run.ndim), np.nan), np.full(n, np.nan), np.full(n, np.nan)
    _ffi.check(run.lib.nfa_sampler_dead(run.h, p, n, _ffi.dptr(theta), _ffi.dptr(lnL), _ffi.dptr(lnw)))
    return theta, lnL, lnw


def dead_points_packed(run, counts):
    off = np.zeros(run.P + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    n = int(off[-1])
    theta, lnL, lnw = np.full((max(n, 1), run.ndim), np.nan), np.full(max(n, 1), np.nan), np.full(max(n, 1), np.nan)
    _ffi.check(run.lib.nfa_sampler_dead_packed(run.h, off.ctypes.data_as(_ffi._lp), _ffi.dptr(theta), _ffi.dptr(lnL), _ffi.dptr(lnw)))
    return off, theta[:n], lnL[:n], lnw[:n]


# ---------------------------------------------------------------------------- the cubes
def _axis(trans, vsys):
    return NU0[trans] * (1.0 - (vsys + np.linspace(30.0, -30.0, N_CHAN)) / CKMS)


@functools.lru_cache(maxsize=None)
def _nh3_cube(n_pix, seed, vsys=0.0, identical=False):
    """NH3 (1,1)+(2,2), one component, 128 channels each: a model at a drawn truth plus noise per pixel (`identical`: every
    pixel the data of the first).  Made and sampled in table mode."""
    import nestfit_amd as engine
    from nestfit_amd.cube import CubeRunner
    rng = np.random.default_rng(seed)
    axes = [_axis(1, vsys), _axis(2, vsys)]
    ut = engine.get_irdc_priors(size=300, vsys=vsys)
    truths = np.stack([vsys + rng.uniform(-1, 1, n_pix), rng.uniform(10, 18, n_pix), rng.uniform(4, 8, n_pix), rng.uniform(14.2, 14.8, n_pix),
                       rng.uniform(0.3, 0.8, n_pix), np.zeros(n_pix)], axis=1)
    probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * N_CHAN)), np.full((1, 2), NOISE), ut, ncomp=1)
    model, _ = probe.predict_batch(np.zeros(n_pix, dtype=np.int32), truths)
    data = model + rng.normal(0, NOISE, model.shape)
    if identical:
        data[:] = data[0]
    return CubeRunner(axes, (1, 2), data, np.full((n_pix, 2), NOISE), ut, ncomp=1)


@functools.lru_cache(maxsize=None)
def _off_band_cube(n_pix, seed):
    """A Gaussian-model cube whose prior velocities, 200 .. 230 km/s, lie wholly off the band of +-20 km/s (a line is cut
    at five widths, at most 15 km/s): the model is exactly zero for every draw and lnL one constant per pixel."""
    import nestfit_amd as engine
    from nestfit_amd.cube import CubeRunner
    nu0 = 110.201354e9
    x = nu0 * (1.0 - np.linspace(20, -20, N_CHAN) / CKMS)
    data = np.random.default_rng(seed).normal(0, NOISE, (n_pix, N_CHAN))
    ut = _simple_priors(engine, [(200.0, 230.0), (0.2, 3.0), (0.0, 5.0)])
    return CubeRunner([x], [1], data, np.full((n_pix, 1), NOISE), ut, ncomp=1, model=2, rest_freqs=[nu0])


# name: (cube, its arguments, pixels, options of the run)
CASES = {
    'finished': (_nh3_cube, (3, 21), 3, dict(nlive=60, seed=33)),
    'maxiter 0': (_nh3_cube, (3, 21), 3, dict(nlive=60, seed=33, maxiter=0)),
    'buffer full': (_nh3_cube, (3, 21), 3, dict(nlive=40, seed=3, cap_iter=30)),
    'own nlive': (_nh3_cube, (3, 21), 3, dict(nlive=(60, 71, 83), seed=33)),
    '8 rows': (_nh3_cube, (3, 21), 3, dict(nlive=8, seed=5, maxiter=0)),                 # nlive = ndim + 2, the smallest there is
    '256 rows': (_nh3_cube, (3, 21), 3, dict(nlive=100, seed=5, maxiter=156)),
    '400 rows': (_nh3_cube, (3, 21), 3, dict(nlive=100, seed=5, maxiter=300)),
    'vsys 1e4': (_nh3_cube, (4, 22, 1e4), 4, dict(nlive=60, seed=9)),
    'identical': (_nh3_cube, (2, 23, 0.0, True), 2, dict(nlive=60, seed=11)),
    'plateau': (_off_band_cube, (2, 24), 2, dict(nlive=50, seed=1, maxiter=200)),
}


@functools.lru_cache(maxsize=None)
def run_case(name):
    """One case, run once for every test that looks at it: the device's tables and statistics (a run kept open), the
    device's results through the front end, the twin's results."""
    import nestfit_amd as engine
    make, args, n_pix, opts = CASES[name]
    opts = dict(opts)
    if isinstance(opts['nlive'], tuple):
        opts['nlive'] = np.array(opts['nlive'])
    try:
        engine.set_exp_mode('table')
        cube = make(*args)
        pix = np.arange(n_pix)
        data = types.SimpleNamespace(name=name, tol=TOL, cube=cube)
        with device_run(cube, pix, **opts) as run:
            data.raw, _ = posterior_tables(run, False)
            data.weighted, data.stats = posterior_tables(run, True)
            data.dead_lnw = [dead_points(run, p, int(run.n_dead[p]))[2] for p in range(n_pix)]
            data.off, data.nl, data.n_iter, data.n_evals, data.n_dead = run.off, run.nl, run.n_iter, run.n_evals, run.n_dead
        kw = dict(tol=TOL, efr=EFR, **opts)
        data.dev = sampler.fit_pixels(cube, pix, device=True, time_limit=20, **kw)
        data.twin = sampler.fit_pixels(cube, pix, device=False, **kw)
        data.truncated = [r.truncated for r in data.dev]
    finally:
        engine.set_exp_mode('fast')
    return data


# ---------------------------------------------------------------------------- A: the statistics
@pytest.mark.parametrize('name', list(CASES))
def test_statistics_of_the_device_against_the_longdouble_reference(engine, name):
    """stats[p] and the weights of `ns_finish_kernel` against `reference_result` of the raw table; the sums within four
    times the numpy double path's own error (floor 1e-13), the rest bit for bit.  Measured: the module's docstring."""
    data = run_case(name)
    for p, r in enumerate(data.dev):                 # the front end's tables are the ones looked at here
        assert np.array_equal(r.posterior, data.weighted[data.off[p]:data.off[p + 1]])
        assert (r.n_iter, r.n_evals) == (data.n_iter[p], data.n_evals[p])
    rows = sorted({int(n) for n in np.diff(data.off)})
    print(f'\n{name}: rows per pixel {rows}, n_iter {data.n_iter.tolist()}')
    check_tables(data)
    if name == 'maxiter 0':
        assert (data.n_dead == 0).all() and (data.stats[:, 1] == -np.inf).all() and all(data.truncated)
    if name == 'buffer full':
        assert (data.n_iter == 30).all() and all(data.truncated)
    if name in ('8 rows', '256 rows', '400 rows'):
        assert rows == [int(name.split()[0])]
    if name in ('finished', 'own nlive', 'vsys 1e4', 'identical'):
        assert not any(data.truncated) and min(rows) > 256
    if name == 'vsys 1e4':                           # |mean| >> sigma in the velocity column
        assert all(r.param_constr[0][0] > 9990 and r.param_constr[1][0] < 0.5 for r in data.dev)
    if name == 'plateau':                            # done before the first round; every row ties with every other: row 0 wins
        lnL = -0.5 * data.raw[:, -2]
        for p, r in enumerate(data.dev):
            a, b = data.off[p], data.off[p + 1]
            assert r.n_iter == 0 and not r.truncated and (lnL[a:b] == lnL[a]).all()
            assert r.lnZ == pytest.approx(lnL[a], rel=1e-14) and abs(r.information) < 1e-9
            assert np.array_equal(r.param_constr[2], data.raw[a, :-2]) and np.array_equal(r.param_constr[3], data.raw[a, :-2])


@pytest.mark.parametrize('name', list(CASES))
def test_every_field_of_a_device_result_is_the_twins(engine, name):
    """`fit_pixels(device=True)` against `fit_pixels(device=False)`, same seed: not lnZ and the table alone."""
    data = run_case(name)
    for d, t in zip(data.dev, data.twin):
        assert (d.n_iter, d.n_evals, d.n_samples, d.n_live, d.n_params) == (t.n_iter, t.n_evals, t.n_samples, t.n_live, t.n_params)
        assert d.truncated == t.truncated
        assert d.lnZ == pytest.approx(t.lnZ, rel=1e-10)
        assert d.max_loglike == pytest.approx(t.max_loglike, rel=1e-10)
        # (the information is a difference of numbers of lnZ's size: rel = 1e-10 of that size)
        assert d.information == pytest.approx(t.information, rel=1e-10, abs=1e-10 * abs(t.lnZ))
        assert d.lnZ_err == pytest.approx(t.lnZ_err, rel=1e-10, abs=1e-10 * math.sqrt(abs(t.lnZ)))
        np.testing.assert_allclose(d.param_constr, t.param_constr, rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(d.posterior, t.posterior, rtol=1e-8, atol=1e-12)


# ---------------------------------------------------------------------------- B: the read-back entry points
def test_dead_and_live_points_are_the_rows_of_the_raw_table(engine):
    """nfa_sampler_dead, nfa_sampler_dead_packed (whole and part), nfa_sampler_live and the raw table of
    nfa_sampler_posterior_packed are four views of the same buffers: bit for bit.  And the raw table normalised on the host
    is the table with weights (exp to an ulp on either side: 8 eps)."""
    make, args, n_pix, opts = CASES['own nlive']
    try:
        engine.set_exp_mode('table')
        cube = make(*args)
        with device_run(cube, np.arange(n_pix), nlive=np.array(opts['nlive']), seed=opts['seed']) as run:
            raw, _ = posterior_tables(run, False)
            weighted, stats = posterior_tables(run, True)
            assert (run.n_iter > 256).all() and (run.n_iter < run.capp).all() and len(set(run.n_iter.tolist())) == 3
            part = np.array([run.n_iter[0] // 2, 0, run.n_iter[2] - 1])
            off_all, T_all, L_all, W_all = dead_points_packed(run, run.n_dead)
            off_part, T_part, L_part, W_part = dead_points_packed(run, part)
            live_T, live_L = np.full((run.P, run.nlive, run.ndim), np.nan), np.full((run.P, run.nlive), np.nan)
            _ffi.check(run.lib.nfa_sampler_live(run.h, _ffi.dptr(live_T), _ffi.dptr(live_L)))
            for p in range(run.P):
                a, nd, nl = int(run.off[p]), int(run.n_dead[p]), int(run.nl[p])
                T, L, W = dead_points(run, p, nd)
                sl = slice(off_all[p], off_all[p + 1])
                assert np.array_equal(T_all[sl], T) and np.array_equal(L_all[sl], L) and np.array_equal(W_all[sl], W)
                sl, k = slice(off_part[p], off_part[p + 1]), int(part[p])
                assert np.array_equal(T_part[sl], T[:k]) and np.array_equal(L_part[sl], L[:k]) and np.array_equal(W_part[sl], W[:k])
                Tk, Lk, Wk = dead_points(run, p, k)
                assert np.array_equal(Tk, T[:k]) and np.array_equal(Lk, L[:k]) and np.array_equal(Wk, W[:k])
                assert np.array_equal(raw[a:a + nd, :run.ndim], T) and np.array_equal(raw[a:a + nd, run.ndim], -2.0 * L)
                assert np.array_equal(raw[a:a + nd, -1], W + L)
                assert np.isfinite(T).all() and (np.diff(L) >= 0).all() and (np.diff(W) < 0).all()     # (in the order they died)
                # a pixel's live points: the first nlive[p] of a stride of the largest count
                assert np.array_equal(raw[a + nd:a + nd + nl, :run.ndim], live_T[p, :nl])
                assert np.array_equal(raw[a + nd:a + nd + nl, run.ndim], -2.0 * live_L[p, :nl])
                assert np.array_equal(raw[a + nd:a + nd + nl, -1], live_L[p, :nl] + run.live_off[p])
                b = int(run.off[p + 1])
                assert np.array_equal(weighted[a:b, :-1], raw[a:b, :-1])
                np.testing.assert_allclose(weighted[a:b, -1], np.exp(raw[a:b, -1] - stats[p, 0]), rtol=8 * np.finfo(float).eps, atol=1e-300)
            # ---- what may not be asked for: more than a pixel holds, a pixel that is not there, no sampler at all
            err = engine.EngineError
            one = np.zeros((int(run.n_iter.max()) + 2) * (run.ndim + 2))
            for p, n in ((0, int(run.n_iter[0]) + 1), (-1, 1), (run.P, 1), (0, -1), (1, int(run.capp.max()) + 1)):
                with pytest.raises(err):
                    _ffi.check(run.lib.nfa_sampler_dead(run.h, p, n, _ffi.dptr(one), _ffi.dptr(one), _ffi.dptr(one)))
            with pytest.raises(err):
                dead_points_packed(run, run.n_dead + np.array([0, 1, 0]))
            more = run.off.copy()
            more[2:] += 1                                # one row more than pixel 1 has
            big = np.zeros((int(more[-1]), run.ndim + 2))
            for offsets in (more, run.off + 1):
                with pytest.raises(err):
                    _ffi.check(run.lib.nfa_sampler_posterior_packed(run.h, offsets.ctypes.data_as(_ffi._lp), _ffi.dptr(run.live_off), _ffi.dptr(big), None))
            fewer = run.off.copy()
            fewer[1:] -= run.n_dead[0] + 1               # one row fewer than pixel 0 has live points
            with pytest.raises(err):
                _ffi.check(run.lib.nfa_sampler_posterior_packed(run.h, fewer.ctypes.data_as(_ffi._lp), _ffi.dptr(run.live_off), _ffi.dptr(big), None))
            lib, d, i = run.lib, _ffi.dptr(one), run.off.ctypes.data_as(_ffi._lp)
        for rc in (lib.nfa_sampler_run(None, 0.5, 0.3, 1, 10, 1, nested.LOG_ZERO, 32), lib.nfa_sampler_dead(None, 0, 1, d, d, d),
                   lib.nfa_sampler_dead_packed(None, i, d, d, d), lib.nfa_sampler_live(None, d, d),
                   lib.nfa_sampler_posterior_packed(None, i, d, d, None), lib.nfa_sampler_counts(None, i, i, None),
                   lib.nfa_sampler_advance(None, 1, None)):
            assert rc != 0
    finally:
        engine.set_exp_mode('fast')


def test_run_is_begin_and_advance(engine):
    """nfa_sampler_run = nfa_sampler_begin with method 1, 10 nd steps and enlarge 1.5, then nfa_sampler_advance to the end
    (include/nestfit_amd.h): the same counts and the same tables, bit for bit."""
    make, args, n_pix, opts = CASES['own nlive']
    try:
        engine.set_exp_mode('table')
        cube = make(*args)
        got = []
        for one_call in (False, True):
            with device_run(cube, np.arange(n_pix), nlive=np.array(opts['nlive']), seed=opts['seed'], one_call=one_call) as run:
                got.append((run.n_iter, run.n_evals, posterior_tables(run, False)[0]) + posterior_tables(run, True))
        for a, b in zip(*got):
            assert np.array_equal(a, b)
        assert (got[0][0] > 256).all()
    finally:
        engine.set_exp_mode('fast')
