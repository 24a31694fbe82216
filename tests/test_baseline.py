"""A polynomial baseline per spectrum profiled out of the likelihood on the GPU (nfa_specset_set_baseline):
chi2_min against numpy's weighted least squares on the engine's and the oracle's spectra, invariance under added
baselines, the old bits back after removing it, every launch form with the same bits, degenerate spectra, the sampler
and the cube driver, and the ring."""
import os
import threading

import numpy as np
import pytest
from numpy.polynomial import legendre

from device_buffers import DeviceArrays
from nestfit_amd import _ffi
from nestfit_amd.synth import freq_axis

pytestmark = pytest.mark.gpu

MODES = ['table', 'fast']
CKMS = 299792.458
N2HP_NU = {1: 93173.7637e6, 2: 186344.8420e6}
GAUSS_NU = 110.201354e9
RTOL_ENGINE = {'table': 1e-10, 'fast': 1e-6}
RTOL_ORACLE = {'table': 1e-9, 'fast': 1e-6}
# Cancellation: chi2_min = sum w d^2 + sum p (w p - 2 w d) - ||L^-1 e||^2 is formed from terms up to sum w d^2 / chi2_min
# times larger than the result, each with a relative rounding error of a few 1e-16 times log2 of the channel count; the
# cases below keep that ratio under MAX_CANCEL (asserted): a few 1e-12 at most against 1e-10.
MAX_CANCEL = 1e4


def _simple_priors(engine, ranges, size=200):
    from scipy import stats
    x = np.linspace(0, 1, size)
    return engine.PriorTransformer([
        engine.Prior(engine.Distribution(lo + x * (hi - lo), stats.uniform(lo, hi - lo).pdf(lo + x * (hi - lo))), k)
        for k, (lo, hi) in enumerate(ranges)])


def _legendre_u(n):
    return (2.0 * np.arange(n) - (n - 1)) / (n - 1)


class Case:
    """Axes, priors and data of `n_pix` pixels of one model: the engine's model spectra of parameters drawn from the
    priors, a baseline of a few sigma (degree 2) and noise -- scalar, or per channel with masked (NaN) channels."""

    def __init__(self, engine, model, ncomp, n_pix=3, n_chan=512, seed=0, varying=False):
        rng = np.random.default_rng(seed + 10 * ncomp + 100 * model)
        self.engine, self.model, self.ncomp, self.n_pix = engine, model, ncomp, n_pix
        self.rest_freqs = None
        if model == 0:
            self.trans = [1, 2]
            self.axes = [freq_axis(t, n_chan) for t in self.trans]
            self.utrans = engine.get_irdc_priors(size=500, vsys=0.0)
        elif model == 1:
            self.trans = [1, 2]                                  # 2-1: more than 26 lines, the WIDE form
            self.axes = [N2HP_NU[t] * (1.0 - np.linspace(20, -20, n) / CKMS) for t, n in zip(self.trans, (n_chan, 1024))]
            self.utrans = _simple_priors(engine, [(-6, 6), (2.8, 20), (-1.5, 1.0), (0.1, 1.5)])
        else:
            self.trans = [1]
            self.axes = [GAUSS_NU * (1.0 - np.linspace(30, -30, 1500) / CKMS)]
            self.rest_freqs = [GAUSS_NU]
            self.utrans = _simple_priors(engine, [(-20, 20), (0.2, 3.0), (0.0, 5.0)])
        self.sizes = [x.size for x in self.axes]
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(int)
        self.chan_tot = int(self.off[-1])
        self.scalar = rng.uniform(0.1, 0.3, (n_pix, len(self.axes)))
        sig = np.repeat(self.scalar, self.sizes, axis=1)
        if varying:
            sig = sig * rng.uniform(0.7, 1.5, sig.shape)
            self.mask = rng.uniform(size=sig.shape) < 0.05
            self.mask[:, 30:50] = True
            sig[self.mask] = np.inf
            self.noise = sig
        else:
            self.mask = np.zeros(sig.shape, dtype=bool)
            self.noise = self.scalar
        zero = self.runner(np.zeros((n_pix, self.chan_tot)))
        self.ndim = zero.ndim
        pix = np.arange(n_pix, dtype=np.int32)
        theta = rng.uniform(size=(n_pix, self.ndim))
        zero.loglikelihood_batch(pix, theta)
        spec, _ = zero.predict_batch(pix, theta)
        bl = np.concatenate([legendre.legval(_legendre_u(n), rng.normal(0, 3, (3, n_pix)) * self.scalar[:, k]).reshape(n_pix, n)
                             for k, n in enumerate(self.sizes)], axis=1)
        self.data = spec + bl + rng.normal(0, 1, spec.shape) * np.repeat(self.scalar, self.sizes, axis=1)
        self.data[self.mask] = np.nan

    def weights_of(self, noise):
        """w = (sigma_ref / sigma_c)^2, 0 where masked, and sigma_ref [n_pix, n_spec]."""
        if noise.shape[1] == self.chan_tot:
            ref = np.stack([noise[:, a:b].min(axis=1) for a, b in zip(self.off[:-1], self.off[1:])], axis=1)
            return (np.repeat(ref, self.sizes, axis=1) / noise) ** 2, ref
        return np.ones((self.n_pix, self.chan_tot)), noise

    def runner(self, data, mode=None, noise=None, **kw):
        from nestfit_amd.cube import CubeRunner
        r = CubeRunner(self.axes, self.trans, data, self.noise if noise is None else noise, self.utrans, ncomp=self.ncomp,
                       model=self.model, rest_freqs=self.rest_freqs, **kw)
        if mode is not None:
            r.set_exp_mode(mode)
        return r

    def chi2_min(self, data, spec, pix, order, noise=None):
        """numpy: min over the baselines of sum w (d - p - b)^2 per (row, spectrum) [B, n_spec] (weighted lstsq on
        legvander), sigma_ref and the cancellation ratio sum w d^2 / chi2_min.  `noise`: other than the case's."""
        w, ref = self.weights_of(self.noise if noise is None else noise)
        d0 = np.where(w > 0, data, 0.0)
        out = np.empty((len(pix), len(self.sizes)))
        ratio = 0.0
        for k, (a, b) in enumerate(zip(self.off[:-1], self.off[1:])):
            V = legendre.legvander(_legendre_u(b - a), order)
            for q in np.unique(pix):
                rows = np.flatnonzero(pix == q)
                sw = np.sqrt(w[q, a:b])
                R = (d0[q, a:b] - spec[rows][:, a:b]) * sw
                coef = np.linalg.lstsq(V * sw[:, None], R.T, rcond=None)[0]
                out[rows, k] = np.sum((R.T - (V * sw[:, None]) @ coef) ** 2, axis=0)
                ratio = max(ratio, np.max(np.sum(w[q, a:b] * d0[q, a:b] ** 2) / np.maximum(out[rows, k], 1e-300)))
        return out, ref, ratio

    def lnl(self, chi2, ref, pix):
        return -np.sum(chi2 / (2 * ref[pix] ** 2), axis=1)

    def oracle_spectra(self, nfo, theta):
        out = np.empty((theta.shape[0], self.chan_tot))
        for i, th in enumerate(theta):
            for k, (t, x) in enumerate(zip(self.trans, self.axes)):
                if self.model == 0:
                    s = nfo.AmmoniaSpectrum(x, np.zeros(x.size), 1.0, t)
                    nfo.amm_predict(s, th)
                elif self.model == 1:
                    s = nfo.DiazenyliumSpectrum(x, np.zeros(x.size), 1.0, t)
                    nfo.nnhp_predict(s, th)
                else:
                    s = nfo.Spectrum(x, np.zeros(x.size), 1.0, rest_freq=GAUSS_NU)
                    nfo.gauss_predict(s, th)
                out[i, self.off[k]:self.off[k + 1]] = s.get_spec()
        return out


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind in 'fc'), what


# ---- 1. against numpy and the oracle ----------------------------------------------------------------------------------
CASES = [(0, 1), (0, 2), (0, 4), (0, 10), (1, 2), (2, 2)]


@pytest.mark.parametrize('model, ncomp', CASES, ids=['nh3-1', 'nh3-2', 'nh3-4', 'nh3-10', 'n2hp-2', 'gauss-2'])
@pytest.mark.parametrize('varying', [False, True], ids=['scalar', 'channel'])
@pytest.mark.parametrize('mode', MODES)
def test_against_numpy_and_the_oracle(engine, nfo, mode, model, ncomp, varying):
    case = Case(engine, model, ncomp, varying=varying)
    rng = np.random.default_rng(7)
    pix = rng.integers(0, case.n_pix, 1000).astype(np.int32)
    U = rng.uniform(size=(1000, case.ndim))
    r = case.runner(case.data, mode)
    theta = U.copy()
    r.loglikelihood_batch(pix, theta)
    spec, _ = r.predict_batch(pix, theta)
    spec_o = case.oracle_spectra(nfo, theta[:200])
    for order in range(4):
        r._ss.set_baseline(order)
        lnl = r.loglikelihood_batch(pix, U.copy())
        spec_b, lnl_p = r.predict_batch(pix, theta)
        _same(spec_b, spec, f'order {order}: spectra out are the model alone')
        _same(lnl_p, lnl, f'order {order}: predict_batch lnL against loglikelihood_batch')
        chi2, ref, ratio = case.chi2_min(case.data, spec, pix, order)
        assert ratio < MAX_CANCEL, ratio
        np.testing.assert_allclose(lnl, case.lnl(chi2, ref, pix), rtol=RTOL_ENGINE[mode], err_msg=f'order {order}')
        chi2_o, _, _ = case.chi2_min(case.data, spec_o, pix[:200], order)
        np.testing.assert_allclose(lnl[:200], case.lnl(chi2_o, ref, pix[:200]), rtol=RTOL_ORACLE[mode],
                                   err_msg=f'order {order}: oracle')
        all_pix = np.arange(case.n_pix)
        chi2_0, _, _ = case.chi2_min(case.data, np.zeros((case.n_pix, case.chan_tot)), all_pix, order)
        np.testing.assert_allclose(r._ss.null_lnZ(), -chi2_0 / (2 * ref ** 2), rtol=1e-10, err_msg=f'order {order}: null')
    # the runner's own order and null_lnZ
    rb = case.runner(case.data, mode, baseline_order=2)
    assert rb.baseline_order == 2
    r._ss.set_baseline(2)
    _same(rb.null_lnZ, r._ss.null_lnZ().sum(axis=1), 'CubeRunner null_lnZ')


# ---- 2. invariance under added baselines ------------------------------------------------------------------------------
@pytest.mark.parametrize('varying', [False, True], ids=['scalar', 'channel'])
@pytest.mark.parametrize('mode', MODES)
def test_added_baselines_change_nothing(engine, mode, varying):
    case = Case(engine, 0, 2, varying=varying, seed=1)
    rng = np.random.default_rng(8)
    pix = rng.integers(0, case.n_pix, 500).astype(np.int32)
    U = rng.uniform(size=(500, case.ndim))
    for order in range(4):
        ref = case.runner(case.data, mode, baseline_order=order)
        want = ref.loglikelihood_batch(pix, U.copy())
        extra = np.concatenate(
            [legendre.legval(_legendre_u(n), rng.choice([-1, 1], (order + 1, case.n_pix)) * rng.uniform(10, 20, (order + 1, case.n_pix))
                             * case.scalar[:, k]).reshape(case.n_pix, n) for k, n in enumerate(case.sizes)], axis=1)
        moved = case.runner(case.data + extra, mode, baseline_order=order)
        np.testing.assert_allclose(moved.loglikelihood_batch(pix, U.copy()), want, rtol=1e-9)
        np.testing.assert_allclose(moved.null_lnZ, ref.null_lnZ, rtol=1e-9)
        # a term of degree order + 1 is not a baseline of this order
        c = np.zeros(order + 2)
        c[-1] = 10.0
        higher = np.concatenate([np.outer(case.scalar[:, k], legendre.legval(_legendre_u(n), c)) for k, n in enumerate(case.sizes)], axis=1)
        other = case.runner(case.data + higher, mode, baseline_order=order)
        assert np.all(np.abs(other.null_lnZ - ref.null_lnZ) > 1e-3 * np.abs(ref.null_lnZ))
        assert np.all(np.abs(other.loglikelihood_batch(pix, U.copy()) - want) > 1e-3 * np.abs(want))


# ---- 3. the old bits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('varying', [False, True], ids=['scalar', 'channel'])
@pytest.mark.parametrize('mode', MODES)
def test_removing_the_baseline_gives_the_old_bits(engine, mode, varying):
    case = Case(engine, 0, 2, varying=varying, seed=2)
    rng = np.random.default_rng(9)
    pix = rng.integers(0, case.n_pix, 600).astype(np.int32)
    U = rng.uniform(size=(600, case.ndim))
    fresh = case.runner(case.data, mode)
    want = fresh.loglikelihood_batch(pix, U.copy())
    theta = U.copy()
    fresh.loglikelihood_batch(pix, theta)
    want_spec, want_lp = fresh.predict_batch(pix, theta)
    r = case.runner(case.data, mode)
    for order in (3, 0):
        r._ss.set_baseline(order)
        got = r.loglikelihood_batch(pix, U.copy())
        assert not np.array_equal(got, want)
        _same(r.predict_batch(pix, theta)[0], want_spec, f'spectra out, order {order}')
        r._ss.set_baseline(-1)
        _same(r.loglikelihood_batch(pix, U.copy()), want, 'lnL after set_baseline(-1)')
        _same(r._ss.null_lnZ(), fresh._ss.null_lnZ(), 'null_lnZ after set_baseline(-1)')
        spec, lp = r.predict_batch(pix, theta)
        _same(spec, want_spec, 'spectra after set_baseline(-1)')
        _same(lp, want_lp, 'predict lnL after set_baseline(-1)')
    # nfa_specset_set_data keeps the order and the basis: a set made with the new data gives the same bits
    lib = _ffi.load()
    r._ss.set_baseline(1)
    new = case.data.copy()
    new[1] += np.linspace(-1, 1, case.chan_tot)
    _ffi.check(lib.nfa_specset_set_data(r._ss.handle, 1, _ffi.dptr(np.ascontiguousarray(new[1]))))
    other = case.runner(new, mode, baseline_order=1)
    _same(r.loglikelihood_batch(pix, U.copy()), other.loglikelihood_batch(pix, U.copy()), 'lnL after set_data')
    _same(r._ss.null_lnZ(), other._ss.null_lnZ(), 'null_lnZ after set_data')


# ---- 4. launch forms ---------------------------------------------------------------------------------------------------
def _dev_batches(runner, batches):
    lib = _ffi.load()
    dev = DeviceArrays(lib, _ffi.check)
    try:
        bufs = []
        for pix, U in batches:
            d_pix, d_u = dev.upload(np.ascontiguousarray(pix, dtype=np.int32)), dev.upload(U)
            d_l = dev.empty(8 * U.shape[0])
            _ffi.check(lib.nfa_runner_loglike_batch_dev(runner._run.handle, d_pix, d_u, d_l, U.shape[0]))
            bufs.append((d_u, d_l, U))
        _ffi.check(lib.nfa_runner_synchronize(runner._run.handle))
        return [(dev.download(d_u, np.empty_like(U)), dev.download(d_l, np.empty(U.shape[0]))) for d_u, d_l, U in bufs]
    finally:
        dev.free()


@pytest.mark.parametrize('varying', [False, True], ids=['scalar', 'channel'])
@pytest.mark.parametrize('mode', MODES)
def test_launch_forms_agree_bit_for_bit(engine, mode, varying):
    case = Case(engine, 0, 2, n_pix=4096, n_chan=1024, seed=3, varying=varying)      # the benchmark's shape
    r = case.runner(case.data, mode, baseline_order=2)
    rng = np.random.default_rng(10)
    pix = rng.permutation(4096).astype(np.int32)
    batches = [(pix, rng.uniform(size=(4096, case.ndim))) for _ in range(8)]
    host = [r.loglikelihood_batch(p, U.copy()) for p, U in batches]
    try:
        for group in (8, 3):
            _ffi.set_option('coalesce', group)
            for k, (_, lnl) in enumerate(_dev_batches(r, [(p, U.copy()) for p, U in batches])):
                _same(lnl, host[k], f'device batch {k}, groups of {group}')
    finally:
        _ffi.set_option('coalesce', 8)
    p0, U0 = batches[0]
    for n in (1000, 512, 100):                  # small launches: two and four waves per unit (resolve_split)
        _same(r.loglikelihood_batch(p0[:n], U0[:n].copy()), host[0][:n], f'{n} rows')
    from nestfit_amd import ammonia
    d = [case.data[p0[0], a:b] for a, b in zip(case.off[:-1], case.off[1:])]
    nz = [case.noise[p0[0], a:b] for a, b in zip(case.off[:-1], case.off[1:])] if varying else list(case.noise[p0[0]])
    single = ammonia.AmmoniaRunner.from_data([[x, dd, z, t] for x, dd, z, t in zip(case.axes, d, nz, case.trans)], case.utrans,
                                             ncomp=2, baseline_order=2)
    single.set_exp_mode(mode)
    assert single.baseline_order == 2
    _same(single.null_lnZ, r.null_lnZ[p0[0]], 'pixel runner null_lnZ')
    th = U0[:5].copy()
    lb = single.loglikelihood_batch(th)
    for k in range(5):                          # (single points from the third on: a captured graph in the fast mode)
        _same(single.loglikelihood(U0[k].copy()), lb[k], f'single point against its batch row {k}')
    _same(lb[0], host[0][0], 'pixel runner against the cube runner')
    # fit_baseline: the baseline numpy fits to data - predict
    base = single.fit_baseline(th[0])
    spec = np.concatenate([s.get_spec() for s in single.spectra])
    w = 1.0 / np.concatenate([np.broadcast_to(np.asarray(z, dtype=float), (x.size,)) for z, x in zip(nz, case.axes)]) ** 2
    full = np.concatenate(d)
    # (the pixel runner's predict follows the process's mode, the cube runner's predict_batch its own: each against numpy
    # on its own spectra)
    spec_c = r.predict_batch(p0[:1], th[:1])[0][0]
    base_c = r.fit_baseline(p0[:1], th[:1])[0]
    for a, b in zip(case.off[:-1], case.off[1:]):
        live = w[a:b] > 0
        V = legendre.legvander(_legendre_u(b - a), 2)
        for got, model in ((base, spec), (base_c, spec_c)):
            coef = np.linalg.lstsq(V[live] * np.sqrt(w[a:b][live])[:, None],
                                   (full[a:b] - model[a:b])[live] * np.sqrt(w[a:b][live]), rcond=None)[0]
            np.testing.assert_allclose(got[a:b], V @ coef, rtol=1e-8, atol=1e-10)


# ---- 5. degenerate spectra ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_spectra_with_few_channels(engine, mode):
    case = Case(engine, 0, 1, n_pix=3, n_chan=256, seed=4, varying=True)
    rng = np.random.default_rng(11)
    pix = rng.integers(0, 3, 300).astype(np.int32)
    U = rng.uniform(size=(300, case.ndim))
    for order in (1, 2, 3):
        noise = case.noise.copy()
        noise[1, :256] = np.inf                                   # pixel 1, spectrum 0: exactly `order` channels left
        noise[1, [3, 100, 200][:order]] = 0.2
        data = case.data.copy()
        data[1, [3, 100, 200][:order]] = rng.normal(0, 1, order)
        r = case.runner(data, mode, noise=noise, baseline_order=order)
        null = r._ss.null_lnZ()
        assert abs(null[1, 0]) <= 1e-12 * abs(null[1, 1]), null
        # the spectrum adds (almost exactly) nothing
        theta = U.copy()
        lnl = r.loglikelihood_batch(pix, theta)
        spec, _ = r.predict_batch(pix, theta)
        chi2, ref, _ = case.chi2_min(data, spec, pix, order, noise=noise)
        sel = pix == 1
        assert np.all(np.abs(chi2[sel, 0]) <= 1e-12 * chi2[sel, 1])
        np.testing.assert_allclose(lnl, case.lnl(chi2, ref, pix), rtol=RTOL_ENGINE[mode], atol=1e-9)


# ---- 6. sampler and cube driver ----------------------------------------------------------------------------------------
def _tilted_pixels(engine, nfo, tilt, n_pix=8, n_chan=256):
    from nestfit_amd.cube import CubeRunner
    rng = np.random.default_rng(5)
    truth = np.array([0.3, 14.0, 6.0, 14.7, 0.4, 0.0])
    axes = [freq_axis(t, n_chan) for t in (1, 2)]
    clean = []
    for t, x in zip((1, 2), axes):
        s = nfo.AmmoniaSpectrum(x, np.zeros(n_chan), 0.1, t)
        nfo.amm_predict(s, truth)
        clean.append(s.get_spec())
    noise = rng.normal(0, 0.1, (n_pix, 2 * n_chan))
    base = np.concatenate(clean)[None, :] + noise
    tilted = base + tilt * 0.1 * np.concatenate([_legendre_u(n_chan) + 1.0] * 2)[None, :]
    ut = engine.get_irdc_priors(size=500, vsys=0.0)
    mk = lambda d, order: CubeRunner(axes, [1, 2], d, np.full((n_pix, 2), 0.1), ut, ncomp=1, baseline_order=order)
    return mk, base, tilted, truth


@pytest.mark.parametrize('mode', MODES)
def test_sampler_with_a_tilted_baseline(engine, nfo, mode):
    from nestfit_amd import sampler
    mk, base, tilted, truth = _tilted_pixels(engine, nfo, tilt=5.0)
    kw = dict(nlive=100, tol=0.5, seed=4)
    pix = np.arange(base.shape[0])
    runs = {}
    for name, data, order in (('flat', base, 1), ('tilted', tilted, 1), ('tilted-none', tilted, None), ('flat-none', base, None)):
        r = mk(data, order)
        r.set_exp_mode(mode)
        runs[name] = (r, sampler.fit_pixels(r, pix, **kw))
    gain = {k: np.array([x.lnZ for x in res]) - r.null_lnZ for k, (r, res) in runs.items()}
    err = {k: np.array([x.lnZ_err for x in res]) for k, (_, res) in runs.items()}
    # with the baseline profiled out, the tilt changes the evidence ratio by no more than the sampler's own error
    assert np.all(np.abs(gain['tilted'] - gain['flat']) <= 3 * np.hypot(err['tilted'], err['flat'])), (gain, err)
    voff = np.array([x.param_constr[3][0] for x in runs['tilted'][1]])
    assert np.all(np.abs(voff - truth[0]) < 0.1), voff
    # without a baseline the tilt spoils the fit: the best likelihood falls far below the flat data's
    best_none = np.array([x.max_loglike for x in runs['tilted-none'][1]])
    best_flat = np.array([x.max_loglike for x in runs['flat-none'][1]])
    assert np.all(best_none < best_flat - 100), (best_none, best_flat)


@pytest.fixture
def exp_mode_restored(engine):
    before = _ffi.load().nfa_get_exp_mode()
    yield
    engine.set_exp_mode(before)


def test_cube_fitter_records_the_order(engine, nfo, tmp_path, exp_mode_restored):
    from nestfit_amd.cubeio import CubeStack, DataCube, NoiseCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    engine.set_exp_mode('fast')
    rng = np.random.default_rng(0)
    n_lon, n_chan = 4, 96
    cubes = []
    for t in (1, 2):
        x = freq_axis(t, n_chan, 12.0)
        data = rng.normal(0, 0.1, (n_chan, 1, n_lon)) + 0.3 * np.linspace(-1, 1, n_chan)[:, None, None]
        s = nfo.AmmoniaSpectrum(x, np.zeros(n_chan), 0.1, t)
        nfo.amm_predict(s, np.array([0.3, 14.0, 6.0, 14.7, 0.5, 0.0]))
        data[:, :, 0] += s.get_spec()[:, None]
        if t == 1:
            data[:, :, 3] = np.nan                               # every channel of pixel 3 masked: nbest = 0 unsampled
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_lon, 'NAXIS2': 1, 'NAXIS3': n_chan,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': float(x.mean())}
        cubes.append(DataCube(SimpleCube(hdr, data), NoiseCube(0.1), trans_id=t))
    fit = CubeFitter(CubeStack(cubes), engine.get_irdc_priors(size=200, vsys=0.0), engine.AmmoniaRunner,
                     runner_kwargs={'baseline_order': 1}, lnZ_thresh=11, ncomp_max=2,
                     mn_kwargs={'nlive': 40, 'tol': 1.0, 'seed': 3, 'maxiter': 600}, nlive_snr_fact=0)
    fit.fit_cube(str(tmp_path / 'bl'), nproc=1)
    with HdfStore(str(tmp_path / 'bl')) as store:
        assert store.hdf.attrs['baseline_order'] == 1
        groups = {g.attrs['i_lon']: g for g in store.iter_pix_groups()}
        assert sorted(groups) == [0, 1, 2, 3]
        assert groups[3].attrs['nbest'] == 0 and '1' not in groups[3]
        assert groups[0].attrs['nbest'] >= 1                     # the line, on a tilt the baseline takes
        for i in (1, 2):
            assert groups[i].attrs['nbest'] == 0                 # a tilt alone is no line


# ---- 7. the ring -------------------------------------------------------------------------------------------------------
def test_ring_serving_of_a_baseline_runner(engine):
    from nestfit_amd import ammonia
    from nestfit_amd.ring import RingClient, RingServer
    case = Case(engine, 0, 2, n_pix=1, n_chan=512, seed=6)
    d = [case.data[0, a:b] for a, b in zip(case.off[:-1], case.off[1:])]
    r = ammonia.AmmoniaRunner.from_data([[x, dd, z, t] for x, dd, z, t in zip(case.axes, d, case.noise[0], case.trans)],
                                        case.utrans, ncomp=2, baseline_order=1)
    r.set_exp_mode('table')
    name = f'nfa_test_ring_bl_{os.getpid()}'
    with RingServer(name, n_slots=1, runner=r) as server:
        with pytest.raises(_ffi.EngineError, match='baseline'):
            server.serve_device(lifetime_ms=20, idle_ms=200)
        t = threading.Thread(target=server.serve, kwargs=dict(max_wait_us=100, idle_ms=20000))
        t.start()
        rng = np.random.default_rng(1)
        U = rng.uniform(size=(40, r.ndim))
        got_t, got_l = [], []
        with RingClient(name, wait_ms=20000) as client:
            for u in U:
                th = u.copy()
                got_l.append(client.loglikelihood(th))
                got_t.append(th)
        server.stop()
        t.join(timeout=30)
        assert not t.is_alive()
    want_t = U.copy()
    want_l = r.loglikelihood_batch(want_t)
    _same(np.array(got_t), want_t, 'ring theta')
    _same(np.array(got_l), want_l, 'ring lnL')
