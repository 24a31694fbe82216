"""A polynomial baseline per spectrum without a GPU: the argument checks of every runner happen on the host
before any device call, the host helper `fit_baseline` agrees with numpy, and the cube driver writes the order into the
store."""
import numpy as np
import pytest

from nestfit_amd import sampler
from nestfit_amd._model import baseline_fit, check_baseline_order
from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
from nestfit_amd.store import HdfStore
from nestfit_amd.synth import freq_axis


@pytest.mark.parametrize('order, want', [(None, None), (-1, None), (0, 0), (1, 1), (2, 2), (3, 3),
                                         (np.int64(2), 2), (np.int32(-1), None)])
def test_accepted_orders(order, want):
    assert check_baseline_order(order) == want


@pytest.mark.parametrize('order', [4, -2, 10, 1.0, 2.5, '1', True, np.float64(1.0), [1]])
def test_rejected_orders(order):
    with pytest.raises(ValueError, match='baseline_order'):
        check_baseline_order(order)


@pytest.mark.parametrize('order', [4, -2, 1.5])
def test_runners_check_the_order_before_any_device_call(order):
    # (no spectra set is made: on a box without a GPU these calls would fail in the engine otherwise)
    import nestfit_amd as na
    from nestfit_amd import gaussian
    from nestfit_amd.cube import CubeRunner
    x = freq_axis(1, 64)
    with pytest.raises(ValueError, match='baseline_order'):
        na.AmmoniaRunner.from_data([[x, np.zeros(64), 0.1, 1]], None, baseline_order=order)
    with pytest.raises(ValueError, match='baseline_order'):
        na.AmmoniaRunner([], None, baseline_order=order)
    with pytest.raises(ValueError, match='baseline_order'):
        na.DiazenyliumRunner.from_data([[x, np.zeros(64), 0.1, 1]], None, baseline_order=order)
    with pytest.raises(ValueError, match='baseline_order'):
        gaussian.GaussianRunner.from_data([x, np.zeros(64), 0.1, 1e11], None, baseline_order=order)
    with pytest.raises(ValueError, match='baseline_order'):
        CubeRunner([x], [1], np.zeros((2, 64)), np.full((2, 1), 0.1), None, baseline_order=order)


def _polyfit_baseline(r, w, order):
    """The same fit in the monomial basis of the channel index (np.polyfit, weights on the residuals)."""
    j = np.arange(r.size, dtype=np.float64)
    live = w > 0
    c = np.polyfit(j[live], r[live], order, w=np.sqrt(w[live]))
    return np.polyval(c, j)


@pytest.mark.parametrize('order', [0, 1, 2, 3])
def test_fit_baseline_against_numpy(order):
    rng = np.random.default_rng(order)
    n = 300
    j = np.arange(n)
    poly = np.polyval(rng.normal(0, 1, order + 1) / np.maximum(1.0, n ** np.arange(order, -1, -1.0)) * 5, j)
    sig = rng.uniform(0.1, 0.3, n)
    sig[40:60] = np.inf                                          # masked channels: their residuals are ignored
    resid = poly + rng.normal(0, 1, n) * np.where(np.isfinite(sig), sig, 0.0)
    resid[40:60] = 1e6
    w = 1.0 / sig ** 2
    got = baseline_fit(resid, w, order)
    np.testing.assert_allclose(got, _polyfit_baseline(resid, w, order), rtol=1e-8, atol=1e-10)
    # a baseline alone is fitted exactly; several spectra at once, a scalar weight
    got = baseline_fit(np.stack([poly, 2 * poly]), 1.0, order)
    np.testing.assert_allclose(got, np.stack([poly, 2 * poly]), rtol=1e-9, atol=1e-9)


def test_fit_baseline_with_few_channels():
    rng = np.random.default_rng(3)
    n = 50
    w = np.zeros(n)
    w[[5, 20, 33]] = 1.0                                         # three unmasked channels: order 3 becomes order 2
    r = rng.normal(0, 1, n)
    got = baseline_fit(r, w, 3)
    np.testing.assert_allclose(got[[5, 20, 33]], r[[5, 20, 33]], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got, _polyfit_baseline(r, w, 2), rtol=1e-7, atol=1e-9)
    assert np.array_equal(baseline_fit(r, np.zeros(n), 2), np.zeros(n))    # nothing unmasked: no baseline


# ---- the store records the order (the cube driver through a stub fit_backend, as in tests/test_fitter_cpu.py) -------
N_CHAN, NOISE = 96, 0.1


def _oracle_backend(fitter, lon, lat, ncomp, nlive, kw):
    from oracle import nfo
    ps = nfo.PriorSet(fitter.utrans.lower())
    runners = []
    for i, j in zip(lon, lat):
        spec_data, _ = fitter.stack.get_spec_data(i, j)
        runners.append(nfo.AmmoniaRunner([nfo.AmmoniaSpectrum(*sd) for sd in spec_data], ps, ncomp=ncomp))

    def loglike(pix, U):
        out = np.empty(U.shape[0])
        for q in np.unique(pix):
            m = pix == q
            sub = U[m]
            out[m] = runners[q].loglikelihood_batch(sub)
            U[m] = sub
        return out
    res = sampler.run_nested(loglike, 6 * ncomp, len(runners), nlive=nlive, batch_target=64, **kw)
    return res, np.array([r.null_lnZ for r in runners]), runners[0].n_chan_tot


def _stack(n_lon=2):
    rng = np.random.default_rng(0)
    cubes = []
    for t in (1, 2):
        x = freq_axis(t, N_CHAN, 12.0)
        data = rng.normal(0, NOISE, (N_CHAN, 1, n_lon))
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_lon, 'NAXIS2': 1, 'NAXIS3': N_CHAN,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': float(x.mean())}
        cubes.append(DataCube(SimpleCube(hdr, data), NOISE, trans_id=t))
    return CubeStack(cubes)


@pytest.mark.parametrize('kwargs, want', [({}, -1), ({'baseline_order': None}, -1), ({'baseline_order': 1}, 1),
                                          ({'baseline_order': 3}, 3)])
def test_store_records_the_baseline_order(tmp_path, kwargs, want):
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    fit = CubeFitter(_stack(), na.get_irdc_priors(size=200, vsys=0.0), na.AmmoniaRunner, runner_kwargs=kwargs,
                     lnZ_thresh=11, ncomp_max=1, mn_kwargs={'nlive': 24, 'tol': 1.0, 'seed': 3, 'maxiter': 100},
                     nlive_snr_fact=0, fit_backend=_oracle_backend)
    fit.fit_cube(str(tmp_path / 'run'), nproc=1)
    with HdfStore(str(tmp_path / 'run')) as store:
        assert store.hdf.attrs['baseline_order'] == want
        assert len(list(store.iter_pix_groups())) == 2
