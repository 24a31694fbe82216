"""An uncertain noise level per spectrum, integrated out of the likelihood: what can be checked without a GPU.

`check_noise_uncertainty`; the restatement (tests/nmarg_restatement.py) at its limits and against a numerical integral over the
precision; `noise_fit` against a numerical integral of the posterior; `cubeio.estimate_noise` on white and on Hanning-smoothed
noise; the constant `Spectrum.prefactor` gains; the store's attribute; and the science on the restatement: an understated
noise inflates every lnL difference, and the marginal takes the inflation back.
"""
import numpy as np
import pytest

import nmarg_restatement as nr

LD = np.longdouble


# ---------------------------------------------------------------------------- the checker
def test_the_checker():
    from nestfit_amd._model import check_noise_uncertainty as chk
    assert chk(None) is None and chk(0) is None and chk(0.0, 3) is None and chk([0, 0.0], 2) is None
    assert np.array_equal(chk(0.2), [0.2]) and np.array_equal(chk(0.2, 3), [0.2, 0.2, 0.2])
    assert np.array_equal(chk((0.1, 0.0, 0.5), 3), [0.1, 0.0, 0.5]) and np.array_equal(chk(np.array([0.3, 0.1])), [0.3, 0.1])
    assert chk(np.float32(0.25), 2).dtype == np.float64 and chk([0.1, 0.2]).dtype == np.float64
    for bad in ('a', True, [0.1, 'b'], -0.1, 0.51, np.nan, np.inf, [0.1, np.nan], [], np.zeros((2, 2)), [[0.1]], {'f': 0.1}):
        with pytest.raises(ValueError, match='noise uncertainty'):
            chk(bad)
    for bad, n in (([0.1], 2), ([0.1, 0.2, 0.3], 2), (np.array([0.1]), 3)):
        with pytest.raises(ValueError, match='noise uncertainty'):
            chk(bad, n)
    # not with a calibration uncertainty, whichever is checked; zeros of either are none
    with pytest.raises(ValueError, match='calibration'):
        chk(0.2, 2, calibration=np.array([0.1, 0.0]))
    assert np.array_equal(chk(0.2, 2, calibration=np.zeros(2)), [0.2, 0.2]) and chk(0, 2, calibration=np.array([0.1, 0.1])) is None


def test_the_fitter_checks_before_any_pixel():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter

    class stack:
        cubes = [None, None]
    assert CubeFitter(stack, None, na.AmmoniaRunner).noise_uncertainty is None
    assert np.array_equal(CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'noise_uncertainty': 0.2}).noise_uncertainty, [0.2, 0.2])
    for value in ('a', 0.6, [0.1], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError, match='noise uncertainty'):
            CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'noise_uncertainty': value})
    with pytest.raises(ValueError, match='calibration'):
        CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'noise_uncertainty': 0.2, 'calibration': 0.1})


# ---------------------------------------------------------------------------- the formula
def test_shape_and_limits():
    from nestfit_amd._model import noise_marginal_lnl, noise_shape
    for f in (0.05, 0.2, 0.3, 0.5):
        a = noise_shape(f)
        assert a == pytest.approx(1.0 / (4.0 * f * f), rel=1e-15) and float(nr.shape(f)) == pytest.approx(a, rel=1e-15)
        # a Gamma(a, rate a): mean 1 and std 1 / sqrt(a) = 2 f, i.e. std of t = tau^(-1/2) is f to first order
        assert 1.0 / np.sqrt(a) == pytest.approx(2.0 * f, rel=1e-14)
    h = np.array([0.0, 0.3, 17.0, 130.0, 4000.0])
    for nu in (4, 256):
        # f -> 0: -h.  The first correction is -(nu / 2) h / a + h^2 / (2 a), so the distance shrinks like f^2
        last = None
        for f in (1e-2, 1e-3, 1e-4):
            dist = np.abs(np.asarray(nr.term(h, nu, f), dtype=np.float64) + h)
            bound = 4 * f * f * (nu / 2 * h + h * h / 2) * 1.01 + 1e-12
            assert (dist <= bound).all(), (nu, f)
            assert last is None or (dist[1:4] < 0.011 * last[1:4]).all()          # (h = 4000 is no small h / a at f = 0.01)
            last = dist
        assert np.array_equal(np.asarray(nr.term(h, nu, 0.0), dtype=np.float64), -h)
        # the package's numpy form is the restatement's, and f = 0 keeps -h to the bit
        for f in (0.05, 0.3, 0.5):
            np.testing.assert_allclose(noise_marginal_lnl(h, nu, f), np.asarray(nr.term(h, nu, f), dtype=np.float64), rtol=1e-14)
        assert np.array_equal(noise_marginal_lnl(h, nu, 0.0), -h)
    # concave in h, slope between -c / a and 0; a rounded-negative h is clamped
    hs = np.linspace(0, 500, 2001)
    t = np.asarray(nr.term(hs, 256, 0.3), dtype=np.float64)
    assert (np.diff(t) < 0).all() and (np.diff(t, 2) > 0).all() and -np.diff(t)[0] / (hs[1] - hs[0]) <= nr.slope(256, 0.3)
    assert float(nr.term(-1e-9, 256, 0.3)) == 0.0 and noise_marginal_lnl(-1e-9, 256, 0.3) == 0.0


def test_the_marginal_is_the_integral_over_the_precision():
    """ln int tau^(nu/2) exp(-tau h) Gamma(tau; a, a) dtau = [lgamma(c) - lgamma(a) - (nu/2) ln a] - c log1p(h / a): the
    restatement's term plus the constant `Spectrum.prefactor` gains, by the trapezoid rule in log space."""
    from math import lgamma
    from nestfit_amd._model import noise_prefactor
    for nu, f, h in ((8, 0.3, 3.7), (64, 0.2, 41.0), (256, 0.5, 90.0), (31, 0.05, 12.0)):
        a = float(nr.shape(f))
        c = a + nu / 2
        mode = (c - 1) / (a + h)
        tau = np.linspace(mode * 1e-3, mode * (1 + 40 / np.sqrt(c)), 400001).astype(LD)
        ln_int = (LD(nu) / 2 + LD(a) - 1) * np.log(tau) - tau * (LD(a) + LD(h)) + LD(a) * np.log(LD(a)) - LD(lgamma(a))
        top = ln_int.max()
        y = np.exp(ln_int - top)
        integral = float(top + np.log(np.sum((y[1:] + y[:-1]) / 2 * np.diff(tau))))
        want = float(nr.term(h, nu, f)) + noise_prefactor(nu, f)
        assert integral == pytest.approx(want, abs=1e-7), (nu, f, h)
        assert noise_prefactor(nu, f) == pytest.approx(lgamma(c) - lgamma(a) - nu / 2 * np.log(a), rel=1e-15)
    assert noise_prefactor(256, None) == 0.0 and noise_prefactor(256, 0.0) == 0.0


def test_the_prefactor_of_a_spectrum():
    from nestfit_amd._model import noise_prefactor
    from nestfit_amd.core import Spectrum
    x = 1e11 + 1e5 * np.arange(200)
    noise = np.full(200, 0.2)
    noise[[3, 50, 51]] = np.inf
    for s, nu in ((Spectrum(x, np.zeros(200), 0.3), 200), (Spectrum(x, np.zeros(200), noise), 197)):
        white = s.prefactor
        assert s.n_chan == nu and s.noise_uncertainty is None
        s.set_noise_uncertainty(0.25)
        assert s.noise_uncertainty == 0.25 and s.prefactor == white + noise_prefactor(nu, 0.25) != white
        s.set_correlation((0.5, 0.25))                       # the two constants add, whichever comes first
        both = s.prefactor
        s.set_noise_uncertainty(None)
        corr_only = s.prefactor
        s.set_noise_uncertainty(0.25)
        assert s.prefactor == both == corr_only + noise_prefactor(nu, 0.25)
        s.set_correlation(None)
        assert s.prefactor == white + noise_prefactor(nu, 0.25)
        s.set_noise_uncertainty(0.0)
        assert s.prefactor == white and s.noise_uncertainty is None                    # to the bit


# ---------------------------------------------------------------------------- fit_noise
def test_fit_noise_against_an_integral_of_the_posterior():
    """tau | d ~ Gamma(c, rate r), c = a + nu / 2, r = a + h; the moments of t = tau^(-1/2) by quadrature over t."""
    from scipy import integrate
    from nestfit_amd._model import noise_fit
    for nu, f, h in ((256, 0.3, 128.0 * 1.69), (256, 0.3, 128.0), (40, 0.5, 10.0), (64, 0.1, 60.0), (4, 0.2, 0.5)):
        a = float(nr.shape(f))
        c, r = a + nu / 2, a + h
        t0 = np.sqrt(r / c)

        def dens(t, k):                                     # p(t) up to a constant: tau^(c-1) e^(-r tau) |dtau/dt|, tau = t^-2
            return np.exp(-(2 * c + 1 - k) * np.log(t / t0) - r / t ** 2 + r / t0 ** 2)
        lo, hi = t0 * 0.2, t0 * 6.0
        m0, m1, m2 = (integrate.quad(dens, lo, hi, args=(k,), epsabs=0, epsrel=1e-12, limit=400, points=[t0])[0] * t0 ** k for k in range(3))
        mean, std = noise_fit(h, nu, f)
        assert mean == pytest.approx(m1 / m0, rel=1e-8), (nu, f, h)
        assert std == pytest.approx(np.sqrt(m2 / m0 - (m1 / m0) ** 2), rel=1e-6), (nu, f, h)
    # a noise stated 1.3 times too small over 256 channels: h ~ 1.69 nu / 2, and the posterior finds the factor
    mean, std = noise_fit(128.0 * 1.69, 256, 0.3)
    assert abs(mean - 1.3) < 3 * std and 0.03 < std < 0.08
    assert noise_fit(50.0, 100, 0.0) == (1.0, 0.0)


def test_half_chi2_is_the_restatements():
    """The numpy chi^2 behind `fit_noise`, for every kind of set, against the restatements' h."""
    import nestfit_amd as na
    from nestfit_amd._model import half_chi2
    rng = np.random.default_rng(5)
    n = 96
    j = np.arange(n)
    pred = 2.0 * np.exp(-0.5 * ((j - 40.3) / 3.0) ** 2)
    data = pred + 0.2 * rng.normal(size=n) + 0.1 + 0.002 * j
    chan = rng.uniform(0.15, 0.3, n)
    masked = chan.copy()
    masked[[5, 38, 39, 40]] = np.inf
    tmpl = na.ripple(n, 17.3)
    taps5 = np.array([0.0, 0.25, 0.5, 0.25, 0.0])
    for noise, kw, rkw in ((0.2, {}, {}), (masked, {}, {}), (masked, dict(order=1), dict(order=1)),
                           (0.2, dict(order=0, templates=tmpl), dict(order=0, templates=tmpl)),
                           (chan, dict(corr=na.HANNING), dict(rho=na.HANNING)),
                           (0.2, dict(corr=na.HANNING, resp=taps5), dict(rho=na.HANNING, taps=(0.25, 0.5, 0.25))),
                           (0.2, dict(resp=taps5), dict(taps=(0.25, 0.5, 0.25)))):
        h, nu = half_chi2(data, pred, noise, **kw)
        want, _ = nr.half_chi2([None, data, noise], pred, **rkw)
        assert h == pytest.approx(float(want[0]), rel=1e-9) and nu == nr.n_unmasked(noise, n)
    assert nr.n_unmasked(masked, n) == n - 4 and nr.n_unmasked(0.2, n) == n


# ---------------------------------------------------------------------------- estimate_noise
def test_estimate_noise_on_white_and_smoothed_noise():
    import nestfit_amd as na
    from nestfit_amd.cubeio import estimate_noise
    rng = np.random.default_rng(17)
    n_pix, n_chan, sigma = 4096, 256, 0.35
    line_free = np.r_[0:100, 156:256]
    n_free = line_free.size
    white = sigma * rng.normal(size=(64, 64, n_chan + 2))
    line = 3.0 * np.exp(-0.5 * ((np.arange(n_chan) - 128) / 6.0) ** 2)
    for name, noise, rho in (('white', white[..., 1:-1], None),
                             ('hanning', 0.25 * white[..., :-2] + 0.5 * white[..., 1:-1] + 0.25 * white[..., 2:], na.HANNING)):
        true = sigma * (1.0 if rho is None else np.sqrt(0.375))
        rms, f = estimate_noise(noise + line + 0.7, line_free, correlation=rho)      # an offset and a line in the other channels
        assert rms.shape == (64, 64)
        n_eff = n_free if rho is None else n_free / (1 + 2 * rho[0] ** 2 + 2 * rho[1] ** 2)
        assert f == pytest.approx(1 / np.sqrt(2 * n_eff), rel=1e-14)
        # the map's mean is the true level (its standard error f / sqrt(n_pix), and a bias of order 1 / n_free for the
        # smoothed noise, whose mean takes more than one degree of freedom) and its scatter IS f: within 5 standard errors
        # of a scatter over n_pix values, 1 / sqrt(2 n_pix), and the edge terms of the correlated sum, 2 / n_free
        assert abs(rms.mean() / true - 1) < 5 * f / np.sqrt(n_pix) + 2.0 / n_free, name
        scatter = rms.std(ddof=1) / rms.mean()
        assert abs(scatter / f - 1) < 5 / np.sqrt(2 * n_pix) + 2.0 / n_free, (name, scatter, f)
    # without the pair the smoothed noise's f is too small by sqrt(1 + 2 rho_1^2 + 2 rho_2^2) = 1.39
    assert estimate_noise(white, line_free)[1] == pytest.approx(f / np.sqrt(1 + 2 * (2 / 3) ** 2 + 2 * (1 / 6) ** 2), rel=1e-12)
    # a DataCube-like object, a mask, a NaN
    class cube:
        data = white[:2, :2, :n_chan].copy()
    cube.data[0, 1, 7] = np.nan
    mask = np.zeros(n_chan, dtype=bool)
    mask[line_free] = True
    rms, f2 = estimate_noise(cube, mask)
    assert f2 == 1 / np.sqrt(2 * n_free) and np.isnan(rms[0, 1]) and np.isfinite(np.delete(rms.ravel(), 1)).all()
    with pytest.raises(ValueError, match='8 line-free'):
        estimate_noise(white, slice(0, 5))


# ---------------------------------------------------------------------------- the store
class _Fitter:
    """What insert_fitter_pars reads of a fitter."""
    lnZ_thresh, ncomp_max, nlive_snr_fact, nlive_quantum = 11, 2, 5, 1
    mn_kwargs = {'nlive': 100, 'tol': 1.0, 'seed': 5}

    class stack:
        cubes = [None, None, None]

    def __init__(self, runner_kwargs):
        self.runner_kwargs = runner_kwargs


@pytest.mark.parametrize('form', ['npz', 'hdf5'])
def test_the_store_carries_the_noise_uncertainty(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import store as st
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    cases = {'number': (0.2, [0.2, 0.2, 0.2]), 'each': ((0.05, 0.0, 0.5), [0.05, 0.0, 0.5]), 'zeros': ((0, 0, 0), None), 'none': (None, None),
             'absent': ('absent', None)}
    for name, (value, want) in cases.items():
        path = str(tmp_path / f'{name}_{form}')
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'baseline_order': 1} if value == 'absent' else {'noise_uncertainty': value}))
        with st.HdfStore(path) as store:
            got = store.read_model_noise_uncertainty()
            assert ('noise_uncertainty' in store.hdf.attrs) == (want is not None)
            if want is None:
                assert got is None
            else:
                assert got.dtype == np.float64 and np.array_equal(got, np.array(want))     # to the bit, in both forms
            assert store.read_model_calibration() is None
    with pytest.raises(ValueError, match='noise uncertainty'):
        with st.HdfStore(str(tmp_path / f'bad_{form}'), nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'noise_uncertainty': (0.1, 0.2)}))            # two values, three cubes


# ---------------------------------------------------------------------------- the science
def test_an_understated_noise_inflates_the_evidence_and_the_marginal_takes_it_back():
    """64 spectra of 256 channels, one Gaussian of peak 1.5 and sigma 4 channels at channel 128.3, unit white noise; the noise
    is stated 1.3 times too small.  Pooled sum of lnL(truth) - lnL(0) against the same sum at the true noise: the white
    likelihood multiplies it by 1.69; with f = 0.3 the ratio is back within 10 % of 1 (numpy: 0.978, and 0.970 where the
    noise is stated correctly -- the price of concavity)."""
    n_spec, n = 64, 256
    rng = np.random.default_rng(11)
    model = 1.5 * np.exp(-0.5 * ((np.arange(n) - 128.3) / 4.0) ** 2)
    data = model[None, :] + rng.normal(size=(n_spec, n))

    def pooled(sigma, f):
        tot = LD(0)
        for d in data:
            row = [None, d, sigma]
            h1, _ = nr.half_chi2(row, model)
            h0, _ = nr.half_chi2(row, np.zeros(n))
            tot += nr.term(h1, n, f)[0] - nr.term(h0, n, f)[0]
        return float(tot)
    def pooled_by_the_package(sigma, f):
        """The same sum through `nestfit_amd._model.noise_marginal_lnl`, the host's form of the device's arithmetic."""
        from nestfit_amd._model import noise_marginal_lnl
        h1 = 0.5 * np.sum((data - model) ** 2, axis=1) / sigma ** 2
        h0 = 0.5 * np.sum(data ** 2, axis=1) / sigma ** 2
        return float(np.sum(noise_marginal_lnl(h1, n, f) - noise_marginal_lnl(h0, n, f)))
    for sigma, f in ((1.0, 0.0), (1.0 / 1.3, 0.0), (1.0 / 1.3, 0.3), (1.0, 0.3)):
        assert pooled_by_the_package(sigma, f) == pytest.approx(pooled(sigma, f), rel=1e-11)
    at_truth = pooled(1.0, 0.0)
    assert at_truth / n_spec == pytest.approx(np.sum(model ** 2) / 2, rel=0.15)           # sum p^2 / 2 = 1.5^2 4 sqrt(pi) / 2 = 7.98 per spectrum
    white = pooled(1.0 / 1.3, 0.0) / at_truth
    marg = pooled(1.0 / 1.3, 0.3) / at_truth
    right = pooled(1.0, 0.3) / at_truth
    print(f'pooled evidence ratios: white at the understated noise {white:.3f}, f = 0.3 {marg:.3f}, f = 0.3 at the right noise {right:.3f}')
    assert white == pytest.approx(1.69, rel=1e-12) and white > 1.6
    assert 0.9 <= marg <= 1.1
    assert marg == pytest.approx(0.978, abs=2e-3) and right == pytest.approx(0.970, abs=2e-3)
