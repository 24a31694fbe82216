"""The runners' host diagnostics over rows (nestfit_amd/_diagnostics.py) and the one option surface of `EngineRunner` and
`CubeRunner` (`_model.SURFACE`): numpy only, no device.

Synthetic rows of 2 spectra (32 and 48 channels), B = 3, with a scalar noise [B, 2] and with a noise per channel [B, 80] one
channel of which is masked (inf, its datum NaN).  Every comparison is bit for bit: the shared functions call the
one-spectrum host functions of `_model` per (spectrum, row) on the same slices, and nothing else."""
import numpy as np
import pytest

SIZES = (32, 48)
OFFSETS = np.array([0, 32, 80])
B = 3
HANNING5 = np.array([0.0, 0.25, 0.5, 0.25, 0.0])


def _rows(per_channel):
    """(data, noise, spec): lines of 2.5 channels' width on a slope, noise of 0.1 .. 0.3; one masked channel per row."""
    rng = np.random.default_rng(7 + per_channel)
    j = np.arange(sum(SIZES), dtype=np.float64)
    spec = np.stack([(1.0 + 0.2 * b) * (np.exp(-0.5 * ((j - 14.3 - b) / 2.5) ** 2) + 0.7 * np.exp(-0.5 * ((j - 55.6 + b) / 2.5) ** 2))
                     for b in range(B)])
    sigma = rng.uniform(0.1, 0.3, (B, len(j) if per_channel else len(SIZES)))
    scatter = sigma if per_channel else np.repeat(sigma, SIZES, axis=1)
    data = 1.1 * spec + 0.3 + 0.004 * j + rng.normal(size=spec.shape) * scatter
    data[1, 20] += 3.0                                       # a spike for the outliers
    if per_channel:
        for b, c in enumerate((5, 40, 79)):
            sigma[b, c], data[b, c] = np.inf, np.nan
    return data, sigma, spec


def _options(per_channel, **kw):
    from nestfit_amd._options import check_options
    return check_options(kw, len(SIZES), SIZES, masked=per_channel)


def _cases(per_channel):
    """(diagnostic, options, extra keywords): every diagnostic with what it goes with; a correlation takes no masked channel."""
    import nestfit_amd as na
    tmpl = [na.ripple(32, 7.3), None]
    yield 'baseline', _options(per_channel, baseline_order=2), {}
    yield 'baseline', _options(per_channel, baseline_order=1, templates=tmpl), {}
    yield 'templates', _options(per_channel, templates=tmpl), {}
    yield 'gain', _options(per_channel, baseline_order=1, calibration=(0.1, 0.0)), {}
    yield 'gain', _options(per_channel, calibration=0.05), {}
    yield 'noise', _options(per_channel, baseline_order=1, templates=tmpl, noise_uncertainty=(0.3, 0.1)), {'filtered': True}
    if not per_channel:
        yield 'noise', _options(per_channel, correlation=na.HANNING, noise_uncertainty=0.2), {'filtered': False}
    yield 'outliers', _options(per_channel, robust=(4.0, 0.0)), {}


def _same(a, b):
    """Bit for bit, whatever the diagnostic returns: an array, a pair of arrays or a list of arrays."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('per_channel', [False, True])
def test_all_rows_are_every_row_alone(per_channel):
    from nestfit_amd import _diagnostics as dg
    data, noise, spec = _rows(per_channel)
    for which, options, how in _cases(per_channel):
        fit = getattr(dg, 'fit_' + which)
        whole = fit(data, noise, spec, OFFSETS, options, **how)
        for b in range(B):
            alone = fit(data[b:b + 1], noise[b:b + 1], spec[b:b + 1], OFFSETS, options, **how)
            part = [a[b:b + 1] for a in whole] if isinstance(whole, (tuple, list)) else whole[b:b + 1]
            assert _same(alone, part), (which, b)


@pytest.mark.parametrize('per_channel', [False, True])
def test_the_diagnostics_are_the_host_functions(per_channel):
    """`baseline_fit`, `nuisance_fit`, `gain_fit`, `half_chi2` + `noise_fit` and `robust_outliers`, called here per spectrum
    and row as the runners called them before there was one implementation."""
    from nestfit_amd import _diagnostics as dg
    from nestfit_amd._model import baseline_fit, channel_weights, gain_fit, half_chi2, noise_fit, nuisance_fit, robust_outliers
    data, noise, spec = _rows(per_channel)
    seen = set()
    for which, o, how in _cases(per_channel):
        got = getattr(dg, 'fit_' + which)(data, noise, spec, OFFSETS, o, **how)
        for k in range(len(SIZES)):
            sl = slice(OFFSETS[k], OFFSETS[k + 1])
            tmpl = None if o.templates is None else o.templates[k]
            for b in range(B):
                d, p = data[b, sl], spec[b, sl]
                sig = noise[b, sl] if per_channel else float(noise[b, k])
                w = channel_weights(sig, SIZES[k])
                assert np.array_equal(w > 0, np.isfinite(np.broadcast_to(sig, w.shape)))
                resid = np.where(w > 0, d - p, 0.0)
                if which == 'baseline' and o.templates is None:
                    assert np.array_equal(got[b, sl], baseline_fit(resid, w, o.baseline_order))
                elif which == 'baseline':
                    assert np.array_equal(got[b, sl], nuisance_fit(resid, w, o.baseline_order, tmpl)[0])
                elif which == 'templates':
                    want = nuisance_fit(resid, w, o.baseline_order, tmpl)[1]
                    assert got[k].shape == (B, 0 if tmpl is None else len(tmpl)) and np.array_equal(got[k][b], want)
                elif which == 'gain':
                    want = gain_fit(d, p, w, 1.0 if per_channel else sig, o.calibration[k], o.baseline_order)
                    assert (got[0][b, k], got[1][b, k]) == want
                elif which == 'noise':
                    corr = None if o.correlation is None else o.correlation[k]
                    h, nu = half_chi2(d, p, sig, o.baseline_order, tmpl, corr, None)
                    assert nu == SIZES[k] - int(per_channel and not np.all(np.isfinite(sig)))
                    assert (got[0][b, k], got[1][b, k]) == noise_fit(h, nu, o.noise_uncertainty[k])
                else:
                    assert np.array_equal(got[b, sl], robust_outliers(d, p, sig, o.robust[k]), equal_nan=True)
        seen.add(which)
    assert seen == set(dg.NEEDS)
    # a spectrum without the option: gain and noise scale 1 +- 0, precision factor 1
    assert np.all(dg.fit_gain(data, noise, spec, OFFSETS, _options(per_channel, calibration=(0.1, 0.0)))[1][:, 1] == 0.0)
    out = dg.fit_outliers(data, noise, spec, OFFSETS, _options(per_channel, robust=(4.0, 0.0)))
    assert out[1, 20] < 0.2 and np.all((out[:, 32:] == 1.0) | np.isnan(out[:, 32:]))
    assert np.isnan(out).sum() == (3 if per_channel else 0)


def test_require_refuses_in_the_runners_words():
    from nestfit_amd import _diagnostics as dg
    plain = _options(False)
    for which, word in (('baseline', 'no baseline'), ('templates', 'no nuisance templates'), ('gain', 'no calibration uncertainty'),
                        ('noise', 'no noise uncertainty'), ('outliers', 'no robust likelihood')):
        with pytest.raises(ValueError, match=word):
            dg.require(which, plain)
    dg.require('baseline', _options(False, baseline_order=0))
    dg.require('baseline', _options(False, templates=[np.ones(32), None]))     # (the nuisance curve of templates alone)
    dg.require('outliers', _options(False, robust=4.0))


def test_a_response_filters_once():
    """One Gaussian line of sigma = 1.5 channels in 64 channels behind a Hanning response, the noise smoothed likewise and
    stated at 1 / 1.3 of its level, f = 0.3.  Rows that are the filtered model meet `half_chi2` without the response, rows
    that are not meet it with the taps, and both are the same answer up to the rounding of the filter; the filtered model
    filtered AGAIN -- what `CubeRunner.fit_noise` did before the rows said which they are -- is another number: 2.4e-2 of
    the mean in this set-up, asserted at > 1e-4."""
    import nestfit_amd as na
    from nestfit_amd import _diagnostics as dg
    from nestfit_amd._model import half_chi2, noise_fit
    from nestfit_amd._options import check_options
    n, f, stated = 64, 0.3, 0.1
    j = np.arange(n, dtype=np.float64)
    p = 1.5 * np.exp(-0.5 * ((j - 30.4) / 1.5) ** 2)
    p_filtered = np.correlate(p, HANNING5, 'same')
    white = np.random.default_rng(3).normal(size=n + 2)
    smooth = (0.25 * white[:-2] + 0.5 * white[1:-1] + 0.25 * white[2:]) / np.sqrt(0.375)
    data = (p_filtered + 1.3 * stated * smooth)[None]
    noise = np.array([[stated]])
    o = check_options(dict(noise_uncertainty=f, **na.smoothed(na.HANNING_RESPONSE)), 1, [n])
    assert np.array_equal(o.response, [HANNING5])
    offsets = np.array([0, n])
    right = dg.fit_noise(data, noise, p_filtered[None], offsets, o, filtered=True)
    h, nu = half_chi2(data[0], p_filtered, stated, None, None, o.correlation[0], None)
    assert (right[0][0, 0], right[1][0, 0]) == noise_fit(h, nu, f)
    unfiltered = dg.fit_noise(data, noise, p[None], offsets, o, filtered=False)
    h, nu = half_chi2(data[0], p, stated, None, None, o.correlation[0], HANNING5)
    assert (unfiltered[0][0, 0], unfiltered[1][0, 0]) == noise_fit(h, nu, f)
    assert unfiltered[0][0, 0] == pytest.approx(right[0][0, 0], rel=1e-12)
    assert abs(right[0][0, 0] - 1.3) < 3 * right[1][0, 0]
    twice = dg.fit_noise(data, noise, p_filtered[None], offsets, o, filtered=False)
    assert abs(twice[0][0, 0] - right[0][0, 0]) > 1e-4 * right[0][0, 0]
    with pytest.raises(TypeError):
        dg.fit_noise(data, noise, p[None], offsets, o)                         # the rows must say which they are


def test_both_runner_classes_have_the_whole_surface():
    """Class attributes only: nothing is instantiated, no library loaded."""
    from nestfit_amd._model import RUNNER_SETS, SURFACE, EngineRunner, RunnerSurface
    from nestfit_amd._options import OPTION_NAMES
    from nestfit_amd.cube import CubeRunner
    assert set(SURFACE) == set(OPTION_NAMES) - {'baseline_order', 'layered'} and len(SURFACE) == 7
    assert set(RUNNER_SETS) == set(SURFACE) | {'baseline_order'}
    for cls in (EngineRunner, CubeRunner):
        assert issubclass(cls, RunnerSurface)
        for name, option in SURFACE.items():
            prop, setter = getattr(cls, name), getattr(cls, 'set_' + name)
            assert isinstance(prop, property) and prop.fset is None and prop.__doc__ == option.value
            assert callable(setter) and setter.__name__ == 'set_' + name and setter.__doc__ == option.sets
            assert 'null_lnZ' in option.sets
        assert callable(cls.set_baseline) and not hasattr(cls, 'set_layered')
        for which in ('baseline', 'templates', 'gain', 'noise', 'outliers'):
            assert callable(getattr(cls, 'fit_' + which))
    assert callable(CubeRunner.set_calibration)
    assert EngineRunner.ONE_PIXEL and not CubeRunner.ONE_PIXEL
