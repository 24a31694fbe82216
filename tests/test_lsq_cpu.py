"""The numpy twin of the normal equations and the Levenberg-Marquardt driver (nestfit_amd/lsq.py) without a GPU: a
`FunctionBackend` over a sum of two Gaussians on two spectra of 70 and 129 channels with different noise levels."""
import numpy as np
import pytest

from nestfit_amd import lsq

X = [np.linspace(-10.0, 10.0, 70), np.linspace(-10.0, 10.0, 129)]
SCALE = (1.0, 0.6)                                          # the second spectrum sees the components fainter
SIGMA = (0.1, 0.2)
TRUTH = np.array([1.0, 0.7, -2.0, 2.5, 1.0, 1.5])           # amplitudes, centres, widths of the two components
LOWER = np.array([0.0, 0.0, -5.0, -5.0, 0.3, 0.3])
UPPER = np.array([3.0, 3.0, 5.0, 5.0, 3.0, 3.0])
STEP = 1e-3 * (UPPER - LOWER)
N_PIX, SEED = 6, 3


def model(pix, theta):
    """spectra [B, 199] of theta[B, 6]"""
    theta = np.asarray(theta)
    out = []
    for x, s in zip(X, SCALE):
        p = 0.0
        for c in range(2):
            a, m, w = theta[:, c, None], theta[:, 2 + c, None], theta[:, 4 + c, None]
            p = p + s * a * np.exp(-0.5 * ((x - m) / w) ** 2)
        out.append(p)
    return np.concatenate(out, axis=1)


def jacobian(theta):
    """J [6, 199] of one theta, analytic"""
    rows = []
    for kind in range(3):
        for c in range(2):
            row = []
            for x, s in zip(X, SCALE):
                a, m, w = theta[c], theta[2 + c], theta[4 + c]
                g = s * np.exp(-0.5 * ((x - m) / w) ** 2)
                row.append((g, a * g * (x - m) / w ** 2, a * g * (x - m) ** 2 / w ** 3)[kind])
            rows.append(np.concatenate(row))
    return np.array(rows)


@pytest.fixture(scope='module')
def toy():
    rng = np.random.default_rng(SEED)
    sigma = np.concatenate([np.full(x.size, s) for x, s in zip(X, SIGMA)])
    data = model(None, np.repeat(TRUTH[None], N_PIX, axis=0)) + rng.normal(size=(N_PIX, 199)) * sigma
    weight = np.repeat((1.0 / sigma ** 2)[None], N_PIX, axis=0)
    return lsq.FunctionBackend(model, data, weight), data, weight, rng


def test_curvature_against_the_analytic_jacobian(toy):
    """The central difference at h = 1e-3 of the range truncates at (h / w)^2 / 6 times a factor of a few, about 1e-4 of
    a column's norm for the narrowest width of 1; with a tenfold margin every entry is held to 1e-3 of the scale of
    its columns, sqrt(A_kk A_ll) (an entry is a weighted scalar product of two columns)."""
    backend, data, weight, _ = toy
    pix = np.arange(N_PIX)
    theta = np.repeat(TRUTH[None], N_PIX, axis=0) * (1.0 + 0.02 * np.sin(np.arange(N_PIX * 6).reshape(N_PIX, 6)))
    ne = backend.normal_equations(pix, theta, STEP, LOWER, UPPER)
    for b in range(N_PIX):
        J = jacobian(theta[b])
        r = data[b] - model(None, theta[b][None])[0]
        A, g, chi2 = (weight[b] * J) @ J.T, (weight[b] * J) @ r, np.sum(weight[b] * r * r)
        d = np.sqrt(np.diag(A))
        assert np.all(np.abs(ne.curv[b] - A) <= 1e-3 * np.outer(d, d))
        assert np.all(np.abs(ne.grad[b] - g) <= 1e-3 * d * np.sqrt(chi2))
        assert abs(ne.chi2[b] - chi2) <= 1e-12 * chi2
        assert np.array_equal(ne.curv[b], ne.curv[b].T)
    only = backend.chi_squared(pix, theta)
    np.testing.assert_allclose(only, ne.chi2, rtol=1e-13)
    # longdouble spectra are reduced in longdouble
    rows, inv = lsq.probe_rows(theta, STEP, LOWER, UPPER)
    spec = model(None, rows.reshape(-1, 6)).reshape(N_PIX, 13, 199)
    ld = lsq.normal_equations_from_spectra(spec.astype(np.longdouble), inv, data, weight)
    assert ld.curv.dtype == np.longdouble
    np.testing.assert_allclose(ld.curv.astype(float), ne.curv, rtol=1e-10, atol=1e-9)


def test_a_clipped_probe_gives_the_one_sided_quotient(toy):
    backend, data, weight, _ = toy
    theta = TRUTH[None].copy()
    theta[0, 0] = UPPER[0]                                   # theta+ is clipped back onto theta
    rows, inv = lsq.probe_rows(theta, STEP, LOWER, UPPER)
    assert rows[0, 1, 0] == UPPER[0] and rows[0, 2, 0] == UPPER[0] - STEP[0]
    assert inv[0, 0] == 1.0 / (rows[0, 1, 0] - rows[0, 2, 0])           # of the doubles as they are
    ne = backend.normal_equations([0], theta, STEP, LOWER, UPPER)
    lo = theta.copy()
    lo[0, 0] -= STEP[0]
    J0 = (model(None, theta)[0] - model(None, lo)[0]) * inv[0, 0]
    np.testing.assert_allclose(ne.curv[0, 0, 0], np.sum(weight[0] * J0 * J0), rtol=1e-13)
    free = backend.normal_equations([0], theta, STEP)                    # without bounds: the central quotient
    assert free.curv[0, 0, 0] != ne.curv[0, 0, 0]
    np.testing.assert_allclose(free.curv[0, 1:, 1:], ne.curv[0, 1:, 1:], rtol=1e-13)


def test_a_parameter_without_a_range_is_fixed(toy):
    backend = toy[0]
    lower, upper = LOWER.copy(), UPPER.copy()
    lower[3] = upper[3] = TRUTH[3]
    ne = backend.normal_equations([1], TRUTH[None], STEP, lower, upper)
    assert np.all(ne.curv[0, 3] == 0) and np.all(ne.curv[0, :, 3] == 0) and ne.grad[0, 3] == 0
    keep = np.arange(6) != 3
    assert np.all(np.diag(ne.curv[0])[keep] > 0)
    res = lsq.fit_pixels(backend, [1], TRUTH[None] * 1.03, lower, upper)
    assert res.status[0] == 'converged' and res.theta[0, 3] == TRUTH[3]
    assert np.all(res.cov[0, 3] == 0) and np.all(res.cov[0, :, 3] == 0) and np.all(np.diag(res.cov[0])[keep] > 0)


def test_masked_channels_and_values_that_are_not_finite(toy):
    backend, data, weight, _ = toy
    w = weight[:2].copy()
    w[:, 5] = 0.0
    d = data[:2].copy()
    d[:, 5] = np.nan                                         # a masked channel: whatever the data hold
    rows, inv = lsq.probe_rows(np.repeat(TRUTH[None], 2, axis=0), STEP, LOWER, UPPER)
    spec = model(None, rows.reshape(-1, 6)).reshape(2, 13, 199)
    spec[0, 0, 5] = np.inf                                   # ... or the model
    ne = lsq.normal_equations_from_spectra(spec, inv, d, w)
    assert np.isfinite(ne.chi2).all() and np.isfinite(ne.curv).all()
    ref = lsq.normal_equations_from_spectra(np.delete(spec, 5, axis=2), inv, np.delete(d, 5, axis=1), np.delete(w, 5, axis=1))
    np.testing.assert_allclose(ne.curv, ref.curv, rtol=1e-13, atol=1e-10)            # (entries that cancel to nothing)
    spec[1, 4, 9] = np.inf                                   # a positive weight: the point is NaN, its neighbour is not
    ne = lsq.normal_equations_from_spectra(spec, inv, d, w)
    assert np.isnan(ne.chi2[1]) and np.isnan(ne.grad[1]).all() and np.isnan(ne.curv[1]).all() and np.isfinite(ne.curv[0]).all()


def test_the_driver_finds_the_minimum(toy):
    backend, data, weight, rng = toy
    pix = np.repeat(np.arange(N_PIX), 2)                     # two starts per pixel
    theta0 = TRUTH * (1.0 + 0.05 * rng.normal(size=(2 * N_PIX, 6)))
    res = lsq.fit_pixels(backend, pix, theta0, LOWER, UPPER)
    assert np.all(res.status == 'converged'), res.status
    assert np.all(res.n_iter < 50) and np.all(res.n_iter > 0)
    ne = backend.normal_equations(pix, res.theta, STEP, LOWER, UPPER)
    diag = np.diagonal(ne.curv, axis1=1, axis2=2)
    assert np.all(np.abs(ne.grad) / np.sqrt(diag) <= 1e-2)   # the distance to the minimum in error bars, ten times xtol
    at_truth = backend.chi_squared(pix, np.repeat(TRUTH[None], 2 * N_PIX, axis=0))
    assert np.all(res.chi2 <= at_truth)
    np.testing.assert_allclose(res.chi2, ne.chi2, rtol=1e-12)
    err = np.sqrt(np.diagonal(res.cov, axis1=1, axis2=2))
    assert np.all(err > 0)
    np.testing.assert_allclose(res.cov, np.linalg.inv(ne.curv), rtol=1e-6)
    assert np.all(np.abs(res.theta[0::2] - res.theta[1::2]) <= 0.01 * err[0::2])     # two starts of one pixel agree
    assert np.all(np.abs(res.theta - TRUTH) <= 5 * err)


def test_pinned_parameters_and_invalid_starts(toy):
    backend = toy[0]
    upper = UPPER.copy()
    upper[0] = 0.8                                           # the data want an amplitude of 1
    theta0 = np.repeat((TRUTH * 0.97)[None], 3, axis=0)
    theta0[1, 2] = np.nan                                    # chi^2 is NaN at the start
    res = lsq.fit_pixels(backend, [0, 1, 2], theta0, LOWER, upper)
    assert list(res.status) == ['converged', 'invalid', 'converged']
    assert res.n_iter[1] == 0 and np.isnan(res.chi2[1])
    for b in (0, 2):
        assert res.theta[b, 0] == 0.8
        assert np.all(res.cov[b, 0] == 0) and np.all(res.cov[b, :, 0] == 0) and np.all(np.diag(res.cov[b])[1:] > 0)
    stuck = lsq.fit_pixels(backend, [0], TRUTH[None] * 1.2, LOWER, UPPER, max_iter=1)
    assert stuck.status[0] == 'max_iter' and stuck.n_iter[0] == 1


def test_two_starts_agree_on_two_component_ammonia(nfo):
    """The condition the GPU end-to-end test rests on, met by the twin alone: two-component ammonia (synth.TRUTH_2COMP) on
    2 x 256 channels with sigma = 0.1 K and the noise of default_rng(3), the CPU oracle as the model -- two different starts of
    a pixel end `converged` within 0.01 of the error bar of one another in every free parameter."""
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    axes = [freq_axis(1, 256), freq_axis(2, 256)]
    spectra = [nfo.AmmoniaSpectrum(x, np.zeros(256), 0.1, t) for x, t in zip(axes, (1, 2))]

    def predict(pix, theta):
        out = np.empty((len(theta), 512))
        for row, th in zip(out, np.ascontiguousarray(theta, dtype=np.float64)):
            for k, s in enumerate(spectra):
                nfo.amm_predict(s, th)
                row[k * 256:(k + 1) * 256] = s.get_spec()
        return out
    rng = np.random.default_rng(3)
    model = predict(None, np.repeat(TRUTH_2COMP[None], 2, axis=0))
    data = model + rng.normal(0, 0.1, (4, 512))[:2]                      # the first two pixels of the GPU test's four
    backend = lsq.FunctionBackend(predict, data, np.full((2, 512), 1.0 / (0.1 * 0.1)))
    lower = np.array([-4.0, -4.0, 7.0, 7.0, 2.8, 2.8, 12.5, 12.5, 0.067, 0.067, 0.0, 0.0])           # the box of the IRDC priors
    upper = np.array([4.0, 4.0, 30.0, 30.0, 12.06, 12.06, 16.5, 16.5, 2.067, 2.067, 0.0, 0.0])
    theta0 = TRUTH_2COMP * (1.0 + 0.02 * np.random.default_rng(9).normal(size=(8, 12)))[:4]         # ... and its first four starts
    res = lsq.fit_pixels(backend, [0, 0, 1, 1], theta0, lower, upper)
    assert np.all(res.status == 'converged'), res.status
    err = np.sqrt(np.diagonal(res.cov, axis1=1, axis2=2))
    assert np.all(err[:, :10] > 0) and np.all(err[:, 10:] == 0)
    assert np.all(np.abs(res.theta[0::2] - res.theta[1::2])[:, :10] <= 0.01 * err[0::2, :10])
    assert np.all(np.abs(res.theta - TRUTH_2COMP)[:, :10] <= 5 * err[:, :10])


def test_prior_box_spans_the_draws():
    class Shifted:
        n_param = 3

        def transform(self, u, ncomp):
            u[:] = np.repeat([2.0, -1.0, 5.0], ncomp) + np.repeat([4.0, 0.0, 0.5], ncomp) * u
    lower, upper = lsq.prior_box(Shifted(), 2, n=512, seed=1)
    assert lower.shape == upper.shape == (6,)
    assert np.all(lower[2:4] == -1.0) and np.all(upper[2:4] == -1.0)     # a constant: no range
    assert np.all((lower[:2] >= 2.0) & (lower[:2] < 2.1) & (upper[:2] <= 6.0) & (upper[:2] > 5.9))
