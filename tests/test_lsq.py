"""The normal equations of a least-squares fit on the device (nfa_runner_normal_equations) and the
Levenberg-Marquardt driver above them, in both numerical modes.

The reference of every comparison is longdouble numpy on the spectra the existing `predict_batch` returns for the same probe
rows.  Tolerances are derived, not tuned.  With N the channels of positive weight, u = 2^-53 and T the columns J_0 .. J_(n-1), r
of a point, every entry of the Gram matrix is held to

    |G_kl - ref| <= (N + 8) u sum_c |w T_k T_l| 1.01

-- a term carries at most eight roundings (two per column: the difference of two spectra and the product with 1 / dtheta, or
the one of d - p; the product with w; the product of the two; the scale 1 / sigma^2), the sum N - 1, and 1.01 covers the
second order.  1 / dtheta, the weights and 1 / sigma^2 are the same doubles on both sides (`lsq.probe_rows`,
`lsq.channel_weights`: the engine's operations in numpy)."""
import ctypes as C

import numpy as np
import pytest

from test_sibling_models import MODES, n2hp_axis

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LD = np.longdouble


def _gram_reference(spec, inv, data, weight):
    """(G [B, n + 1, n + 1], bound) in longdouble from spectra [B, R, C] of the probe rows."""
    B, R, _ = spec.shape
    n = (R - 1) // 2
    spec, data, weight = spec.astype(LD), np.asarray(data).astype(LD), np.asarray(weight).astype(LD)
    keep = weight > 0
    T = np.zeros((B, n + 1, spec.shape[2]), dtype=LD)
    with np.errstate(invalid='ignore'):
        T[:, n] = np.where(keep, data - spec[:, 0], 0)
    if n:
        T[:, :n] = np.where(keep[:, None, :], (spec[:, 1::2] - spec[:, 2::2]) * inv.astype(LD)[:, :, None], 0)
    w = np.where(keep, weight, 0)[:, None, :]
    G = np.einsum('bkc,blc->bkl', w * T, T)
    S = np.einsum('bkc,blc->bkl', w * np.abs(T), np.abs(T))
    N = keep.sum(axis=1)
    return G, (N[:, None, None] + 8) * U * S * LD(1.01)


def _check(ne, spec, inv, data, weight, what=''):
    """A `NormalEquations` record of the device against the spectra of the same probe rows."""
    from nestfit_amd import lsq
    G, tol = _gram_reference(spec, inv, data, weight)
    n = G.shape[1] - 1
    for name, got, ref, bound in (('chi2', ne.chi2, G[:, n, n], tol[:, n, n]), ('grad', ne.grad, G[:, :n, n], tol[:, :n, n]),
                                  ('curv', ne.curv, G[:, :n, :n], tol[:, :n, :n])):
        err = np.abs(got.astype(LD) - ref)
        assert np.all(err <= bound), (what, name, float(np.max(err / np.maximum(bound, LD(1e-300)))))
    assert np.array_equal(ne.curv, np.swapaxes(ne.curv, 1, 2))              # both triangles hold one number
    twin = lsq.normal_equations_from_spectra(spec.astype(LD), inv, data, np.asarray(weight).astype(LD))
    assert np.all(np.abs(twin.curv - G[:, :n, :n]) <= tol[:, :n, :n] * 1e-3)  # the twin in longdouble is that reference
    return G


def _cube_case(runner, pix, theta, step, lower, upper, chunk_rows=None, what=''):
    from nestfit_amd import lsq
    pix = np.asarray(pix, dtype=np.int32)
    rows, inv = lsq.probe_rows(theta, step, lower, upper)
    B, R, n = rows.shape
    spec, _ = runner.predict_batch(np.repeat(pix, R), rows.reshape(B * R, n))
    data, weight = lsq.channel_weights(runner, pix, LD)
    ne = runner.normal_equations(pix, theta, step, lower, upper, chunk_rows=chunk_rows)
    assert ne.chi2.shape == (B,) and ne.grad.shape == (B, n) and ne.curv.shape == (B, n, n)
    _check(ne, spec.reshape(B, R, -1), inv, data, weight, what)
    assert np.isfinite(ne.chi2).all() and np.isfinite(ne.curv).all()
    return ne


def _jitter(rng, truth, rows, scale=0.03):
    return np.ascontiguousarray(truth * (1.0 + scale * rng.normal(size=(rows, np.size(truth)))))


def _box(truth):
    truth = np.asarray(truth, dtype=np.float64)
    span = np.maximum(np.abs(truth), 1.0)
    return truth - span, truth + span


@pytest.fixture(scope='module')
def ammonia(engine):
    """Ammonia on two spectra of 70 and 129 channels, three pixels, one and two components."""
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_1COMP, TRUTH_2COMP, freq_axis
    rng = np.random.default_rng(21)
    axes = [freq_axis(1, 70, 20.0), freq_axis(2, 129, 20.0)]
    data, noise = rng.normal(0, 0.2, (3, 199)), np.array([[0.2, 0.3], [0.25, 0.2], [0.2, 0.2]])
    return {n: (CubeRunner(axes, (1, 2), data, noise, None, ncomp=n), truth) for n, truth in ((1, TRUTH_1COMP), (2, TRUTH_2COMP))}, axes


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2])
def test_gram_entries(ammonia, mode, ncomp):
    """ndim = 6 and 12; B = 1, 3, 9; chunk_rows = 64 holds four or two points, so several chunks; and the default."""
    runner, truth = ammonia[0][ncomp]
    runner.set_exp_mode(mode)
    rng = np.random.default_rng(5 + ncomp)
    lower, upper = _box(truth)
    step = 1e-3 * (upper - lower)
    for B in (1, 3, 9):
        theta = _jitter(rng, truth, B)
        pix = (np.arange(B) % 3).astype(np.int32)
        small = _cube_case(runner, pix, theta, step, lower, upper, chunk_rows=64, what=(ncomp, B, 64))
        whole = _cube_case(runner, pix, theta, step, lower, upper, what=(ncomp, B, None))
        again = runner.normal_equations(pix, theta, step, lower, upper, chunk_rows=64)
        assert all(np.array_equal(a, b) for a, b in zip(small, again))       # the same arguments: the same bits
        assert np.array_equal(runner.chi_squared(pix, theta), small.chi2)    # chi^2 alone: the full call's bits
        assert np.array_equal(whole.chi2, small.chi2)
        assert np.all(np.diagonal(small.curv, axis1=1, axis2=2)[:, :5 * ncomp] > 0)
        other = runner.normal_equations(np.roll(pix, 1) if B > 1 else (pix + 1) % 3, theta, step, lower, upper)
        assert not np.array_equal(other.chi2, small.chi2)                    # the pixel matters
        only_grad = runner.normal_equations(pix, theta, step, lower, upper, want_curvature=False)
        assert only_grad.curv is None and np.array_equal(only_grad.grad, whole.grad)
    none = runner.normal_equations(np.zeros(0, np.int32), np.zeros((0, 6 * ncomp)), step)
    assert none.chi2.shape == (0,) and none.curv.shape == (0, 6 * ncomp, 6 * ncomp)      # B = 0: a no-op


@pytest.mark.parametrize('mode', MODES)
def test_other_models(engine, mode):
    """N2H+ with ndim = 8 and the Gaussian model with eight components, ndim = 24: the cap."""
    from nestfit_amd.cube import CubeRunner
    rng = np.random.default_rng(40)
    n2hp = np.array([-1.0, 1.2, 9.0, 6.0, 0.6, 1.2, 0.4, 0.5])
    runner = CubeRunner([n2hp_axis(1, 150)], (1,), rng.normal(0, 0.2, (2, 150)), np.full((2, 1), 0.2), None, ncomp=2, model=1)
    runner.set_exp_mode(mode)
    lower, upper = _box(n2hp)
    _cube_case(runner, [1, 0, 1], _jitter(rng, n2hp, 3), 1e-3 * (upper - lower), lower, upper, chunk_rows=64, what='n2hp')

    nu0 = 110.201354e9
    x = nu0 * (1.0 - np.linspace(20, -20, 131) / 299792.458)
    gauss = np.concatenate([np.linspace(-14, 14, 8), 0.8 + 0.1 * np.arange(8), 2.0 + 0.3 * np.arange(8)])
    runner = CubeRunner([x], [1], rng.normal(0, 0.1, (2, 131)), np.full((2, 1), 0.1), None, ncomp=8, model=2, rest_freqs=[nu0])
    runner.set_exp_mode(mode)
    assert runner.ndim == 24
    lower, upper = _box(gauss)
    step = 1e-3 * (upper - lower)
    ne = _cube_case(runner, [0, 1, 1], _jitter(rng, gauss, 3, 0.01), step, lower, upper, chunk_rows=64, what='gauss 64')
    assert np.all(np.diagonal(ne.curv, axis1=1, axis2=2) > 0)
    _cube_case(runner, [0, 1, 1], _jitter(rng, gauss, 3, 0.01), step, lower, upper, what='gauss')
    # nine components, ndim = 27: refused
    nine = CubeRunner([x], [1], np.zeros((1, 131)), np.full((1, 1), 0.1), None, ncomp=9, model=2, rest_freqs=[nu0])
    with pytest.raises(engine.EngineError, match='NFA_LSQ_MAX_DIM'):
        nine.normal_equations([0], np.ones((1, 27)), np.ones(27))
    with pytest.raises(engine.EngineError, match='NFA_LSQ_MAX_DIM'):
        nine.chi_squared([0], np.ones((1, 27)))


@pytest.mark.parametrize('mode', MODES)
def test_set_kinds(ammonia, engine, mode):
    """A noise per channel with masked channels, a continuum, layered transfer and the filled LTE mix."""
    from nestfit_amd import lsq
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP
    axes = ammonia[1]
    rng = np.random.default_rng(50)
    lower, upper = _box(TRUTH_2COMP)
    step = 1e-3 * (upper - lower)
    theta = _jitter(rng, TRUTH_2COMP, 3)
    data = rng.normal(0, 0.2, (2, 199))
    sigma = rng.uniform(0.15, 0.4, (2, 199))
    sigma[:, [3, 69, 70, 150]] = np.inf
    sigma[1, 100:110] = np.inf
    data[0, 69] = data[1, 104] = np.nan                                      # planted under the mask: must not show
    masked = CubeRunner(axes, (1, 2), data, sigma, None, ncomp=2)
    masked.set_exp_mode(mode)
    ne = _cube_case(masked, [0, 1, 0], theta, step, lower, upper, chunk_rows=64, what='masked')
    _, weight = lsq.channel_weights(masked, [0, 1], np.float64)
    assert (weight == 0).sum() == 4 + 14 and np.isfinite(ne.grad).all()

    tc = np.array([[30.0, 28.0], [0.0, 0.0], [3.0, 12.5]])
    cont = CubeRunner(axes, (1, 2), rng.normal(0, 0.2, (3, 199)), np.full((3, 2), 0.2), None, ncomp=2, continuum=tc)
    cont.set_exp_mode(mode)
    a = _cube_case(cont, [0, 1, 2], theta, step, lower, upper, chunk_rows=64, what='continuum')
    b = cont.normal_equations(np.array([2, 1, 0], np.int32), theta, step, lower, upper)
    assert not np.array_equal(a.curv[0], b.curv[0]) and np.array_equal(a.curv[1], b.curv[1])     # the pixel's continuum it is

    n2hp = np.array([-1.0, 1.2, 9.0, 6.0, 0.6, 1.2, 0.4, 0.5])
    lo8, hi8 = _box(n2hp)
    raw = rng.normal(0, 0.2, (2, 150))
    layered = CubeRunner([n2hp_axis(1, 150)], (1,), raw, np.full((2, 1), 0.2), None, ncomp=2, model=1, layered=True)
    summed = CubeRunner([n2hp_axis(1, 150)], (1,), raw, np.full((2, 1), 0.2), None, ncomp=2, model=1)
    for r in (layered, summed):
        r.set_exp_mode(mode)
    th8 = _jitter(rng, n2hp, 3)
    a = _cube_case(layered, [0, 1, 1], th8, 1e-3 * (hi8 - lo8), lo8, hi8, chunk_rows=64, what='layered')
    assert not np.array_equal(a.curv, summed.normal_equations(np.array([0, 1, 1], np.int32), th8, 1e-3 * (hi8 - lo8), lo8, hi8).curv)

    # the filled LTE mix on a single-pixel runner: one species on one transition, two components of five parameters
    import mix_restatement as mr
    from test_lte_fill import draw_params
    from test_lte_mix import _rows
    mol, ks, iso, isos = mr.test_species(engine)
    rows = _rows((ks[1],), seed=71)
    run = engine.LteMix([mol], fill=True).Runner.from_data(rows, None, ncomp=2)
    run.set_exp_mode(mode)
    thetas = np.stack([draw_params(rng, 2, mol, iso, k, n_species=1) for k in range(3)])
    lo, hi = _box(thetas[0])
    st = 1e-3 * (hi - lo)
    probe, inv = lsq.probe_rows(thetas, st, lo, hi)
    spec, _ = run.predict_batch(probe.reshape(-1, 10))
    x, d, noise, _ = rows[0]
    ne = run.normal_equations(thetas, st, lo, hi, chunk_rows=64)
    _check(ne, spec.reshape(3, 21, -1), inv, np.repeat(d[None], 3, axis=0), np.full((3, d.size), 1.0 / (noise * noise)), 'filled')
    assert np.array_equal(run.chi_squared(thetas), ne.chi2) and np.isfinite(ne.curv).all()


@pytest.mark.parametrize('mode', MODES)
def test_clipped_probes_fixed_parameters_and_refused_calls(ammonia, engine, mode):
    from nestfit_amd import _ffi, lsq
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP
    runner, truth = ammonia[0][2]
    runner.set_exp_mode(mode)
    axes = ammonia[1]
    lower, upper = _box(truth)
    step = 1e-3 * (upper - lower)
    theta = _jitter(np.random.default_rng(60), truth, 2)
    theta[0, 4] = upper[4]                                                   # theta+ is clipped back onto theta: one-sided
    fixed_lo, fixed_hi = lower.copy(), upper.copy()
    fixed_lo[7] = fixed_hi[7] = truth[7]                                     # no range: fixed
    ne = _cube_case(runner, [0, 2], theta, step, fixed_lo, fixed_hi, chunk_rows=64, what='clipped')
    assert np.all(ne.curv[:, 7] == 0) and np.all(ne.curv[:, :, 7] == 0) and np.all(ne.grad[:, 7] == 0)
    free = runner.normal_equations(np.array([0, 2], np.int32), theta, step)
    assert free.curv[0, 4, 4] != ne.curv[0, 4, 4] and free.curv[1, 4, 4] == ne.curv[1, 4, 4]
    rows, inv = lsq.probe_rows(theta, step, fixed_lo, fixed_hi)
    assert rows[0, 9, 4] == upper[4] == theta[0, 4] and inv[0, 7] == 0

    lib = _ffi.load()
    pix = np.zeros(2, np.int32)
    out = [np.empty(2), np.empty((2, 12)), np.empty((2, 12, 12))]

    def call(r, pix=pix, theta=theta, B=2, step=step, lower=None, upper=None, chunk=0, chi2=out[0], grad=out[1], curv=out[2]):
        p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        rc = lib.nfa_runner_normal_equations(r._run.handle, None if pix is None else pix.ctypes.data_as(_ffi._ip), p(theta), B, p(step),
                                             p(lower), p(upper), chunk, p(chi2), p(grad), p(curv))
        return rc, lib.nfa_last_error().decode()
    ARG, STATE = 1, 3
    assert call(runner)[0] == 0
    for kw, word in ((dict(theta=None), 'null'), (dict(chi2=None), 'null'), (dict(step=None), 'without step'),
                     (dict(step=None, curv=None), 'without step'), (dict(step=np.where(np.arange(12) == 3, 0.0, step)), 'step'),
                     (dict(step=np.where(np.arange(12) == 3, np.inf, step)), 'step'), (dict(step=np.where(np.arange(12) == 3, np.nan, step)), 'step'),
                     (dict(lower=upper, upper=lower), 'lower bound'), (dict(chunk=100), 'multiple of 64'), (dict(chunk=-64), 'multiple of 64'),
                     (dict(pix=np.array([0, 3], np.int32)), 'pixel'), (dict(pix=np.array([-1, 0], np.int32)), 'pixel')):
        rc, why = call(runner, **kw)
        assert rc == ARG and word in why, (kw, rc, why)
    one = ammonia[0][1][0]
    th1 = np.ascontiguousarray(theta[:, :6])
    assert call(one, theta=th1, step=step[:6], chunk=64)[0] == 0             # 13 rows fit 64 ...
    rc, why = call(runner, chunk=0, B=0, theta=None, chi2=None)
    assert rc == 0                                                           # B = 0: a no-op
    assert call(runner, step=None, grad=None, curv=None)[0] == 0             # chi^2 alone needs no step

    # every likelihood that is not -chi^2 / 2 of white noise is refused with its sentence
    from nestfit_amd import HANNING, HANNING_RESPONSE, ripple
    data, noise = np.zeros((2, 199)), np.full((2, 2), 0.2)
    refused = (('baseline', dict(baseline_order=1)), ('templates', dict(templates=[ripple(70, 20.0), None])),
               ('calibration', dict(calibration=0.1)), ('correlated', dict(correlation=HANNING)),
               ('response', dict(response=HANNING_RESPONSE)), ('noise uncertainty', dict(noise_uncertainty=0.2)),
               ('robust', dict(robust=4.0)))
    for word, kw in refused:
        r = CubeRunner(axes, (1, 2), data, noise, None, ncomp=2, **kw)
        rc, why = call(r)
        assert rc == STATE and word in why and why.endswith('takes no normal equations'), (word, rc, why)
        rc, why = call(r, step=None, grad=None, curv=None)
        assert rc == STATE and word in why
        with pytest.raises(engine.EngineError, match=word):
            r.chi_squared(pix, theta)
        assert np.isfinite(r.predict_batch(pix, theta)[1]).all()            # and the runner is as good as before
    assert np.isfinite(runner.normal_equations(pix, theta, step).curv).all()


@pytest.mark.parametrize('mode', MODES)
def test_consistency_with_the_likelihood(ammonia, mode):
    """For two rows of one pixel chi2_a - chi2_b = -2 (lnL_a - lnL_b) of `predict_batch` within 32 N u sum W (|d| + |p|)^2: both
    sides are sums of N terms bounded by that, and each carries at most 8 roundings."""
    from nestfit_amd import lsq
    runner, truth = ammonia[0][2]
    runner.set_exp_mode(mode)
    theta = _jitter(np.random.default_rng(70), truth, 8)
    for p in range(3):
        pix = np.full(8, p, np.int32)
        spec, lnl = runner.predict_batch(pix, theta)
        chi2 = runner.chi_squared(pix, theta)
        data, weight = lsq.channel_weights(runner, pix)
        bound = 32 * 199 * U * np.sum(weight * (np.abs(data) + np.abs(spec)) ** 2, axis=1)
        for a in range(8):
            for b in range(a):
                assert abs((chi2[a] - chi2[b]) + 2.0 * (lnl[a] - lnl[b])) <= bound[a] + bound[b], (p, a, b)
        assert np.ptp(chi2) > 1.0


@pytest.fixture(scope='module')
def two_components(engine):
    """Synthetic two-component ammonia (synth.TRUTH_2COMP) on 2 x 256 channels, four pixels, sigma = 0.1 K."""
    import nestfit_amd as na
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP, freq_axis
    rng = np.random.default_rng(3)
    axes = [freq_axis(1, 256), freq_axis(2, 256)]
    ut = na.get_irdc_priors(size=500, vsys=0.0)
    before = na.get_exp_mode()
    na.set_exp_mode('table')
    try:
        probe = CubeRunner(axes, (1, 2), np.zeros((1, 512)), np.full((1, 2), 0.1), ut, ncomp=2)
        model, _ = probe.predict_batch(np.zeros(4, np.int32), np.repeat(TRUTH_2COMP[None], 4, axis=0))
    finally:
        na.set_exp_mode(before)
    data = model + rng.normal(0, 0.1, model.shape)
    return axes, data, ut, rng


@pytest.mark.parametrize('mode', MODES)
def test_fit_pixels_on_the_device_and_through_predict_batch(two_components, mode):
    from nestfit_amd import lsq
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_2COMP
    axes, data, ut, _ = two_components
    runner = CubeRunner(axes, (1, 2), data, np.full((4, 2), 0.1), ut, ncomp=2)
    runner.set_exp_mode(mode)
    lower, upper = lsq.prior_box(ut, 2)
    assert lower[10] == upper[10] == 0.0 and np.all(lower[:10] < TRUTH_2COMP[:10]) and np.all(TRUTH_2COMP[:10] < upper[:10])
    pix = np.repeat(np.arange(4), 2)
    theta0 = _jitter(np.random.default_rng(9), TRUTH_2COMP, 8, 0.02)
    dev = lsq.fit_pixels(lsq.DeviceBackend(runner), pix, theta0, lower, upper)
    host = lsq.fit_pixels(lsq.PredictBackend(runner), pix, theta0, lower, upper)
    assert np.all(dev.status == 'converged') and np.all(host.status == 'converged'), (dev.status, host.status)
    err = np.sqrt(np.diagonal(dev.cov, axis1=1, axis2=2))
    assert np.all(err[:, :10] > 0) and np.all(err[:, 10:] == 0)
    worst = np.max(np.abs(dev.theta - host.theta)[:, :10] / err[:, :10])
    starts = np.max(np.abs(dev.theta[0::2] - dev.theta[1::2])[:, :10] / err[0::2, :10])
    print(f'lsq {mode}: device against predict_batch {worst:.2e} error bars, two starts {starts:.2e}; iterations {dev.n_iter}')
    assert worst <= 0.01 and starts <= 0.01
    assert np.all(np.abs(dev.theta - TRUTH_2COMP)[:, :10] <= 5 * err[:, :10])
    assert np.all(dev.chi2 <= runner.chi_squared(pix, np.repeat(TRUTH_2COMP[None], 8, axis=0)))
    np.testing.assert_allclose(dev.cov, host.cov, rtol=1e-6, atol=1e-12)


def test_fit_cube(two_components, engine):
    """A 2 x 2 stack: maps of the right shapes with the truth inside five error bars."""
    from nestfit_amd import lsq
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.synth import NU0, TRUTH_2COMP
    axes, data, ut, _ = two_components
    cubes = []
    for k, t in enumerate((1, 2)):
        f = axes[k]
        hdr = {'BUNIT': 'K', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz', 'CRVAL3': float(f[0]), 'CDELT3': float((f[-1] - f[0]) / 255),
               'CRPIX3': 1.0, 'RESTFRQ': NU0[t], 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CRVAL1': 270.0, 'CRVAL2': -20.0,
               'CDELT1': -1e-3, 'CDELT2': 1e-3, 'CRPIX1': 1.0, 'CRPIX2': 1.0, 'CUNIT1': 'deg', 'CUNIT2': 'deg',
               'NAXIS1': 2, 'NAXIS2': 2, 'NAXIS3': 256, 'NAXIS': 3}
        arr = data[:, k * 256:(k + 1) * 256].reshape(2, 2, 256).transpose(2, 1, 0)      # (chan, lat, lon); pixel p = i_lon * 2 + i_lat
        cubes.append(DataCube(SimpleCube(hdr, arr), 0.1, trans_id=t))
    engine.set_exp_mode('table')
    fit = lsq.fit_cube(CubeStack(cubes), ut, engine.AmmoniaRunner, ncomp=2, n_draws=2048, n_starts=4, seed=1)
    assert fit.params.shape == fit.errors.shape == (12, 2, 2)
    assert fit.chi2.shape == fit.status.shape == fit.lnL.shape == (2, 2)
    assert np.all(fit.status == 'converged'), fit.status
    assert np.isfinite(fit.lnL).all() and np.all(fit.chi2 < 512 + 5 * np.sqrt(2 * 512))
    off = np.abs(fit.params - TRUTH_2COMP[:, None, None])[:10] / fit.errors[:10]
    print(f'fit_cube: chi2 {fit.chi2.ravel()}, truth within {off.max():.2f} error bars')
    assert np.all(off <= 5) and np.all(fit.errors[10:] == 0)
