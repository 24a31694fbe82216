"""An uncertain noise level per spectrum integrated out on the device (nfa_specset_set_noise_uncertainty,
`noise_uncertainty=`): lnl_of_item turns the chi^2 parts of every set kind into -(a + nu / 2) log1p(h / a).

Two references.  The transform alone: the SAME set's lnL without the uncertainty, L0 = -h, through -c log1p(-L0 / a) in
float64 -- a division, a product and two log1p implementations of <= 2 ulp each: 16 eps |got|.  The whole: tests/
nmarg_restatement.py (longdouble, the chi^2 of the restatements that exist) on model spectra of the oracle, with the bound

    |lnL - want| <= max_s (c_s / a_s) LNL_RTOL[mode] M + 16 eps sum_s |lnL_s|

M and LNL_RTOL the kind's own (tests/test_templates.py, test_correlation.py): the existing bound on h carried through
|d lnL_s / d h| <= c / a, plus the transform's rounding.
"""
import functools
import os
import threading

import numpy as np
import pytest

import nmarg_restatement as nr
import tmpl_cases as tc
from test_calibration import GAUSS_NU, _make, _models, _priors
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands import _served_by_the_ring
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, _simple_priors
from test_templates import DV, _boundary_case, _gauss_axis

pytestmark = pytest.mark.gpu

NFA_ERR_ARG = 1
EPS = np.finfo(np.float64).eps


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _a_c(f, nu):
    """(a, c) as the engine forms them, in float64."""
    a = 1.0 / (4.0 * f * f)
    return a, a + 0.5 * nu


def _transform(L0, f, nu):
    a, c = _a_c(f, nu)
    return -c * np.log1p(np.maximum(-L0, 0.0) / a)


# ---------------------------------------------------------------------------- 1. exactness of the transform
def _kinds(na, n):
    """(label, noise, runner keywords) of the one-spectrum sets: every kind of chi^2 part there is."""
    return (('scalar', 0.1, {}),
            ('channel noise, masked', tc.channel_noise(n, 7 * n), {}),
            ('baseline 1', 0.1, dict(baseline_order=1)),
            ('ripple', 0.1, dict(templates=[na.ripple(n, n / 2.3)])),
            ('correlated', 0.1, dict(correlation=na.HANNING)),
            ('smoothed', 0.1, dict(**na.smoothed(na.HANNING_RESPONSE))))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2])
def test_the_transform_is_exact(engine, ncomp, mode, mode_guard):
    """One-spectrum Gaussian sets of 4, 64, 65 and 300 channels, 64 rows: got = -c log1p(-L0 / a) within 16 eps |got|, L0 the
    same set's lnL without the uncertainty; spectra out to the bit those of the set without it; null_lnZ likewise.

    Measured on an MI355X, the worst |got - want| / (16 eps |got|): table 0.084 (1 component), 0.076 (2); fast 0.072, 0.072."""
    import nestfit_amd as na
    engine.set_exp_mode(mode)
    worst = 0.0
    for n in (4, 64, 65, 300):
        x, thetas, preds, data = _boundary_case(n, ncomp)
        for label, noise, kw in _kinds(na, n):
            nu = nr.n_unmasked(noise, n)
            run = engine.GaussianRunner.from_data([x, np.array(data), noise, GAUSS_NU], None, ncomp=ncomp, **kw)
            spec0, L0 = run.predict_batch(thetas)
            null0 = run.null_lnZ
            for f in (0.05, 0.3, 0.5):
                run.set_noise_uncertainty(f)
                assert np.array_equal(run.noise_uncertainty, [f])
                spec, got = run.predict_batch(thetas)
                want = _transform(L0, f, nu)
                dev = np.abs(got - want) / (16 * EPS * np.abs(got) + 1e-300)
                assert np.isfinite(got).all() and (got <= 0).all() and (dev <= 1.0).all(), (n, label, f, dev.max())
                worst = max(worst, float(dev.max()))
                assert np.array_equal(spec, spec0)
                assert np.array_equal(run.predict_batch(thetas, want_spectra=False)[1], got)
                assert abs(run.null_lnZ - _transform(null0, f, nu)) <= 16 * EPS * abs(run.null_lnZ)
            run.set_noise_uncertainty(None)
            assert run.noise_uncertainty is None and run.null_lnZ == null0
            assert np.array_equal(run.predict_batch(thetas, want_spectra=False)[1], L0)
    print(f'transform {mode} ncomp={ncomp}: worst |got - want| / (16 eps |got|) {worst:.3f}')


# ---------------------------------------------------------------------------- 2. several spectra, against the restatement
@functools.lru_cache(maxsize=None)
def _rows(name, ncomp, chan):
    """The rows [axis, data, noise, what] of a model case: the truth's spectra plus noise; chan: a noise per channel with masked
    channels."""
    axes, _, clean, _, _ = _models(name, ncomp)
    rng = np.random.default_rng(900 + 7 * ncomp + (50 if chan else 0) + len(name))
    rows, at = [], 0
    for k, (x, what) in enumerate(axes):
        n = x.size
        noise = tc.channel_noise(n, 31 + k, base=0.1) if chan else NOISE
        scatter = np.where(np.isfinite(noise), noise, 0.0) * np.ones(n)
        rows.append([x, clean[at:at + n] + rng.normal(0, 1, n) * scatter, noise, what])
        at += n
    return rows


@functools.lru_cache(maxsize=None)
def _restated(name, ncomp, chan, f):
    _, _, _, _, preds = _models(name, ncomp)
    out = nr.restate(_rows(name, ncomp, chan), preds, f)
    null = nr.restate(_rows(name, ncomp, chan), np.zeros((1, preds.shape[1])), f)
    return out, null


def _against_the_restatement(engine, name, ncomp, mode, fs, chans=(False, True)):
    engine.set_exp_mode(mode)
    _, _, _, thetas, _ = _models(name, ncomp)
    worst = 0.0
    for chan in chans:
        rows = _rows(name, ncomp, chan)
        for f in fs:
            (want, M, mag, slope), (null_want, null_M, _, _) = _restated(name, ncomp, chan, f)
            run = _make(engine, name, rows, None, ncomp, noise_uncertainty=f)
            assert np.array_equal(run.noise_uncertainty, f)
            _, lnl = run.predict_batch(np.array(thetas), want_spectra=False)
            bound = slope * LNL_RTOL[mode] * M + 16 * EPS * mag
            dev = np.abs(lnl - want) / bound
            assert np.isfinite(lnl).all() and (dev <= 1.0).all(), (chan, f, dev.max(), int(np.argmax(dev)))
            worst = max(worst, float(dev.max()))
            # ... and the uncertainty is what makes the difference
            plain = _make(engine, name, rows, None, ncomp)
            assert (np.abs(plain.predict_batch(np.array(thetas), want_spectra=False)[1] - want) > 100 * bound).sum() > N_ROWS // 2
            assert abs(run.null_lnZ - null_want[0]) <= 1e-12 * null_M[0] * slope, (run.null_lnZ, null_want[0])
    print(f'noise uncertainty {name} {mode} ncomp={ncomp}: worst |got - want| / bound {worst:.2e}')
    return worst


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [2, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2), 300 channels, 200 rows, f = (0.1, 0.3) and (0.2, 0): a scalar noise and a noise per channel with
    masked channels.  Measured on an MI355X, the worst |got - want| over the bound for 2 and 4 components: table 5.6e-9, 2.4e-9
    (the bound is c / a = 55 times 1e-9 M, the deviation a few 1e-16 M); fast 2.1e-4, 1.5e-4."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode, ((0.1, 0.3), (0.2, 0.0)))


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances.  Measured on an MI355X: table 1.5e-9 of the bound, fast 3.2e-6."""
    _against_the_restatement(engine, 'n2hp', 2, mode, ((0.3,),))


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_layered_mix_against_the_restatement(engine, mode, mode_guard):
    """A blend and a line of two species, filled and layered, two layers: FILL and LAYER on.  Measured on an MI355X: table 1.0e-9
    of the bound, fast 1.0e-4."""
    _against_the_restatement(engine, 'filled', 2, mode, ((0.1, 0.3), (0.2, 0.0)))


@pytest.mark.parametrize('mode', MODES)
def test_a_spectrum_without_uncertainty_keeps_its_bits(engine, mode, mode_guard):
    """f = (0.2, 0): the second spectrum's term is the plain set's to the bit -- at p = 0 in null_lnZ's own column, and at every
    row as the sum, in spectrum order, of the first spectrum's marginal term and the second's plain one (one-spectrum sets)."""
    engine.set_exp_mode(mode)
    rows = _rows('ammonia', 2, True)
    _, _, _, thetas, _ = _models('ammonia', 2)
    thetas = np.array(thetas)
    mixed = _make(engine, 'ammonia', rows, None, 2, noise_uncertainty=(0.2, 0.0))
    plain = _make(engine, 'ammonia', rows, None, 2)
    first = _make(engine, 'ammonia', rows[:1], None, 2, noise_uncertainty=0.2)
    second = _make(engine, 'ammonia', rows[1:], None, 2)
    null_m, null_p = mixed._ss.null_lnZ(), plain._ss.null_lnZ()
    assert null_m[0, 1] == null_p[0, 1] and null_m[0, 0] != null_p[0, 0]
    assert null_m[0, 0] == first._ss.null_lnZ()[0, 0]
    t1 = first.predict_batch(thetas, want_spectra=False)[1]
    l2 = second.predict_batch(thetas, want_spectra=False)[1]
    assert np.array_equal(mixed.predict_batch(thetas, want_spectra=False)[1], t1 + l2)


# ---------------------------------------------------------------------------- 3. null_lnZ
@pytest.mark.parametrize('mode', MODES)
def test_null_lnz_is_the_likelihood_without_a_line(engine, mode, mode_guard):
    """null_lnZ is the device's lnL at a parameter vector whose line lies far off the band, to the bit (spectra of one row of
    64 channels and less, where the two sums run in one order), and the restatement's at p = 0 within 1e-12 M c / a."""
    import nestfit_amd as na
    engine.set_exp_mode(mode)
    for n in (4, 64):
        x, thetas, preds, data = _boundary_case(n, 1)
        away = np.array([[4000.0, 1.0, 2.0]])
        for label, noise, kw in _kinds(na, n):
            rows = [[x, np.array(data), noise, GAUSS_NU]]
            run = engine.GaussianRunner.from_data(rows[0], None, ncomp=1, noise_uncertainty=0.3, **kw)
            spec, lnl = run.predict_batch(away)
            assert not spec.any()
            assert lnl[0] == run.null_lnZ == float(run._ss.null_lnZ().sum()), (n, label, lnl[0], run.null_lnZ)
            rho = [kw['correlation']] if 'correlation' in kw else None
            taps = [kw['response']] if 'response' in kw else None
            want, M, _, slope = nr.restate(rows, np.zeros((1, n)), (0.3,), kw.get('baseline_order'), kw.get('templates'), rho, taps)
            assert abs(run.null_lnZ - want[0]) <= 1e-12 * M[0] * slope, (n, label)


# ---------------------------------------------------------------------------- 4. every launch form
@pytest.mark.parametrize('mode', MODES)
def test_the_same_bits_on_every_route(engine, mode, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingClient, RingServer
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _priors(engine, 'ammonia')
    rows = _rows('ammonia', 2, False)
    kw = dict(noise_uncertainty=(0.1, 0.3))
    run = _make(engine, 'ammonia', rows, ut, 2, **kw)
    bare = _make(engine, 'ammonia', rows, ut, 2)
    # host and device batches, coalescing 8 and 1, single points and a handful
    U, theta, lnl = _routes(engine, run, rng)
    assert not np.array_equal(bare.loglikelihood_batch(U.copy()), lnl)
    for split in (1, 2, 4):                                                   # ... whatever the row split of a small launch
        _ffi.set_option('lnl_split', split)
        run_s = _make(engine, 'ammonia', rows, ut, 2, **kw)                   # (a runner reads the option when it is made)
        for k in (0, 7, 150):
            u = U[k].copy()
            assert run_s.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k]), split
        few = U[20:31].copy()
        assert np.array_equal(run_s.loglikelihood_batch(few), lnl[20:31]), split
        assert np.array_equal(run_s.loglikelihood_batch(U[:300].copy()), lnl[:300]), split
        assert np.array_equal(run_s.predict_batch(theta[:40])[1], lnl[:40]), split
    _ffi.set_option('lnl_split', 0)
    lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
    assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
    # the resident ring kernel, and the host's serving loop
    tr_, lr_ = _served_by_the_ring(run, U[:24], f'nfa_test_ring_nmarg_dev_{os.getpid()}')
    assert np.array_equal(tr_, theta[:24]) and np.array_equal(lr_, lnl[:24])
    ring = f'nfa_test_ring_nmarg_{os.getpid()}'
    with RingServer(ring, n_slots=1, runner=run) as server:
        t = threading.Thread(target=server.serve, kwargs=dict(max_wait_us=100, idle_ms=20000))
        t.start()
        got_t, got_l = [], []
        with RingClient(ring, wait_ms=20000) as client:
            for row in U[:24]:
                th = row.copy()
                got_l.append(client.loglikelihood(th))
                got_t.append(th)
        server.stop()
        t.join(timeout=30)
        assert not t.is_alive()
    assert np.array_equal(np.array(got_t), theta[:24]) and np.array_equal(np.array(got_l), lnl[:24])
    # predict_batch's lnL, with spectra out and without, whatever the batch; the spectra those of the set without the uncertainty
    spec, pl = run.predict_batch(theta[:40])
    assert np.array_equal(pl, lnl[:40]) and np.array_equal(run.predict_batch(theta[:40], want_spectra=False)[1], lnl[:40])
    assert np.array_equal(spec, bare.predict_batch(theta[:40])[0])
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]


@pytest.mark.parametrize('mode', MODES)
def test_a_nan_row_stays_nan(engine, mode, mode_guard):
    """A NaN parameter, or a NaN in the data, gives NaN as in every other set (tests/test_layered.py), never the marginal's
    largest value 0: through batches, a single point, the ring's host loop and the resident ring kernel; also where the part is
    clamped at 0 (templates).  The sampler's update turns NaN into log_zero and relies on it."""
    from nestfit_amd import _ffi
    from nestfit_amd._model import noise_marginal_lnl
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    ut = _priors(engine, 'ammonia')
    rows = _rows('ammonia', 2, False)
    _, _, _, thetas, _ = _models('ammonia', 2)
    thetas = np.array(thetas[:64])
    bad = thetas.copy()
    at = (5, 17, 40, 63)
    bad[at, (0, 5, 6, 9)] = np.nan
    keep = ~np.isin(np.arange(64), at)
    for kw in ({}, dict(baseline_order=1, templates=tc.model_templates(2, 'both'))):
        run = _make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=(0.1, 0.3), **kw)
        plain = _make(engine, 'ammonia', rows, ut, 2, **kw)
        good = run.predict_batch(thetas, want_spectra=False)[1]
        lnl, lnl_p = (r.predict_batch(bad, want_spectra=False)[1] for r in (run, plain))
        assert np.array_equal(np.isnan(lnl), np.isnan(lnl_p)) and np.isnan(lnl).any(), (lnl[list(at)], lnl_p[list(at)])
        assert np.array_equal(lnl[keep], good[keep]) and np.isfinite(good).all() and (good < 0).all()
        for k in at:                                                            # a batch of one row
            assert np.isnan(run.predict_batch(bad[k:k + 1], want_spectra=False)[1][0]) == np.isnan(lnl_p[k])
    # a NaN in the data of an unmasked channel: every row of every route is NaN
    run = _make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=(0.1, 0.3))
    data = np.ascontiguousarray(np.concatenate([r[1] for r in rows]))
    data[17] = np.nan
    _ffi.check(lib.nfa_specset_set_data(run._ss.handle, 0, _ffi.dptr(data)))
    U = np.random.default_rng(31).uniform(size=(40, 12))
    assert np.isnan(run.loglikelihood_batch(U.copy())).all()                    # host batch
    assert np.isnan(run.loglikelihood_batch(U[:5].copy())).all()                # a handful
    assert all(np.isnan([run.loglikelihood(U[k].copy()) for _ in range(4)]).all() for k in (0, 7))      # single points, the captured graph
    assert np.isnan(_served_by_the_ring(run, U[:8], f'nfa_test_ring_nmarg_nan_{os.getpid()}')[1]).all()   # the resident ring kernel
    assert np.isnan(_through_a_broker(engine, run, U[:16].reshape(4, 4, -1))[0]).all()
    assert np.isnan(run._ss.null_lnZ()[0, 0]) and np.isfinite(run._ss.null_lnZ()[0, 1])
    # ... and the host's numpy form agrees
    assert np.isnan(noise_marginal_lnl(np.nan, 300, 0.3)) and np.isnan(noise_marginal_lnl(np.array([np.nan, 1.0]), 300, 0.3)[0])


# ---------------------------------------------------------------------------- 5. nu per pixel
@pytest.mark.parametrize('mode', MODES)
def test_every_pixel_counts_its_own_channels(engine, mode, mode_guard):
    """A CubeRunner of 2 x 2 pixels with different masked channels: each pixel's lnL and null_lnZ are those of its own
    one-pixel runner."""
    from nestfit_amd.cube import CubeRunner
    engine.set_exp_mode(mode)
    n, n_pix = 130, 4
    rng = np.random.default_rng(29)
    velo, x = _gauss_axis(n)
    thetas = np.stack([np.array([velo[40 + 7 * k] + 0.1, 1.5 * DV * 2, 1.0 + 0.2 * k]) for k in range(8)])
    j = np.arange(n)
    noise = rng.uniform(0.1, 0.2, (n_pix, n))
    data = rng.normal(0, 1, (n_pix, n)) * noise + 1.2 * np.exp(-0.5 * ((j - 60.0) / 3.0) ** 2)
    for p, masked in enumerate(([], [3], list(range(60, 70)), list(range(0, 128, 2)))):
        noise[p, masked] = np.inf
    kw = dict(ncomp=1, model=2, rest_freqs=[GAUSS_NU], noise_uncertainty=0.3)
    cube = CubeRunner([x], [-1], data, noise, None, **kw)
    assert np.array_equal(cube.noise_uncertainty, [0.3])
    nus = [n, n - 1, n - 10, n - 64]
    for p in range(n_pix):
        one = CubeRunner([x], [-1], data[p:p + 1], noise[p:p + 1], None, **kw)
        got = cube.predict_batch(np.full(8, p, dtype=np.int32), thetas, want_spectra=False)[1]
        assert np.array_equal(got, one.predict_batch(np.zeros(8, dtype=np.int32), thetas, want_spectra=False)[1]), p
        assert cube.null_lnZ[p] == one.null_lnZ[0]
        # ... and nu is what the pixel's mask leaves
        one.set_noise_uncertainty(None)
        L0 = one.predict_batch(np.zeros(8, dtype=np.int32), thetas, want_spectra=False)[1]
        assert (np.abs(got - _transform(L0, 0.3, nus[p])) <= 16 * EPS * np.abs(got)).all(), p
    mean, std = cube.fit_noise(np.arange(n_pix), np.tile(np.array([velo[60], 3.0 * DV, 1.2]), (n_pix, 1)))
    assert mean.shape == std.shape == (n_pix, 1) and (np.abs(mean - 1.0) < 4 * std).all() and (std > 0.03).all() and (std < 0.12).all()


# ---------------------------------------------------------------------------- 6. state
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('chan', [False, True])
def test_setting_and_removing_on_a_live_runner(engine, chan, mode, mode_guard):
    import nestfit_amd as na
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    rows = _rows('ammonia', 2, chan)
    ut = _priors(engine, 'ammonia')
    U = np.random.default_rng(19).uniform(size=(300, 12))
    u = np.full(12, 0.41)
    f = np.array([0.1, 0.3])

    def bits(run):
        """host batch, a single point (whose graph is captured on the third call), null_lnZ"""
        return run.loglikelihood_batch(U.copy()), [run.loglikelihood(u.copy()) for _ in range(4)][-1], run._ss.null_lnZ()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    fresh = bits(_make(engine, 'ammonia', rows, ut, 2))
    made = _make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=f)
    only = bits(made)
    run = _make(engine, 'ammonia', rows, ut, 2)
    out = np.zeros(2)
    assert lib.nfa_specset_noise_uncertainty(run._ss.handle, None) == 0 and lib.nfa_specset_noise_uncertainty(None, None) == 0
    plain_null = run.null_lnZ
    for turn in range(2):
        run.set_noise_uncertainty(f)
        assert lib.nfa_specset_noise_uncertainty(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out, f)
        got = bits(run)
        assert same(got, only) and not np.array_equal(got[0], fresh[0]) and got[1] != fresh[1]
        assert run.null_lnZ == made.null_lnZ == float(got[2].sum()) and run.null_lnZ != plain_null       # null_lnZ follows
        assert [s.noise_uncertainty for s in run.spectra] == [0.1, 0.3]
        run.set_noise_uncertainty((0.2, 0.0))                                                       # one for another
        assert not same(bits(run), only)
        run.set_noise_uncertainty(None if turn else (0, 0))
        assert run.noise_uncertainty is None and lib.nfa_specset_noise_uncertainty(run._ss.handle, None) == 0
        assert same(bits(run), fresh) and run.null_lnZ == plain_null, turn                         # the fresh set's bits
        assert all(s.noise_uncertainty is None for s in run.spectra)
    # the setter commutes with the others: the same bits in either order and as a set made that way
    others = [('set_baseline', 1, dict(baseline_order=1)), ('set_templates', tc.model_templates(2, 'mixed'), dict(templates=tc.model_templates(2, 'mixed')))]
    if not chan:                                                                                    # (no masked channel under a correlation or a response)
        others += [('set_correlation', na.HANNING, dict(correlation=na.HANNING)),
                   ('set_response', na.HANNING_RESPONSE, dict(response=na.HANNING_RESPONSE))]
    for setter, value, kw in others:
        want = bits(_make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=f, **kw))
        bare = _make(engine, 'ammonia', rows, ut, 2, **kw)
        without = bits(bare)
        a = _make(engine, 'ammonia', rows, ut, 2)
        a.set_noise_uncertainty(f)
        getattr(a, setter)(value)
        b = _make(engine, 'ammonia', rows, ut, 2)
        getattr(b, setter)(value)
        b.set_noise_uncertainty(f)
        assert same(bits(a), want) and same(bits(b), want) and not same(want, without), setter
        assert a.null_lnZ == b.null_lnZ == float(want[2].sum()), setter
        a.set_noise_uncertainty(None)
        assert same(bits(a), without) and a.null_lnZ == bare.null_lnZ, setter
        # ... and the other one removed from under the uncertainty: the uncertain set alone, its null_lnZ too
        getattr(b, setter)(None)
        assert same(bits(b), only) and b.null_lnZ == made.null_lnZ == float(only[2].sum()), setter
    # new data for such a set (nfa_specset_set_data): a set made with them
    rng = np.random.default_rng(23)
    new = [[r[0], r[1] + rng.normal(0, 0.05, r[1].size), r[2], r[3]] for r in rows]
    data = np.ascontiguousarray(np.concatenate([r[1] for r in new]))
    _ffi.check(lib.nfa_specset_set_data(made._ss.handle, 0, _ffi.dptr(data)))
    again = _make(engine, 'ammonia', new, ut, 2, noise_uncertainty=f)
    changed = made.loglikelihood_batch(U.copy())
    assert np.array_equal(changed, again.loglikelihood_batch(U.copy())) and not np.array_equal(changed, only[0])
    assert np.array_equal(made._ss.null_lnZ(), again._ss.null_lnZ())


@pytest.mark.parametrize('mode', MODES)
def test_no_uncertainty_is_the_runner_without_the_argument(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    rows = _rows('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    bare = _make(engine, 'ammonia', rows, ut, 2)
    U, theta, lnl = _routes(engine, bare, np.random.default_rng(7))
    for f in (None, 0, (0.0, 0.0)):
        run = _make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=f)
        assert run.noise_uncertainty is None
        U2, theta2, lnl2 = _routes(engine, run, np.random.default_rng(7))
        assert np.array_equal(U2, U) and np.array_equal(theta2, theta) and np.array_equal(lnl2, lnl)
        assert run.null_lnZ == bare.null_lnZ


def test_refusals(engine, mode_guard):
    from nestfit_amd import _ffi
    lib = _ffi.load()
    rows = _rows('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    U = np.random.default_rng(3).uniform(size=(200, 12))
    out = np.zeros(2)

    def rc_of(run, f):
        f = np.ascontiguousarray(f, dtype=np.float64)
        return lib.nfa_specset_set_noise_uncertainty(run._ss.handle, _ffi.dptr(f))
    # bad values through the C ABI: NFA_ERR_ARG with a reason, and the set is what it was -- with an uncertainty, or not
    for run, state in ((_make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=(0.1, 0.3)), 1), (_make(engine, 'ammonia', rows, ut, 2), 0)):
        before = run.loglikelihood_batch(U.copy())
        for bad in ((0.1, np.nan), (np.inf, 0.1), (-0.01, 0.1), (0.1, 0.5000001), (0.1, -np.inf)):
            assert rc_of(run, bad) == NFA_ERR_ARG and b'noise uncertainty' in lib.nfa_last_error(), bad
            assert lib.nfa_specset_noise_uncertainty(run._ss.handle, _ffi.dptr(out)) == state
            assert state == 0 or np.array_equal(out, [0.1, 0.3])
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    assert lib.nfa_specset_set_noise_uncertainty(None, None) == NFA_ERR_ARG
    run = _make(engine, 'ammonia', rows, ut, 2)
    assert rc_of(run, (0.5, 0.0)) == 0 and lib.nfa_specset_noise_uncertainty(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out, [0.5, 0.0])
    # a calibrated set takes none, from the C ABI and from Python: the set as it was
    cal = _make(engine, 'ammonia', rows, ut, 2, calibration=0.1)
    before = cal.loglikelihood_batch(U.copy())
    assert rc_of(cal, (0.2, 0.2)) == NFA_ERR_ARG
    words = lib.nfa_last_error()
    assert b'noise uncertainty' in words and b'calibration' in words
    assert lib.nfa_specset_noise_uncertainty(cal._ss.handle, None) == 0
    assert rc_of(cal, (0.0, 0.0)) == 0                                          # removing what is not there is no error
    with pytest.raises(ValueError, match='noise uncertainty'):
        cal.set_noise_uncertainty(0.2)
    with pytest.raises(ValueError, match='noise uncertainty'):
        _make(engine, 'ammonia', rows, ut, 2, calibration=0.1, noise_uncertainty=0.2)
    assert np.array_equal(cal.loglikelihood_batch(U.copy()), before) and np.array_equal(cal.calibration, [0.1, 0.1])
    # ... and the other way round, in the same words
    run = _make(engine, 'ammonia', rows, ut, 2, noise_uncertainty=0.2)
    before = run.loglikelihood_batch(U.copy())
    c = np.array([0.1, 0.1])
    assert lib.nfa_specset_set_calibration(run._ss.handle, _ffi.dptr(c)) == NFA_ERR_ARG and lib.nfa_last_error() == words
    assert lib.nfa_specset_calibration(run._ss.handle, None) == 0
    assert lib.nfa_specset_set_calibration(run._ss.handle, None) == 0
    with pytest.raises(ValueError, match='noise uncertainty'):
        run.set_calibration(0.1)
    assert np.array_equal(run.loglikelihood_batch(U.copy()), before) and np.array_equal(run.noise_uncertainty, [0.2, 0.2])


# ---------------------------------------------------------------------------- 7. fit_noise
@pytest.mark.parametrize('mode', MODES)
def test_fit_noise_finds_an_understated_noise(engine, mode, mode_guard):
    """One Gaussian spectrum of 256 channels whose noise is stated 1.3 times too small: the posterior of the scale at the truth
    is 1.3 within its width, whatever the set profiles out or correlates; the runner's own chi^2 is the device's."""
    import nestfit_amd as na
    engine.set_exp_mode(mode)
    n = 256
    velo, x = _gauss_axis(n)
    truth = np.array([velo[128] + 0.1, 4.0 * DV, 1.5])
    rng = np.random.default_rng(11)
    white = rng.normal(size=n + 2)
    probe = engine.GaussianRunner.from_data([x, np.zeros(n), 1.0, GAUSS_NU], None, ncomp=1)
    model = probe.predict_batch(truth.reshape(1, -1))[0][0]
    for kw, noise in (({}, white[1:-1]), (dict(baseline_order=1), white[1:-1]), (dict(templates=[na.ripple(n, 37.3)]), white[1:-1]),
                      (dict(correlation=na.HANNING), (0.25 * white[:-2] + 0.5 * white[1:-1] + 0.25 * white[2:]) / np.sqrt(0.375))):
        run = engine.GaussianRunner.from_data([x, model + noise, 1.0 / 1.3, GAUSS_NU], None, ncomp=1, noise_uncertainty=0.3, **kw)
        mean, std = run.fit_noise(truth)
        assert mean.shape == std.shape == (1,) and abs(mean[0] - 1.3) < 3 * std[0] and 0.03 < std[0] < 0.08, (kw.keys(), mean, std)
        # the h behind it is the device's: lnL = -c log1p(h / a)
        from nestfit_amd._model import half_chi2, noise_marginal_lnl
        h, nu = half_chi2(run.spectrum.data, run.spectrum.get_spec(), run.spectrum.noise, kw.get('baseline_order'),
                          kw['templates'][0] if 'templates' in kw else None, kw.get('correlation'))
        lnl = run.predict_batch(truth.reshape(1, -1), want_spectra=False)[1][0]
        assert nu == n and lnl == pytest.approx(noise_marginal_lnl(h, nu, 0.3), rel=10 * LNL_RTOL[mode])
    with pytest.raises(ValueError, match='noise uncertainty'):
        probe.fit_noise(truth)


def _smoothed_noise(rng, shape):
    """Unit-variance white noise smoothed with the Hanning kernel along the last axis."""
    white = rng.normal(size=(*shape[:-1], shape[-1] + 2))
    return (0.25 * white[..., :-2] + 0.5 * white[..., 1:-1] + 0.25 * white[..., 2:]) / np.sqrt(0.375)


def _noise_scale_of(data, filtered_model, noise, rho, f):
    """`noise_fit` of the chi^2 of a model that is filtered already: ONE filter, the set's own."""
    from nestfit_amd._model import half_chi2, noise_fit
    return noise_fit(*half_chi2(data, filtered_model, noise, None, None, rho, None), f)


@pytest.mark.parametrize('mode', MODES)
def test_fit_noise_of_a_cube_filters_the_model_once(engine, mode, mode_guard):
    """A Gaussian cube of one spectrum of 64 channels and 2 pixels, lines of sigma = 1.5 channels, `smoothed(HANNING_RESPONSE)`
    and f = 0.3; the data are the filtered model plus Hanning-smoothed noise stated at 1 / 1.3 of its level.  `fit_noise` is
    `noise_fit` of the chi^2 of `predict_batch`'s spectra, which ARE the filtered model, to rel 1e-12: the same numpy on the
    same bits (filtering them again moved the mean by 2e-2).  A GaussianRunner of each pixel, whose spectrum holds the
    unfiltered model and whose chi^2 filters it on the host, agrees to rel 1e-9: the rounding of a five-tap sum."""
    import nestfit_amd as na
    from nestfit_amd.cube import CubeRunner
    engine.set_exp_mode(mode)
    n, stated, f = 64, 0.1, 0.3
    velo, x = _gauss_axis(n)
    theta = np.array([[velo[30] + 0.1 * DV, 1.5 * DV, 1.5], [velo[41] - 0.2 * DV, 1.5 * DV, 0.8]])
    pix = np.arange(2, dtype=np.int32)
    kw = dict(ncomp=1, model=2, rest_freqs=[GAUSS_NU], **na.smoothed(na.HANNING_RESPONSE))
    probe = CubeRunner([x], [-1], np.zeros((1, n)), np.full((1, 1), stated), None, **kw)
    model, _ = probe.predict_batch(np.zeros(2, dtype=np.int32), theta)
    data = model + 1.3 * stated * _smoothed_noise(np.random.default_rng(23), model.shape)
    cube = CubeRunner([x], [-1], data, np.full((2, 1), stated), None, noise_uncertainty=f, **kw)
    mean, std = cube.fit_noise(pix, theta)
    assert mean.shape == std.shape == (2, 1)
    spec = cube.predict_batch(pix, theta)[0]
    assert np.array_equal(spec, model)
    for b in range(2):
        want = _noise_scale_of(data[b], spec[b], stated, cube.correlation[0], f)
        print(f'cube fit_noise {mode} pixel {b}: {mean[b, 0]!r} +- {std[b, 0]!r}, want {want!r}')
        assert (mean[b, 0], std[b, 0]) == pytest.approx(want, rel=1e-12)
        run = engine.GaussianRunner.from_data([x, data[b], stated, GAUSS_NU], None, ncomp=1, noise_uncertainty=f,
                                              **na.smoothed(na.HANNING_RESPONSE))
        one = run.fit_noise(theta[b])
        print(f'     GaussianRunner: {one[0][0]!r} +- {one[1][0]!r}')
        assert (one[0][0], one[1][0]) == pytest.approx((mean[b, 0], std[b, 0]), rel=1e-9)


@pytest.mark.parametrize('mode', MODES)
def test_fit_noise_of_a_layered_runner_filters_the_model_once(engine, mode, mode_guard):
    """A layered HyperfineRunner of two spectra of 64 channels, one component, the same response and f: `predict` goes through
    the runner's set, so the spectra hold the FILTERED model, and `fit_noise` is `noise_fit` of their chi^2 without another
    filter, to rel 1e-12."""
    import nestfit_amd as na
    import hf_restatement as hfr
    engine.set_exp_mode(mode)
    n, stated, f = 64, 0.05, 0.3
    tables = [engine.LineTable(72.4e9, [0.0], [1.0], name='one'), engine.LineTable(86.1e9, [-3.0, 2.0], [0.4, 0.6], name='two')]
    axes = [t.nu * (1.0 - np.linspace(10.0, -10.0, n) / hfr.CKMS) for t in tables]
    theta = np.array([0.3, 9.0, 0.2, 0.7])
    kw = dict(ncomp=1, layered=True, noise_uncertainty=f, **na.smoothed(na.HANNING_RESPONSE))
    probe = engine.HyperfineRunner.from_data([[x, np.zeros(n), stated, t] for x, t in zip(axes, tables)], None, **kw)
    model = probe.predict_batch(theta[None])[0][0]
    data = model + 1.3 * stated * _smoothed_noise(np.random.default_rng(29), (2, n)).reshape(-1)
    run = engine.HyperfineRunner.from_data([[x, data[k * n:(k + 1) * n], stated, t] for k, (x, t) in enumerate(zip(axes, tables))],
                                           None, **kw)
    mean, std = run.fit_noise(theta)
    assert mean.shape == std.shape == (2,)
    spec = run.predict_batch(theta[None])[0][0]
    assert np.array_equal(spec, model) and np.array_equal(np.concatenate([s.get_spec() for s in run.spectra]), spec)
    for k in range(2):
        want = _noise_scale_of(data[k * n:(k + 1) * n], spec[k * n:(k + 1) * n], stated, run.correlation[k], f)
        print(f'layered fit_noise {mode} spectrum {k}: {mean[k]!r} +- {std[k]!r}, want {want!r}')
        assert (mean[k], std[k]) == pytest.approx(want, rel=1e-12)


def test_a_cube_takes_and_drops_a_calibration(engine):
    """`CubeRunner.set_calibration`, the setter the one option surface gives the cube: on, the lnL is another; off, the one
    before, bit for bit; null_lnZ does not move."""
    from nestfit_amd.cube import CubeRunner
    n = 64
    velo, x = _gauss_axis(n)
    theta = np.array([[velo[30], 1.5 * DV, 1.5], [velo[41], 1.5 * DV, 0.8]])
    pix = np.arange(2, dtype=np.int32)
    data = np.random.default_rng(31).normal(0, 0.1, (2, n))
    cube = CubeRunner([x], [-1], data, np.full((2, 1), 0.1), None, ncomp=1, model=2, rest_freqs=[GAUSS_NU])
    before, null = cube.predict_batch(pix, theta, want_spectra=False)[1], cube.null_lnZ.copy()
    cube.set_calibration(0.1)
    assert np.array_equal(cube.calibration, [0.1]) and np.array_equal(cube.null_lnZ, null)
    assert not np.any(cube.predict_batch(pix, theta, want_spectra=False)[1] == before)
    cube.set_calibration(None)
    assert cube.calibration is None and np.array_equal(cube.null_lnZ, null)
    assert np.array_equal(cube.predict_batch(pix, theta, want_spectra=False)[1], before)


# ---------------------------------------------------------------------------- 8. the device sampler
def test_the_device_sampler_follows_the_twin(engine):
    """One Gaussian component, 64 channels, nlive 50, noise_uncertainty = 0.2: `fit_pixels(device=True)` against the numpy
    twin on the GPU's likelihood, as tests/test_sampler_dims.py does it for plain sets -- counts equal, lnZ to 1e-10, the table
    to rtol 1e-8; and the uncertainty is in it: another lnZ than the plain cube's."""
    from nestfit_amd import sampler
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import CKMS
    n, n_pix, noise = 64, 2, 0.1
    nu0 = 110.201354e9
    x = nu0 * (1.0 - np.linspace(20, -20, n) / CKMS)
    ut = _simple_priors(engine, [(-15, 15), (0.2, 3.0), (0.0, 5.0)])
    truths = np.array([[-2.0, 0.8, 2.0], [-1.7, 0.8, 2.0]])
    rng = np.random.default_rng(41)
    try:
        engine.set_exp_mode('table')
        kw = dict(ncomp=1, model=2, rest_freqs=[nu0])
        probe = CubeRunner([x], [-1], np.zeros((1, n)), np.full((1, 1), noise), ut, **kw)
        model, _ = probe.predict_batch(np.zeros(n_pix, dtype=np.int32), truths)
        data = model + rng.normal(0, 1.3 * noise, model.shape)
        cube = CubeRunner([x], [-1], data, np.full((n_pix, 1), noise), ut, noise_uncertainty=0.2, **kw)
        plain = CubeRunner([x], [-1], data, np.full((n_pix, 1), noise), ut, **kw)
        opts = dict(nlive=50, maxiter=400, tol=0.5, efr=0.3, seed=7, batch_target=2048)
        pix = np.arange(n_pix)
        dev = sampler.fit_pixels(cube, pix, device=True, time_limit=60, **opts)
        twin = sampler.fit_pixels(cube, pix, device=False, **opts)
        bare = sampler.fit_pixels(plain, pix, device=True, time_limit=60, **opts)
        for d, t, b in zip(dev, twin, bare):
            assert (d.n_iter, d.n_evals) == (t.n_iter, t.n_evals), (d.n_iter, t.n_iter, d.n_evals, t.n_evals)
            assert d.n_iter >= 4 * 50
            assert d.lnZ == pytest.approx(t.lnZ, rel=1e-10)
            np.testing.assert_allclose(d.posterior, t.posterior, rtol=1e-8, atol=1e-12)
            assert abs(d.lnZ - b.lnZ) > 1.0
    finally:
        engine.set_exp_mode('fast')


# ---------------------------------------------------------------------------- 9. the cube route
def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 2 x 2 cube of two lines through CubeFitter(runner_kwargs={'noise_uncertainty': ...}): the store carries the attribute,
    and the fit is the runner's."""
    import hf_restatement as hfr
    from nestfit_amd import hyperfine
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    tables = [engine.LineTable(72.4e9, [0.0], [1.0], name='one'), engine.LineTable(86.1e9, [-3.0, 2.0], [0.4, 0.6], name='two')]
    n_chan, n_side, noise = 128, 2, 0.05
    truth = np.array([0.3, 9.0, 0.2, 0.7])
    ranges = [(-2, 2), (4.0, 20.0), (-1.0, 1.0), (0.2, 1.5)]
    f = (0.2, 0.1)
    cubes = []
    for k, t in enumerate(tables):
        x = t.nu * (1.0 - np.linspace(10.0, -10.0, n_chan) / hfr.CKMS)
        clean = hfr.hf_predict(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(t), truth)
        data = np.random.default_rng(40 + k).normal(0, 1.3 * noise, (n_chan, n_side, n_side)) + clean[:, None, None]
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': t.nu}
        cubes.append(DataCube(SimpleCube(hdr, data), noise, lines=t))
    stack = CubeStack(cubes)
    ut = _simple_priors(engine, ranges)
    mn = {'nlive': 100, 'tol': 1.0, 'seed': 5}
    fitter = CubeFitter(stack, ut, hyperfine.HyperfineRunner, runner_kwargs={'noise_uncertainty': f}, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs=mn, nlive_snr_fact=0)
    assert np.array_equal(fitter.noise_uncertainty, f)
    runner, lon, lat = stack.to_device(ut, ncomp=1, model=3, noise_uncertainty=f)
    assert np.array_equal(runner.noise_uncertainty, f)
    mean, std = runner.fit_noise(np.arange(4), np.tile(truth, (4, 1)))
    assert mean.shape == (4, 2) and (np.abs(mean - 1.3) < 4 * std).all()
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    bare = CubeFitter(stack, ut, hyperfine.HyperfineRunner, lnZ_thresh=11, ncomp_max=1, mn_kwargs=mn, nlive_snr_fact=0)
    bare.fit_cube(str(tmp_path / 'bare'), nproc=1)
    with HdfStore(path) as store, HdfStore(str(tmp_path / 'bare')) as plain:
        got = store.read_model_noise_uncertainty()
        assert got.dtype == np.float64 and np.array_equal(got, f)
        assert plain.read_model_noise_uncertainty() is None and 'noise_uncertainty' not in plain.hdf.attrs
        groups = list(store.iter_pix_groups())
        plains = {(int(g.attrs['i_lon']), int(g.attrs['i_lat'])): g for g in plain.iter_pix_groups()}
        assert len(groups) == 4 and len(plains) == 4
        where = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(lon, lat))}
        for g in groups:
            i, j = int(g.attrs['i_lon']), int(g.attrs['i_lat'])
            fit = g['1']
            best = np.ascontiguousarray(np.asarray(fit['bestfit_params'][...], dtype=np.float64).reshape(1, -1))
            at = runner.predict_batch(np.array([where[(i, j)]]), best, want_spectra=False)[1][0]
            assert at == pytest.approx(float(fit.attrs['max_loglike']), rel=1e-9)
            assert float(fit.attrs['max_loglike']) != float(plains[(i, j)]['1'].attrs['max_loglike'])
