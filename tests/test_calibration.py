"""A calibration uncertainty per spectrum on the device (nfa_specset_set_calibration, `calibration=`): the gain g ~
N(1, s^2) of every spectrum is integrated out of the likelihood in closed form inside the calibrated kind of
lnl_kernel_kind.

The reference is tests/calib_restatement.py (the unsimplified closed form in longdouble, checked against a numerical integral
in tests/test_calibration_cpu.py) on model spectra of the other restatements and the oracle, at the sizes of the sibling
tests: 300 channels (four full rows of 64 and one of 44), 200 parameter rows, both modes.  The data of a case are a truth
spectrum times a gain per spectrum (1.12, 0.90), plus a ramp where a baseline is fitted, plus noise.  Even rows are theta
within a few percent of the truth, odd rows anywhere in the prior, so that A / sigma^2 runs from << 1 to >> 1 / s^2.

The bound.  lnL is a difference of large terms where the model dwarfs the data, so deviations are measured against the
size of the terms, M = sum_s (C + 2 |B| + A) / (2 sigma^2) + log1p(s^2 A / sigma^2) / 2, in the spirit of test_layered.py's
S: |got - want| <= k LNL_RTOL[mode] M with k = 1 -- every term carries the mode's relative error on `pred` once.

Measured on an MI355X, the worst |got - want| / M over the rows, baselines and noise kinds of a case (bound 1e-9 table, 1e-6 fast):

    ammonia (1,1)+(2,2), 1..3 components    table 7.0e-16, 6.5e-16, 6.7e-16    fast 2.1e-8, 1.5e-8, 1.2e-8
    N2H+ 2-1 (wide), 2 components           table 7.4e-16                      fast 8.7e-9
    a line table, 3 components              table 6.3e-16                      fast 8.3e-9
    a filled, layered mix, 2 layers         table 5.7e-16                      fast 1.3e-8
    a Gaussian runner, 2 components         table 9.0e-16                      fast 3.6e-9
    ammonia with cal = (0, 0.2)             table 5.5e-16                      fast 1.3e-8
    N2H+ 2-1, 10 components, one unit per workgroup    table 3.5e-16           fast 4.8e-9

k = 1 holds with a factor of 47 and more to spare; no case needs more.  The sampler run's numbers are in its test's docstring.
"""
import functools
import os

import numpy as np
import pytest

import calib_restatement as cr
import hf_restatement as hfr
import layer_restatement as lay
import lte_restatement as lr
from test_hyperfine import _through_a_broker
from test_layered import LINES3, MODELS, _ranges, _runner, _species, _spectra, draw_layers
from test_lte import _routes
from test_lte_bands_cpu import N_CHAN
from test_lte_cpu import B_ROT, MU
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _simple_priors

pytestmark = pytest.mark.gpu

GAINS = (1.12, 0.90)
CAL = {'ammonia': (0.1, 0.2), 'n2hp': (0.1,), 'lines': (0.15,), 'filled': (0.05, 0.3), 'gauss': (0.1,)}
GAUSS_NU = 110.201354e9
GAUSS_RANGES = [(-30, 30), (0.3, 5.0), (-2.0, 8.0)]             # voff, sigm, peak
ORDERS = (None, 0, 3)
K_BOUND = 1
NFA_ERR_ARG = 1


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


# ---------------------------------------------------------------------------- the cases
def _axes(name, na):
    """[(axis, what the restatement and the runner need of the spectrum)]; the Gaussian model: one spectrum and its rest frequency."""
    if name == 'gauss':
        return [(GAUSS_NU * (1.0 - np.linspace(40.0, -40.0, N_CHAN) / hfr.CKMS), GAUSS_NU)]
    return _spectra(name, na)


def _draw(rng, name, ncomp, row, truth):
    """Even rows: within a few percent of the truth (2 % of each parameter's size, 0.02 at the least).  Odd rows: anywhere in
    the prior; every fourth of them with every component thin (the low end of its depth parameter, peaks of mK for the
    Gaussians), so that a model far below the noise is among them whatever the number of components."""
    if row % 2 == 0:
        return truth + rng.normal(0, 0.02, truth.size) * np.maximum(np.abs(truth), 1.0)
    thin = row % 8 == 1
    if name == 'gauss':
        theta = np.concatenate([rng.uniform(lo, hi, ncomp) for lo, hi in GAUSS_RANGES])
        if thin:
            theta[2 * ncomp:] *= 1e-3
        return theta
    theta = draw_layers(rng, name, ncomp, 1)
    if thin:
        m = MODELS[name]
        theta[m['depth_row'] * ncomp:(m['depth_row'] + 1) * ncomp] = m['depth'][0] + rng.uniform(0.0, 0.3, ncomp)
        if name == 'filled':
            theta[4 * ncomp:5 * ncomp] = m['depth'][0] - rng.uniform(0.5, 2.0, ncomp)          # the isotopologue's column
    return theta


def _truth(name, ncomp):
    if name == 'gauss':
        return np.concatenate([np.linspace(-6.0, 9.0, ncomp), np.linspace(1.2, 2.5, ncomp), np.linspace(3.0, 1.5, ncomp)])
    return draw_layers(np.random.default_rng(700 + ncomp), name, ncomp, 0)


def _predict(nfo, na, name, axes, tbgs, theta):
    """The model spectra of the case's spectra, concatenated: the oracle's, or the restatements'; `filled` is layered."""
    out = []
    for (x, what), tbg in zip(axes, tbgs):
        if name in ('ammonia', 'n2hp', 'gauss'):
            s = (nfo.AmmoniaSpectrum(x, np.zeros(x.size), 1.0, what) if name == 'ammonia'
                 else nfo.DiazenyliumSpectrum(x, np.zeros(x.size), 1.0, what) if name == 'n2hp'
                 else nfo.Spectrum(x, np.zeros(x.size), 1.0, rest_freq=what))
            {'ammonia': nfo.amm_predict, 'n2hp': nfo.nnhp_predict, 'gauss': nfo.gauss_predict}[name](s, theta)
            out.append(s.get_spec())
        elif name == 'lines':
            out.append(hfr.hf_predict(nfo, x, tbg, hfr.table_of(what), theta))
        else:
            mol, ks, iso, isos = _species()
            out.append(lay.mix_layered(nfo, x, tbg, what, (mol, iso), theta, fill=True)[0])
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def _models(name, ncomp):
    """(axes, truth, its spectra, thetas, their spectra) of a case, computed once."""
    import nestfit_amd as na
    from oracle import nfo
    axes = _axes(name, na)
    tbgs = [hfr.tbg_of(nfo, x) for x, _ in axes]
    truth = _truth(name, ncomp)
    rng = np.random.default_rng(4000 + 10 * len(name) + ncomp)
    thetas = np.stack([_draw(rng, name, ncomp, k, truth) for k in range(N_ROWS)])
    clean = _predict(nfo, na, name, axes, tbgs, truth)
    preds = np.stack([_predict(nfo, na, name, axes, tbgs, th) for th in thetas])
    for a in (truth, thetas, clean, preds):
        a.setflags(write=False)
    return axes, truth, clean, thetas, preds


@functools.lru_cache(maxsize=None)
def _data(name, ncomp, order, chan):
    """The rows [axis, data, noise, what] of a case: the truth times the gains, a ramp where a baseline is fitted, noise.  chan: a
    noise per channel over 0.1..0.3 K that masks a stretch of 20 channels on the line and a few others."""
    axes, truth, clean, _, _ = _models(name, ncomp)
    rng = np.random.default_rng(50 + ncomp + (0 if order is None else 10 * (order + 1)) + (100 if chan else 0))
    rows = []
    for k, (x, what) in enumerate(axes):
        p = clean[k * N_CHAN:(k + 1) * N_CHAN]
        noise = NOISE
        if chan:
            noise = rng.uniform(0.1, 0.3, N_CHAN)
            at = int(np.argmax(np.abs(p)))
            noise[max(0, at - 12):at + 8] = np.inf
            noise[rng.integers(0, N_CHAN, 5)] = np.inf
        scatter = np.where(np.isfinite(noise), noise, 0.0)
        ramp = 0.0 if order is None else 0.3 + 0.4 * np.linspace(-1.0, 1.0, N_CHAN)
        rows.append([x, GAINS[k] * p + ramp + rng.normal(0, 1, N_CHAN) * scatter, noise, what])
    return rows


@functools.lru_cache(maxsize=None)
def _reference(name, ncomp, order, chan, cal=None):
    """(rows, thetas, lnL of the restatement, M, A / sigma^2 of every row and spectrum)."""
    _, _, _, thetas, preds = _models(name, ncomp)
    rows = _data(name, ncomp, order, chan)
    cal = CAL[name] if cal is None else cal
    want, M, a = np.zeros(N_ROWS), np.zeros(N_ROWS), np.zeros((N_ROWS, len(rows)))
    for i, pred in enumerate(preds):
        for k, (_, d, noise, _) in enumerate(rows):
            p = pred[k * N_CHAN:(k + 1) * N_CHAN]
            want[i] += float(cr.marginal_lnl(d, p, noise, cal[k], order))
            M[i] += float(cr.magnitude(d, p, noise, cal[k], order))
            a[i, k] = float(cr.products(d, p, noise, order)[0])
    for arr in (want, M, a):
        arr.setflags(write=False)
    return rows, thetas, want, M, a


def _make(engine, name, rows, ut, ncomp, **kw):
    if name == 'gauss':
        return engine.GaussianRunner.from_data(rows[0], ut, ncomp=ncomp, **kw)
    return _runner(engine, name, rows, ut, ncomp, **({'layered': True} if name == 'filled' else {}), **kw)


def _priors(engine, name):
    return _simple_priors(engine, GAUSS_RANGES if name == 'gauss' else _ranges(name))


# ---------------------------------------------------------------------------- 1. lnL against the restatement
def _against_the_restatement(engine, name, ncomp, mode, chans=(False,)):
    engine.set_exp_mode(mode)
    worst = 0.0
    for chan in chans:
        for order in ORDERS:
            rows, thetas, want, M, a = _reference(name, ncomp, order, chan)
            s2 = np.array(CAL[name]) ** 2
            # the draws hold what they are meant to hold: models far below the noise and far above the calibration's reach
            assert a.min() < 0.1 and (a * s2).max() > 100.0, (a.min(), (a * s2).max())
            run = _make(engine, name, rows, None, ncomp, baseline_order=order, calibration=CAL[name])
            assert np.array_equal(run.calibration, CAL[name]) and run.baseline_order == order
            _, lnl = run.predict_batch(np.array(thetas), want_spectra=False)
            dev = np.abs(lnl - want) / M
            print(f'calibrated {name} {mode} ncomp={ncomp} baseline={order} channel noise={chan}: worst |got - want| / M {dev.max():.2e} '
                  f'(bound {K_BOUND * LNL_RTOL[mode]:.0e}), |lnL| {np.abs(want).min():.3g} .. {np.abs(want).max():.3g}')
            assert np.isfinite(lnl).all() and (dev <= K_BOUND * LNL_RTOL[mode]).all(), (order, chan, dev.max())
            # ... and the calibration is what makes the difference
            plain = _make(engine, name, rows, None, ncomp, baseline_order=order)
            assert plain.calibration is None
            assert (np.abs(plain.predict_batch(np.array(thetas), want_spectra=False)[1] - want) > 100 * LNL_RTOL[mode] * M).sum() > N_ROWS // 2
            worst = max(worst, float(dev.max()))
    return worst


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2), cal (0.1, 0.2): a scalar noise and a noise per channel with a masked stretch; baselines None, 0, 3."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode, chans=(False, True))


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances."""
    _against_the_restatement(engine, 'n2hp', 2, mode)


@pytest.mark.parametrize('mode', MODES)
def test_a_line_table_against_the_restatement(engine, mode, mode_guard):
    _against_the_restatement(engine, 'lines', 3, mode)


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_layered_mix_against_the_restatement(engine, mode, mode_guard):
    """A blend and a line of two species, filled and layered, two layers, cal (0.05, 0.3): FILL and LAYER on."""
    _against_the_restatement(engine, 'filled', 2, mode, chans=(False, True))


@pytest.mark.parametrize('mode', MODES)
def test_a_gaussian_runner_against_the_restatement(engine, mode, mode_guard):
    _against_the_restatement(engine, 'gauss', 2, mode)


# ---------------------------------------------------------------------------- 2. s = 0
@pytest.mark.parametrize('mode', MODES)
def test_no_uncertainty_for_one_spectrum_of_a_calibrated_set(engine, mode, mode_guard):
    """cal = (0, 0.2): the first spectrum keeps its plain chi^2, the second is marginalised."""
    engine.set_exp_mode(mode)
    for order in (None, 1):
        rows, thetas, want, M, _ = _reference('ammonia', 2, order, False, cal=(0.0, 0.2))
        run = _make(engine, 'ammonia', rows, None, 2, baseline_order=order, calibration=(0, 0.2))
        assert np.array_equal(run.calibration, [0.0, 0.2])
        _, lnl = run.predict_batch(np.array(thetas), want_spectra=False)
        dev = np.abs(lnl - want) / M
        print(f'cal (0, 0.2) {mode} baseline={order}: worst |got - want| / M {dev.max():.2e}')
        assert (dev <= K_BOUND * LNL_RTOL[mode]).all()


@pytest.mark.parametrize('mode', MODES)
def test_a_spectrum_without_uncertainty_keeps_its_bits(engine, mode, mode_guard):
    """The s2 == 0 select of the epilogue and p = 0, to the bit.  Two spectra of one line table, four components (the general
    component form with and without a calibration), a baseline of order 1; the second spectrum's axis lies 500 km/s off, so no
    line reaches it and its model is zero in every row.  With cal = (0, 0.2) the first spectrum has s = 0 and the second A = B =
    0: both parts are the uncalibrated set's, so lnL is, bit for bit."""
    engine.set_exp_mode(mode)
    table = engine.LineTable(*LINES3, name='three')
    rng = np.random.default_rng(29)
    rows = [[LINES3[0] * (1.0 - (np.linspace(20.0, -20.0, N_CHAN) + off) / hfr.CKMS), rng.normal(0.5, NOISE, N_CHAN), NOISE, table]
            for off in (0.0, 500.0)]
    thetas = np.stack([draw_layers(rng, 'lines', 4, k) for k in range(N_ROWS)])
    bare = engine.HyperfineRunner.from_data(rows, None, ncomp=4, baseline_order=1)
    spec, want = bare.predict_batch(thetas)
    assert np.abs(spec[:, :N_CHAN]).max() > 1.0 and not spec[:, N_CHAN:].any()
    got = engine.HyperfineRunner.from_data(rows, None, ncomp=4, baseline_order=1, calibration=(0, 0.2)).predict_batch(thetas, want_spectra=False)[1]
    assert np.array_equal(got, want)
    other = engine.HyperfineRunner.from_data(rows, None, ncomp=4, baseline_order=1, calibration=(0.1, 0.2)).predict_batch(thetas, want_spectra=False)[1]
    assert (other != want).sum() > N_ROWS // 2


@pytest.mark.parametrize('mode', MODES)
def test_a_launch_whose_sixth_slot_does_not_fit(engine, mode, mode_guard):
    """N2H+ 2-1 (40 lines), ten components, two waves per unit: in the table mode a baseline set's workgroup of eight waves
    holds four units in 158 KB, the calibrated set's would need 166 KB, and plan_lnl gives it one unit per workgroup
    (tests/test_calibration_cpu.py holds the plan to that).  The bits are those of one wave per unit, and the restatement's
    within the bound."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rows, thetas, want, M, _ = _reference('n2hp', 10, 1, False)
    lnl = {}
    for split in (1, 2):
        _ffi.set_option('lnl_split', split)
        run = _make(engine, 'n2hp', rows, None, 10, baseline_order=1, calibration=CAL['n2hp'])       # (a runner reads the option when it is made)
        lnl[split] = run.predict_batch(np.array(thetas), want_spectra=False)[1]
    _ffi.set_option('lnl_split', 0)
    assert np.array_equal(lnl[1], lnl[2]) and np.isfinite(lnl[2]).all()
    dev = np.abs(lnl[2] - want) / M
    print(f'calibrated n2hp {mode} ncomp=10, one unit per workgroup: worst |got - want| / M {dev.max():.2e}')
    assert (dev <= K_BOUND * LNL_RTOL[mode]).all()


@pytest.mark.parametrize('mode', MODES)
def test_no_calibration_is_the_runner_without_the_argument(engine, mode, mode_guard):
    """calibration=None, 0 and (0, 0): the bits of a runner built without the argument, through host batches, device batches and
    single points -- the set's former kernels (two components: the unrolled, packed forms)."""
    engine.set_exp_mode(mode)
    rows = _data('ammonia', 2, None, False)
    ut = _priors(engine, 'ammonia')
    bare = _runner(engine, 'ammonia', rows, ut, 2)
    U, theta, lnl = _routes(engine, bare, np.random.default_rng(7))
    for cal in (None, 0, (0, 0), 0.0, np.zeros(2)):
        run = _runner(engine, 'ammonia', rows, ut, 2, calibration=cal)
        assert run.calibration is None
        U2, theta2, lnl2 = _routes(engine, run, np.random.default_rng(7))
        assert np.array_equal(U2, U) and np.array_equal(theta2, theta) and np.array_equal(lnl2, lnl), cal
        assert run.null_lnZ == bare.null_lnZ
    with pytest.raises(ValueError, match='no calibration uncertainty'):
        bare.fit_gain(theta[0])


# ---------------------------------------------------------------------------- 3. setting and removing, 4. null_lnZ
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('chan', [False, True])
def test_setting_and_removing_on_a_live_runner(engine, chan, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    rows = _data('ammonia', 2, 0, chan)
    ut = _priors(engine, 'ammonia')
    rng = np.random.default_rng(19)
    U = rng.uniform(size=(300, 12))
    u = np.full(12, 0.41)

    def bits(run):
        """host batch, a single point (whose graph is captured on the third call), null_lnZ"""
        return run.loglikelihood_batch(U.copy()), [run.loglikelihood(u.copy()) for _ in range(4)][-1], run._ss.null_lnZ()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    fresh, fresh_b1 = bits(_runner(engine, 'ammonia', rows, ut, 2)), bits(_runner(engine, 'ammonia', rows, ut, 2, baseline_order=1))
    cal_only = bits(_runner(engine, 'ammonia', rows, ut, 2, calibration=(0.1, 0.2)))
    run = _runner(engine, 'ammonia', rows, ut, 2)
    out = np.zeros(2)
    assert lib.nfa_specset_calibration(run._ss.handle, _ffi.dptr(out)) == 0 and lib.nfa_specset_calibration(None, None) == 0
    assert same(bits(run), fresh)
    for turn in range(2):
        run.set_calibration((0.1, 0.2))
        assert lib.nfa_specset_calibration(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out, [0.1, 0.2])
        got = bits(run)
        assert same(got, cal_only) and not np.array_equal(got[0], fresh[0]) and got[1] != fresh[1]
        assert np.array_equal(got[2], fresh[2])                                       # 4. null_lnZ: the uncalibrated set's, to the bit
        run.set_calibration(None if turn else (0, 0))
        assert run.calibration is None and lib.nfa_specset_calibration(run._ss.handle, None) == 0
        assert same(bits(run), fresh), turn
    # the two setters commute
    a, b = _runner(engine, 'ammonia', rows, ut, 2), _runner(engine, 'ammonia', rows, ut, 2)
    a.set_baseline(1), a.set_calibration((0.1, 0.2))
    b.set_calibration((0.1, 0.2)), b.set_baseline(1)
    both = bits(a)
    assert same(both, bits(b)) and same(both, bits(_runner(engine, 'ammonia', rows, ut, 2, baseline_order=1, calibration=(0.1, 0.2))))
    assert not np.array_equal(both[0], cal_only[0]) and not np.array_equal(both[0], fresh_b1[0])
    assert np.array_equal(both[2], fresh_b1[2])                                       # 4. ... with a baseline: the baseline-only model's
    # removing the baseline from a calibrated set: a set calibrated without one; removing the calibration then: the fresh set
    a.set_baseline(None)
    assert same(bits(a), cal_only)
    b.set_calibration(None)
    assert same(bits(b), fresh_b1)
    a.set_calibration(None)
    assert same(bits(a), fresh)
    # new data for a calibrated set (nfa_specset_set_data): a set made with them
    other = _data('ammonia', 2, 3, chan)
    if not chan:
        c = _runner(engine, 'ammonia', rows, ut, 2, calibration=(0.1, 0.2))
        data = np.ascontiguousarray(np.concatenate([r[1] for r in other]))
        _ffi.check(lib.nfa_specset_set_data(c._ss.handle, 0, _ffi.dptr(data)))
        made = _runner(engine, 'ammonia', other, ut, 2, calibration=(0.1, 0.2))
        assert np.array_equal(c.loglikelihood_batch(U.copy()), made.loglikelihood_batch(U.copy()))


# ---------------------------------------------------------------------------- 5. every launch form
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, name, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _priors(engine, name)
    for order in (None, 1):
        rows = _data(name, 2, 0 if order is None else 3, False)
        kw = dict(baseline_order=order, calibration=CAL[name])
        run = _make(engine, name, rows, ut, 2, **kw)
        # host and device batches, coalescing 8 and 1, single points and a handful
        U, theta, lnl = _routes(engine, run, rng)
        assert not np.array_equal(_make(engine, name, rows, ut, 2, baseline_order=order).loglikelihood_batch(U.copy()), lnl)
        for split in (1, 2, 4):                                                   # ... whatever the row split of a small launch
            _ffi.set_option('lnl_split', split)
            run_s = _make(engine, name, rows, ut, 2, **kw)                        # (a runner reads the option when it is made)
            for k in (0, 7, 150):
                u = U[k].copy()
                assert run_s.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k]), split
            few = U[20:31].copy()
            assert np.array_equal(run_s.loglikelihood_batch(few), lnl[20:31]), split
            assert np.array_equal(run_s.loglikelihood_batch(U[:300].copy()), lnl[:300]), split
        _ffi.set_option('lnl_split', 0)
        lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
        assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
        # predict_batch's lnL, with spectra out and without, whatever the batch
        spec, pl = run.predict_batch(theta[:40])
        assert np.array_equal(pl, lnl[:40]) and np.array_equal(run.predict_batch(theta[:40], want_spectra=False)[1], lnl[:40])
        for k in (0, 13, 39):
            s1, l1 = run.predict_batch(theta[k:k + 1])
            assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]


# ---------------------------------------------------------------------------- 6. spectra out
@pytest.mark.parametrize('mode', MODES)
def test_spectra_out_are_the_model_at_unit_gain(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    # a layered set with a baseline takes the general form with and without a calibration: the same bits
    _, _, _, thetas, preds = _models('filled', 2)
    rows = _data('filled', 2, 3, False)
    spec, _ = _make(engine, 'filled', rows, None, 2, baseline_order=3, calibration=CAL['filled']).predict_batch(np.array(thetas))
    want, _ = _make(engine, 'filled', rows, None, 2, baseline_order=3).predict_batch(np.array(thetas))
    assert np.array_equal(spec, want) and np.abs(spec).max() > 1.0
    # an unlayered two-component ammonia set leaves the unrolled form for the general one: within TIGHT
    _, _, _, thetas, preds = _models('ammonia', 2)
    rows = _data('ammonia', 2, None, False)
    spec, _ = _make(engine, 'ammonia', rows, None, 2, calibration=CAL['ammonia']).predict_batch(np.array(thetas))
    want, _ = _make(engine, 'ammonia', rows, None, 2).predict_batch(np.array(thetas))
    scale = np.maximum(np.abs(want), np.abs(preds))
    assert np.array_equal(spec == 0, want == 0) and (np.abs(spec - want) <= TIGHT[mode] * scale + 4e-15).all()
    print(f'calibrated ammonia {mode}: spectra out against the unrolled form: same bits {np.array_equal(spec, want)}')


# ---------------------------------------------------------------------------- 7. fit_gain
@pytest.mark.parametrize('mode', MODES)
def test_fit_gain_against_the_restatement(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    for name, ncomp, order, chan in (('ammonia', 2, None, False), ('ammonia', 2, 3, True), ('filled', 2, 3, False), ('gauss', 2, 0, False)):
        _, truth, clean, _, _ = _models(name, ncomp)
        rows = _data(name, ncomp, order, chan)
        run = _make(engine, name, rows, None, ncomp, baseline_order=order, calibration=CAL[name])
        mean, std = run.fit_gain(np.array(truth))
        for k, (_, d, noise, _) in enumerate(rows):
            want_mean, want_std = cr.gain_posterior(d, clean[k * N_CHAN:(k + 1) * N_CHAN], noise, CAL[name][k], order)
            assert mean[k] == pytest.approx(float(want_mean), rel=10 * TIGHT[mode]) and std[k] == pytest.approx(float(want_std), rel=10 * TIGHT[mode])
            assert abs(mean[k] - GAINS[k]) < 3 * std[k] and std[k] < CAL[name][k], (name, k, mean[k], std[k])      # (narrower than the prior)
    # a spectrum without an uncertainty: gain 1 exactly
    rows = _data('ammonia', 2, None, False)
    mean, std = _make(engine, 'ammonia', rows, None, 2, calibration=(0, 0.2)).fit_gain(np.array(_models('ammonia', 2)[1]))
    assert mean[0] == 1.0 and std[0] == 0.0 and abs(mean[1] - GAINS[1]) < 3 * std[1]


# ---------------------------------------------------------------------------- 8. refusals
def test_refusals(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingServer
    lib = _ffi.load()
    for name in ('ammonia', 'filled', 'gauss'):
        rows = _data(name, 2, None, False)
        run = _make(engine, name, rows, _priors(engine, name), 2, calibration=CAL[name])
        with RingServer(f'nfa_test_ring_cal_{os.getpid()}', n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match='no form for a calibration uncertainty: use nfa_ring_serve'):
                server.serve_device(lifetime_ms=20, idle_ms=100)
            # ... and the C entry point says NFA_ERR_ARG
            assert lib.nfa_ring_serve_device(server.handle, run._run.handle, 20, 100) == NFA_ERR_ARG
        u = np.full(run.ndim, 0.5)                                        # ... and a single point takes the batch path
        assert np.isfinite(run.loglikelihood(u))
    # bad values through the C ABI: NFA_ERR_ARG, and the set is what it was
    rows = _data('ammonia', 2, None, False)
    run = _make(engine, 'ammonia', rows, _priors(engine, 'ammonia'), 2, calibration=(0.1, 0.2))
    U = np.random.default_rng(3).uniform(size=(200, 12))
    before = run.loglikelihood_batch(U.copy())
    for bad in ((0.1, np.nan), (np.inf, 0.1), (-0.01, 0.1), (0.1, 1.0001), (-np.inf, 0.0)):
        arr = np.array(bad, dtype=np.float64)
        assert lib.nfa_specset_set_calibration(run._ss.handle, _ffi.dptr(arr)) == NFA_ERR_ARG
        assert b'calibration uncertainty' in lib.nfa_last_error()
        out = np.zeros(2)
        assert lib.nfa_specset_calibration(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out, [0.1, 0.2])
    assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    assert lib.nfa_specset_set_calibration(None, None) == NFA_ERR_ARG
    # the same on a set without one: it stays without
    bare = _make(engine, 'ammonia', rows, _priors(engine, 'ammonia'), 2)
    before = bare.loglikelihood_batch(U.copy())
    arr = np.array([0.1, 2.0])
    assert lib.nfa_specset_set_calibration(bare._ss.handle, _ffi.dptr(arr)) == NFA_ERR_ARG and lib.nfa_specset_calibration(bare._ss.handle, None) == 0
    assert np.array_equal(bare.loglikelihood_batch(U.copy()), before)


# ---------------------------------------------------------------------------- 9. the cube route
def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 2 x 2 cube of two lines with unlike gains through CubeFitter(runner_kwargs={'calibration': ...}): the store carries the
    attribute, and the fit is the runner's."""
    from nestfit_amd import hyperfine, sampler
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    tables = [engine.LineTable(72.4e9, [0.0], [1.0], name='one'), engine.LineTable(86.1e9, [-3.0, 2.0], [0.4, 0.6], name='two')]
    n_chan, n_side, noise, cal = 128, 2, 0.05, (0.1, 0.2)
    truth = np.array([0.3, 9.0, 0.2, 0.7])
    ranges = [(-2, 2), (4.0, 20.0), (-1.0, 1.0), (0.2, 1.5)]
    cubes, xs = [], []
    for k, t in enumerate(tables):
        x = t.nu * (1.0 - np.linspace(10.0, -10.0, n_chan) / hfr.CKMS)
        clean = hfr.hf_predict(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(t), truth)
        data = np.random.default_rng(40 + k).normal(0, noise, (n_chan, n_side, n_side)) + GAINS[k] * clean[:, None, None]
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': t.nu}
        cubes.append(DataCube(SimpleCube(hdr, data), noise, lines=t))
        xs.append(x)
    stack = CubeStack(cubes)
    ut = _simple_priors(engine, ranges)
    mn = {'nlive': 100, 'tol': 1.0, 'seed': 5}
    fitter = CubeFitter(stack, ut, hyperfine.HyperfineRunner, runner_kwargs={'calibration': cal}, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs=mn, nlive_snr_fact=0)
    assert np.array_equal(fitter.calibration, cal)
    runner, lon, lat = stack.to_device(ut, ncomp=1, model=3, calibration=cal)
    assert np.array_equal(runner.calibration, cal)
    mean, std = runner.fit_gain(np.arange(4), np.tile(truth, (4, 1)))
    assert mean.shape == (4, 2) and (np.abs(mean - np.array(GAINS)) < 4 * std).all()
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    bare = CubeFitter(stack, ut, hyperfine.HyperfineRunner, lnZ_thresh=11, ncomp_max=1, mn_kwargs=mn, nlive_snr_fact=0)
    bare.fit_cube(str(tmp_path / 'bare'), nproc=1)
    with HdfStore(path) as store, HdfStore(str(tmp_path / 'bare')) as plain:
        assert np.array_equal(store.read_model_calibration(), cal) and np.array_equal(np.asarray(store.hdf.attrs['calibration']), cal)
        assert plain.read_model_calibration() is None and 'calibration' not in plain.hdf.attrs
        groups = list(store.iter_pix_groups())
        plains = {(int(g.attrs['i_lon']), int(g.attrs['i_lat'])): g for g in plain.iter_pix_groups()}
        assert len(groups) == 4 and len(plains) == 4
        where = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(lon, lat))}
        for g in groups:
            i, j = int(g.attrs['i_lon']), int(g.attrs['i_lat'])
            fit = g['1']
            best = np.ascontiguousarray(np.asarray(fit['bestfit_params'][...], dtype=np.float64).reshape(1, -1))
            # the fit is the calibrated runner's: the cube runner and the pixel's own runner give the store's best lnL at its best point
            at = runner.predict_batch(np.array([where[(i, j)]]), best, want_spectra=False)[1][0]
            assert at == pytest.approx(float(fit.attrs['max_loglike']), rel=1e-9)
            rows = [[x, np.ascontiguousarray(spec), noise, t] for (x, spec, _, _), t in zip(stack.get_spec_data(i, j)[0], tables)]
            one = engine.HyperfineRunner.from_data(rows, ut, ncomp=1, calibration=cal)
            assert one.predict_batch(best, want_spectra=False)[1][0] == pytest.approx(at, rel=1e-9)
            # ... and a fit that takes the scales as exact cannot reach it
            assert float(fit.attrs['max_loglike']) > float(plains[(i, j)]['1'].attrs['max_loglike']) + 20.0


# ---------------------------------------------------------------------------- 10. a sampler run that shows the point
SAMPLER_TRUTH = np.array([0.3, 12.0, 13.0, 0.6])              # voff, tex, lncol, sigm
SAMPLER_GAINS = (1.15, 0.87, 1.0)
SAMPLER_NOISE = 0.05
SAMPLER_RANGES = [(-2, 2), (5.0, 30.0), (12.0, 14.0), (0.2, 1.5)]
# On the CPU with the restatement (seed 23, 300 channels a spectrum): the calibrated lnL (cal = 0.1) at the truth
CAL_LNL_AT_TRUTH = -463.61
# ... and the largest uncalibrated lnL there is (scipy.optimize.minimize, Nelder-Mead from the truth: at tex = 10.82, lncol = 13.04)
UNCAL_LNL_MAX = -2111.35


def _sampler_rows(nfo, na):
    temps = np.geomspace(5.0, 40.0, 32)
    mol = na.Molecule('rotor', temps, lr.rotor_partition(B_ROT, temps))
    lines = [mol.transition(*lr.rotor_transition(B_ROT, MU, J), name=f'{J + 1}-{J}') for J in range(3)]      # one line each
    rng = np.random.default_rng(23)
    rows, clean = [], []
    for t, g in zip(lines, SAMPLER_GAINS):
        x = lr.axis(t.nu, N_CHAN, 12.0)
        p = lr.lte_predict(nfo, x, hfr.tbg_of(nfo, x), t, SAMPLER_TRUTH)
        clean.append(p)
        rows.append([x, g * p + rng.normal(0, SAMPLER_NOISE, N_CHAN), SAMPLER_NOISE, t])
    return rows, clean


def test_run_multinest_with_miscalibrated_transitions(engine, nfo, mode_guard):
    """Three single-line transitions of one molecule, one component, the spectra's scales off by 1.15, 0.87 and 1.0, noise 0.05 K
    against lines of 3.6 to 5.4 K.  The fit that takes the scales as exact gives a tex that is confidently wrong and cannot
    reach the noise; with calibration=0.1 the best lnL is higher by at least half the margin found on the CPU (calibrated lnL
    at the truth -463.61, the largest uncalibrated lnL -2111.35: a margin of 1647.7) and tex is the truth's within its posterior
    width.

    Measured on an MI355X (nlive 200, seed 5): calibrated best lnL -462.15, lnZ -482.5 +- 0.30, tex 11.67 +- 0.35 (truth 12);
    uncalibrated best lnL -2111.44, lnZ -2136.3 +- 0.34, tex 10.820 +- 0.030 -- 39 of its standard deviations from the truth."""
    from nestfit_amd import sampler
    rows, clean = _sampler_rows(nfo, engine)
    at_truth = float(sum(cr.marginal_lnl(d, p, noise, 0.1) for (_, d, noise, _), p in zip(rows, clean)))
    assert at_truth == pytest.approx(CAL_LNL_AT_TRUTH, abs=0.01)
    margin = CAL_LNL_AT_TRUTH - UNCAL_LNL_MAX
    assert margin >= 50
    ut = _simple_priors(engine, SAMPLER_RANGES)
    out = {}
    for cal in (0.1, None):
        run = engine.LteRunner.from_data(rows, ut, ncomp=1, calibration=cal)
        out[cal] = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=200, seed=5)
    res, plain = out[0.1], out[None]
    (mean, std), (pmean, pstd) = res.param_constr[:2], plain.param_constr[:2]
    print(f'calibrated: best lnL {res.max_loglike:.2f}, lnZ {res.lnZ:.1f} +- {res.lnZ_err:.2f}, tex {mean[1]:.3f} +- {std[1]:.3f}; '
          f'uncalibrated: best lnL {plain.max_loglike:.2f}, lnZ {plain.lnZ:.1f} +- {plain.lnZ_err:.2f}, tex {pmean[1]:.3f} +- {pstd[1]:.3f}; '
          f'truth {SAMPLER_TRUTH[1]}')
    assert res.max_loglike - plain.max_loglike >= margin / 2
    assert abs(mean[1] - SAMPLER_TRUTH[1]) < 3 * std[1]
    assert plain.max_loglike <= UNCAL_LNL_MAX + 0.5            # (the optimiser's maximum is the largest there is)
