"""Nuisance templates profiled out with the baseline on the device (nfa_specset_set_templates, `templates=`):
chi2_min over span{P_0..P_K, t_1..t_T} in lnl_kernel_side (tmpl), eight moments where the baseline form has four.

The reference is tests/tmpl_restatement.py (weighted least squares by QR in longdouble, no moments) on model spectra of the
oracle and the other restatements, never the device's.

The bound.  |lnL - want| <= LNL_RTOL[mode] M, M = sum over the spectra of (sum w d^2 + 2 sum w |d| |p| + sum w p^2) / (2
sigma_ref^2): every term carries the mode's relative error on `pred` once (1e-9 table, 1e-6 fast).  A relative tolerance on lnL
is wrong here, because the templates can take chi2_min far below its terms.  The moment form's own loss against the QR is about
cond x 2e-16 M, and tests/test_templates_cpu.py holds every template set below to cond <= 1e3.
"""
import functools
import os
import threading

import numpy as np
import pytest

import hf_restatement as hfr
import tmpl_cases as tc
import tmpl_restatement as tr
from test_calibration import GAUSS_NU, _make, _models, _priors
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, _simple_priors

pytestmark = pytest.mark.gpu

NFA_ERR_ARG = 1
DV = 0.5                                                     # km/s per channel of the Gaussian spectra


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _gauss_axis(n):
    velo = (0.5 * (n - 1) - np.arange(n)) * DV               # descending velocity, ascending frequency
    return velo, GAUSS_NU * (1.0 - velo / hfr.CKMS)


def _gauss_spectra(x, thetas):
    from oracle import nfo
    out = np.empty((len(thetas), x.size))
    for k, th in enumerate(thetas):
        s = nfo.Spectrum(x, np.zeros(x.size), 1.0, rest_freq=GAUSS_NU)
        nfo.gauss_predict(s, th)
        out[k] = s.get_spec()
    return out


def _nuisance(n, rng, sigma):
    """A tilt and ripples of the test templates' periods and arbitrary phases, a few sigma each: what the templates are for."""
    j = np.arange(n)
    u = (2.0 * j - (n - 1)) / max(n - 1, 1)
    return sigma * (rng.normal(0, 3) + rng.normal(0, 3) * u + sum(rng.normal(0, 2) * np.sin(2 * np.pi * j * c / n + rng.uniform(0, 6.28))
                                                                  for c in (2.3, 3.7)))


# ---------------------------------------------------------------------------- 1. row and part boundaries
@functools.lru_cache(maxsize=None)
def _boundary_case(n, ncomp):
    """A Gaussian-model spectrum of n channels and 64 parameter rows of `ncomp` lines of sigma ~ 1.5 channels centred (within a
    fifth of a channel) on channels 63, 64, 127, 128 -- the seams of the rows of 64 channels -- and on 0 and n - 1."""
    rng = np.random.default_rng(2000 + 10 * n + ncomp)
    velo, x = _gauss_axis(n)
    centres = [c for c in (63, 64, 127, 128, 0, n - 1) if c < n]
    thetas = np.empty((64, 3 * ncomp))
    for k in range(64):
        at = [centres[(k + 3 * c) % len(centres)] for c in range(ncomp)]
        thetas[k, :ncomp] = [velo[a] + rng.uniform(-0.2, 0.2) * DV for a in at]
        thetas[k, ncomp:2 * ncomp] = 1.5 * DV * rng.uniform(0.8, 1.25, ncomp)
        thetas[k, 2 * ncomp:] = rng.uniform(0.5, 3.0, ncomp)
    preds = _gauss_spectra(x, thetas)
    data = preds[0] + _nuisance(n, rng, 0.1) + rng.normal(0, 0.1, n)
    for a in (thetas, preds, data):
        a.setflags(write=False)
    return x, thetas, preds, data


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2])
def test_row_and_part_boundaries(engine, ncomp, mode, mode_guard):
    """N = 4 .. 300, every order -1, 0, 1, 3 with 1, 2 and 4 templates, a scalar noise and a noise per channel with masked
    channels (astride the first seam among them); null_lnZ with every one of them.

    Measured on an MI355X, the worst |got - want| / M: table 7.0e-16 (1 component), 7.0e-16 (2); fast 8.1e-8, 8.9e-8."""
    engine.set_exp_mode(mode)
    worst = 0.0
    for n in tc.BOUNDARY_SIZES:
        x, thetas, preds, data = _boundary_case(n, ncomp)
        assert np.abs(preds).max(axis=1).min() > 0.1                          # every row has its line inside the spectrum
        for chan in (False, True):
            noise = tc.channel_noise(n, 7 * n) if chan else 0.1
            rows = [[x, np.array(data), noise, GAUSS_NU]]
            run = engine.GaussianRunner.from_data(rows[0], None, ncomp=ncomp)
            plain_spec, _ = run.predict_batch(thetas)
            for order in tc.ORDERS:
                run.set_baseline(None if order < 0 else order)
                for count in tc.COUNTS:
                    t = tc.templates(n, count)
                    run.set_templates([t])
                    assert np.array_equal(run.templates[0], t) and run.baseline_order == (None if order < 0 else order)
                    spec, lnl = run.predict_batch(thetas)
                    want, M = tr.restate(rows, preds, order, [t])
                    dev = np.abs(lnl - want) / M
                    assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (n, chan, order, count, dev.max(), int(np.argmax(dev)))
                    worst = max(worst, float(dev.max()))
                    assert np.array_equal(spec, plain_spec)                   # spectra out: the model without nuisance terms
                    assert np.array_equal(run.predict_batch(thetas, want_spectra=False)[1], lnl)
                    null_want, null_M = tr.restate(rows, np.zeros((1, n)), order, [t])
                    assert abs(run.null_lnZ - null_want[0]) <= 1e-12 * null_M[0], (n, chan, order, count)
    print(f'row boundaries {mode} ncomp={ncomp}: worst |got - want| / M {worst:.2e} (bound {LNL_RTOL[mode]:.0e})')


# ---------------------------------------------------------------------------- 2. models
def _sizes(rows):
    return [np.size(r[0]) for r in rows]


@functools.lru_cache(maxsize=None)
def _data(name, ncomp, chan):
    """The rows [axis, data, noise, what] of a model case: the truth's spectra, a tilt and ripples, noise; chan: a noise per
    channel with masked channels."""
    axes, _, clean, _, _ = _models(name, ncomp)
    rng = np.random.default_rng(600 + 7 * ncomp + (50 if chan else 0) + len(name))
    rows, at = [], 0
    for k, (x, what) in enumerate(axes):
        n = x.size
        noise = tc.channel_noise(n, 31 + k, base=0.1) if chan else NOISE
        scatter = np.where(np.isfinite(noise), noise, 0.0) * np.ones(n)
        rows.append([x, clean[at:at + n] + _nuisance(n, rng, NOISE) + rng.normal(0, 1, n) * scatter, noise, what])
        at += n
    return rows


def _against_the_restatement(engine, name, ncomp, mode, orders=tc.ORDERS, chans=(False, True)):
    engine.set_exp_mode(mode)
    _, _, _, thetas, preds = _models(name, ncomp)
    worst = 0.0
    for chan in chans:
        rows = _data(name, ncomp, chan)
        assert all(n == tc.N_CHAN for n in _sizes(rows))
        for which in ('mixed', 'both'):
            tmpl = tc.model_templates(len(rows), which)
            for order in orders:
                bl = None if order < 0 else order
                want, M = tr.restate(rows, preds, order, tmpl)
                run = _make(engine, name, rows, None, ncomp, baseline_order=bl, templates=tmpl)
                assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(run.templates, tmpl))
                _, lnl = run.predict_batch(np.array(thetas), want_spectra=False)
                dev = np.abs(lnl - want) / M
                assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (which, order, chan, dev.max())
                worst = max(worst, float(dev.max()))
                # ... and the templates are what makes the difference
                plain = _make(engine, name, rows, None, ncomp, baseline_order=bl).predict_batch(np.array(thetas), want_spectra=False)[1]
                assert (np.abs(plain - want) > 100 * LNL_RTOL[mode] * M).sum() > N_ROWS // 2
                null_want, null_M = tr.restate(rows, np.zeros((1, preds.shape[1])), order, tmpl)
                assert abs(run.null_lnZ - null_want[0]) <= 1e-12 * null_M[0], (run.null_lnZ, null_want[0])
    print(f'templates {name} {mode} ncomp={ncomp}: worst |got - want| / M {worst:.2e} (bound {LNL_RTOL[mode]:.0e})')
    return worst


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2), 300 channels, 200 rows: four templates on (1,1) and none on (2,2), and two and one.

    Measured on an MI355X, the worst |got - want| / M for 1, 2, 4 components: table 3.9e-16, 4.9e-16, 4.3e-16; fast 6.4e-9,
    1.2e-8, 7.0e-9."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode)


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances.  Measured on an MI355X: table 4.1e-16, fast 6.0e-9."""
    _against_the_restatement(engine, 'n2hp', 2, mode)


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_layered_mix_against_the_restatement(engine, mode, mode_guard):
    """A blend and a line of two species, filled and layered, two layers: FILL and LAYER on.  Measured on an MI355X: table
    3.7e-16, fast 6.1e-9."""
    _against_the_restatement(engine, 'filled', 2, mode)


# ---------------------------------------------------------------------------- 4. every launch form
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, name, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _priors(engine, name)
    rows = _data(name, 2, True)
    kw = dict(baseline_order=1, templates=tc.model_templates(2, 'mixed'))
    run = _make(engine, name, rows, ut, 2, **kw)
    bare = _make(engine, name, rows, ut, 2, baseline_order=1)
    # host and device batches, coalescing 8 and 1, single points and a handful
    U, theta, lnl = _routes(engine, run, rng)
    assert not np.array_equal(bare.loglikelihood_batch(U.copy()), lnl)
    for split in (1, 2, 4):                                                   # ... whatever the row split of a small launch
        _ffi.set_option('lnl_split', split)
        run_s = _make(engine, name, rows, ut, 2, **kw)                        # (a runner reads the option when it is made)
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
    # predict_batch's lnL, with spectra out and without, whatever the batch; the spectra those of the set without templates
    spec, pl = run.predict_batch(theta[:40])
    assert np.array_equal(pl, lnl[:40]) and np.array_equal(run.predict_batch(theta[:40], want_spectra=False)[1], lnl[:40])
    assert np.array_equal(spec, bare.predict_batch(theta[:40])[0])
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]


# ---------------------------------------------------------------------------- 5. state
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('chan', [False, True])
def test_setting_and_removing_on_a_live_runner(engine, chan, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    rows = _data('ammonia', 2, chan)
    ut = _priors(engine, 'ammonia')
    U = np.random.default_rng(19).uniform(size=(300, 12))
    u = np.full(12, 0.41)
    mixed, both = tc.model_templates(2, 'mixed'), tc.model_templates(2, 'both')

    def bits(run):
        """host batch, a single point (whose graph is captured on the third call), null_lnZ"""
        return run.loglikelihood_batch(U.copy()), [run.loglikelihood(u.copy()) for _ in range(4)][-1], run._ss.null_lnZ()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    fresh = bits(_make(engine, 'ammonia', rows, ut, 2))
    with_bl = bits(_make(engine, 'ammonia', rows, ut, 2, baseline_order=1))
    made = _make(engine, 'ammonia', rows, ut, 2, templates=mixed)
    tmpl_only = bits(made)
    made_both = _make(engine, 'ammonia', rows, ut, 2, baseline_order=1, templates=both)
    tmpl_bl = bits(made_both)
    run = _make(engine, 'ammonia', rows, ut, 2)
    counts = np.zeros(2, dtype=np.int32)
    vals = np.zeros((4, 2 * tc.N_CHAN))
    assert lib.nfa_specset_templates(run._ss.handle, None, None) == 0 and lib.nfa_specset_templates(None, None, None) == 0
    plain_null = run.null_lnZ
    for turn in range(2):
        run.set_templates(mixed)
        assert lib.nfa_specset_templates(run._ss.handle, _ffi.dptr(vals), counts.ctypes.data_as(_ffi._ip)) == 1
        assert counts.tolist() == [4, 0] and np.array_equal(vals[:, :tc.N_CHAN], mixed[0]) and not vals[:, tc.N_CHAN:].any()     # the caller's values
        got = bits(run)
        assert same(got, tmpl_only) and not np.array_equal(got[0], fresh[0]) and got[1] != fresh[1]
        assert run.null_lnZ == made.null_lnZ == float(got[2].sum()) and run.null_lnZ != plain_null                 # null_lnZ follows
        # templates then a baseline, the other order, and a set made that way: the same bits
        run.set_templates(both)
        run.set_baseline(1)
        assert same(bits(run), tmpl_bl) and run.null_lnZ == made_both.null_lnZ
        run.set_templates(None)
        assert run.templates is None and lib.nfa_specset_templates(run._ss.handle, None, None) == 0
        assert same(bits(run), with_bl)
        run.set_templates(both)                                                   # ... the baseline first
        assert same(bits(run), tmpl_bl)
        run.set_baseline(None)
        run.set_templates(None if turn else [None, None])
        assert same(bits(run), fresh) and run.null_lnZ == plain_null, turn       # the fresh set's bits
    # new data for a templated set (nfa_specset_set_data): a set made with them
    rng = np.random.default_rng(23)
    new = [[r[0], r[1] + rng.normal(0, 0.05, r[1].size), r[2], r[3]] for r in rows]
    data = np.ascontiguousarray(np.concatenate([r[1] for r in new]))
    _ffi.check(lib.nfa_specset_set_data(made_both._ss.handle, 0, _ffi.dptr(data)))
    again = _make(engine, 'ammonia', new, ut, 2, baseline_order=1, templates=both)
    changed = made_both.loglikelihood_batch(U.copy())
    assert np.array_equal(changed, again.loglikelihood_batch(U.copy())) and not np.array_equal(changed, tmpl_bl[0])
    assert np.array_equal(made_both._ss.null_lnZ(), again._ss.null_lnZ())


@pytest.mark.parametrize('mode', MODES)
def test_no_templates_is_the_runner_without_the_argument(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    rows = _data('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    bare = _make(engine, 'ammonia', rows, ut, 2)
    U, theta, lnl = _routes(engine, bare, np.random.default_rng(7))
    for tmpl in (None, [None, None], [np.zeros((0, tc.N_CHAN)), None]):
        run = _make(engine, 'ammonia', rows, ut, 2, templates=tmpl)
        assert run.templates is None
        U2, theta2, lnl2 = _routes(engine, run, np.random.default_rng(7))
        assert np.array_equal(U2, U) and np.array_equal(theta2, theta) and np.array_equal(lnl2, lnl)
        assert run.null_lnZ == bare.null_lnZ


# ---------------------------------------------------------------------------- 6. rank
@pytest.mark.parametrize('mode', MODES)
def test_the_rank_rule(engine, mode, mode_guard):
    """Directions the span already holds add nothing: a constant beside order 0, a template given twice, P_1 beside order 1;
    and a spectrum with fewer unmasked channels than basis functions is fitted exactly."""
    engine.set_exp_mode(mode)
    n = 129
    x, thetas, preds, data = _boundary_case(n, 2)
    rows = [[x, np.array(data), 0.1, GAUSS_NU]]
    M = tr.restate(rows, preds, 1, None)[1]
    one = tc.templates(n, 1)

    def lnl_of(order, tmpl, noise=0.1):
        run = engine.GaussianRunner.from_data([x, np.array(data), noise, GAUSS_NU], None, ncomp=2, baseline_order=order,
                                              templates=None if tmpl is None else [tmpl])
        return run.predict_batch(thetas, want_spectra=False)[1]
    worst = 0.0
    for what, a, b in (('a constant beside order 0', lnl_of(0, np.full((1, n), 7.0)), lnl_of(0, None)),
                       ('a template given twice', lnl_of(1, np.concatenate([one, -3.0 * one])), lnl_of(1, one)),
                       ('P_1 beside order 1', lnl_of(1, np.linspace(-2.0, 2.0, n)[None, :]), lnl_of(1, None))):
        dev = np.abs(a - b) / M
        worst = max(worst, float(dev.max()))
        assert np.isfinite(a).all() and (dev <= LNL_RTOL[mode]).all(), (what, dev.max())
    # five live channels across the spectrum, two of them under the lines, and eight functions
    noise = np.full(n, np.inf)
    noise[[2, 37, 64, 99, 127]] = 0.1
    lnl = lnl_of(3, tc.templates(n, 4), noise)
    rows_m = [[x, np.array(data), noise, GAUSS_NU]]
    bound = LNL_RTOL[mode] * tr.restate(rows_m, preds, 3, [tc.templates(n, 4)])[1]
    assert (np.abs(lnl) <= bound).all(), float((np.abs(lnl) / bound).max())
    print(f'rank {mode}: worst deviation / M {worst:.2e}; five channels, eight functions: worst |lnL| / bound {float((np.abs(lnl) / bound).max()):.2e}')


# ---------------------------------------------------------------------------- 7. the science
@pytest.mark.parametrize('mode', MODES)
def test_a_ripple_of_known_period_is_taken_out(engine, mode, mode_guard):
    """One spectrum of 256 channels without noise: a Gaussian line, a tilt and a ripple of 0.5 sigma with a period of 37.3
    channels.  With K = 1 and ripple(256, 37.3), lnL over a (peak, voff) grid is largest at the truth and 0 there within the
    bound; with K = 1 alone lnL at the truth is the restatement's value, about -N a^2 / (4 sigma^2) = -16, and the grid's
    maximum is elsewhere or as low.

    Measured on an MI355X: with the templates lnL at the truth 2.2e-14 (table), -1.1e-14 (fast); without, -16.05 in both modes, and
    the largest of the grid -14.97 at another point."""
    import nestfit_amd as na
    engine.set_exp_mode(mode)
    n, sigma, amp = tc.SCI_N, tc.SCI_SIGMA, tc.SCI_AMP * tc.SCI_SIGMA
    velo, x = _gauss_axis(n)
    truth = np.array([3.0, 2.0, 0.6])                                           # voff, sigm (four channels), peak
    peaks, voffs = truth[2] + 0.02 * np.arange(-5, 6), truth[0] + 0.1 * np.arange(-5, 6)
    grid = np.array([[v, truth[1], p] for p in peaks for v in voffs])
    at = 5 * 11 + 5
    assert np.array_equal(grid[at], truth)
    preds = _gauss_spectra(x, grid)
    u = (2.0 * np.arange(n) - (n - 1)) / (n - 1)
    wave = amp * np.sin(2 * np.pi * np.arange(n) / tc.SCI_PERIOD + tc.SCI_PHASE)
    data = preds[at] + 0.4 * sigma + 0.7 * sigma * u + wave
    rows = [[x, data, sigma, GAUSS_NU]]
    tmpl = na.ripple(n, tc.SCI_PERIOD)
    with_t = engine.GaussianRunner.from_data(rows[0], None, ncomp=1, baseline_order=1, templates=[tmpl])
    without = engine.GaussianRunner.from_data(rows[0], None, ncomp=1, baseline_order=1)
    lnl, plain = (r.predict_batch(grid, want_spectra=False)[1] for r in (with_t, without))
    want, M = tr.restate(rows, preds, 1, [tmpl])
    want_plain, _ = tr.restate(rows, preds, 1, None)
    bound = LNL_RTOL[mode] * M
    assert int(np.argmax(lnl)) == at and abs(lnl[at]) <= bound[at] and (np.abs(lnl - want) <= bound).all()
    assert (np.delete(lnl, at) < lnl[at] - 0.01).all()                          # a maximum that stands out
    expected = -n * amp ** 2 / (4 * sigma ** 2)
    assert abs(want_plain[at] - expected) < 0.1 * abs(expected)                 # (the tilt takes a little of the ripple)
    assert abs(plain[at] - want_plain[at]) <= bound[at]
    assert int(np.argmax(plain)) != at or plain.max() <= want_plain[at] + bound[at]
    print(f'{mode}: with the templates lnL at the truth {lnl[at]:.2e}; without {plain[at]:.2f} (N a^2 / 4 sigma^2 = {-expected:.1f}), the '
          f'largest of the grid {plain.max():.2f} at {"the truth" if int(np.argmax(plain)) == at else "another point"}')
    # the curve and the amplitudes that were taken out
    curve = with_t.fit_baseline(truth)
    assert np.abs(curve - (data - preds[at])).max() < 5e-6                    # (K: the modes' own error on the model spectrum)
    a_sin, a_cos = with_t.fit_templates(truth)[0]
    assert a_sin == pytest.approx(amp * np.cos(tc.SCI_PHASE), abs=1e-4 * amp) and a_cos == pytest.approx(amp * np.sin(tc.SCI_PHASE), abs=1e-4 * amp)


# ---------------------------------------------------------------------------- 8. refusals
def test_refusals(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingClient, RingServer
    lib = _ffi.load()
    why = 'the resident kernel has no form for nuisance templates: use nfa_ring_serve'
    for name in ('ammonia', 'gauss'):
        rows = _data(name, 2, False)
        tmpl = tc.model_templates(len(rows), 'mixed')
        run = _make(engine, name, rows, _priors(engine, name), 2, templates=tmpl)
        ring = f'nfa_test_ring_tmpl_{os.getpid()}'
        with RingServer(ring, n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match=why):
                server.serve_device(lifetime_ms=20, idle_ms=100)
            assert lib.nfa_ring_serve_device(server.handle, run._run.handle, 20, 100) == NFA_ERR_ARG
            # ... and nfa_ring_serve serves it
            t = threading.Thread(target=server.serve, kwargs=dict(max_wait_us=100, idle_ms=20000))
            t.start()
            U = np.random.default_rng(1).uniform(size=(24, run.ndim))
            got_t, got_l = [], []
            with RingClient(ring, wait_ms=20000) as client:
                for row in U:
                    th = row.copy()
                    got_l.append(client.loglikelihood(th))
                    got_t.append(th)
            server.stop()
            t.join(timeout=30)
            assert not t.is_alive()
        want_t = U.copy()
        want_l = run.loglikelihood_batch(want_t)
        assert np.array_equal(np.array(got_t), want_t) and np.array_equal(np.array(got_l), want_l)
        assert np.isfinite(run.loglikelihood(np.full(run.ndim, 0.5)))          # a single point takes the batch path
    rows = _data('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    U = np.random.default_rng(3).uniform(size=(200, 12))
    n2 = 2 * tc.N_CHAN
    mixed = tc.model_templates(2, 'mixed')
    vals = np.zeros((4, n2))
    vals[:, :tc.N_CHAN] = mixed[0]

    def rc_of(run, t, counts):
        t = np.ascontiguousarray(t, dtype=np.float64)
        c = np.ascontiguousarray(counts, dtype=np.int32)
        return lib.nfa_specset_set_templates(run._ss.handle, _ffi.dptr(t), c.ctypes.data_as(_ffi._ip))
    # bad values through the C ABI: NFA_ERR_ARG with a reason, and the set is what it was -- templated, or not
    bad_nan, bad_inf, bad_zero = vals.copy(), vals.copy(), vals.copy()
    bad_nan[1, 17] = np.nan
    bad_inf[0, 299] = np.inf
    bad_zero[2, :tc.N_CHAN] = 0.0
    out_n = np.zeros(2, dtype=np.int32)
    for run, state in ((_make(engine, 'ammonia', rows, ut, 2, templates=mixed), 1), (_make(engine, 'ammonia', rows, ut, 2), 0)):
        before = run.loglikelihood_batch(U.copy())
        for t, counts in ((bad_nan, [4, 0]), (bad_inf, [4, 0]), (bad_zero, [4, 0]), (vals, [5, 0]), (vals, [-1, 0]), (vals, [4, 1])):
            assert rc_of(run, t, counts) == NFA_ERR_ARG and b'nuisance templates' in lib.nfa_last_error(), counts
            assert lib.nfa_specset_templates(run._ss.handle, None, out_n.ctypes.data_as(_ffi._ip)) == state
            assert state == 0 or out_n.tolist() == [4, 0]
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    assert lib.nfa_specset_set_templates(None, None, None) == NFA_ERR_ARG
    # the slots above a spectrum's count are not read: NaN there is no error
    run = _make(engine, 'ammonia', rows, ut, 2, templates=mixed)
    before = run.loglikelihood_batch(U.copy())
    unused = vals.copy()
    unused[:, tc.N_CHAN:] = np.nan
    assert rc_of(run, unused, [4, 0]) == 0 and np.array_equal(run.loglikelihood_batch(U.copy()), before)
    # templates on a set with a calibration, a correlation or a response: refused, the set as it was
    import nestfit_amd as na
    for kw, reason in (({'calibration': 0.1}, b'calibration'), ({'correlation': na.HANNING}, b'correlated channel noise'),
                       ({'response': na.HANNING_RESPONSE}, b'channel response')):
        run = _make(engine, 'ammonia', rows, ut, 2, **kw)
        before = run.loglikelihood_batch(U.copy())
        assert rc_of(run, vals, [4, 0]) == NFA_ERR_ARG and reason in lib.nfa_last_error() and b'nuisance templates' in lib.nfa_last_error()
        assert lib.nfa_specset_templates(run._ss.handle, None, None) == 0
        assert rc_of(run, vals, [0, 0]) == 0                                    # removing what is not there is no error
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
        with pytest.raises(ValueError, match='nuisance templates'):
            run.set_templates(mixed)
        with pytest.raises(ValueError, match='nuisance templates'):
            _make(engine, 'ammonia', rows, ut, 2, templates=mixed, **kw)
    # ... and the other way round: a templated set takes none of the three
    run = _make(engine, 'ammonia', rows, ut, 2, templates=mixed)
    before = run.loglikelihood_batch(U.copy())
    cal, rho, taps = np.array([0.1, 0.1]), np.array([na.HANNING, na.HANNING]), np.array([[0.0, 0.25, 0.5, 0.25, 0.0]] * 2)
    for call, arr in ((lib.nfa_specset_set_calibration, cal), (lib.nfa_specset_set_correlation, rho), (lib.nfa_specset_set_response, taps)):
        assert call(run._ss.handle, _ffi.dptr(arr)) == NFA_ERR_ARG and b'nuisance templates' in lib.nfa_last_error()
        assert call(run._ss.handle, None) == 0
    assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    for setter, value in ((run.set_calibration, 0.1), (run.set_correlation, na.HANNING), (run.set_response, na.HANNING_RESPONSE)):
        with pytest.raises(ValueError, match='nuisance templates'):
            setter(value)
    assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    # ... but masked channels, a noise per channel, filled and layered sets: yes (tests 1, 2 and 4)


# ---------------------------------------------------------------------------- 9. the cube route
def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 2 x 2 cube of two lines under a ripple through CubeFitter(runner_kwargs={'templates': ...}): the store carries the
    templates, and the fit is the templated runner's."""
    from nestfit_amd import hyperfine
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    import nestfit_amd as na
    tables = [engine.LineTable(72.4e9, [0.0], [1.0], name='one'), engine.LineTable(86.1e9, [-3.0, 2.0], [0.4, 0.6], name='two')]
    n_chan, n_side, noise = 128, 2, 0.05
    truth = np.array([0.3, 9.0, 0.2, 0.7])
    ranges = [(-2, 2), (4.0, 20.0), (-1.0, 1.0), (0.2, 1.5)]
    tmpl = [na.ripple(n_chan, 23.7), None]
    cubes = []
    for k, t in enumerate(tables):
        x = t.nu * (1.0 - np.linspace(10.0, -10.0, n_chan) / hfr.CKMS)
        clean = hfr.hf_predict(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(t), truth)
        wave = 0.0 if k else 4 * noise * np.sin(2 * np.pi * np.arange(n_chan) / 23.7 + 1.1)
        data = np.random.default_rng(40 + k).normal(0, noise, (n_chan, n_side, n_side)) + (clean + wave)[:, None, None]
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': t.nu}
        cubes.append(DataCube(SimpleCube(hdr, data), noise, lines=t))
    stack = CubeStack(cubes)
    ut = _simple_priors(engine, ranges)
    mn = {'nlive': 100, 'tol': 1.0, 'seed': 5}
    fitter = CubeFitter(stack, ut, hyperfine.HyperfineRunner, runner_kwargs={'templates': tmpl}, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs=mn, nlive_snr_fact=0)
    assert np.array_equal(fitter.templates[0], tmpl[0]) and fitter.templates[1] is None
    runner, lon, lat = stack.to_device(ut, ncomp=1, model=3, templates=tmpl)
    assert np.array_equal(runner.templates[0], tmpl[0]) and runner.templates[1] is None
    amps = runner.fit_templates(np.arange(4), np.tile(truth, (4, 1)))
    assert amps[0].shape == (4, 2) and amps[1].shape == (4, 0)
    assert np.abs(np.hypot(amps[0][:, 0], amps[0][:, 1]) - 4 * noise).max() < 0.2 * 4 * noise          # the ripple's amplitude
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    bare = CubeFitter(stack, ut, hyperfine.HyperfineRunner, lnZ_thresh=11, ncomp_max=1, mn_kwargs=mn, nlive_snr_fact=0)
    bare.fit_cube(str(tmp_path / 'bare'), nproc=1)
    with HdfStore(path) as store, HdfStore(str(tmp_path / 'bare')) as plain:
        got = store.read_model_templates()
        assert len(got) == 2 and got[1] is None and np.array_equal(got[0], tmpl[0])
        assert plain.read_model_templates() is None and 'nuisance_templates' not in plain.hdf
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
            # ... and a fit that knows nothing of the ripple cannot reach it: N a^2 / (4 sigma^2) = 128 x 16 / 4 = 512
            assert float(fit.attrs['max_loglike']) > float(plains[(i, j)]['1'].attrs['max_loglike']) + 200.0
