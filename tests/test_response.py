"""A channel response on the device (nfa_specset_set_response, `response=`): the model that meets the data is
p~_j = sum_k h_k p_{j+k}, formed in lnl_kernel_side (resp), whose rows advance by 58 channels: a lane evaluates the model two channels
before the one whose p~ it holds, four wave shifts and five multiply-adds make p~, and two lanes of p~ are the halo of the
correlated form.

The reference is tests/resp_restatement.py (the filter as a loop over the taps and the dense Q of corr_restatement.py, in
extended precision) on model spectra of the oracle and the other restatements, never the device's.

The bound.  |lnL - want| <= LNL_RTOL[mode] M, M = sum over the spectra of (|d|^T |Q| |d| + 2 |d|^T |Q| |p~| + |p~|^T |Q| |p~|) / 2
(Q with the noise in it): every term carries the mode's relative error on `pred` once (1e-9 table, 1e-6 fast), and a
filtered value is a sum of five such.  Spectra out: |p~ - filtered(p)| <= 8 eps sum_k |h_k| |p_{j+k}| per channel in both
modes, p the same runner's spectra without the response -- the filter is five fp64 operations on values of the same code.

Measured on an MI355X, the worst |got - want| / M (bound 1e-9 table, 1e-6 fast):

    row boundaries (N = 4 .. 300), 1 and 2 components        table 9.9e-16, 4.6e-16    fast 1.0e-7, 5.8e-8
    ammonia (1,1)+(2,2), 1, 2, 4 components                  table 3.8e-16, 8.1e-16, 3.9e-16    fast 5.2e-9, 1.6e-8, 4.7e-9
    N2H+ 2-1 (wide), 2 components                            table 3.1e-16    fast 5.7e-9
    a filled, layered mix, 2 layers                          table 4.1e-16    fast 7.5e-9

Spectra out: at most 1.5 eps sum_k |h_k| |p_{j+k}| in both modes (bound 8).
"""
import functools
import os

import numpy as np
import pytest

import hf_restatement as hfr
import resp_restatement as rr
from test_calibration import GAUSS_NU, _make, _models, _priors
from test_correlation import AR1, HANNING, MIXED, _data, _pairs
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands_cpu import N_CHAN
from test_sibling_models import LNL_RTOL, MODES, TIGHT

pytestmark = pytest.mark.gpu

HANNING_RESPONSE = (0.25, 0.5, 0.25)
BINOMIAL = tuple(np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0)
SKEW = (0.1, 0.2, 0.4, 0.25, 0.05)                           # asymmetric: a lane that took p_{j-k} for p_{j+k} shows
IDENTITY = (0.0, 1.0, 0.0)
NFA_ERR_ARG = 1
EPS = np.finfo(np.float64).eps


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _taps(taps, n_spec):
    """One response for all spectra, or one per spectrum: a list of n_spec tap tuples."""
    return [tuple(taps)] * n_spec if np.ndim(taps[0]) == 0 else [tuple(t) for t in taps]


def _show(taps):
    return [np.round(t, 3).tolist() for t in _taps(taps, 1)] if np.ndim(taps[0]) else np.round(taps, 3).tolist()


def _taps5(taps, n_spec):
    return np.array([np.asarray(rr.taps5(t), dtype=np.float64) for t in _taps(taps, n_spec)])


def restate(rows, preds, taps, rho=None):
    """(lnL, M) in float64 of model rows preds[B, chan_tot] against the data rows [axis, data, noise, what], each spectrum seen
    through its taps, under the pairs `rho` (None: white noise)."""
    preds = np.atleast_2d(preds)
    want, M = np.zeros(preds.shape[0], dtype=np.longdouble), np.zeros(preds.shape[0], dtype=np.longdouble)
    at = 0
    pairs = _pairs((0.0, 0.0) if rho is None else rho, len(rows))
    for (x, d, noise, _), h, pair in zip(rows, _taps(taps, len(rows)), pairs):
        n = x.size
        l, m = rr.lnl_rows(d, preds[:, at:at + n], noise, h, pair)
        want, M, at = want + l, M + m, at + n
    return np.asarray(want, dtype=np.float64), np.asarray(M, dtype=np.float64)


# ---------------------------------------------------------------------------- 1. row boundaries
BOUNDARY_SIZES = (4, 5, 57, 58, 59, 60, 115, 116, 117, 118, 300)
BOUNDARY_TAPS = {'hanning': HANNING_RESPONSE, 'binomial': BINOMIAL, 'skew': SKEW}
DV = 0.5                                                     # km/s per channel of the boundary spectra


@functools.lru_cache(maxsize=None)
def _boundary_case(n, ncomp):
    """A Gaussian-model spectrum of n channels, 64 parameter rows of `ncomp` lines of sigma ~ 1.5 channels centred (within a
    fifth of a channel) on channels 55 .. 60 and 114 .. 117 -- the rows' seams at a stride of 58, their halo and the two
    channels a row evaluates before its own -- and on 0 and n - 1, where the response reaches beyond the spectrum.  A scalar
    noise and a noise per channel."""
    from oracle import nfo
    rng = np.random.default_rng(2000 + 10 * n + ncomp)
    velo = (0.5 * (n - 1) - np.arange(n)) * DV               # descending velocity, ascending frequency
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    centres = [c for c in (55, 56, 57, 58, 59, 60, 114, 115, 116, 117, 0, n - 1, 0, n - 1) if c < n]
    thetas = np.empty((64, 3 * ncomp))
    for k in range(64):
        at = [centres[(k + 5 * c) % len(centres)] for c in range(ncomp)]
        thetas[k, :ncomp] = [velo[a] + rng.uniform(-0.2, 0.2) * DV for a in at]
        thetas[k, ncomp:2 * ncomp] = 1.5 * DV * rng.uniform(0.8, 1.25, ncomp)
        thetas[k, 2 * ncomp:] = rng.uniform(0.5, 3.0, ncomp)
    preds = np.empty((64, n))
    for k, th in enumerate(thetas):
        s = nfo.Spectrum(x, np.zeros(n), 1.0, rest_freq=GAUSS_NU)
        nfo.gauss_predict(s, th)
        preds[k] = s.get_spec()
    data = np.asarray(rr.filtered(preds[0], HANNING_RESPONSE), dtype=np.float64) + 0.1 * rng.normal(size=n)
    chan_noise = rng.uniform(0.08, 0.2, n)
    for a in (x, thetas, preds, data, chan_noise):
        a.setflags(write=False)
    return x, data, chan_noise, thetas, preds


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2])
def test_row_boundaries(engine, ncomp, mode, mode_guard):
    engine.set_exp_mode(mode)
    worst = 0.0
    for n in BOUNDARY_SIZES:
        x, data, chan_noise, thetas, preds = _boundary_case(n, ncomp)
        assert np.abs(preds).max(axis=1).min() > 0.1                          # every row has its line inside the spectrum
        # ... and some rows at either end (the reference's line windows end before the last channel: its model is 0 there)
        assert (np.abs(preds[:, 0]) > 0.4).any() and (np.abs(preds[:, -2]) > 0.4).any()
        for k, (tname, taps) in enumerate(BOUNDARY_TAPS.items()):
            for corr in (None, HANNING):
                # (scalar and per-channel noise alternate over the sizes, taps and the correlation: every size sees both)
                for noise in ((0.1, chan_noise) if n in (4, 58, 59, 117, 300) else ((0.1, chan_noise)[(k + (corr is None)) % 2],)):
                    rows = [[x, data, noise, GAUSS_NU]]
                    want, M = restate(rows, preds, taps, corr)
                    run = engine.GaussianRunner.from_data(rows[0], None, ncomp=ncomp, response=taps, correlation=corr)
                    assert np.array_equal(run.response, _taps5(taps, 1)) and (run.correlation is None) == (corr is None)
                    spec, lnl = run.predict_batch(np.array(thetas))
                    dev = np.abs(lnl - want) / M
                    worst = max(worst, float(dev.max()))
                    assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (n, tname, corr, np.ndim(noise), dev.max(), int(np.argmax(dev)))
                    assert np.array_equal(run.predict_batch(np.array(thetas), want_spectra=False)[1], lnl)
                    # spectra out are p~: every channel written once, the halo lanes' none
                    pt = np.asarray(rr.filtered(preds, taps), dtype=np.float64)
                    scale = np.asarray(rr.filtered_scale(preds, taps), dtype=np.float64)
                    assert (np.abs(spec - pt) <= TIGHT[mode] * scale + 1e-12).all(), (n, tname)
    print(f'row boundaries {mode} ncomp={ncomp}: worst |got - want| / M {worst:.2e} (bound {LNL_RTOL[mode]:.0e})')


# ---------------------------------------------------------------------------- 2. models
def _against_the_restatement(engine, name, ncomp, mode, cases, chans=(False,)):
    """cases: (taps, rho or None).  The data are test_correlation's rows of the case (the truth plus AR(2) noise)."""
    engine.set_exp_mode(mode)
    _, _, _, thetas, preds = _models(name, ncomp)
    worst = 0.0
    for chan in chans:
        rows = _data(name, ncomp, chan)
        plain = _make(engine, name, rows, None, ncomp)
        plain_lnl = plain.predict_batch(np.array(thetas), want_spectra=False)[1]
        for taps, rho in cases:
            want, M = restate(rows, preds, taps, rho)
            run = _make(engine, name, rows, None, ncomp, response=taps, correlation=rho)
            assert np.array_equal(run.response, _taps5(taps, len(rows)))
            _, lnl = run.predict_batch(np.array(thetas), want_spectra=False)
            dev = np.abs(lnl - want) / M
            print(f'response {name} {mode} ncomp={ncomp} taps={_show(taps)} rho={rho} channel noise={chan}: '
                  f'worst |got - want| / M {dev.max():.2e} (bound {LNL_RTOL[mode]:.0e})')
            assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (taps, rho, chan, dev.max())
            # ... and the response is what makes the difference; null_lnZ has none to make
            base, _ = restate(rows, preds, IDENTITY, rho)
            assert (np.abs(base - want) > 1e-3 * np.abs(want)).sum() > len(thetas) // 2
            if rho is None:
                assert run.null_lnZ == plain.null_lnZ and (np.abs(plain_lnl - want) > 1e-3 * np.abs(want)).sum() > len(thetas) // 2
            worst = max(worst, float(dev.max()))
    return worst


MODEL_CASES = ((HANNING_RESPONSE, None), (HANNING_RESPONSE, HANNING), (BINOMIAL, (0.8, 0.4)), (SKEW, MIXED))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2), 300 channels, 200 rows: a scalar noise and a noise per channel; one response for both spectra and one
    per spectrum, one of them the identity."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode, MODEL_CASES + (((HANNING_RESPONSE, IDENTITY), (HANNING, (0.0, 0.0))),), chans=(False, True))


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances."""
    _against_the_restatement(engine, 'n2hp', 2, mode, MODEL_CASES[:3])


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_layered_mix_against_the_restatement(engine, mode, mode_guard):
    """A blend and a line of two species, filled and layered, two layers: FILL and LAYER on; also a response per spectrum, the
    second spectrum unfiltered."""
    _against_the_restatement(engine, 'filled', 2, mode, (MODEL_CASES[0], MODEL_CASES[1], (SKEW, None), ((HANNING_RESPONSE, IDENTITY), None),
                                                         ((HANNING_RESPONSE, IDENTITY), HANNING)), chans=(False, True))


# ---------------------------------------------------------------------------- 3. spectra out
@pytest.mark.parametrize('mode', MODES)
def test_spectra_out_are_the_filtered_model(engine, mode, mode_guard):
    """predict_batch's spectra of a set with a response against `filtered()` of the same runner's spectra once the response is
    removed: 8 eps sum_k |h_k| |p_{j+k}| per channel in both modes."""
    engine.set_exp_mode(mode)
    for name, ncomp in (('filled', 2), ('ammonia', 2), ('ammonia', 4), ('gauss', 2)):
        _, _, _, thetas, preds = _models(name, ncomp)
        rows = _data(name, ncomp, False)
        sizes = [r[0].size for r in rows]
        for taps, rho in ((HANNING_RESPONSE, HANNING), (SKEW, None), ((BINOMIAL, IDENTITY)[:len(rows)] if len(rows) > 1 else BINOMIAL, None)):
            run = _make(engine, name, rows, None, ncomp, response=taps, correlation=rho)
            spec, _ = run.predict_batch(np.array(thetas))
            run.set_response(None)
            assert run.response is None
            base, _ = run.predict_batch(np.array(thetas))
            worst, at = 0.0, 0
            for n, h in zip(sizes, _taps(taps, len(rows))):
                want = np.asarray(rr.filtered(base[:, at:at + n], h), dtype=np.longdouble)
                bound = 8 * EPS * np.asarray(rr.filtered_scale(base[:, at:at + n], h), dtype=np.float64)
                err = np.abs(np.asarray(spec[:, at:at + n] - want, dtype=np.float64))
                assert (err <= bound).all(), (name, ncomp, taps, float((err / np.maximum(bound, 1e-300)).max()))
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) * 8)
                assert np.array_equal(spec[:, at:at + n] == 0, np.asarray(want == 0))
                at += n
            print(f'response {name} ncomp={ncomp} {mode} taps={_show(taps)}: spectra out against filtered(): '
                  f'worst {worst:.2f} eps sum |h||p|')


# ---------------------------------------------------------------------------- 4. every launch form
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, name, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _priors(engine, name)
    rows = _data(name, 2, True)
    # (ammonia: a response and a correlation per spectrum; the filled mix: a response alone, over white coefficients)
    kw = dict(response=(HANNING_RESPONSE, SKEW), correlation=(HANNING, MIXED)) if name == 'ammonia' else dict(response=(BINOMIAL, IDENTITY))
    run = _make(engine, name, rows, ut, 2, **kw)
    # host and device batches, coalescing 8 and 1, single points and a handful
    U, theta, lnl = _routes(engine, run, rng)
    assert not np.array_equal(_make(engine, name, rows, ut, 2, correlation=kw.get('correlation')).loglikelihood_batch(U.copy()), lnl)
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


# ---------------------------------------------------------------------------- 5. the set's state
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
    resp, resp5 = (HANNING_RESPONSE, SKEW), _taps5((HANNING_RESPONSE, SKEW), 2)

    def bits(run):
        """host batch, a single point (whose graph is captured on the third call), null_lnZ"""
        return run.loglikelihood_batch(U.copy()), [run.loglikelihood(u.copy()) for _ in range(4)][-1], run._ss.null_lnZ()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    fresh_run = _make(engine, 'ammonia', rows, ut, 2)
    fresh = bits(fresh_run)
    corr_only = bits(_make(engine, 'ammonia', rows, ut, 2, correlation=HANNING))
    resp_only_run = _make(engine, 'ammonia', rows, ut, 2, response=resp)
    resp_only = bits(resp_only_run)
    made = _make(engine, 'ammonia', rows, ut, 2, response=resp, correlation=HANNING)
    both = bits(made)
    assert not np.array_equal(resp_only[0], fresh[0]) and not np.array_equal(both[0], corr_only[0]) and not np.array_equal(both[0], resp_only[0])
    # null_lnZ has no model in it: equal to the bit with and without a response
    assert resp_only_run.null_lnZ == fresh_run.null_lnZ and np.array_equal(resp_only[2], fresh[2]) and np.array_equal(both[2], corr_only[2])
    out5, out2 = np.zeros((2, 5)), np.zeros((2, 2))
    run = _make(engine, 'ammonia', rows, ut, 2)
    assert lib.nfa_specset_response(run._ss.handle, _ffi.dptr(out5)) == 0 and lib.nfa_specset_response(None, None) == 0
    for turn in range(2):
        # the response, then the correlation
        run.set_response(resp)
        assert lib.nfa_specset_response(run._ss.handle, _ffi.dptr(out5)) == 1 and np.array_equal(out5, resp5) and np.array_equal(run.response, resp5)
        assert lib.nfa_specset_correlation(run._ss.handle, _ffi.dptr(out2)) == 0 and run.correlation is None      # white coefficients are no correlation
        assert same(bits(run), resp_only) and run.null_lnZ == fresh_run.null_lnZ
        run.set_correlation(HANNING)
        assert lib.nfa_specset_correlation(run._ss.handle, _ffi.dptr(out2)) == 1 and np.array_equal(out2, [HANNING, HANNING])
        assert lib.nfa_specset_response(run._ss.handle, _ffi.dptr(out5)) == 1 and np.array_equal(out5, resp5)
        assert same(bits(run), both) and run.null_lnZ == made.null_lnZ
        # the response leaves a correlated set: the correlated set's bits
        run.set_response(None if turn else (0, 1, 0))
        assert run.response is None and lib.nfa_specset_response(run._ss.handle, None) == 0
        assert lib.nfa_specset_correlation(run._ss.handle, None) == 1 and same(bits(run), corr_only)
        # the other order: the correlation is there, then the response
        run.set_response(resp)
        assert same(bits(run), both)
        # the correlation leaves a set with a response: white coefficients
        run.set_correlation(None)
        assert lib.nfa_specset_correlation(run._ss.handle, None) == 0 and lib.nfa_specset_response(run._ss.handle, None) == 1
        assert same(bits(run), resp_only)
        # one response for another, and none: the fresh set's bits (a scalar noise: no weights again)
        run.set_response(BINOMIAL)
        assert not np.array_equal(run.loglikelihood_batch(U.copy()), resp_only[0])
        run.set_response(None)
        assert lib.nfa_specset_response(run._ss.handle, None) == 0 and same(bits(run), fresh) and run.null_lnZ == fresh_run.null_lnZ, turn
    # new data for a set with a response (nfa_specset_set_data): a set made with them
    rng = np.random.default_rng(23)
    new = [[r[0], r[1] + rng.normal(0, 0.05, r[1].size), r[2], r[3]] for r in rows]
    data = np.ascontiguousarray(np.concatenate([r[1] for r in new]))
    for live, kw, before in ((made, dict(response=resp, correlation=HANNING), both), (resp_only_run, dict(response=resp), resp_only)):
        _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 0, _ffi.dptr(data)))
        again = _make(engine, 'ammonia', new, ut, 2, **kw)
        changed = live.loglikelihood_batch(U.copy())
        assert np.array_equal(changed, again.loglikelihood_batch(U.copy())) and not np.array_equal(changed, before[0])
        assert np.array_equal(live._ss.null_lnZ(), again._ss.null_lnZ())


@pytest.mark.parametrize('mode', MODES)
def test_no_response_is_the_runner_without_the_argument(engine, mode, mode_guard):
    """response=None, the identity and the identity per spectrum: the bits of a runner built without the argument."""
    engine.set_exp_mode(mode)
    rows = _data('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    bare = _make(engine, 'ammonia', rows, ut, 2)
    U, theta, lnl = _routes(engine, bare, np.random.default_rng(7))
    for resp in (None, (0, 1, 0), (0, 0, 1, 0, 0), [IDENTITY, IDENTITY]):
        run = _make(engine, 'ammonia', rows, ut, 2, response=resp)
        assert run.response is None
        U2, theta2, lnl2 = _routes(engine, run, np.random.default_rng(7))
        assert np.array_equal(U2, U) and np.array_equal(theta2, theta) and np.array_equal(lnl2, lnl), resp
        assert run.null_lnZ == bare.null_lnZ


# ---------------------------------------------------------------------------- 6. refusals
def test_refusals(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingServer
    lib = _ffi.load()
    for name, kw in (('ammonia', dict(response=HANNING_RESPONSE)), ('gauss', dict(response=SKEW, correlation=HANNING))):
        rows = _data(name, 2, False)
        run = _make(engine, name, rows, _priors(engine, name), 2, **kw)
        with RingServer(f'nfa_test_ring_resp_{os.getpid()}', n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match='no form for a channel response: use nfa_ring_serve'):
                server.serve_device(lifetime_ms=20, idle_ms=100)
            assert lib.nfa_ring_serve_device(server.handle, run._run.handle, 20, 100) == NFA_ERR_ARG
            assert b'correlated' not in lib.nfa_last_error()
        assert np.isfinite(run.loglikelihood(np.full(run.ndim, 0.5)))          # a single point takes the batch path
    rows = _data('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    U = np.random.default_rng(3).uniform(size=(200, 12))
    out = np.zeros((2, 5))
    h5, i5 = [0.0, 0.25, 0.5, 0.25, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0]

    def rc_of(run, value):
        arr = np.ascontiguousarray(value, dtype=np.float64)
        return lib.nfa_specset_set_response(run._ss.handle, _ffi.dptr(arr))
    # bad taps through the C ABI: NFA_ERR_ARG, and the set is what it was -- with a response, or not
    for run, state in ((_make(engine, 'ammonia', rows, ut, 2, response=HANNING_RESPONSE), 1), (_make(engine, 'ammonia', rows, ut, 2), 0),
                       (_make(engine, 'ammonia', rows, ut, 2, correlation=HANNING), 0)):
        before = run.loglikelihood_batch(U.copy())
        for bad in ([h5, [0.0, np.nan, 0.5, 0.25, 0.25]], [[np.inf, 0.0, 0.5, 0.25, 0.25], h5], [h5, [0.0, 0.25, 0.5, 0.3, 0.0]],
                    [[0.0, 0.5, 0.0, 0.5, 0.0], h5], [h5, [0.0, 0.6, -0.2, 0.6, 0.0]], [i5, [0.1, 0.2, 0.4, 0.2, 0.1 + 1e-8]]):
            assert rc_of(run, bad) == NFA_ERR_ARG and b'channel response' in lib.nfa_last_error(), bad
            assert lib.nfa_specset_response(run._ss.handle, _ffi.dptr(out)) == state
            assert state == 0 or np.array_equal(out, [h5, h5])
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    assert lib.nfa_specset_set_response(None, None) == NFA_ERR_ARG
    # a response on a set with a masked channel, a baseline or a calibration: refused, the set as it was
    noise = np.full(N_CHAN, 0.2)
    noise[17] = np.inf
    masked_rows = [[r[0], r[1], noise, r[3]] for r in rows]
    for kw, rws, why in (({}, masked_rows, b'masked channel'), ({'baseline_order': 1}, rows, b'baseline'), ({'calibration': 0.1}, rows, b'calibration')):
        run = _make(engine, 'ammonia', rws, ut, 2, **kw)
        before = run.loglikelihood_batch(U.copy())
        assert rc_of(run, [h5, h5]) == NFA_ERR_ARG and why in lib.nfa_last_error() and b'channel response' in lib.nfa_last_error()
        assert lib.nfa_specset_response(run._ss.handle, None) == 0
        assert rc_of(run, [i5, i5]) == 0                                        # removing what is not there is no error
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
        with pytest.raises(ValueError, match='channel response'):
            run.set_response(HANNING_RESPONSE)
        with pytest.raises(ValueError, match='channel response'):                  # ... and where the runner is made
            _make(engine, 'ammonia', rws, ut, 2, response=HANNING_RESPONSE, **kw)
    # ... and the other way round: a set with a response takes neither, and says why in its own words
    cal = np.array([0.1, 0.1])
    for kw in (dict(response=HANNING_RESPONSE), dict(response=HANNING_RESPONSE, correlation=HANNING)):
        run = _make(engine, 'ammonia', rows, ut, 2, **kw)
        before = run.loglikelihood_batch(U.copy())
        assert lib.nfa_specset_set_baseline(run._ss.handle, 1) == NFA_ERR_ARG and b'channel response' in lib.nfa_last_error()
        assert b'correlated' not in lib.nfa_last_error()
        assert lib.nfa_specset_set_calibration(run._ss.handle, _ffi.dptr(cal)) == NFA_ERR_ARG and b'channel response' in lib.nfa_last_error()
        assert b'correlated' not in lib.nfa_last_error()
        assert lib.nfa_specset_set_baseline(run._ss.handle, -1) == 0 and lib.nfa_specset_set_calibration(run._ss.handle, None) == 0
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
        with pytest.raises(ValueError, match='channel response'):
            run.set_baseline(1)
        with pytest.raises(ValueError, match='channel response'):
            run.set_calibration(0.1)
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    # a spectrum of fewer than four channels
    x = rows[0][0][:3]
    tiny = engine.AmmoniaRunner.from_data([[x, np.zeros(3), 0.1, 1]], None, ncomp=1)
    assert rc_of(tiny, [h5]) == NFA_ERR_ARG and b'4 channels' in lib.nfa_last_error() and b'channel response' in lib.nfa_last_error()


# ---------------------------------------------------------------------------- 7. the science
SCIENCE_NOISE = 0.1


@pytest.mark.parametrize('mode', MODES)
def test_the_response_removes_the_width_bias(engine, nfo, mode, mode_guard):
    """One spectrum of 128 channels, the data a Hanning-smoothed Gaussian of sigma = 1 channel without noise: over
    test_response_cpu.py's (peak, sigm) grid the likelihood with response=HANNING_RESPONSE is largest at the truth, where
    |lnL| <= LNL_RTOL M; without the response it is largest where the restatement's is: a line 1.24 times too wide and 0.81
    times too high."""
    engine.set_exp_mode(mode)
    n = rr.BIAS_N
    velo = (rr.BIAS_CENTRE - np.arange(n)) * DV              # the line's centre at 0 km/s, off the channel grid
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    s = nfo.Spectrum(x, np.zeros(n), 1.0, rest_freq=GAUSS_NU)
    nfo.gauss_predict(s, np.array([0.0, rr.BIAS_SIGM * DV, rr.BIAS_PEAK]))
    truth = s.get_spec()
    # (the restatement's line in channels, to the 1e-5 of the reference's FastExp)
    assert np.abs(truth - rr.gaussian(rr.BIAS_PEAK, rr.BIAS_SIGM)).max() <= 1e-4
    data = np.asarray(rr.filtered(truth, HANNING_RESPONSE), dtype=np.float64)
    peaks, sigms = np.meshgrid(rr.BIAS_PEAKS, rr.BIAS_SIGMS * DV, indexing='ij')
    theta = np.stack([np.zeros(peaks.size), sigms.ravel(), peaks.ravel()], axis=1)
    # what numpy says of the same grid, on the oracle's model spectra
    models = np.empty((theta.shape[0], n))
    for k, th in enumerate(theta):
        nfo.gauss_predict(s, th)
        models[k] = s.get_spec()
    biased = rr.bias_argmin(-np.asarray(rr.lnl_rows(data, models, SCIENCE_NOISE, rr.IDENTITY)[0], dtype=np.float64).reshape(peaks.shape))
    assert rr.BIAS_SIGMS[biased[1]] >= 1.15 * rr.BIAS_SIGM and rr.BIAS_PEAKS[biased[0]] <= 0.9 * rr.BIAS_PEAK
    got = {}
    for resp in (HANNING_RESPONSE, None):
        # (the grid goes in as physical parameters, the batch likelihood of predict_batch: a prior's quantile table has a few
        # hundred entries and would move every grid point by more than the grid's step resolves at the truth)
        run = engine.GaussianRunner.from_data([x, data, SCIENCE_NOISE, GAUSS_NU], None, ncomp=1, response=resp)
        lnl = run.predict_batch(theta, want_spectra=False)[1]
        got[resp] = rr.bias_argmin(-lnl.reshape(peaks.shape))
        if resp is not None:
            at = int(np.ravel_multi_index(rr.BIAS_TRUE, peaks.shape))
            _, M = rr.lnl(data, truth, SCIENCE_NOISE, HANNING_RESPONSE)
            print(f'the science {mode}: |lnL| at the truth {abs(lnl[at]):.3e}, bound {LNL_RTOL[mode] * float(M):.3e}')
            assert abs(lnl[at]) <= LNL_RTOL[mode] * float(M)
    print(f'the science {mode}: argmax (peak, sigm) with the response {got[HANNING_RESPONSE]}, without {got[None]} '
          f'= {rr.BIAS_PEAKS[got[None][0]]:.2f} x peak, {rr.BIAS_SIGMS[got[None][1]]:.2f} x sigm')
    assert got[HANNING_RESPONSE] == rr.BIAS_TRUE
    assert got[None] == biased
