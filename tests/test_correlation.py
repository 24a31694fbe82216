"""Channel noise correlated along the spectral axis on the device (nfa_specset_set_correlation, `correlation=`):
chi^2 = (d - p)^T Q (d - p) with Q = diag(u) R^-1 diag(u) pentadiagonal, in lnl_kernel_side (corr), whose rows advance by 62 channels
with a halo of two lanes.

The reference is tests/corr_restatement.py (R as a Toeplitz matrix from the autocorrelation recursion, chi^2 from a dense
solve) on model spectra of the oracle and the other restatements, never the device's.

The bound.  |lnL - want| <= LNL_RTOL[mode] M, M = sum over the spectra of (|d|^T |Q| |d| + 2 |d|^T |Q| |p| + |p|^T |Q| |p|) /
(2 sigma_ref^2): every term carries the mode's relative error on `pred` once (1e-9 table, 1e-6 fast); the dense solve's own
error, cond eps <= 1e-13, is far inside.

Measured on an MI355X, the worst |got - want| / M (bound 1e-9 table, 1e-6 fast):

    row boundaries (N = 4 .. 300, 1 and 2 components)       table 9.3e-17    fast 1.9e-8
    ammonia (1,1)+(2,2), 1, 2, 3, 4 components              table 1.7e-16, 1.7e-16, 1.6e-16, 2.0e-16    fast 2.3e-9, 6.1e-9, 2.2e-9, 2.3e-9
    N2H+ 2-1 (wide), 2 components                           table 1.7e-16    fast 1.6e-9
    a filled, layered mix, 2 layers                         table 1.3e-16    fast 3.0e-9
    a Gaussian runner, 2 components                         table 1.6e-16    fast 1.5e-8

Spectra out of a correlated set equal the uncorrelated set's to the bit in both modes (asserted within TIGHT).
"""
import functools
import os

import numpy as np
import pytest

import corr_restatement as cs
import hf_restatement as hfr
from test_calibration import GAUSS_NU, GAUSS_RANGES, _make, _models, _priors
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands_cpu import N_CHAN
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _simple_priors

pytestmark = pytest.mark.gpu

HANNING = (2.0 / 3.0, 1.0 / 6.0)
AR1 = (0.5, 0.25)
MIXED = (0.3, -0.2)
NFA_ERR_ARG = 1


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


# ---------------------------------------------------------------------------- the restatement, many rows at once
def _pairs(rho, n_spec):
    rho = np.asarray(rho, dtype=np.float64)
    return np.tile(rho, (n_spec, 1)) if rho.ndim == 1 else rho


def restate(rows, preds, rho):
    """(lnL, M) of model rows preds[B, chan_tot] against the data rows [axis, data, noise, what] under the pairs `rho`:
    corr_restatement's expressions with the dense solve and inverse of a spectrum shared by the rows."""
    preds = np.atleast_2d(preds)
    want, M = np.zeros(preds.shape[0]), np.zeros(preds.shape[0])
    at = 0
    for (x, d, noise, _), pair in zip(rows, _pairs(rho, len(rows))):
        n = x.size
        p = preds[:, at:at + n]
        at += n
        Cm = cs.covariance(noise, pair, n)
        r = d[None, :] - p
        want += -0.5 * np.sum(r * np.linalg.solve(Cm, r.T).T, axis=1)
        A = np.abs(np.linalg.inv(Cm))
        ad, ap = np.abs(d), np.abs(p)
        M += 0.5 * (ad @ A @ ad + 2.0 * (ap @ (A @ ad)) + np.sum(ap * (ap @ A), axis=1))
    return want, M


@functools.lru_cache(maxsize=None)
def _data(name, ncomp, chan):
    """The rows of a case: the truth's spectra plus AR(2) noise of Hanning's pair scaled by the noise; chan: a noise per channel
    over 0.1 .. 0.3 K (no channel masked: a correlated set takes none)."""
    axes, truth, clean, _, _ = _models(name, ncomp)
    rng = np.random.default_rng(900 + 7 * ncomp + (50 if chan else 0))
    rows, at = [], 0
    for x, what in axes:
        n = x.size
        noise = rng.uniform(0.1, 0.3, n) if chan else NOISE
        rows.append([x, clean[at:at + n] + noise * cs.ar2_noise(rng, HANNING, (n,)), noise, what])
        at += n
    return rows


def _against_the_restatement(engine, name, ncomp, mode, rhos, chans=(False,)):
    engine.set_exp_mode(mode)
    _, _, _, thetas, preds = _models(name, ncomp)
    worst = 0.0
    for chan in chans:
        rows = _data(name, ncomp, chan)
        plain = _make(engine, name, rows, None, ncomp).predict_batch(np.array(thetas), want_spectra=False)[1]
        for rho in rhos:
            want, M = restate(rows, preds, rho)
            run = _make(engine, name, rows, None, ncomp, correlation=rho)
            assert np.array_equal(run.correlation, _pairs(rho, len(rows)))
            _, lnl = run.predict_batch(np.array(thetas), want_spectra=False)
            dev = np.abs(lnl - want) / M
            print(f'correlated {name} {mode} ncomp={ncomp} rho={np.round(np.ravel(rho), 3).tolist()} channel noise={chan}: worst |got - want| / M '
                  f'{dev.max():.2e} (bound {LNL_RTOL[mode]:.0e}), |lnL| {np.abs(want).min():.3g} .. {np.abs(want).max():.3g}')
            assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (rho, chan, dev.max())
            # ... and the correlation is what makes the difference
            assert (np.abs(plain - want) > 1e-3 * np.abs(want)).sum() > N_ROWS // 2
            null_want, null_M = restate(rows, np.zeros((1, preds.shape[1])), rho)
            assert abs(run.null_lnZ - null_want[0]) <= 1e-12 * null_M[0], (run.null_lnZ, null_want[0])
            worst = max(worst, float(dev.max()))
    return worst


# ---------------------------------------------------------------------------- 1. row boundaries
BOUNDARY_SIZES = (4, 61, 62, 63, 64, 65, 123, 124, 125, 126, 300)
DV = 0.5                                                     # km/s per channel of the boundary spectra


def _boundary_case(nfo, n, ncomp):
    """A Gaussian-model spectrum of n channels, 64 parameter rows of `ncomp` lines of sigma ~ 1.5 channels centred (within a
    fifth of a channel) on channels 61, 62, 63, 123, 124 -- the rows' seams at a stride of 62 -- and on 0 and n - 1."""
    rng = np.random.default_rng(1000 + 10 * n + ncomp)
    velo = (0.5 * (n - 1) - np.arange(n)) * DV               # descending velocity, ascending frequency
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    centres = [c for c in (61, 62, 63, 123, 124, 0, n - 1) if c < n]
    thetas = np.empty((64, 3 * ncomp))
    for k in range(64):
        at = [centres[(k + 3 * c) % len(centres)] for c in range(ncomp)]
        thetas[k, :ncomp] = [velo[a] + rng.uniform(-0.2, 0.2) * DV for a in at]
        thetas[k, ncomp:2 * ncomp] = 1.5 * DV * rng.uniform(0.8, 1.25, ncomp)
        thetas[k, 2 * ncomp:] = rng.uniform(0.5, 3.0, ncomp)
    preds = np.empty((64, n))
    for k, th in enumerate(thetas):
        s = nfo.Spectrum(x, np.zeros(n), 1.0, rest_freq=GAUSS_NU)
        nfo.gauss_predict(s, th)
        preds[k] = s.get_spec()
    data = preds[0] + 0.1 * cs.ar2_noise(rng, HANNING, (n,))
    return [[x, data, 0.1, GAUSS_NU]], thetas, preds


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2])
def test_row_boundaries(engine, nfo, ncomp, mode, mode_guard):
    engine.set_exp_mode(mode)
    for n in BOUNDARY_SIZES:
        rows, thetas, preds = _boundary_case(nfo, n, ncomp)
        assert np.abs(preds).max(axis=1).min() > 0.1                          # every row has its line inside the spectrum
        want, M = restate(rows, preds, HANNING)
        run = engine.GaussianRunner.from_data(rows[0], None, ncomp=ncomp, correlation=HANNING)
        spec, lnl = run.predict_batch(thetas)
        dev = np.abs(lnl - want) / M
        print(f'row boundaries {mode} N={n} ncomp={ncomp}: worst |got - want| / M {dev.max():.2e} (bound {LNL_RTOL[mode]:.0e})')
        assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (n, dev.max(), int(np.argmax(dev)))
        assert np.array_equal(run.predict_batch(thetas, want_spectra=False)[1], lnl)
        # spectra out: every channel written once, the halo lanes' none
        assert (np.abs(spec - preds) <= TIGHT[mode] * np.maximum(np.abs(preds), np.abs(spec)) + 1e-12).all(), n
        null_want, null_M = restate(rows, np.zeros((1, n)), HANNING)
        assert abs(run.null_lnZ - null_want[0]) <= 1e-12 * null_M[0]


# ---------------------------------------------------------------------------- 2. models
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2), 300 channels, 200 rows: a scalar noise and a noise per channel; one pair for both spectra and a pair
    per spectrum, one of them white."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode, (HANNING, AR1, MIXED, (HANNING, (0.0, 0.0))), chans=(False, True))


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances."""
    _against_the_restatement(engine, 'n2hp', 2, mode, (HANNING, AR1, MIXED))


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_layered_mix_against_the_restatement(engine, mode, mode_guard):
    """A blend and a line of two species, filled and layered, two layers: FILL and LAYER on."""
    _against_the_restatement(engine, 'filled', 2, mode, (HANNING, MIXED, (HANNING, (0.0, 0.0))), chans=(False, True))


@pytest.mark.parametrize('mode', MODES)
def test_a_gaussian_runner_against_the_restatement(engine, mode, mode_guard):
    _against_the_restatement(engine, 'gauss', 2, mode, (HANNING, AR1, MIXED))


# ---------------------------------------------------------------------------- 3. every launch form
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, name, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _priors(engine, name)
    rows = _data(name, 2, True)
    kw = dict(correlation=(HANNING, MIXED))
    run = _make(engine, name, rows, ut, 2, **kw)
    # host and device batches, coalescing 8 and 1, single points and a handful
    U, theta, lnl = _routes(engine, run, rng)
    assert not np.array_equal(_make(engine, name, rows, ut, 2).loglikelihood_batch(U.copy()), lnl)
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


# ---------------------------------------------------------------------------- 4. spectra out
@pytest.mark.parametrize('mode', MODES)
def test_spectra_out_are_the_model(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    for name, ncomp in (('filled', 2), ('ammonia', 2), ('ammonia', 4)):
        _, _, _, thetas, preds = _models(name, ncomp)
        rows = _data(name, ncomp, False)
        spec, _ = _make(engine, name, rows, None, ncomp, correlation=HANNING).predict_batch(np.array(thetas))
        want, _ = _make(engine, name, rows, None, ncomp).predict_batch(np.array(thetas))
        scale = np.maximum(np.abs(want), np.abs(preds))
        assert np.array_equal(spec == 0, want == 0) and (np.abs(spec - want) <= TIGHT[mode] * scale + 4e-15).all()
        print(f'correlated {name} ncomp={ncomp} {mode}: spectra out against the uncorrelated set: same bits {np.array_equal(spec, want)}')


# ---------------------------------------------------------------------------- 5. values and setters
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

    def bits(run):
        """host batch, a single point (whose graph is captured on the third call), null_lnZ"""
        return run.loglikelihood_batch(U.copy()), [run.loglikelihood(u.copy()) for _ in range(4)][-1], run._ss.null_lnZ()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a, b))
    fresh = bits(_make(engine, 'ammonia', rows, ut, 2))
    made = _make(engine, 'ammonia', rows, ut, 2, correlation=HANNING)
    corr_only = bits(made)
    other = bits(_make(engine, 'ammonia', rows, ut, 2, correlation=(AR1, MIXED)))
    run = _make(engine, 'ammonia', rows, ut, 2)
    out = np.zeros((2, 2))
    assert lib.nfa_specset_correlation(run._ss.handle, _ffi.dptr(out)) == 0 and lib.nfa_specset_correlation(None, None) == 0
    assert same(bits(run), fresh)
    white_null = run.null_lnZ
    for turn in range(2):
        run.set_correlation(HANNING)
        assert lib.nfa_specset_correlation(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out, [HANNING, HANNING])
        got = bits(run)
        assert same(got, corr_only) and not np.array_equal(got[0], fresh[0]) and got[1] != fresh[1]
        assert run.null_lnZ == made.null_lnZ == float(got[2].sum()) and run.null_lnZ != white_null        # null_lnZ follows
        want, M = restate(rows, np.zeros((1, 2 * N_CHAN)), HANNING)
        assert abs(run.null_lnZ - want[0]) <= 1e-12 * M[0]
        assert all(s.correlation == HANNING for s in run.spectra)
        run.set_correlation((AR1, MIXED))                                             # one correlation for another
        assert same(bits(run), other)
        run.set_correlation(None if turn else (0, 0))
        assert run.correlation is None and lib.nfa_specset_correlation(run._ss.handle, None) == 0
        assert same(bits(run), fresh) and run.null_lnZ == white_null, turn
        assert all(s.correlation is None for s in run.spectra)
    # new data for a correlated set (nfa_specset_set_data): a set made with them, under the same noise (per channel: Q d is
    # formed again with u != 1)
    rng = np.random.default_rng(23)
    new = [[r[0], r[1] + rng.normal(0, 0.05, r[1].size), r[2], r[3]] for r in rows]
    data = np.ascontiguousarray(np.concatenate([r[1] for r in new]))
    _ffi.check(lib.nfa_specset_set_data(made._ss.handle, 0, _ffi.dptr(data)))
    again = _make(engine, 'ammonia', new, ut, 2, correlation=HANNING)
    changed = made.loglikelihood_batch(U.copy())
    assert np.array_equal(changed, again.loglikelihood_batch(U.copy())) and not np.array_equal(changed, corr_only[0])
    assert np.array_equal(made._ss.null_lnZ(), again._ss.null_lnZ())


@pytest.mark.parametrize('mode', MODES)
def test_no_correlation_is_the_runner_without_the_argument(engine, mode, mode_guard):
    """correlation=None, (0, 0) and zeros per spectrum: the bits of a runner built without the argument through host batches,
    device batches and single points, and its null_lnZ."""
    engine.set_exp_mode(mode)
    rows = _data('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    bare = _make(engine, 'ammonia', rows, ut, 2)
    U, theta, lnl = _routes(engine, bare, np.random.default_rng(7))
    for corr in (None, (0, 0), np.zeros((2, 2)), [(0.0, 0.0), (0, 0)]):
        run = _make(engine, 'ammonia', rows, ut, 2, correlation=corr)
        assert run.correlation is None
        U2, theta2, lnl2 = _routes(engine, run, np.random.default_rng(7))
        assert np.array_equal(U2, U) and np.array_equal(theta2, theta) and np.array_equal(lnl2, lnl), corr
        assert run.null_lnZ == bare.null_lnZ


def test_refusals(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingServer
    lib = _ffi.load()
    for name in ('ammonia', 'gauss'):
        rows = _data(name, 2, False)
        run = _make(engine, name, rows, _priors(engine, name), 2, correlation=HANNING)
        with RingServer(f'nfa_test_ring_corr_{os.getpid()}', n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match='no form for correlated channel noise: use nfa_ring_serve'):
                server.serve_device(lifetime_ms=20, idle_ms=100)
            assert lib.nfa_ring_serve_device(server.handle, run._run.handle, 20, 100) == NFA_ERR_ARG
        assert np.isfinite(run.loglikelihood(np.full(run.ndim, 0.5)))          # a single point takes the batch path
    rows = _data('ammonia', 2, False)
    ut = _priors(engine, 'ammonia')
    U = np.random.default_rng(3).uniform(size=(200, 12))
    out = np.zeros((2, 2))

    def rc_of(run, value):
        arr = np.ascontiguousarray(value, dtype=np.float64)
        return lib.nfa_specset_set_correlation(run._ss.handle, _ffi.dptr(arr))
    # bad values through the C ABI: NFA_ERR_ARG, and the set is what it was -- correlated, or not
    for run, state in ((_make(engine, 'ammonia', rows, ut, 2, correlation=HANNING), 1), (_make(engine, 'ammonia', rows, ut, 2), 0)):
        before = run.loglikelihood_batch(U.copy())
        for bad in ([HANNING, (np.nan, 0.1)], [(np.inf, 0.1), HANNING], [(1.0, 0.5), HANNING], [HANNING, (0.9, 0.6)], [HANNING, (0.5, 1.0)],
                    [(0.99, 0.965), HANNING]):
            assert rc_of(run, bad) == NFA_ERR_ARG and b'noise correlation' in lib.nfa_last_error(), bad
            assert lib.nfa_specset_correlation(run._ss.handle, _ffi.dptr(out)) == state
            assert state == 0 or np.array_equal(out, [HANNING, HANNING])
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    assert lib.nfa_specset_set_correlation(None, None) == NFA_ERR_ARG
    # a correlation on a set with a masked channel, a baseline or a calibration: refused, the set as it was
    noise = np.full(N_CHAN, 0.2)
    noise[17] = np.inf
    masked_rows = [[r[0], r[1], noise, r[3]] for r in rows]
    for kw, rws, why in (({}, masked_rows, b'masked channel'), ({'baseline_order': 1}, rows, b'baseline'), ({'calibration': 0.1}, rows, b'calibration')):
        run = _make(engine, 'ammonia', rws, ut, 2, **kw)
        before = run.loglikelihood_batch(U.copy())
        assert rc_of(run, [HANNING, HANNING]) == NFA_ERR_ARG and why in lib.nfa_last_error()
        assert lib.nfa_specset_correlation(run._ss.handle, None) == 0
        assert rc_of(run, np.zeros((2, 2))) == 0                                # removing what is not there is no error
        assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
        with pytest.raises(ValueError, match='correlation'):
            run.set_correlation(HANNING)
    # ... and the other way round: a correlated set takes neither
    run = _make(engine, 'ammonia', rows, ut, 2, correlation=HANNING)
    before = run.loglikelihood_batch(U.copy())
    assert lib.nfa_specset_set_baseline(run._ss.handle, 1) == NFA_ERR_ARG and b'correlated channel noise' in lib.nfa_last_error()
    cal = np.array([0.1, 0.1])
    assert lib.nfa_specset_set_calibration(run._ss.handle, _ffi.dptr(cal)) == NFA_ERR_ARG and b'correlated channel noise' in lib.nfa_last_error()
    assert lib.nfa_specset_set_baseline(run._ss.handle, -1) == 0 and lib.nfa_specset_set_calibration(run._ss.handle, None) == 0
    assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    with pytest.raises(ValueError, match='noise correlation'):
        run.set_baseline(1)
    with pytest.raises(ValueError, match='noise correlation'):
        run.set_calibration(0.1)
    assert np.array_equal(run.loglikelihood_batch(U.copy()), before)
    # a spectrum of fewer than four channels
    x = rows[0][0][:3]
    tiny = engine.AmmoniaRunner.from_data([[x, np.zeros(3), 0.1, 1]], None, ncomp=1)
    arr = np.array([HANNING])
    assert lib.nfa_specset_set_correlation(tiny._ss.handle, _ffi.dptr(arr)) == NFA_ERR_ARG and b'4 channels' in lib.nfa_last_error()


# ---------------------------------------------------------------------------- 6. the calibration of the likelihood
def test_the_likelihood_is_calibrated_with_the_correlation_and_not_without(engine, mode_guard):
    """512 pixels of true AR(2) noise with Hanning's pair, N = 256, one spectrum, through a CubeRunner: -2 sigma^2 lnL at p = 0, in units of sigma^2.
    With correlation=HANNING its mean is N within four standard errors and its variance 2N within [0.75, 1.25]; without, the
    variance is above 1.6 times 2N (expected 2 sum rho_k^2 ~ 2.2).  The same figures come out of the restatement on the CPU
    (tests/test_correlation_cpu.py).

    Measured on an MI355X: with the correlation mean 254.74 (-1.26 standard errors), variance / 2N 0.986; without, 1.914."""
    from nestfit_amd.cube import CubeRunner
    engine.set_exp_mode('table')
    data = np.array(cs.calibration_pixels(HANNING))
    velo = (0.5 * (cs.CAL_N - 1) - np.arange(cs.CAL_N)) * DV
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    noise = np.full((cs.CAL_PIX, 1), cs.CAL_SIGMA)
    pix = np.arange(cs.CAL_PIX)
    theta = np.tile([0.0, 1.0, 0.0], (cs.CAL_PIX, 1))                          # a line of zero height: p = 0
    figures = {}
    for corr in (HANNING, None):
        run = CubeRunner([x], [-1], data, noise, None, ncomp=1, model=2, rest_freqs=[GAUSS_NU], correlation=corr)
        lnl = run.predict_batch(pix, theta, want_spectra=False)[1]
        assert np.allclose(lnl, run.null_lnZ, rtol=1e-13, atol=0)
        figures[corr] = cs.calibration_figures(-2.0 * lnl)              # (-2 sigma^2 lnL in units of sigma^2)
        want = np.array([cs.lnl(d, np.zeros(cs.CAL_N), cs.CAL_SIGMA, corr or (0.0, 0.0)) for d in data[:16]])
        assert np.allclose(lnl[:16], want, rtol=1e-11, atol=0)
    (mean, z, ratio), (wmean, wz, wratio) = figures[HANNING], figures[None]
    print(f'with the correlation: mean {mean:.2f} ({z:+.2f} standard errors from {cs.CAL_N}), variance / 2N {ratio:.3f}; '
          f'without: mean {wmean:.2f}, variance / 2N {wratio:.3f}')
    assert abs(z) <= 4.0 and 0.75 <= ratio <= 1.25
    assert wratio > 1.6


# ---------------------------------------------------------------------------- 7. a sampler run that shows the point
SAMPLER_TRUTH = np.array([0.4, 2.0, 0.5])                     # voff (km/s), sigm (km/s: four channels), peak (K)
SAMPLER_NOISE = 0.1
SAMPLER_RANGES = [(-10.0, 10.0), (0.5, 6.0), (0.0, 3.0)]


def test_run_multinest_on_correlated_noise(engine, nfo, mode_guard):
    """One Gaussian component of four channels' width, peak five times the noise, on true AR(2) noise with Hanning's pair: with
    the correlation the posterior of voff is wider than the white likelihood's (p^T C^-1 p / p^T p ~ 0.5: about 1.35 times), and
    lnZ - null_lnZ is smaller.

    Measured on an MI355X (nlive 200, seed 5): with the correlation voff 0.165 +- 0.216, lnZ - null_lnZ 54.9; without, voff
    0.106 +- 0.140, lnZ - null_lnZ 106.8 -- a width 1.54 times too small and an evidence difference 1.95 times too large."""
    from nestfit_amd import sampler
    n = 256
    velo = (0.5 * (n - 1) - np.arange(n)) * DV
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    s = nfo.Spectrum(x, np.zeros(n), 1.0, rest_freq=GAUSS_NU)
    nfo.gauss_predict(s, SAMPLER_TRUTH)
    data = s.get_spec() + SAMPLER_NOISE * cs.ar2_noise(np.random.default_rng(31), HANNING, (n,))
    ut = _simple_priors(engine, SAMPLER_RANGES)
    out = {}
    for corr in (HANNING, None):
        run = engine.GaussianRunner.from_data([x, data, SAMPLER_NOISE, GAUSS_NU], ut, ncomp=1, correlation=corr)
        res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=200, seed=5)
        out[corr] = (res, run.null_lnZ)
    (res, null), (plain, pnull) = out[HANNING], out[None]
    (mean, std), (pmean, pstd) = res.param_constr[:2], plain.param_constr[:2]
    print(f'with the correlation: voff {mean[0]:.3f} +- {std[0]:.3f}, lnZ - null_lnZ {res.lnZ - null:.1f}; '
          f'without: voff {pmean[0]:.3f} +- {pstd[0]:.3f}, lnZ - null_lnZ {plain.lnZ - pnull:.1f}; truth {SAMPLER_TRUTH[0]}')
    assert std[0] > pstd[0]
    assert abs(mean[0] - SAMPLER_TRUTH[0]) < 4 * std[0]
    assert res.lnZ - null < plain.lnZ - pnull
