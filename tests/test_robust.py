"""A robust likelihood on the device (nfa_specset_set_robust, `robust=`): Student-t channel noise with nu degrees
of freedom per spectrum, lnL_s = -(nu + 1) / 2 sum_j log1p(a_j (d_j - p_j)^2), in lnl_kernel_side (robust) -- the weighted form over
g = a / (1 + a d^2) and g d with log1p(t) where the weighted form adds t.

The reference is tests/robust_restatement.py (the direct sum in longdouble; no g, no difference form) on model spectra of the
oracle and the other restatements, never the device's.

The bound.  |lnL - want| <= LNL_RTOL[mode] M (1e-9 table, 1e-6 fast) with
    M = sum_s (nu + 1) / 2 sum_j [log1p(a d^2) + g (p^2 + 2 |d p|) max(1, 1 / (1 + t))],
robust_restatement.magnitude_spectrum: the difference form's terms in absolute value, and the derivative of log1p at t.
null_lnZ: within 1e-12 M of the restatement at p = 0, and the kernel's own value there to the bit.

Measured on an MI355X, the worst |got - want| / M (bound 1e-9 table, 1e-6 fast; the fast mode's logarithm is fp32):

    row boundaries (N = 4 .. 300), 1 and 2 components        table 3.5e-16, 3.2e-16    fast 3.2e-8, 2.4e-8
    ammonia (1,1)+(2,2), 1, 2, 4 components                  table 3.9e-16, 3.8e-16, 2.5e-16    fast 1.2e-8, 1.3e-8, 6.7e-9
    N2H+ 2-1 (wide), 2 components                            table 2.5e-16    fast 5.8e-9
    a filled, layered mix, 2 layers                          table 3.1e-16    fast 1.3e-8
"""
import functools
import os

import numpy as np
import pytest

import hf_restatement as hfr
import robust_restatement as rr
from test_calibration import GAUSS_NU, _make, _models, _priors
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, _simple_priors

pytestmark = pytest.mark.gpu


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _check(run, thetas, rows, preds, nu, mode, what):
    """predict_batch's lnL of `run` against the restatement within the bound, with and without spectra out; null_lnZ within
    1e-12 M.  Returns the worst |got - want| / M."""
    want, M = rr.restate(rows, preds, nu)
    spec, lnl = run.predict_batch(np.array(thetas))
    dev = np.abs(lnl - want) / M
    print(f'robust {what} {mode} nu={np.ravel(nu).tolist()}: worst |got - want| / M {dev.max():.2e} (bound {LNL_RTOL[mode]:.0e}), '
          f'|lnL| {np.abs(want).min():.3g} .. {np.abs(want).max():.3g}')
    assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (what, nu, float(dev.max()), int(np.argmax(dev)))
    assert np.array_equal(run.predict_batch(np.array(thetas), want_spectra=False)[1], lnl)
    null_want, null_M = rr.restate(rows, np.zeros((1, preds.shape[1])), nu)
    assert abs(run.null_lnZ - null_want[0]) <= 1e-12 * null_M[0], (run.null_lnZ, null_want[0])
    return float(dev.max()), spec


# ---------------------------------------------------------------------------- 1. row boundaries
BOUNDARY_SIZES = (4, 63, 64, 65, 127, 128, 129, 300)
DV = 0.5                                                     # km/s per channel of the boundary spectra


@functools.lru_cache(maxsize=None)
def _boundary_case(n, ncomp, chan):
    """A Gaussian-model spectrum of n channels and 64 parameter rows of `ncomp` lines of sigma ~ 1.5 channels centred (within a
    fifth of a channel) on channels 63, 64, 127, 128 -- the rows' seams -- and on 0 and n - 1.  The data: row 0's model, noise
    of 0.1, and spikes of 5 .. 40 sigma, one of them under row 0's first line.  chan: a noise per channel over 0.05 .. 0.2 with
    channels 62 .. 65, astride the first seam, and channel 1 masked."""
    from oracle import nfo
    rng = np.random.default_rng(2000 + 10 * n + ncomp)
    velo = (0.5 * (n - 1) - np.arange(n)) * DV               # descending velocity, ascending frequency
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    centres = [c for c in (63, 64, 127, 128, 0, n - 1) if c < n]
    thetas = np.empty((64, 3 * ncomp))
    at0 = None
    for k in range(64):
        at = [centres[(k + 3 * c) % len(centres)] for c in range(ncomp)]
        at0 = at if k == 0 else at0
        thetas[k, :ncomp] = [velo[a] + rng.uniform(-0.2, 0.2) * DV for a in at]
        thetas[k, ncomp:2 * ncomp] = 1.5 * DV * rng.uniform(0.8, 1.25, ncomp)
        thetas[k, 2 * ncomp:] = rng.uniform(0.5, 3.0, ncomp)
    preds = np.empty((64, n))
    for k, th in enumerate(thetas):
        s = nfo.Spectrum(x, np.zeros(n), 1.0, rest_freq=GAUSS_NU)
        nfo.gauss_predict(s, th)
        preds[k] = s.get_spec()
    noise = rng.uniform(0.05, 0.2, n) if chan else 0.1
    sig = np.broadcast_to(noise, (n,))
    data = preds[0] + rng.normal(0, 1, n) * sig
    spikes = [(at0[0], 12.0)] + [(int(c), float(h)) for c, h in zip(rng.integers(0, n, 3), (5.0, 22.0, 40.0))]
    for c, h in spikes:
        data[c] += h * sig[c]
    if chan:
        noise[[c for c in (1, 62, 63, 64, 65) if c < n]] = np.inf
    for a in (thetas, preds, data):
        a.setflags(write=False)
    return [[x, data, noise, GAUSS_NU]], thetas, preds


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2])
def test_row_boundaries(engine, ncomp, mode, mode_guard):
    engine.set_exp_mode(mode)
    worst = 0.0
    for n in BOUNDARY_SIZES:
        for chan in (False, True):
            rows, thetas, preds = _boundary_case(n, ncomp, chan)
            assert np.abs(preds).max(axis=1).min() > 0.1                      # every row has its line inside the spectrum
            run = engine.GaussianRunner.from_data(rows[0], None, ncomp=ncomp)
            plain_spec, plain_lnl = run.predict_batch(np.array(thetas))
            for nu in (1, 4, 100):
                run.set_robust(nu)
                assert np.array_equal(run.robust, [nu])
                dev, spec = _check(run, thetas, rows, preds, nu, mode, f'row boundaries N={n} ncomp={ncomp} channel noise={chan}')
                worst = max(worst, dev)
                assert np.array_equal(spec, plain_spec)                       # spectra out: the set's without it, to the bit
                # null_lnZ is the kernel's own value at p = 0: a line of zero peak, and a line off the band
                zero = np.array(thetas[:2])
                zero[0, 2 * ncomp:] = 0.0
                zero[1, :ncomp] = 1e4
                assert (run.predict_batch(zero)[1] == run.null_lnZ).all()
            run.set_robust(None)
            assert np.array_equal(run.predict_batch(np.array(thetas))[1], plain_lnl)
    print(f'robust row boundaries {mode} ncomp={ncomp}: worst |got - want| / M {worst:.2e}')


# ---------------------------------------------------------------------------- 2. models
@functools.lru_cache(maxsize=None)
def _data(name, ncomp, chan):
    """The rows of a case: the truth's spectra, noise, and per spectrum spikes of 5 .. 40 sigma, one under the strongest line.
    chan: a noise per channel over 0.1 .. 0.3 K with channels 62 .. 66, astride the first seam, and three others masked."""
    axes, truth, clean, _, _ = _models(name, ncomp)
    rng = np.random.default_rng(1200 + 7 * ncomp + (50 if chan else 0))
    rows, at = [], 0
    for x, what in axes:
        n = x.size
        p = clean[at:at + n]
        at += n
        noise = rng.uniform(0.1, 0.3, n) if chan else NOISE
        sig = np.broadcast_to(noise, (n,))
        d = p + rng.normal(0, 1, n) * sig
        for c, h in [(int(np.argmax(np.abs(p))), 9.0)] + list(zip(rng.integers(0, n, 3).tolist(), (5.0, 15.0, 40.0))):
            d[c] += h * sig[c]
        if chan:
            noise[62:67] = np.inf
            noise[rng.integers(0, n, 3)] = np.inf
        d.setflags(write=False)
        rows.append([x, d, noise, what])
    return rows


def _against_the_restatement(engine, name, ncomp, mode, nus, chans=(False, True)):
    engine.set_exp_mode(mode)
    _, _, _, thetas, preds = _models(name, ncomp)
    worst = 0.0
    for chan in chans:
        rows = _data(name, ncomp, chan)
        run = _make(engine, name, rows, None, ncomp)
        plain_spec, plain = run.predict_batch(np.array(thetas))
        for nu in nus:
            run.set_robust(nu)
            dev, spec = _check(run, thetas, rows, preds, nu, mode, f'{name} ncomp={ncomp} channel noise={chan}')
            worst = max(worst, dev)
            assert np.array_equal(spec, plain_spec)                           # spectra out do not change
            want = rr.restate(rows, preds, nu)[0]
            assert (np.abs(plain - want) > 1e-3 * np.abs(want)).sum() > N_ROWS // 2      # ... and the likelihood does
    print(f'robust {name} {mode} ncomp={ncomp}: worst |got - want| / M {worst:.2e} (bound {LNL_RTOL[mode]:.0e})')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2), 300 channels, 200 rows: one nu for both spectra, a Gaussian spectrum beside a robust one, two nu."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode, (4, (4, 0), (2, 10)))


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1, 40 lines: the WIDE instances."""
    _against_the_restatement(engine, 'n2hp', 2, mode, (4, 1), chans=(False,))


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_layered_mix_against_the_restatement(engine, mode, mode_guard):
    """A blend and a line of two species, filled and layered, two layers: FILL and LAYER on."""
    _against_the_restatement(engine, 'filled', 2, mode, (4, (4, 0), (2, 10)))


# ---------------------------------------------------------------------------- 3. every launch form
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, name, mode, mode_guard):
    """Host and device batches, coalesce 1 and 8, lnl_split 1, 2 and 4, a single point, a broker, predict_batch with and
    without spectra out."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _priors(engine, name)
    rows = _data(name, 2, True)
    kw = dict(robust=(4, 2))
    run = _make(engine, name, rows, ut, 2, **kw)
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
    spec, pl = run.predict_batch(theta[:40])
    assert np.array_equal(pl, lnl[:40]) and np.array_equal(run.predict_batch(theta[:40], want_spectra=False)[1], lnl[:40])
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]


# ---------------------------------------------------------------------------- 4. per-pixel indexing
@pytest.mark.parametrize('mode', MODES)
def test_every_pixel_reads_its_own_streams(engine, mode, mode_guard):
    """Four pixels x two spectra of a CubeRunner, robust=(4, 0): every pixel's lnL, spectra and null_lnZ are, to the bit, those
    of a one-pixel runner over that pixel, in batches whose rows interleave the pixels; and new data for one pixel
    (nfa_specset_set_data) change that pixel alone, to the bits of a runner made with them."""
    from nestfit_amd import _ffi
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import freq_axis
    from test_layered import _ranges
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(44)
    n = 192
    axes = [freq_axis(1, n, 20.0), freq_axis(2, n, 20.0)]
    data = rng.normal(0, 0.2, (4, 2 * n))
    data[:, 70] += 4.0
    ut = _simple_priors(engine, _ranges('ammonia'))
    for noise in (rng.uniform(0.1, 0.3, (4, 2)), rng.uniform(0.1, 0.3, (4, 2 * n))):
        cube = CubeRunner(axes, (1, 2), data, noise, ut, ncomp=2, robust=(4, 0))
        assert np.array_equal(cube.robust, [4.0, 0.0]) and np.array_equal(cube._ss.get_robust(), [4.0, 0.0])
        B = 256
        pix = rng.integers(0, 4, B).astype(np.int32)
        U = rng.uniform(size=(B, cube.ndim))
        theta = U.copy()
        lnl = cube.loglikelihood_batch(pix, theta)
        spec, lnl_p = cube.predict_batch(pix, theta)
        assert np.isfinite(lnl).all()

        def one_pixel(p, d):
            one = CubeRunner(axes, (1, 2), d[p:p + 1], noise[p:p + 1], ut, ncomp=2, robust=(4, 0))
            rows = np.flatnonzero(pix == p)
            zeros = np.zeros(rows.size, dtype=np.int32)
            assert np.array_equal(one.loglikelihood_batch(zeros, U[rows].copy()), lnl[rows]), p
            want_spec, want_lnl = one.predict_batch(zeros, theta[rows])
            assert np.array_equal(want_spec, spec[rows]) and np.array_equal(want_lnl, lnl_p[rows]), p
            assert one.null_lnZ[0] == cube._ss.null_lnZ().sum(axis=1)[p]
        for p in range(4):
            one_pixel(p, data)
        w = cube.fit_outliers(pix[:8], theta[:8])
        assert w.shape == (8, 2 * n) and (w[:, :n] > 0).all() and (w[:, :n] <= 1.25).all() and (w[:, n:] == 1.0).all()
        new = data.copy()
        new[2] = rng.normal(0, 0.2, 2 * n)
        _ffi.check(_ffi.load().nfa_specset_set_data(cube._ss.handle, 2, _ffi.dptr(np.ascontiguousarray(new[2]))))
        keep = lnl.copy()
        theta = U.copy()
        lnl = cube.loglikelihood_batch(pix, theta)
        spec, lnl_p = cube.predict_batch(pix, theta)
        assert np.array_equal(lnl[pix != 2], keep[pix != 2]) and (lnl[pix == 2] != keep[pix == 2]).all()
        for p in (1, 2):
            one_pixel(p, new)


# ---------------------------------------------------------------------------- 5. setters
def _bits(run, thetas):
    spec, lnl = run.predict_batch(thetas)
    return spec.tobytes() + lnl.tobytes()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('chan', [False, True])
def test_setting_replacing_and_removing_on_a_live_runner(engine, chan, mode, mode_guard):
    """Set, replace and remove give the bits of a set made that way, a single point's captured graph included; new data give
    the bits of a set made with them; nu = 0 everywhere is the plain set."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    name, ncomp = 'ammonia', 2
    _, _, _, thetas, _ = _models(name, ncomp)
    thetas = np.array(thetas[:96])
    ut = _priors(engine, name)
    rows = _data(name, ncomp, chan)
    u = np.full(6 * ncomp, 0.41)
    made = {k: _make(engine, name, rows, ut, ncomp, **kw) for k, kw in
            (('plain', {}), ('a', {'robust': 4}), ('b', {'robust': (2, 10)}), ('c', {'robust': (0, 4)}))}
    want = {k: _bits(r, thetas) for k, r in made.items()}
    assert len(set(want.values())) == len(want)
    null = {k: r.null_lnZ for k, r in made.items()}
    assert len(set(null.values())) == len(null)
    point = {k: [r.loglikelihood(u.copy()) for _ in range(4)][-1] for k, r in made.items()}      # (the graph is captured on the third call)
    run = _make(engine, name, rows, ut, ncomp)
    assert lib.nfa_specset_robust(run._ss.handle, None) == 0 and lib.nfa_specset_robust(None, None) == 0
    for turn in range(2):
        for k, nu in (('a', 4), ('b', (2, 10)), ('a', (4, 4)), ('c', (0, 4))):
            run.set_robust(nu)
            out = np.zeros(2)
            assert lib.nfa_specset_robust(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out, np.broadcast_to(nu, (2,)))
            assert _bits(run, thetas) == want[k] and run.null_lnZ == null[k], (turn, k)
            assert [run.loglikelihood(u.copy()) for _ in range(4)][-1] == point[k]
        run.set_robust(np.zeros(2) if turn else None)                          # all zeros removes, like None
        assert run.robust is None and lib.nfa_specset_robust(run._ss.handle, None) == 0
        assert _bits(run, thetas) == want['plain'] and run.null_lnZ == null['plain'] and run.loglikelihood(u.copy()) == point['plain']
    assert _bits(_make(engine, name, rows, ut, ncomp, robust=0), thetas) == want['plain']
    # new data (nfa_specset_set_data): a set made with them, the degrees of freedom kept -- and after removal the plain set's
    new = [[r[0], np.ascontiguousarray(r[1][::-1]), r[2], r[3]] for r in rows]
    live = _make(engine, name, rows, ut, ncomp, robust=(4, 0))
    _bits(live, thetas)
    _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 0, _ffi.dptr(np.ascontiguousarray(np.concatenate([r[1] for r in new])))))
    fresh = _make(engine, name, new, ut, ncomp, robust=(4, 0))
    assert _bits(live, thetas) == _bits(fresh, thetas)
    got, ref = np.empty((1, 2)), np.empty((1, 2))
    _ffi.check(lib.nfa_specset_null_lnz(live._ss.handle, _ffi.dptr(got)))
    _ffi.check(lib.nfa_specset_null_lnz(fresh._ss.handle, _ffi.dptr(ref)))
    assert np.array_equal(got, ref)
    live.set_robust(None)
    assert _bits(live, thetas) == _bits(_make(engine, name, new, ut, ncomp), thetas)


# ---------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_set_as_it_was(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingServer
    lib = _ffi.load()
    name, ncomp = 'ammonia', 2
    _, _, _, thetas, _ = _models(name, ncomp)
    thetas = np.array(thetas[:64])
    rows = _data(name, ncomp, False)
    ut = _priors(engine, name)
    n = rows[0][0].size

    def refused(run, call, why):
        before = _bits(run, thetas)
        with pytest.raises(engine.EngineError, match=why):
            _ffi.check(call())
        assert _bits(run, thetas) == before

    # the domain
    plain = _make(engine, name, rows, ut, ncomp)
    rob = _make(engine, name, rows, ut, ncomp, robust=(4, 2))
    for run in (plain, rob):
        for bad in ((0.5, 4.0), (4.0, np.nan), (np.inf, 4.0), (-1.0, 4.0), (4.0, 1e6 + 1)):
            refused(run, lambda: lib.nfa_specset_set_robust(run._ss.handle, _ffi.dptr(np.array(bad))), 'a robust likelihood takes finite degrees of freedom')
    assert np.array_equal(rob._ss.get_robust(), [4.0, 2.0]) and plain._ss.get_robust() is None
    with pytest.raises(engine.EngineError, match='null argument'):
        _ffi.check(lib.nfa_specset_set_robust(None, None))
    for bad in ([4.0], [4.0, 4.0, 4.0], 0.5):                                  # on the host, before any device call
        before = _bits(rob, thetas)
        with pytest.raises(ValueError, match='robust must be'):
            rob.set_robust(bad)
        assert _bits(rob, thetas) == before
    # the seven setters a robust likelihood does not go with, in both orders
    nu = np.array([4.0, 0.0])
    cal, rho, taps = np.array([0.1, 0.0]), np.array([[0.5, 0.25], [0.0, 0.0]]), np.array([[0.0, 0.25, 0.5, 0.25, 0.0]] * 2)
    tmpl, counts = np.zeros((4, 2 * n)), np.array([1, 0], dtype=np.int32)
    tmpl[0, :n] = np.sin(np.arange(n) / 7.0)
    others = {'baseline': lambda h: lib.nfa_specset_set_baseline(h, 1),
              'calibration uncertainty': lambda h: lib.nfa_specset_set_calibration(h, _ffi.dptr(cal)),
              'noise correlation|correlated channel noise': lambda h: lib.nfa_specset_set_correlation(h, _ffi.dptr(rho)),
              'channel response': lambda h: lib.nfa_specset_set_response(h, _ffi.dptr(taps)),
              'nuisance templates': lambda h: lib.nfa_specset_set_templates(h, _ffi.dptr(tmpl), counts.ctypes.data_as(_ffi._ip)),
              'noise uncertainty': lambda h: lib.nfa_specset_set_noise_uncertainty(h, _ffi.dptr(np.array([0.2, 0.0]))),
              'continuum background': lambda h: lib.nfa_specset_set_continuum(h, _ffi.dptr(np.array([[30.0, 0.0]])))}
    for what, setter in others.items():
        refused(rob, lambda: setter(rob._ss.handle), f'a set with a robust likelihood takes no ({what})')
        other = _make(engine, name, rows, ut, ncomp)
        _ffi.check(setter(other._ss.handle))
        refused(other, lambda: lib.nfa_specset_set_robust(other._ss.handle, _ffi.dptr(nu)), f'a set with (a |an )?({what}) takes no robust likelihood')
        assert lib.nfa_specset_robust(other._ss.handle, None) == 0
        _ffi.check(lib.nfa_specset_set_robust(other._ss.handle, _ffi.dptr(np.zeros(2))))       # no robust likelihood: nothing to refuse
    # ... and the runner's setters say so on the host
    for call in (lambda: rob.set_baseline(1), lambda: rob.set_calibration(0.1), lambda: rob.set_correlation(engine.HANNING),
                 lambda: rob.set_response(engine.HANNING_RESPONSE), lambda: rob.set_templates([engine.ripple(n, 9.3), None]),
                 lambda: rob.set_noise_uncertainty(0.1), lambda: rob.set_continuum(3.0)):
        before = _bits(rob, thetas)
        with pytest.raises(ValueError, match='a robust likelihood'):
            call()
        assert _bits(rob, thetas) == before
    # the resident kernel, in words of its own; a single point takes the batch path
    with RingServer(f'nfa_test_ring_rob_{os.getpid()}', n_slots=1, runner=rob) as server:
        with pytest.raises(engine.EngineError, match='no form for a robust likelihood: use nfa_ring_serve'):
            server.serve_device(lifetime_ms=20, idle_ms=100)
    assert np.isfinite(rob.loglikelihood(np.full(rob.ndim, 0.5)))


# ---------------------------------------------------------------------------- 7. the sampler
SCI_RANGES = [(-8 * DV, 8 * DV), (0.5 * DV, 6 * DV), (0.0, 3.0)]                # voff, sigm, peak


def test_the_device_sampler_on_the_spiked_line(engine, mode_guard):
    """The science case of tests/test_robust_cpu.py on the device sampler (nlive 200, seed 5): a line of peak 1.0 and sigma = 3
    channels at channel 150 of 300, noise 0.2, spikes of +12 and +9 sigma three and five channels away.  With robust=4 the
    posterior of voff covers the truth within three of its widths and lnZ - null_lnZ is positive; without it the fitted centre
    is farther from the truth, and fit_outliers names the two channels.

    Measured on an MI355X: with robust=4 voff -0.26 +- 0.49 channels, peak 0.97 +- 0.13, lnZ - null_lnZ = 20.1; without it voff
    -2.11 +- 0.28 channels, peak 1.46 +- 0.11, lnZ - null_lnZ = 128.4."""
    from nestfit_amd import sampler
    n = 300
    _, data, _ = rr.spiked_line(0)
    velo = (150.0 - np.arange(n)) * DV                          # channel 150 at 0 km/s; descending velocity, ascending frequency
    x = GAUSS_NU * (1.0 - velo / hfr.CKMS)
    ut = _simple_priors(engine, SCI_RANGES)
    off = {}
    for nu in (4, None):
        run = engine.GaussianRunner.from_data([x, data, 0.2, GAUSS_NU], ut, ncomp=1, robust=nu)
        res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=200, seed=5)
        mean, std = res.param_constr[0], res.param_constr[1]
        off[nu] = abs(mean[0]) / DV
        print(f'robust={nu}: lnZ {res.lnZ:.1f} +- {res.lnZ_err:.2f}, null_lnZ {run.null_lnZ:.1f}, lnZ - null_lnZ {res.lnZ - run.null_lnZ:.1f}; '
              f'voff {mean[0] / DV:.2f} +- {std[0] / DV:.2f} channels, sigm {mean[1] / DV:.2f} channels, peak {mean[2]:.2f} +- {std[2]:.2f}')
        if nu:
            assert abs(mean[0]) < 3 * std[0] and res.lnZ - run.null_lnZ > 0
            w = run.fit_outliers(mean)
            assert len(w) == 1 and w[0].shape == (n,) and sorted(np.argsort(w[0])[:2]) == [153, 155] and np.median(w[0]) > 0.9
    assert off[None] > off[4]
