"""A continuum background behind the components on the device (nfa_specset_set_continuum, `continuum=`): every
component's g = T0 (y - tbg) becomes g - Tc in lnl_kernel_side (cont), the baseline form with one more flag.

The reference is tests/cont_restatement.py on the draws of tests/cont_cases.py (tests/test_continuum_cpu.py holds both to
the sibling restatements and to what is said of the draws below), at the sizes of the sibling tests: 300 channels -- four
full rows of 64 and one of 44 -- and 200 parameter rows, in both modes.

The bounds.  Spectra: |got - want| <= ncomp TIGHT[mode] S + the floor of tests/test_layered.py's helper, with the zero pattern
S's, S = sum_c (|g_c| + Tc) |a_c|: g_c - Tc cancels where J(tex) ~ J(Tcmb) + Tc, so the model's own value is no scale.  lnL:
|got - want| <= LNL_RTOL[mode] M with tests/tmpl_restatement.py's M = sum over the spectra of (sum w d^2 + 2 sum w |d| |p| +
sum w p^2) / (2 sigma_ref^2) and S in |p|'s place.

Measured on an MI355X, the worst |got - want| / S and |lnL - want| / M over the rows, the two transfers (summed, layered), the
two continuum rows, the two noises and the two baselines of a case:

    case                         table  /S        /M         fast  /S        /M
    ammonia (1,1)+(2,2), 1       1.9e-15   3.9e-16        2.8e-7    6.9e-8
    ammonia, 2                   2.9e-15   3.9e-16        2.8e-7    6.1e-8
    ammonia, 3                   2.1e-15   3.5e-16        2.9e-7    5.1e-8
    ammonia, 4                   2.4e-15   3.5e-16        2.5e-7    5.5e-8
    N2H+ 2-1 + 1-0 (WIDE), 2     9.9e-16   4.1e-16        2.6e-7    3.3e-8
    a line table, 3              9.0e-16   6.2e-16        2.5e-7    3.8e-8
    a filled mix, 2              1.1e-15   3.6e-16        2.5e-7    1.6e-8

(bounds: ncomp x 1e-11 and 1e-9 in the table mode, ncomp x 5e-7 and 1e-6 in the fast mode).
"""
import functools
import os

import numpy as np
import pytest

import cont_cases as cc
import cont_restatement as cr
import tmpl_restatement as tr
from test_hyperfine import _through_a_broker
from test_layered import _check_layered, _ranges, _runner, _tex_of
from test_lte import _routes
from test_lte_mix import N_ROWS, NOISE
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _simple_priors

pytestmark = pytest.mark.gpu


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


# ---------------------------------------------------------------------------- 1. parity
@functools.lru_cache(maxsize=None)
def _lnl_reference(name, ncomp, which, layered, chan, order):
    """(rows, lnL of the restatement's spectra, M with S in |p|'s place), once for both modes."""
    import nestfit_amd as na
    spec, S = cc.evaluate(name, ncomp, which, layered)
    rows = cc.data_rows(name, na, seed=100 + ncomp, chan=chan)
    want = tr.restate(rows, spec, -1 if order is None else order, None)[0]
    M, at = np.zeros(len(spec), dtype=tr.LD), 0
    for x, d, noise, _ in rows:
        M += tr.magnitude(d, S[:, at:at + x.size], noise)
        at += x.size
    want.setflags(write=False)
    return rows, want, M.astype(np.float64)


def _against_the_restatement(engine, name, ncomp, mode):
    engine.set_exp_mode(mode)
    _, thetas, _ = cc.reference(name, ncomp)
    thetas = np.array(thetas)
    worst, worst_lnl = 0.0, 0.0
    for layered in (False, True):
        for which in ('high', 'low'):
            # the draws contain what they are meant to contain (the restatement's own spectra: tests/test_continuum_cpu.py)
            cc.check_draws(name, ncomp, which, layered)
        for chan in (False, True):
            for order in (None, 1):
                rows = cc.data_rows(name, engine, seed=100 + ncomp, chan=chan)
                run = _runner(engine, name, rows, None, ncomp, layered=layered, baseline_order=order)
                for which in ('high', 'low'):
                    tc = cc.pairs(name)[which]
                    run.set_continuum(tc)
                    assert np.array_equal(run.continuum, tc) and run.layered is layered and run.baseline_order == order
                    want, S = cc.evaluate(name, ncomp, which, layered)
                    _, want_lnl, M = _lnl_reference(name, ncomp, which, layered, chan, order)
                    spec, lnl = run.predict_batch(thetas)
                    for sp, ws, s, th in zip(spec, want, S, thetas):                    # every row, every channel
                        worst = max(worst, _check_layered(sp, ws, s, mode, ncomp, _tex_of(name, th, ncomp)))
                    dev = np.abs(lnl - want_lnl) / M
                    assert np.isfinite(lnl).all() and (dev <= LNL_RTOL[mode]).all(), (layered, which, chan, order, float(dev.max()))
                    worst_lnl = max(worst_lnl, float(dev.max()))
                    assert np.array_equal(run.predict_batch(thetas, want_spectra=False)[1], lnl)
                    # what the draws exercise, of the device's own spectra (the first spectrum: the one with Tc > 0 in both rows)
                    first = spec[:, :spec.shape[1] // 2]
                    if which == 'high':
                        assert (first[first != 0] < 0).all() and (first != 0).any(axis=1).sum() > 0.9 * N_ROWS
                    else:
                        assert (first.min(axis=1) < -1e-3).sum() >= N_ROWS // 10 and (first.max(axis=1) > 1e-3).sum() >= N_ROWS // 10
    print(f'continuum {name} {mode} ncomp={ncomp}: worst |got - want| / S {worst:.2e} (bound {ncomp * TIGHT[mode]:.1e}), '
          f'|lnL - want| / M {worst_lnl:.2e} (bound {LNL_RTOL[mode]:.0e})')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
def test_ammonia_against_the_restatement(engine, ncomp, mode, mode_guard):
    """NH3 (1,1) + (2,2): the oracle's one-component predictions before (35, 0) K and (3, 2.4) K."""
    _against_the_restatement(engine, 'ammonia', ncomp, mode)


@pytest.mark.parametrize('mode', MODES)
def test_diazenylium_wide_against_the_restatement(engine, mode, mode_guard):
    """N2H+ 2-1 (40 lines: the WIDE instances) beside 1-0."""
    _against_the_restatement(engine, 'n2hp', 2, mode)


@pytest.mark.parametrize('mode', MODES)
def test_a_line_table_against_the_restatement(engine, mode, mode_guard):
    _against_the_restatement(engine, 'lines', 3, mode)


@pytest.mark.parametrize('mode', MODES)
def test_a_filled_mix_against_the_restatement(engine, mode, mode_guard):
    """a_c = f_c (1 - e^-tau_c): ((g - Tc [- pred]) f) a, two components, before (35, 0) K and (12, 9.6) K."""
    _against_the_restatement(engine, 'filled', 2, mode)


# ---------------------------------------------------------------------------- 2. per-pixel indexing
N_CUBE = 192
TC_ROWS = np.array([[30.0, 28.0], [0.0, 0.0], [3.0, 0.0], [0.0, 12.5], [7.25, 7.5]])      # one row per pixel, one all zero


def _cube(engine, ut, tc, pixels=None, ncomp=2, **kw):
    """A CubeRunner over the pixels `pixels` (all five) of one five-pixel data set; tc: their continuum rows."""
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import freq_axis
    rng = np.random.default_rng(44)
    axes = [freq_axis(1, N_CUBE, 20.0), freq_axis(2, N_CUBE, 20.0)]
    data = rng.normal(0, 0.2, (5, 2 * N_CUBE))
    noise = rng.uniform(0.1, 0.3, (5, 2))
    sel = np.arange(5) if pixels is None else np.asarray(pixels)
    return CubeRunner(axes, (1, 2), data[sel], noise[sel], ut, ncomp=ncomp, continuum=tc, **kw)


@pytest.mark.parametrize('mode', MODES)
def test_every_pixel_reads_its_own_continuum(engine, mode, mode_guard):
    """Five pixels x two spectra, another Tc row per pixel, one row all zero: every pixel's lnL and spectra are, to the bit,
    those of a one-pixel runner with that row (the zero row: a runner without a continuum) -- in batches whose rows
    interleave the pixels, through the device-pointer entry, and through the device sampler."""
    from nestfit_amd import _ffi, sampler
    from test_device_batches import _run_on_device
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(7)
    ut = _simple_priors(engine, _ranges('ammonia'))
    cube = _cube(engine, ut, TC_ROWS)
    assert np.array_equal(cube.continuum, TC_ROWS) and np.array_equal(cube._ss.get_continuum(), TC_ROWS)
    B = 320
    pix = rng.integers(0, 5, B).astype(np.int32)                      # interleaved
    U = rng.uniform(size=(B, cube.ndim))
    theta = U.copy()
    lnl = cube.loglikelihood_batch(pix, theta)
    spec, lnl_p = cube.predict_batch(pix, theta)
    assert np.isfinite(lnl).all()
    ones = []
    for p in range(5):
        one = _cube(engine, ut, TC_ROWS[p:p + 1], pixels=[p])
        assert (one.continuum is None) == (p == 1)
        ones.append(one)
        rows = np.flatnonzero(pix == p)
        th = U[rows].copy()
        want = one.loglikelihood_batch(np.zeros(rows.size, dtype=np.int32), th)
        assert np.array_equal(th, theta[rows]) and np.array_equal(want, lnl[rows]), p
        want_spec, want_lnl = one.predict_batch(np.zeros(rows.size, dtype=np.int32), theta[rows])
        assert np.array_equal(want_spec, spec[rows]) and np.array_equal(want_lnl, lnl_p[rows]), p
        assert one.null_lnZ[0] == cube.null_lnZ[p]
    # ... the rows differ by their pixel's continuum, not only by their data
    same_data = _cube(engine, ut, None)
    assert (same_data.loglikelihood_batch(pix, U.copy())[pix != 1] != lnl[pix != 1]).all()
    # the device-pointer entry, held and launched together and one by one
    batches = [(pix[:256], U[:256].copy()), (pix[64:320], U[64:320].copy())]
    for coalesce in (8, 1):
        _ffi.set_option('coalesce', coalesce)
        got = _run_on_device(_ffi, cube._run.handle, batches)
        assert np.array_equal(got[0][1], lnl[:256]) and np.array_equal(got[1][1], lnl[64:320]) and np.array_equal(got[1][0], theta[64:320])
    _ffi.set_option('coalesce', 8)
    # the device sampler: pixel p alone in slot 0 of either runner draws the same points and must find the same evidence
    for p in (0, 3):
        kw = dict(nlive=40, tol=2.0, seed=11, maxiter=600)
        a = sampler.fit_pixels(cube, np.array([p]), **kw)[0]
        b = sampler.fit_pixels(ones[p], np.array([0]), **kw)[0]
        assert a.lnZ == b.lnZ and a.max_loglike == b.max_loglike and np.isfinite(a.lnZ), p


# ---------------------------------------------------------------------------- 3. launch forms and setters
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['ammonia', 'filled'])
def test_the_same_bits_on_every_route(engine, nfo, name, mode, mode_guard):
    """Host and device batches, coalesce 1 and 8, lnl_split 1, 2 and 4, a single point, a broker, predict_batch with and
    without spectra out."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, _ranges(name))
    rows = cc.data_rows(name, engine, seed=3)
    tc = cc.pairs(name)['low']
    run = _runner(engine, name, rows, ut, 2, layered=True, continuum=tc)
    plain = _runner(engine, name, rows, ut, 2, layered=True)
    U, theta, lnl = _routes(engine, run, rng)
    assert (plain.loglikelihood_batch(U.copy()) != lnl).all()
    for split in (4, 2, 1):
        _ffi.set_option('lnl_split', split)
        run_s = _runner(engine, name, rows, ut, 2, layered=True, continuum=tc)   # (a runner reads the option when it is made)
        for k in (0, 7, 150):
            u = U[k].copy()
            assert run_s.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k]), split
        few = U[20:31].copy()
        assert np.array_equal(run_s.loglikelihood_batch(few), lnl[20:31]), split
        assert np.array_equal(run_s.loglikelihood_batch(U[:200].copy()), lnl[:200]), split
    _ffi.set_option('lnl_split', 0)
    lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
    assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
    spec, pl = run.predict_batch(theta[:40])
    assert np.array_equal(pl, lnl[:40]) or np.allclose(pl, lnl[:40], rtol=LNL_RTOL[mode], atol=0)
    assert np.array_equal(run.predict_batch(theta[:40], want_spectra=False)[1], pl)
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]
    # `predict` of such a runner: the runner's own set, spectrum by spectrum
    run.predict(np.array(theta[2]))
    assert np.array_equal(np.concatenate([s.get_spec() for s in run.spectra]), spec[2])
    assert sum(s.loglikelihood for s in run.spectra) == pytest.approx(pl[2], rel=1e-12)
    assert spec[:40].min() < 0


def _bits(run, thetas):
    spec, lnl = run.predict_batch(thetas)
    return spec.tobytes() + lnl.tobytes()


@pytest.mark.parametrize('mode', MODES)
def test_the_setters(engine, mode, mode_guard):
    """Set, replace and remove give the bits of a set made that way; set_baseline and set_continuum commute; new data give
    the bits of a set made with them; null_lnZ is the set's without a continuum, to the bit, with and without a baseline; and
    Tc == 0 is the plain set."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    lib = _ffi.load()
    name, ncomp = 'ammonia', 2
    _, thetas, _ = cc.reference(name, ncomp)
    thetas = np.array(thetas[:96])
    ut = _simple_priors(engine, _ranges(name))
    a, b = (30.0, 0.0), (2.0, 5.5)
    u = np.full(6 * ncomp, 0.41)
    for chan in (False, True):
        rows = cc.data_rows(name, engine, seed=5, chan=chan)
        made = {k: _runner(engine, name, rows, ut, ncomp, **kw) for k, kw in
                (('plain', {}), ('a', {'continuum': a}), ('b', {'continuum': b}), ('bl', {'baseline_order': 1}),
                 ('a+bl', {'continuum': a, 'baseline_order': 1}), ('a+nu', {'continuum': a, 'noise_uncertainty': 0.2}))}
        want = {k: _bits(r, thetas) for k, r in made.items()}
        assert len(set(want.values())) == len(want)
        null = {k: r.null_lnZ for k, r in made.items()}
        # null_lnZ: the null model has no absorber
        assert null['a'] == null['plain'] == null['b'] and null['a+bl'] == null['bl'] and null['a+bl'] != null['plain']
        got = np.empty((1, 2))
        _ffi.check(lib.nfa_specset_null_lnz(made['a']._ss.handle, _ffi.dptr(got)))
        ref = np.empty((1, 2))
        _ffi.check(lib.nfa_specset_null_lnz(made['plain']._ss.handle, _ffi.dptr(ref)))
        assert np.array_equal(got, ref)
        run = _runner(engine, name, rows, ut, ncomp)
        point = {}
        for k, r in made.items():
            point[k] = r.loglikelihood(u.copy())                              # (a single point: its graph is captured)
        assert lib.nfa_specset_continuum(run._ss.handle, None) == 0 and lib.nfa_specset_continuum(None, None) == 0
        for turn in range(2):
            run.set_continuum(a)
            out = np.zeros((1, 2))
            assert lib.nfa_specset_continuum(run._ss.handle, _ffi.dptr(out)) == 1 and np.array_equal(out[0], a)
            assert _bits(run, thetas) == want['a'] and run.loglikelihood(u.copy()) == point['a'] and run.null_lnZ == null['a']
            run.set_continuum(b)                                               # replaced
            assert _bits(run, thetas) == want['b'] and run.loglikelihood(u.copy()) == point['b']
            run.set_continuum(a)
            run.set_baseline(1)                                                # the continuum first, then the baseline
            assert _bits(run, thetas) == want['a+bl'] and run.null_lnZ == null['a+bl'] and run.loglikelihood(u.copy()) == point['a+bl']
            run.set_continuum(None)                                            # removed: the baseline stays
            assert run.continuum is None and _bits(run, thetas) == want['bl'] and run.null_lnZ == null['bl']
            run.set_continuum(a)                                               # the baseline first, then the continuum
            assert _bits(run, thetas) == want['a+bl']
            run.set_baseline(None)
            assert _bits(run, thetas) == want['a'] and run.null_lnZ == null['a']
            run.set_noise_uncertainty(0.2)
            assert _bits(run, thetas) == want['a+nu'] and run.null_lnZ == null['a+nu']
            run.set_noise_uncertainty(None)
            run.set_continuum(np.zeros(2) if turn else None)                   # all zeros removes, like None
            assert lib.nfa_specset_continuum(run._ss.handle, None) == 0
            assert _bits(run, thetas) == want['plain'] and run.loglikelihood(u.copy()) == point['plain'] and run.null_lnZ == null['plain']
        # Tc == 0 from the start is the plain set
        assert _bits(_runner(engine, name, rows, ut, ncomp, continuum=0.0), thetas) == want['plain']
        # new data (nfa_specset_set_data): a set made with them, the continuum kept
        new = cc.data_rows(name, engine, seed=6, chan=chan)
        for order in (None, 1):
            live = _runner(engine, name, rows, ut, ncomp, continuum=a, baseline_order=order)
            _bits(live, thetas)
            _ffi.check(lib.nfa_specset_set_data(live._ss.handle, 0, _ffi.dptr(np.ascontiguousarray(np.concatenate([r[1] for r in new])))))
            fresh = _runner(engine, name, new, ut, ncomp, continuum=a, baseline_order=order)
            assert _bits(live, thetas) == _bits(fresh, thetas)
            ref = np.empty((1, 2))
            _ffi.check(lib.nfa_specset_null_lnz(live._ss.handle, _ffi.dptr(got)))
            _ffi.check(lib.nfa_specset_null_lnz(fresh._ss.handle, _ffi.dptr(ref)))
            assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_set_as_it_was(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingServer
    lib = _ffi.load()
    name, ncomp = 'ammonia', 2
    _, thetas, _ = cc.reference(name, ncomp)
    thetas = np.array(thetas[:64])
    rows = cc.data_rows(name, engine, seed=5)
    ut = _simple_priors(engine, _ranges(name))
    n = rows[0][0].size

    def refused(run, call, why):
        before = _bits(run, thetas)
        with pytest.raises(engine.EngineError, match=why):
            _ffi.check(call())
        assert _bits(run, thetas) == before

    # values and the model
    plain = _runner(engine, name, rows, ut, ncomp)
    cont = _runner(engine, name, rows, ut, ncomp, continuum=(30.0, 3.0))
    for run in (plain, cont):
        for bad in ((-1.0, 3.0), (np.nan, 3.0), (3.0, np.inf)):
            refused(run, lambda: lib.nfa_specset_set_continuum(run._ss.handle, _ffi.dptr(np.array(bad))), 'finite brightness temperature >= 0')
    assert np.array_equal(cont._ss.get_continuum(), [[30.0, 3.0]]) and plain._ss.get_continuum() is None
    with pytest.raises(engine.EngineError, match='null argument'):
        _ffi.check(lib.nfa_specset_set_continuum(None, None))
    x = rows[0][0]
    gauss = engine.GaussianRunner.from_data([x, rows[0][1], NOISE, float(x[n // 2])], None, ncomp=2)
    g_thetas = np.tile([0.0, 1.0, 0.5, 0.7, 1.0, 2.0], (4, 1))
    before = _bits(gauss, g_thetas)
    with pytest.raises(engine.EngineError, match='Gaussian model has no optical depth'):
        _ffi.check(lib.nfa_specset_set_continuum(gauss._ss.handle, _ffi.dptr(np.array([3.0]))))
    assert _bits(gauss, g_thetas) == before and lib.nfa_specset_continuum(gauss._ss.handle, None) == 0
    for call in (lambda: gauss.set_continuum(3.0), lambda: engine.GaussianRunner.from_data([x, rows[0][1], NOISE, float(x[n // 2])], None, continuum=3.0)):
        with pytest.raises(ValueError, match='Gaussian model'):
            call()
    # wrong shapes: on the host, before any device call
    for bad in ([1.0], [1.0, 2.0, 3.0], np.ones((1, 2)), np.ones((2, 2))):
        before = _bits(cont, thetas)
        with pytest.raises(ValueError, match='continuum must be'):
            cont.set_continuum(bad)
        assert _bits(cont, thetas) == before
    cube = _cube(engine, ut, TC_ROWS)
    for bad in (np.ones((4, 2)), np.ones((5, 3)), np.ones(3)):
        with pytest.raises(ValueError, match='continuum must be'):
            cube.set_continuum(bad)
    assert np.array_equal(cube._ss.get_continuum(), TC_ROWS)
    # the four setters a continuum does not go with, in both orders and in the same words
    cal, rho, taps = np.array([0.1, 0.0]), np.array([[0.5, 0.25], [0.0, 0.0]]), np.array([[0.0, 0.25, 0.5, 0.25, 0.0]] * 2)
    tmpl, counts = np.zeros((4, 2 * n)), np.array([1, 0], dtype=np.int32)
    tmpl[0, :n] = np.sin(np.arange(n) / 7.0)
    tc = np.array([[30.0, 3.0]])
    others = {'calibration uncertainty': lambda h: lib.nfa_specset_set_calibration(h, _ffi.dptr(cal)),
              'correlated channel noise': lambda h: lib.nfa_specset_set_correlation(h, _ffi.dptr(rho)),
              'channel response': lambda h: lib.nfa_specset_set_response(h, _ffi.dptr(taps)),
              'nuisance templates': lambda h: lib.nfa_specset_set_templates(h, _ffi.dptr(tmpl), counts.ctypes.data_as(_ffi._ip))}
    for what, setter in others.items():
        words = f'a set with (a |an )?{what} takes no continuum background'
        refused(cont, lambda: setter(cont._ss.handle), words)
        other = _runner(engine, name, rows, ut, ncomp)
        _ffi.check(setter(other._ss.handle))
        refused(other, lambda: lib.nfa_specset_set_continuum(other._ss.handle, _ffi.dptr(tc)), words)
        assert lib.nfa_specset_continuum(other._ss.handle, None) == 0
        _ffi.check(lib.nfa_specset_set_continuum(other._ss.handle, _ffi.dptr(np.zeros((1, 2)))))      # no continuum: nothing to refuse
    # the resident kernel, in words of its own; a single point takes the batch path
    for run in (cont, _runner(engine, name, rows, ut, 1, continuum=3.0, baseline_order=1)):
        with RingServer(f'nfa_test_ring_cont_{os.getpid()}', n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match='no form for a continuum background: use nfa_ring_serve'):
                server.serve_device(lifetime_ms=20, idle_ms=100)
        assert np.isfinite(run.loglikelihood(np.full(run.ndim, 0.5)))


# ---------------------------------------------------------------------------- 5. science
SCI_TRUTH = np.array([0.3, 12.0, 6.0, 14.65, 0.5, 0.0])             # voff, trot, tex, ntot, sigm, orth: tau(1,1) ~ 2
SCI_RANGES = [(-4.0, 4.0), (8.0, 20.0), (2.8, 12.0), (13.0, 16.0), (0.15, 1.5), (0.0, 0.5)]
SCI_TC, SCI_NOISE, SCI_N = (30.0, 28.0), 0.5, 128


def test_run_multinest_fits_an_absorption_line(engine, nfo, mode_guard):
    """NH3 (1,1) + (2,2), one component of tex = 6 K and tau(1,1) ~ 2 before Tc = (30, 28) K: 20 K deep at a noise of 0.5 K.  With
    the continuum tex, voff and sigm lie within three posterior standard deviations of the truth and lnZ - null_lnZ is far
    above the fitter's default threshold, 11; without it no prior makes the model negative, and the same data are reported
    empty.

    Measured on an MI355X (nlive 100, seed 5): with the continuum lnZ -157.5 +- 0.4 against null_lnZ -7501.0, lnZ - null_lnZ =
    7343.5, voff 0.307 +- 0.007, tex 5.86 +- 0.71, sigm 0.492 +- 0.007; without it lnZ -7505.2, lnZ - null_lnZ = -4.3."""
    from nestfit_amd import sampler
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.synth import freq_axis
    import inspect
    lnz_thresh = inspect.signature(CubeFitter.__init__).parameters['lnZ_thresh'].default
    rng = np.random.default_rng(23)
    rows = []
    for trans, tc in zip((1, 2), SCI_TC):
        x = freq_axis(trans, SCI_N, 20.0)
        clean = cr.amm_cont(nfo, x, trans, SCI_TRUTH, tc)[0]
        assert clean.min() < (-15.0 if trans == 1 else -2.0) and clean.max() <= 0
        rows.append([x, clean + rng.normal(0, SCI_NOISE, SCI_N), SCI_NOISE, trans])
    ut = _simple_priors(engine, SCI_RANGES)
    gain = {}
    for tc in (SCI_TC, None):
        run = engine.AmmoniaRunner.from_data(rows, ut, ncomp=1, continuum=tc)
        res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=5)
        gain[tc is not None] = (res.lnZ - run.null_lnZ, res)
        print(f'continuum {tc}: lnZ {res.lnZ:.1f} +- {res.lnZ_err:.2f}, null_lnZ {run.null_lnZ:.1f}, lnZ - null_lnZ {res.lnZ - run.null_lnZ:.1f}; '
              f'mean {res.param_constr[0]}, std {res.param_constr[1]}')
    with_c, res = gain[True]
    mean, std = res.param_constr[0], res.param_constr[1]
    for k in (0, 2, 4):                                                   # voff, tex, sigm
        assert abs(mean[k] - SCI_TRUTH[k]) < 3 * std[k], (k, mean[k], std[k])
    assert std[2] < 1.0 and std[0] < 0.1 and std[4] < 0.1                  # constrained, not the prior's width
    assert with_c > lnz_thresh and gain[False][0] < lnz_thresh


# ---------------------------------------------------------------------------- 6. the cube route
def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 3 x 3 cube of absorption lines through CubeFitter with continuum maps, one pixel NaN in the map (skipped) and one with
    Tc = 0 (an emission line there): the store round-trips the maps in both formats, postprocess_run refuses a runner whose
    continuum differs, and peak_intensity is negative where the line absorbs.  (Both store formats: tests/test_continuum_cpu.py.)"""
    from nestfit_amd import ammonia
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    from nestfit_amd.synth import freq_axis
    n_chan, noise = 128, 0.5
    maps = [np.full((3, 3), SCI_TC[0]), np.full((3, 3), SCI_TC[1])]        # (lat, lon)
    for m in maps:
        m[0, 0] = 0.0
    maps[0][1, 2] = np.nan
    rng = np.random.default_rng(31)
    cubes = []
    for trans, tc_map in zip((1, 2), maps):
        x = freq_axis(trans, n_chan, 20.0)
        data = rng.normal(0, noise, (n_chan, 3, 3))
        for b in range(3):
            for l in range(3):
                truth = SCI_TRUTH + np.array([0.2 * (l - 1), 0, 0.3 * (b - 1), 0, 0, 0])
                if b == 0 and l == 0:
                    truth[2], truth[3] = 9.0, 15.0                            # the pixel without a continuum: a line in emission
                data[:, b, l] += cr.amm_cont(nfo, x, trans, truth, np.nan_to_num(tc_map[b, l]))[0]
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': 3, 'NAXIS2': 3, 'NAXIS3': n_chan, 'BUNIT': 'K',
               'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz', 'CRVAL3': float(x[0]),
               'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': float(x[n_chan // 2])}
        cubes.append(DataCube(SimpleCube(hdr, data), noise, trans_id=trans, continuum=tc_map))
    stack = CubeStack(cubes)
    ut = _simple_priors(engine, SCI_RANGES)
    runner, lon, lat = stack.to_device(ut, ncomp=1)
    assert lon.size == 8 and runner.continuum.shape == (8, 2)
    assert np.array_equal(runner.continuum, np.stack([maps[0][lat, lon], maps[1][lat, lon]], axis=1))
    fitter = CubeFitter(stack, ut, ammonia.AmmoniaRunner, lnZ_thresh=11, ncomp_max=1, mn_kwargs={'nlive': 60, 'tol': 2.0, 'seed': 5},
                        nlive_snr_fact=0)
    assert fitter.continuum.shape == (2, 3, 3)
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        got = store.read_model_continuum()
        assert got.dtype == np.float64 and np.array_equal(got, np.stack(maps), equal_nan=True)
        groups = list(store.iter_pix_groups())
        assert len(groups) == 8 and all(g.attrs['nbest'] == 1 for g in groups)        # the NaN pixel is skipped; every other detects
        with pytest.raises(ValueError, match='the runner has none'):                  # before any product is written
            pp.postprocess_run(store, stack, runner=engine.AmmoniaRunner.from_data(stack.get_spec_data(1, 1)[0], ut, ncomp=1))
        other = engine.AmmoniaRunner.from_data(stack.get_spec_data(1, 1)[0], ut, ncomp=1, continuum=(1.0, 2.0))
        with pytest.raises(ValueError, match="runner's continuum differs"):
            pp.postprocess_run(store, stack, runner=other)
        pp.postprocess_run(store, stack, runner=runner, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])               # (t, m, b, l)
        integ = np.asarray(store.hdf[f'{store.dpath}/integrated_intensity'])
        assert peak.shape == (2, 1, 3, 3) and np.isnan(peak[:, 0, 1, 2]).all()
        absorbs = np.ones((3, 3), dtype=bool)
        absorbs[0, 0] = absorbs[1, 2] = False
        assert (peak[0, 0][absorbs] < -10.0).all() and (peak[1, 0][absorbs] < -1.0).all() and (integ[:, 0][:, absorbs] < 0).all()
        assert (peak[:, 0, 0, 0] > 0.2).all() and (integ[:, 0, 0, 0] > 0).all()       # Tc = 0 there: the line emits
        # the model cube of a component is that component against its pixel's continuum
        spec = np.asarray(store.hdf[f'{store.dpath}/model_spec/trans1'])            # (m, S, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                     # (m, p, b, l)
        k = int(np.flatnonzero((lon == 1) & (lat == 2))[0])
        one, _ = runner.predict_batch(np.array([k], dtype=np.int32), np.ascontiguousarray(pmap[:1, :, 2, 1]))
        assert np.allclose(spec[0, :, 2, 1], one[0, :n_chan].astype(np.float32), rtol=1e-5, atol=1e-6)
        assert np.nanmin(spec[0, :, 2, 1]) == pytest.approx(peak[0, 0, 2, 1], rel=1e-5)
