"""The excitation-grid model on the device (nestfit_amd/excitation.py, nfa_specset_create_grid): every transition of
a pixel reads an excitation temperature and an optical depth of its own from a grid over kinetic temperature, density and
column density per line width -- grid_derive_kernel between the two stages, lnl_kernel_side (texs) behind it.

The reference is tests/grid_restatement.py -- the header's rule with `math` in doubles, then the numpy restatement of
c_hf_predict (tests/hf_restatement.py) once per spectrum with that spectrum's tex -- at the tolerances tests/test_lte.py holds
the LTE model to: zero pattern exact, spectra TIGHT, lnL LNL_RTOL; with a baseline, DESIGN 4.15's bound LNL_RTOL M.  The grids
are closed forms over lte_restatement's rigid rotor (grid_restatement.rotor_grid): at every theta of these tests the spectra's
tex differ by a factor 1.5 and more (asserted), so a kernel that reads one tex per component fails by far more than that."""
import ctypes as C
import functools
import os
import threading

import numpy as np
import pytest

import grid_restatement as gr
import hf_restatement as hfr
import layer_restatement as lay
import lte_restatement as lr
import tmpl_restatement as tr
from test_device_batches import _run_on_device
from test_hyperfine import _through_a_broker
from test_layered import _check_layered
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _check_spec, _simple_priors

pytestmark = pytest.mark.gpu

N_CHAN, N_ROWS, NOISE = 160, 200, 0.2          # 200 rows: three whole set-up groups of 64 and one of 8
RANGES = [(-6, 6), (7.0, 70.0), (4.4, 5.8), (11.8, 14.2), (0.1, 1.5)]      # wider than AXES_546: the clamped outside included
AXES_64 = (list(np.geomspace(9.0, 60.0, 64)), [4.7, 5.1, 5.5], [11.5, 12.5, 13.5, 14.5])


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _tables(engine, n_spec, axes=gr.AXES_546, wide=False):
    """The transitions of a runner of n_spec spectra: 1-0; 1-0 and 3-2; all three."""
    grid, t10, t21, t32 = gr.rotor_grid(engine, axes, wide=wide)
    return grid, ((t10,), (t10, t32), (t10, t21, t32))[n_spec - 1]


def _axis(t):
    return lr.axis(t.nu, N_CHAN, 45.0 if t.n > 26 else 20.0)


def _rows(tables, seed, noise=NOISE):
    rng = np.random.default_rng(seed)
    return [[_axis(t), rng.normal(0, NOISE, N_CHAN), noise, t] for t in tables]


def draw_params(rng, ncomp, grid, row):
    """The grid's coordinates below an axis, above it, exactly on a node and in between, in turn by row, component and axis;
    voff and sigm over the ranges a fit would use."""
    sigm = 10 ** rng.uniform(-1.0, 0.2, ncomp)
    x = np.empty((3, ncomp))
    for c in range(ncomp):
        for k, a in enumerate((grid.tkin, grid.lnden, grid.lncd)):
            kind = (row + c + k) % 4
            lo, hi = float(a[0]), float(a[-1])
            span = max(hi - lo, 1.0)
            x[k, c] = (rng.uniform(lo - 0.3 * span, lo) if kind == 0 else rng.uniform(hi, hi + 0.3 * span) if kind == 1
                       else a[rng.integers(0, a.size)] if kind == 2 else rng.uniform(lo, hi))
    x[0] = np.maximum(x[0], 3.0)
    return np.concatenate([rng.uniform(-6, 6, ncomp), x[0], x[1], x[2] + np.log10(gr.FWHM * sigm), sigm])


@functools.lru_cache(maxsize=None)
def _reference(n_spec, ncomp, which='546'):
    """(rows, thetas, spectra, lnL) of the restatement, computed once for both modes."""
    import nestfit_amd as na
    from oracle import nfo
    axes = {'546': gr.AXES_546, '111': gr.AXES_111, '64': AXES_64}[which]
    grid, tables = _tables(na, n_spec, axes)
    rows = _rows(tables, seed=10 * n_spec + ncomp)
    rng = np.random.default_rng(2000 + 10 * n_spec + ncomp)
    thetas = np.stack([draw_params(rng, ncomp, grid, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    want = [gr.restated(nfo, rows, th, tbgs) for th in thetas]
    spec, lnl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    if n_spec > 1:
        assert min(gr.tex_spread(tables, th) for th in thetas) > 1.5
    spec.setflags(write=False), lnl.setflags(write=False), thetas.setflags(write=False)
    return rows, thetas, spec, lnl


def _against_the_reference(engine, mode, n_spec, ncomp, which='546'):
    engine.set_exp_mode(mode)
    rows, thetas, want_spec, want_lnl = _reference(n_spec, ncomp, which)
    grid = rows[0][3].grid
    if which != '111':
        tk = thetas[:, ncomp:2 * ncomp]
        assert (tk < grid.tkin[0]).any() and (tk > grid.tkin[-1]).any() and np.isin(tk, grid.tkin).any()
    run = engine.GridRunner.from_data(rows, None, ncomp=ncomp)
    assert (run.ndim, run.n_params, run.n_spec, run.n_chan_tot, run.n_model) == (5 * ncomp, 5 * ncomp, n_spec, n_spec * N_CHAN, 5)
    assert run.null_lnZ == pytest.approx(sum(-np.sum(d ** 2) / (2 * s ** 2) for _, d, s, _ in rows), rel=1e-13)
    spec, lnl = run.predict_batch(np.array(thetas))
    worst, worst_lnl = 0.0, 0.0
    for sp, ll, ws, wl in zip(spec, lnl, want_spec, want_lnl):
        worst = max(worst, _check_spec(sp, ws, mode))
        worst_lnl = max(worst_lnl, abs(ll - wl) / abs(wl))
    print(f'grid {which} {mode} n_spec={n_spec} ncomp={ncomp}: worst relative Tb error {worst:.2e}, lnL {worst_lnl:.2e}')
    assert worst < TIGHT[mode]
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    # ... and per spectrum through grid_predict
    run.predict(np.array(thetas[1]))
    got = np.concatenate([s.get_spec() for s in run.spectra])
    assert _check_spec(got, want_spec[1], mode) < TIGHT[mode]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
@pytest.mark.parametrize('n_spec', [1, 2, 3])
def test_spectra_and_lnl_against_the_restatement(engine, n_spec, ncomp, mode, mode_guard):
    _against_the_reference(engine, mode, n_spec, ncomp)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('which', ['111', '64'])
def test_the_grid_of_one_node_and_the_axis_of_64(engine, which, mode, mode_guard):
    _against_the_reference(engine, mode, 2, 2, which)


@pytest.mark.parametrize('mode', MODES)
def test_one_spectrum_against_the_hyperfine_runner(engine, nfo, mode, mode_guard):
    """The hyperfine model fed the restatement's tex and ltau runs the same line arithmetic on the same lines."""
    engine.set_exp_mode(mode)
    grid, (t10,) = _tables(engine, 1)
    rng = np.random.default_rng(61)
    worst = 0.0
    for ncomp in (1, 3):
        rows = _rows((t10,), seed=5)
        plain = [[rows[0][0], rows[0][1], NOISE, engine.LineTable(t10.nu, t10.voff, t10.tau_wts)]]
        run = engine.GridRunner.from_data(rows, None, ncomp=ncomp)
        hyp = engine.HyperfineRunner.from_data(plain, None, ncomp=ncomp)
        thetas = np.stack([draw_params(rng, ncomp, grid, k) for k in range(64)])
        got, lnl = run.predict_batch(thetas)
        want, want_lnl = hyp.predict_batch(np.stack([gr.hf_params(t10, th) for th in thetas]))
        for g, w in zip(got, want):
            worst = max(worst, _check_spec(g, w, mode))
        np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    assert worst < TIGHT[mode]


# ---------------------------------------------------------------------------- the same bits on every route
def _routes(engine, run, rng, n_rows=513):
    """Host batch, device-pointer batches (coalesced and not), single points and a handful: one set of bits."""
    from nestfit_amd import _ffi
    U = rng.uniform(size=(n_rows, run.ndim))
    theta = U.copy()
    lnl = run.loglikelihood_batch(theta)
    assert np.isfinite(lnl).all()
    batches = [(None, rng.uniform(size=(256, run.ndim))) for _ in range(3)] + [(None, U[:200].copy())]
    for coalesce in (8, 1):
        _ffi.set_option('coalesce', coalesce)
        got = _run_on_device(_ffi, run._run.handle, batches)
        assert np.array_equal(got[-1][1], lnl[:200]) and np.array_equal(got[-1][0], theta[:200]), coalesce
    _ffi.set_option('coalesce', 8)
    for k in (0, 7, 150):                                   # single points: the batch path
        u = U[k].copy()
        assert run.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k])
    few = U[20:31].copy()                                   # a broker's handful
    assert np.array_equal(run.loglikelihood_batch(few), lnl[20:31]) and np.array_equal(few, theta[20:31])
    return U, theta, lnl


@pytest.mark.parametrize('mode', MODES)
def test_the_same_bits_on_every_route(engine, nfo, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, RANGES)
    _, tables = _tables(engine, 2)
    rows = _rows(tables, seed=3)
    run = engine.GridRunner.from_data(rows, ut, ncomp=2)
    U, theta, lnl = _routes(engine, run, rng)
    for split in (1, 2, 4):                                 # the rows of a unit over 1, 2 and 4 waves
        _ffi.set_option('lnl_split', split)
        other = engine.GridRunner.from_data(rows, ut, ncomp=2)
        assert np.array_equal(other.loglikelihood_batch(U[:200].copy()), lnl[:200]), split
    _ffi.set_option('lnl_split', 0)
    lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
    assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
    # predict_batch: whatever the batch, with and without spectra out, and grid_predict per spectrum
    spec, pl = run.predict_batch(theta[:40])
    assert np.array_equal(run.predict_batch(theta[:40], want_spectra=False)[1], pl)
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]
    np.testing.assert_allclose(pl, lnl[:40], rtol=LNL_RTOL[mode])
    run.predict(theta[3])
    assert np.array_equal(np.concatenate([s.get_spec() for s in run.spectra]), spec[3])
    assert _check_spec(spec[3], gr.restated(nfo, rows, theta[3])[0], mode) < TIGHT[mode]
    for k in (0, 100, 512):
        assert lnl[k] == pytest.approx(gr.restated(nfo, rows, theta[k])[1], rel=LNL_RTOL[mode])
    # the 30-line table: the wide instances
    _, wide = _tables(engine, 2, wide=True)
    rows_w = _rows(wide, seed=4)
    run_w = engine.GridRunner.from_data(rows_w, ut, ncomp=2)
    _, theta_w, lnl_w = _routes(engine, run_w, rng, n_rows=256)
    for k in (0, 100, 255):
        assert lnl_w[k] == pytest.approx(gr.restated(nfo, rows_w, theta_w[k])[1], rel=LNL_RTOL[mode])
    spec_w, _ = run_w.predict_batch(theta_w[:8])
    assert max(_check_spec(sp, gr.restated(nfo, rows_w, th)[0], mode) for sp, th in zip(spec_w, theta_w[:8])) < TIGHT[mode]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('order', [None, 0, 3])
def test_channel_noise_masked_channels_and_a_baseline(engine, nfo, order, mode, mode_guard):
    """A noise per channel with masked channels, with and without a baseline: the restatement's spectra under
    tmpl_restatement's weighted least squares, at DESIGN 4.15's bound."""
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(7)
    _, tables = _tables(engine, 2)
    rows = _rows(tables, seed=9)
    for row in rows:
        sig = rng.uniform(0.1, 0.3, N_CHAN)
        sig[rng.integers(0, N_CHAN, 5)] = np.inf
        row[1] = row[1] + 0.3 * np.linspace(-1, 1, N_CHAN) ** 2
        row[2] = sig
    grid = tables[0].grid
    thetas = np.stack([draw_params(rng, 2, grid, k) for k in range(48)])
    run = engine.GridRunner.from_data(rows, None, ncomp=2, baseline_order=order)
    spec, lnl = run.predict_batch(thetas)
    plain = [[x, d, NOISE, t] for x, d, _, t in rows]
    preds = np.stack([gr.restated(nfo, plain, th)[0] for th in thetas])
    assert max(_check_spec(sp, p, mode) for sp, p in zip(spec, preds)) < TIGHT[mode]
    want, M = tr.restate(rows, preds, order, None)
    dev = np.abs(lnl - want)
    print(f'grid {mode} order={order}: worst |lnL - want| / M {np.max(dev / M):.2e}')
    assert (dev <= LNL_RTOL[mode] * M).all()
    # the same bits from the unit cube's route and through the setter
    late = engine.GridRunner.from_data(rows, None, ncomp=2)
    late.set_baseline(order)
    assert np.array_equal(late.predict_batch(thetas)[1], lnl)


@pytest.mark.parametrize('mode', MODES)
def test_layered_transfer_with_an_excitation_per_spectrum(engine, nfo, mode, mode_guard):
    """layer_restatement's rule on the per-spectrum quantities: every spectrum layered with its own tex of every component."""
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(19)
    ncomp = 3
    grid, tables = _tables(engine, 2)
    rows = _rows(tables, seed=12)
    thetas = np.stack([draw_params(rng, ncomp, grid, k) for k in range(48)])
    thetas[:, :ncomp] = rng.uniform(-1.5, 1.5, (48, ncomp))                     # the layers overlap
    run = engine.GridRunner.from_data(rows, None, ncomp=ncomp, layered=True)
    summed = engine.GridRunner.from_data(rows, None, ncomp=ncomp)
    spec, lnl = run.predict_batch(thetas)
    worst, worst_lnl, differs = 0.0, 0.0, 0
    for sp, ll, th in zip(spec, lnl, thetas):
        want, S, want_lnl = [], [], 0.0
        for x, d, noise, t in rows:
            hp = gr.hf_params(t, th)
            w, s = lay.hf_layered(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(t), hp)
            worst = max(worst, _check_layered(sp[len(want) * N_CHAN:(len(want) + 1) * N_CHAN], w, s, mode, ncomp, hp[ncomp:2 * ncomp]))
            want.append(w)
            S.append(s)
            want_lnl += hfr.loglike(d, w, noise)
        worst_lnl = max(worst_lnl, abs(ll - want_lnl) / abs(want_lnl))
        assert ll == pytest.approx(want_lnl, rel=LNL_RTOL[mode])
        differs += int(np.max(np.abs(sp - summed.predict_batch(th[None])[0][0])) > 1e-3)
    print(f'grid layered {mode}: worst |got - want| / S {worst:.2e}, lnL {worst_lnl:.2e}')
    assert differs > 24                                                          # the layers do absorb one another


@pytest.mark.parametrize('mode', MODES)
def test_unit_cube_in_lnl_out_and_a_noise_uncertainty(engine, nfo, mode, mode_guard):
    from nestfit_amd._model import noise_marginal_lnl
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(78)
    ut = _simple_priors(engine, RANGES)
    ps = nfo.PriorSet(ut.lower())
    _, tables = _tables(engine, 3)
    rows = _rows(tables, seed=6)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    for ncomp in (1, 2):
        run = engine.GridRunner.from_data(rows, ut, ncomp=ncomp)
        U = rng.uniform(size=(N_ROWS, 5 * ncomp))
        theta = U.copy()
        lnl = run.loglikelihood_batch(theta)
        marg = engine.GridRunner.from_data(rows, ut, ncomp=ncomp, noise_uncertainty=0.1)
        lnl_m = marg.loglikelihood_batch(U.copy())
        for k in range(0, N_ROWS, 5):
            want_theta = U[k].copy()
            ps.transform(want_theta, ncomp)
            np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
            pred, want = gr.restated(nfo, rows, theta[k], tbgs)
            assert lnl[k] == pytest.approx(want, rel=LNL_RTOL[mode])
            h = [-hfr.loglike(d, pred[i * N_CHAN:(i + 1) * N_CHAN], s) for i, (_, d, s, _) in enumerate(rows)]
            assert lnl_m[k] == pytest.approx(float(np.sum(noise_marginal_lnl(h, N_CHAN, 0.1))), rel=10 * LNL_RTOL[mode])


# ---------------------------------------------------------------------------- what is refused
def _bits(run, thetas):
    spec, lnl = run.predict_batch(thetas)
    return spec.tobytes(), lnl.tobytes()


def test_the_six_refused_options_leave_the_set_as_it_was(engine, mode_guard):
    from nestfit_amd import _ffi
    from nestfit_amd.ring import RingClient, RingServer
    lib = _ffi.engine()
    grid, tables = _tables(engine, 2)
    rows = _rows(tables, seed=21)
    ut = _simple_priors(engine, RANGES)
    thetas = np.stack([draw_params(np.random.default_rng(5), 2, grid, k) for k in range(8)])
    n = N_CHAN
    cal, rho, taps = np.array([0.1, 0.0]), np.array([[0.5, 0.25], [0.0, 0.0]]), np.array([[0.0, 0.25, 0.5, 0.25, 0.0]] * 2)
    tmpl, counts = np.zeros((4, 2 * n)), np.array([1, 0], dtype=np.int32)
    tmpl[0, :n] = np.sin(np.arange(n) / 7.0)
    tc, nu = np.array([[30.0, 3.0]]), np.array([4.0, 0.0])
    setters = {'calibration uncertainty': (lambda h: lib.nfa_specset_set_calibration(h, _ffi.dptr(cal)), lib.nfa_specset_calibration),
               'noise correlation': (lambda h: lib.nfa_specset_set_correlation(h, _ffi.dptr(rho)), lib.nfa_specset_correlation),
               'channel response': (lambda h: lib.nfa_specset_set_response(h, _ffi.dptr(taps)), lib.nfa_specset_response),
               'nuisance templates': (lambda h: lib.nfa_specset_set_templates(h, _ffi.dptr(tmpl), counts.ctypes.data_as(_ffi._ip)), None),
               'continuum background': (lambda h: lib.nfa_specset_set_continuum(h, _ffi.dptr(tc)), lib.nfa_specset_continuum),
               'robust likelihood': (lambda h: lib.nfa_specset_set_robust(h, _ffi.dptr(nu)), lib.nfa_specset_robust)}
    python = {'calibration uncertainty': dict(calibration=0.1), 'noise correlation': dict(correlation=(0.5, 0.25)),
              'channel response': dict(response=(0.25, 0.5, 0.25)), 'nuisance templates': dict(templates=[tmpl[:1, :n], None]),
              'continuum background': dict(continuum=3.0), 'robust likelihood': dict(robust=4.0)}
    # both orders: before and after the options the model does take
    for dressed in (False, True):
        run = engine.GridRunner.from_data(rows, ut, ncomp=2, **(dict(baseline_order=2, layered=True, noise_uncertainty=0.1) if dressed else {}))
        before = _bits(run, thetas)
        for what, (setter, getter) in setters.items():
            assert setter(run._ss.handle) == 1                                       # NFA_ERR_ARG
            assert lib.nfa_last_error().decode() == 'a set of the excitation-grid model takes no ' + what
            assert getter is None or getter(run._ss.handle, None) == 0
            assert _bits(run, thetas) == before, what
            (name, value), = python[what].items()
            with pytest.raises(ValueError, match='a set of the excitation-grid model takes no ' + what):
                getattr(run, 'set_' + name)(value)
            with pytest.raises(ValueError, match='a set of the excitation-grid model takes no ' + what):
                engine.GridRunner.from_data(rows, ut, ncomp=2, **python[what])
            assert _bits(run, thetas) == before, what
        if not dressed:                                                              # ... and the taken ones after a refusal
            run.set_baseline(2)
            run._ss.set_layered(True)
            run.set_noise_uncertainty(0.1)
            assert _bits(run, thetas) != before
        # switching an option off is no request: nothing to refuse
        _ffi.check(lib.nfa_specset_set_robust(run._ss.handle, None))
        _ffi.check(lib.nfa_specset_set_continuum(run._ss.handle, _ffi.dptr(np.zeros((1, 2)))))
    # the resident kernel, in words of its own; nfa_ring_serve serves, with the batch path's bits
    run = engine.GridRunner.from_data(rows, ut, ncomp=2)
    name = f'nfa_test_ring_grid_{os.getpid()}'
    with RingServer(name, n_slots=1, runner=run) as server:
        with pytest.raises(engine.EngineError, match='the resident kernel has no form for an excitation per spectrum: use nfa_ring_serve'):
            server.serve_device(lifetime_ms=20, idle_ms=100)
    U = np.random.default_rng(12).uniform(size=(12, run.ndim))
    want_theta = U.copy()
    want = run.loglikelihood_batch(want_theta)
    errors = []
    with RingServer(name + 'h', n_slots=1, runner=run) as server:
        def serve():
            try:
                server.serve(idle_ms=10000)
            except Exception as e:                                    # pragma: no cover
                errors.append(e)
        th = threading.Thread(target=serve)
        th.start()
        client = RingClient(name + 'h', wait_ms=10000)
        theta = U.copy()
        lnl = np.array([client.loglikelihood(row) for row in theta])
        client.close()
        server.stop()
        th.join(timeout=30)
        assert not th.is_alive() and not errors
    assert np.array_equal(lnl, want) and np.array_equal(theta, want_theta)


def _create_grid(lib, n_lines=(1,), nus=(1e11,), voff=(0.0,), wts=(1.0,), tkin=(10.0, 20.0), lnden=(3.0, 4.0, 5.0), lncd=(13.0,),
                 tex=None, ltau=None, n_axes=None, noise='scalar', n=64):
    from nestfit_amd import _ffi
    n_spec = len(n_lines)
    xs = [np.linspace(1e11, 1.0001e11, n) for _ in range(n_spec)]
    xp = (_ffi._dp * n_spec)(*[_ffi.dptr(x) for x in xs])
    sizes = np.full(n_spec, n, dtype=np.int64)
    n_lines = np.asarray(n_lines, dtype=np.int32)
    nus, voff, wts, tkin, lnden, lncd = (np.ascontiguousarray(a, dtype=np.float64) for a in (nus, voff, wts, tkin, lnden, lncd))
    nt, nn, nc = n_axes or (tkin.size, lnden.size, lncd.size)
    cells = max(nt * nn * nc, 1) * n_spec if 0 < nt * nn * nc <= 1 << 20 else n_spec
    tex = np.ascontiguousarray(np.full(cells, 8.0) if tex is None else tex, dtype=np.float64)
    ltau = np.ascontiguousarray(np.zeros(cells) if ltau is None else ltau, dtype=np.float64)
    data = np.zeros((1, n * n_spec))
    sc, ch = np.full((1, n_spec), 0.1), np.full((1, n * n_spec), 0.1)
    h = C.c_void_p()
    rc = lib.nfa_specset_create_grid(C.byref(h), n_spec, sizes.ctypes.data_as(_ffi._lp), n_lines.ctypes.data_as(_ffi._ip),
                                     _ffi.dptr(nus), _ffi.dptr(voff), _ffi.dptr(wts), nt, _ffi.dptr(tkin), nn, _ffi.dptr(lnden), nc,
                                     _ffi.dptr(lncd), _ffi.dptr(tex), _ffi.dptr(ltau), xp, 1, _ffi.dptr(data),
                                     _ffi.dptr(sc) if noise in ('scalar', 'both') else None,
                                     _ffi.dptr(ch) if noise in ('channel', 'both') else None)
    msg = lib.nfa_last_error().decode()
    if rc == 0:
        lib.nfa_specset_destroy(h)
    return rc, msg


def test_the_creator_refuses_invalid_arguments_with_a_message(engine):
    from nestfit_amd import _ffi
    lib = _ffi.engine()
    ERR_ARG = 1
    assert _create_grid(lib)[0] == 0 and _create_grid(lib, noise='channel')[0] == 0
    assert _create_grid(lib, tkin=(10.0,), lnden=(3.0,), lncd=(13.0,))[0] == 0
    assert _create_grid(lib, tkin=np.arange(1.0, 65.0), lnden=np.arange(64.0), lncd=np.arange(16.0))[0] == 0     # 65536 nodes
    assert _create_grid(lib, n_lines=(2,), voff=(0.0, 1.0), wts=(0.5, 0.5 + 5e-7))[0] == 0
    bad_tex, bad_ltau = np.full(6, 8.0), np.zeros(6)
    bad = [
        (dict(n_axes=(0, 3, 1)), '1..64 nodes (tkin)'), (dict(n_axes=(2, 65, 1)), '1..64 nodes (lnden)'), (dict(n_axes=(2, 3, -1)), '1..64 nodes (lncd)'),
        (dict(tkin=np.arange(1.0, 65.0), lnden=np.arange(64.0), lncd=np.arange(17.0)), 'at most 65536 nodes'),
        (dict(tkin=(10.0, 10.0)), 'strictly ascending (tkin)'), (dict(tkin=(20.0, 10.0)), 'strictly ascending (tkin)'),
        (dict(lnden=(3.0, np.nan, 5.0)), 'strictly ascending (lnden)'), (dict(lnden=(3.0, 4.0, np.inf)), 'strictly ascending (lnden)'),
        (dict(lncd=(-np.inf,)), 'strictly ascending (lncd)'),
        (dict(tex=np.where(np.arange(6) == 4, 0.0, bad_tex)), 'cut the grid'), (dict(tex=np.where(np.arange(6) == 4, -3.0, bad_tex)), 'cut the grid'),
        (dict(tex=np.where(np.arange(6) == 5, np.nan, bad_tex)), 'node 5'), (dict(tex=np.where(np.arange(6) == 0, np.inf, bad_tex)), 'finite and positive'),
        (dict(ltau=np.where(np.arange(6) == 2, np.nan, bad_ltau)), 'optical depth'), (dict(ltau=np.where(np.arange(6) == 2, -np.inf, bad_ltau)), 'optical depth'),
        (dict(n_lines=(2,), voff=(0.0, 1.0), wts=(0.5, 0.4)), 'sum to 1'), (dict(wts=(2.0,)), 'sum to 1'),
        # every check of nfa_specset_create_lines
        (dict(n_lines=(0,)), 'lines'), (dict(nus=(0.0,)), 'rest frequency'), (dict(voff=(np.nan,)), 'velocity offset'),
        (dict(wts=(-1.0,)), 'weight'), (dict(n_lines=(2,), voff=(0.0, 1.0), wts=(0.0, 0.0)), 'all zero'),
        (dict(noise='none'), 'exactly one'), (dict(noise='both'), 'exactly one'),
    ]
    for kw, word in bad:
        rc, msg = _create_grid(lib, **kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)
    # the other creators refuse model 5, as they refuse 3 and 4: it needs its tables
    x = np.linspace(1e11, 1.0001e11, 64)
    xp = (_ffi._dp * 1)(_ffi.dptr(x))
    sizes, trans = np.array([64], dtype=np.int64), np.array([1], dtype=np.int32)
    data, noise, nu = np.zeros((1, 64)), np.full((1, 1), 0.1), np.array([1e11])
    h = C.c_void_p()
    for create, sig in ((lib.nfa_specset_create_model, noise), (lib.nfa_specset_create_channel_noise, np.full((1, 64), 0.1))):
        rc = create(C.byref(h), 5, 1, sizes.ctypes.data_as(_ffi._lp), trans.ctypes.data_as(_ffi._ip), _ffi.dptr(nu), xp, 1,
                    _ffi.dptr(data), _ffi.dptr(sig))
        assert rc == ERR_ARG and 'nfa_specset_create_grid' in lib.nfa_last_error().decode()
    # the Python route: the prior program must cover five parameters
    _, (t10,) = _tables(engine, 1)
    s = engine.GridSpectrum(_axis(t10), np.zeros(N_CHAN), 0.1, t10)
    with pytest.raises(engine.EngineError, match='prior program'):
        engine.GridRunner([s], _simple_priors(engine, RANGES[:4]), ncomp=1)


# ---------------------------------------------------------------------------- downstream: least squares and moments
def test_normal_equations_and_predict_moments_of_a_grid_runner(engine, mode_guard):
    """`normal_equations` against `lsq.normal_equations_from_spectra`'s reference on the runner's own `predict_batch` rows at
    tests/test_lsq.py's bound (`_check`), and `predict_moments` against numpy on `predict_batch` (`moments.moments_of`)."""
    from nestfit_amd import lsq
    from nestfit_amd.moments import moments_of
    from test_lsq import _check
    engine.set_exp_mode('table')
    rng = np.random.default_rng(41)
    _, tables = _tables(engine, 2)
    rows = _rows(tables, seed=15)
    run = engine.GridRunner.from_data(rows, None, ncomp=2)
    inside = [(-3, 3), (12.0, 50.0), (4.8, 5.4), (12.6, 13.6), (0.3, 1.0)]
    lo, hi = (np.repeat([b[k] for b in inside], 2) for k in (0, 1))
    thetas = rng.uniform(lo, hi, (3, 10))
    st = 1e-3 * (hi - lo)
    probe, inv = lsq.probe_rows(thetas, st, lo, hi)
    spec, _ = run.predict_batch(probe.reshape(-1, 10))
    data = np.concatenate([r[1] for r in rows])
    ne = run.normal_equations(thetas, st, lo, hi, chunk_rows=64)
    _check(ne, spec.reshape(3, 21, -1), inv, np.repeat(data[None], 3, axis=0), np.full((3, data.size), 1.0 / (NOISE * NOISE)), 'grid')
    assert np.array_equal(run.chi_squared(thetas), ne.chi2) and np.isfinite(ne.curv).all()
    assert np.all(np.diagonal(ne.curv, axis1=1, axis2=2) > 0)                    # every parameter moves the model, lnden too
    # weighted moments of the model spectra against numpy on predict_batch's rows
    many = rng.uniform(lo, hi, (40, 10))
    w = rng.uniform(0.1, 1.0, 40)
    mom = run.predict_moments(many, w)
    want = moments_of(run.predict_batch(many)[0], w, np.array([0, 40]))
    np.testing.assert_allclose(mom.mean, want[0], rtol=2e-7, atol=1e-30)        # tests/test_posterior_moments.py's bound
    np.testing.assert_allclose(mom.std, want[1], rtol=2e-7, atol=1e-30)


# ---------------------------------------------------------------------------- sampling
B_FIT, MU_FIT = 46.5e9, 3.4e-18
TRUTH_FIT = np.array([0.3, 25.0, 6.0, 13.3, 0.5])       # n = ncrit of the 3-2 line
FIT_RANGES = [(-3, 3), (10.0, 55.0), (4.8, 6.8), (12.2, 14.2), (0.2, 1.2)]
FIT_AXES = (list(np.linspace(8.0, 60.0, 14)), list(np.linspace(4.5, 7.0, 11)), list(np.linspace(11.0, 15.0, 9)))


def fit_rows(na, nfo, seed=17, noise=0.01, n_chan=160):
    """1-0 and 3-2 of one component at TRUTH_FIT on a grid that covers FIT_RANGES: (rows, grid)."""
    grid, t10, _, t32 = gr.rotor_grid(na, FIT_AXES, name='fit grid')
    rng = np.random.default_rng(seed)
    rows = []
    for t in (t10, t32):
        x = lr.axis(t.nu, n_chan, 16.0)
        rows.append([x, gr.grid_predict(nfo, x, hfr.tbg_of(nfo, x), t, TRUTH_FIT) + rng.normal(0, noise, n_chan), noise, t])
    return rows, grid


def test_run_multinest_recovers_tkin_density_and_column(engine, nfo, mode_guard):
    """One component over 1-0 (close to thermal: tkin) and 3-2 (n = its critical density: the density), 160 channels each;
    tkin, lnden and lncol within 5 posterior standard deviations of the truth."""
    from nestfit_amd import lsq, sampler
    assert gr.NCRIT[2] == 10 ** TRUTH_FIT[2]
    rows, grid = fit_rows(engine, nfo)
    assert gr.tex_spread([r[3] for r in rows], TRUTH_FIT) > 1.5
    ut = _simple_priors(engine, FIT_RANGES)
    assert grid.covers(*lsq.prior_box(ut, 1))
    run = engine.GridRunner.from_data(rows, ut, ncomp=1)
    res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=200, seed=5)
    mean, std = res.param_constr[0], res.param_constr[1]
    print(f'lnZ - null_lnZ = {res.lnZ - run.null_lnZ:.1f}; mean {mean}, std {std}, truth {TRUTH_FIT}')
    assert res.lnZ - run.null_lnZ > 11                              # the fitter's default lnZ_thresh
    for k in (1, 2, 3):
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])


def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube over 1-0 and 3-2: fit_cube, the store with its grid, the map products; and, on the same stack and store
    without a change to either, `lsq.fit_cube` and `generate_posterior_profiles`."""
    from nestfit_amd import lsq, postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    grid, t10, _, t32 = gr.rotor_grid(engine, FIT_AXES, name='fit grid')
    rng = np.random.default_rng(31)
    n_side, n_chan, noise = 4, 128, 0.02
    truths = np.stack([rng.uniform(-1, 1, 16), rng.uniform(18.0, 32.0, 16), rng.uniform(5.7, 6.3, 16), rng.uniform(13.1, 13.5, 16),
                       rng.uniform(0.4, 0.7, 16)], axis=1)

    def cubes_of(tables):
        out = []
        for k, tab in enumerate(tables):
            x = lr.axis(tab.nu, n_chan, 16.0)
            tbg = hfr.tbg_of(nfo, x)
            data = np.random.default_rng(100 + k).normal(0, noise, (n_chan, n_side, n_side))
            for p, th in enumerate(truths):
                data[:, p // n_side, p % n_side] += gr.grid_predict(nfo, x, tbg, tab, th)
            hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
                   'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
                   'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': tab.nu}
            out.append(DataCube(SimpleCube(hdr, data), noise, lines=tab))
        return out
    stack = CubeStack(cubes_of((t10, t32)))
    ut = _simple_priors(engine, FIT_RANGES)
    fitter = CubeFitter(stack, ut, engine.GridRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 60, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (5, 5, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'grid' and store.read_model_lines() == [t10, t32]
        assert np.array_equal(np.asarray(store.hdf['/model_grid/tkin'][...]), grid.tkin)
        groups = list(store.iter_pix_groups())
        assert len(groups) == 16 and all(g.attrs['nbest'] == 1 for g in groups)
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])              # (t, m, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                    # (m, p, b, l)
        assert peak.shape == (2, 1, 4, 4) and np.isfinite(peak).all()
        predict = pp._device_predictor(store, stack)                               # table mode, like the products
        rows = [[dc.xarr, np.zeros(n_chan), 1.0, dc.lines] for dc in stack.cubes]
        worst = 0.0
        for l in range(4):
            for b in range(4):
                th = np.ascontiguousarray(pmap[0, :, b, l])
                truth = truths[b * n_side + l]                                     # (truth k sits at lat k // 4, lon k % 4)
                assert abs(th[0] - truth[0]) < 0.3 and abs(th[1] - truth[1]) < 5.0 and abs(th[2] - truth[2]) < 0.3 and abs(th[3] - truth[3]) < 0.2
                got, _, _ = predict(np.array([l]), np.array([b]), th[None, :], True)
                worst = max(worst, _check_spec(got[0], gr.restated(nfo, rows, th)[0], 'table'))
                for k, sl in enumerate((slice(0, n_chan), slice(n_chan, 2 * n_chan))):
                    assert peak[k, 0, b, l] == got[0][sl].max()
        assert worst < TIGHT['table']
        # posterior-mean model cubes of the same store, unchanged
        pp.generate_posterior_profiles(store, stack)
        assert any('post' in name for name in store.hdf[store.dpath])
    # a stack with a changed table is refused: by the check and by the device predictor
    warmer = grid.transition(t32.nu, np.array(t32.tex) * 1.01, t32.ltau, name='3-2')
    with HdfStore(path) as store:
        other = CubeStack(cubes_of((t10, warmer)))
        with pytest.raises(ValueError, match='line tables differ'):
            pp.check_model_lines(store, other)
        with pytest.raises(ValueError, match='line tables differ'):
            pp._device_predictor(store, other)
    # least squares on the same stack
    engine.set_exp_mode('table')
    fit = lsq.fit_cube(stack, ut, engine.GridRunner, ncomp=1, n_draws=2048, n_starts=4, seed=1)
    assert fit.params.shape == fit.errors.shape == (5, 4, 4) and np.all(fit.status == 'converged'), fit.status
    off = np.abs(fit.params - truths.T.reshape(5, 4, 4)) / fit.errors
    print(f'grid fit_cube: truth within {off.max():.2f} error bars')
    assert np.all(off <= 5)
