"""The hyperfine model of caller-supplied line tables on the device (nestfit_amd/hyperfine.py, nfa_specset_create_lines).

Two references.  A shipped N2H+ table handed back through `LineTable` must give the N2H+ model's bits, whatever the
route (the kernels read the same rows either way).  Any other table is held to the numpy restatement of c_hf_predict
(tests/hf_restatement.py, pinned to the oracle in tests/test_hyperfine_cpu.py) at the tolerances
tests/test_sibling_models.py holds N2H+ to: zero pattern exact, spectra TIGHT, lnL LNL_RTOL."""
import ctypes as C

import numpy as np
import pytest

import hf_restatement as hfr
from test_device_batches import _run_on_device
from test_hyperfine_cpu import draw_params, n2hp_axis
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _check_spec, _simple_priors

pytestmark = pytest.mark.gpu

RANGES = [(-6, 6), (2.8, 20), (-1.5, 1.0), (0.1, 1.5)]


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    engine.set_exp_mode('fast')


# ---------------------------------------------------------------------------- same table, same bits
def _pair(engine, nfo, rng, trans, ncomp, noise_of=None, spectra=None, **kw):
    """A DiazenyliumRunner and a HyperfineRunner on copies of the same tables, data and priors: two spectra, the
    transition `trans` and its neighbour (so every such set holds a table of 40 lines or more: the wide forms), or the
    (transition, channels) pairs of `spectra`."""
    ut = _simple_priors(engine, RANGES)
    rows_d, rows_h = [], []
    truth = np.array([-1.0, 8.0, 0.3, 0.4])
    for t, n in spectra or ((trans, 1024), (trans % 3 + 1, 700)):
        x = n2hp_axis(t, n)
        sc = nfo.DiazenyliumSpectrum(x, np.zeros(n), 0.15, t)
        nfo.nnhp_predict(sc, truth)
        data = sc.get_spec() + rng.normal(0, 0.15, n)
        noise = 0.15 if noise_of is None else noise_of(rng, n)
        rows_d.append([x, data, noise, t])
        rows_h.append([x, data, noise, engine.LineTable.builtin('diazenylium', t)])
    return (engine.DiazenyliumRunner.from_data(rows_d, ut, ncomp=ncomp, **kw),
            engine.HyperfineRunner.from_data(rows_h, ut, ncomp=ncomp, **kw))


def _same_bits(engine, rd, rh, rng, n_rows=513):
    U = rng.uniform(size=(n_rows, rd.ndim))
    Ud, Uh = U.copy(), U.copy()
    ld, lh = rd.loglikelihood_batch(Ud), rh.loglikelihood_batch(Uh)
    assert np.array_equal(Ud, Uh) and np.array_equal(ld, lh, equal_nan=True)
    assert rd.null_lnZ == rh.null_lnZ
    for k in (0, 7, 150):                                   # single points
        ud, uh = U[k].copy(), U[k].copy()
        assert rd.loglikelihood(ud) == rh.loglikelihood(uh) == ld[k] and np.array_equal(ud, uh)
    few_d, few_h = U[20:31].copy(), U[20:31].copy()
    assert np.array_equal(rd.loglikelihood_batch(few_d), rh.loglikelihood_batch(few_h)) and np.array_equal(few_d, few_h)
    sd, pd = rd.predict_batch(Ud[:40])                      # spectra out (theta in)
    sh, ph = rh.predict_batch(Uh[:40])
    assert np.array_equal(sd, sh) and np.array_equal(pd, ph)
    rd.predict(Ud[3])
    rh.predict(Uh[3])
    for a, b in zip(rd.spectra, rh.spectra):
        assert np.array_equal(a.get_spec(), b.get_spec()) and a.loglikelihood == b.loglikelihood
        assert np.array_equal(a.tbg_arr, b.tbg_arr) and a.null_lnZ == b.null_lnZ
    return U, Ud, ld


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('trans', [1, 2, 3])
def test_builtin_table_gives_the_diazenylium_bits(engine, nfo, trans, mode, mode_guard):
    """Every set here holds a table of 40 or 45 lines beside `trans`: the wide forms, whose single points go through the
    batch kernels.  The narrow forms, the point kernel and a broker are test_narrow_builtin_table_... below."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(100 + trans)
    rd, rh = _pair(engine, nfo, rng, trans, ncomp=2)
    assert (rh.ndim, rh.n_params, rh.n_spec, rh.n_chan_tot, rh.n_model) == (8, 8, 2, 1724, 4)
    U, theta, lnl = _same_bits(engine, rd, rh, rng)
    # device-pointer batches, coalesced and not: the host call's bits from both runners
    batches = [(None, rng.uniform(size=(256, 8))) for _ in range(5)] + [(None, U[:200].copy())]
    for coalesce in (8, 1):
        _ffi.set_option('coalesce', coalesce)
        gd = _run_on_device(_ffi, rd._run.handle, batches)
        gh = _run_on_device(_ffi, rh._run.handle, batches)
        for (td, ldv), (th, lhv) in zip(gd, gh):
            assert np.array_equal(td, th) and np.array_equal(ldv, lhv, equal_nan=True), (trans, mode, coalesce)
        assert np.array_equal(gh[-1][1], lnl[:200]) and np.array_equal(gh[-1][0], theta[:200])
    _ffi.set_option('coalesce', 8)
    # a baseline of order 1, and a noise per channel (with masked channels)
    _same_bits(engine, *_pair(engine, nfo, rng, trans, ncomp=2, baseline_order=1), rng, n_rows=192)

    def chan_noise(r, n):
        s = r.uniform(0.1, 0.3, n)
        s[r.integers(0, n, 9)] = np.inf
        return s
    _same_bits(engine, *_pair(engine, nfo, rng, trans, ncomp=1, noise_of=chan_noise), rng, n_rows=192)


NARROW = ((1, 1024), (1, 700))             # N2H+ 1-0 twice: 15 lines, the narrow forms


def _through_a_broker(engine, run, U):
    """lnL and theta of the rows U[threads, calls, ndim], every thread a serial caller of one broker on `run`."""
    import threading
    from nestfit_amd.broker import LikelihoodBroker
    n_threads, n_calls = U.shape[:2]
    theta, lnl, errors = U.copy(), np.zeros(U.shape[:2]), []
    broker = LikelihoodBroker(run, max_batch=64, max_wait_us=2000, n_clients=n_threads)

    def caller(k):
        try:
            for j in range(n_calls):
                lnl[k, j] = broker.loglikelihood(theta[k, j])
        except Exception as e:                                    # pragma: no cover
            errors.append(e)
    threads = [threading.Thread(target=caller, args=(k,)) for k in range(n_threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    broker.close()
    assert not errors
    return lnl, theta


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3])
def test_narrow_builtin_table_gives_the_diazenylium_bits(engine, nfo, ncomp, mode, mode_guard):
    """At most 26 lines and ndim <= 24, what most tables of one's own will be: the narrow likelihood forms (two
    components: the packed windows), the point kernel for single points and handfuls, a broker's batches, device
    batches coalesced and not, a baseline and a channel noise."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(500 + ncomp)
    rd, rh = _pair(engine, nfo, rng, 1, ncomp=ncomp, spectra=NARROW)
    U, theta, lnl = _same_bits(engine, rd, rh, rng)
    batches = [(None, rng.uniform(size=(256, rd.ndim))) for _ in range(5)] + [(None, U[:200].copy())]
    for coalesce in (8, 1):
        _ffi.set_option('coalesce', coalesce)
        gd = _run_on_device(_ffi, rd._run.handle, batches)
        gh = _run_on_device(_ffi, rh._run.handle, batches)
        for (td, ldv), (th, lhv) in zip(gd, gh):
            assert np.array_equal(td, th) and np.array_equal(ldv, lhv, equal_nan=True), (ncomp, mode, coalesce)
        assert np.array_equal(gh[-1][1], lnl[:200]) and np.array_equal(gh[-1][0], theta[:200])
    _ffi.set_option('coalesce', 8)
    Ub = U[:12 * 20].reshape(12, 20, rd.ndim)
    ld, td = _through_a_broker(engine, rd, Ub)
    lh, th = _through_a_broker(engine, rh, Ub)
    assert np.array_equal(ld, lh) and np.array_equal(td, th)
    assert np.array_equal(lh.ravel(), lnl[:240]) and np.array_equal(th.reshape(240, -1), theta[:240])
    if ncomp == 2:
        _same_bits(engine, *_pair(engine, nfo, rng, 1, ncomp=2, spectra=NARROW, baseline_order=1), rng, n_rows=192)

        def chan_noise(r, n):
            s = r.uniform(0.1, 0.3, n)
            s[r.integers(0, n, 9)] = np.inf
            return s
        _same_bits(engine, *_pair(engine, nfo, rng, 1, ncomp=2, spectra=NARROW, noise_of=chan_noise), rng, n_rows=192)


@pytest.mark.parametrize('mode', MODES)
def test_narrow_tables_loglikelihood_against_the_restatement(engine, nfo, mode, mode_guard):
    """The 1-line and the 3-line table, 1-3 components: unit cube in, theta and lnL out through the narrow likelihood
    forms (a batch), the point kernel (single points, a handful) and a broker."""
    engine.set_exp_mode(mode)
    one, three, _ = synthetic_tables(engine)
    rng = np.random.default_rng(79)
    ut = _simple_priors(engine, RANGES)
    ps = nfo.PriorSet(ut.lower())
    rows = [[_axis(one, 256, 20.0), rng.normal(0, 0.2, 256), 0.2, one],
            [_axis(three, 1024, 20.0), rng.normal(0, 0.2, 1024), 0.2, three]]
    for ncomp in (1, 2, 3):
        run = engine.HyperfineRunner.from_data(rows, ut, ncomp=ncomp)
        U = rng.uniform(size=(128, 4 * ncomp))
        theta = U.copy()
        lnl = run.loglikelihood_batch(theta)
        for k in range(0, 128, 4):
            want_theta = U[k].copy()
            ps.transform(want_theta, ncomp)
            np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
            assert lnl[k] == pytest.approx(_restated(nfo, rows, theta[k])[1], rel=LNL_RTOL[mode])
        for k in (0, 4, 64):                                 # the point kernel: the batch's bits
            u = U[k].copy()
            assert run.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k])
        few = U[8:19].copy()
        assert np.array_equal(run.loglikelihood_batch(few), lnl[8:19]) and np.array_equal(few, theta[8:19])
        lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
        assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])


def test_run_multinest_takes_the_same_path(engine, nfo, mode_guard):
    """N2H+ 1-0 alone: the narrow forms, the sampler's own route."""
    from nestfit_amd import sampler
    rd, rh = _pair(engine, nfo, np.random.default_rng(7), 1, ncomp=1, spectra=((1, 1024),))
    a = sampler.run_multinest(rd, sampler.Dumper(sampler.MemoryGroup()), nlive=60, seed=2)
    b = sampler.run_multinest(rh, sampler.Dumper(sampler.MemoryGroup()), nlive=60, seed=2)
    assert (a.lnZ, a.n_iter, a.n_evals) == (b.lnZ, b.n_iter, b.n_evals)


# ---------------------------------------------------------------------------- other tables against the restatement
def synthetic_tables(engine):
    """Seeded: 1 line; 3 lines of unequal weights; 40 lines at distinct offsets over +-40 km/s."""
    rng = np.random.default_rng(1234)
    one = engine.LineTable(72.4e9, [0.0], [1.0], name='one')
    three = engine.LineTable(88.6318e9, [-7.1, 0.0, 4.9], [0.2, 0.5, 0.3], name='three')
    v40 = np.sort(rng.uniform(-40, 40, 40))
    assert np.unique(v40).size == 40
    rng.shuffle(v40)
    forty = engine.LineTable(144.2e9, v40, rng.uniform(0.005, 0.06, 40), name='forty')
    return one, three, forty


def _axis(table, n, vhalf):
    return table.nu * (1.0 - np.linspace(vhalf, -vhalf, n) / hfr.CKMS)


def _restated(nfo, rows, theta):
    """(spectra of the rows concatenated, lnL) of the restatement for one parameter vector."""
    preds = [hfr.hf_predict(nfo, x, hfr.tbg_of(nfo, x), hfr.table_of(tab), theta) for x, _, _, tab in rows]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl


@pytest.mark.parametrize('mode', MODES)
def test_synthetic_tables_against_the_restatement(engine, nfo, mode, mode_guard):
    engine.set_exp_mode(mode)
    one, three, forty = synthetic_tables(engine)
    rng = np.random.default_rng(77)
    worst = 0.0
    for (ta, tb), (na_, nb) in (((one, three), (256, 1024)), ((three, forty), (1024, 256)), ((forty, one), (1024, 1024))):
        rows = []
        for tab, n in ((ta, na_), (tb, nb)):
            x = _axis(tab, n, 55.0 if tab is forty else 20.0)
            rows.append([x, rng.normal(0, 0.2, n), 0.2, tab])
        for ncomp in (1, 2, 3):
            run = engine.HyperfineRunner.from_data(rows, None, ncomp=ncomp)
            assert run.null_lnZ == pytest.approx(sum(-np.sum(d ** 2) / (2 * s ** 2) for _, d, s, _ in rows), rel=1e-13)
            thetas = np.stack([draw_params(rng, ncomp) for _ in range(6)])
            spec, lnl = run.predict_batch(thetas)
            for th, sp, ll in zip(thetas, spec, lnl):
                want, want_lnl = _restated(nfo, rows, th)
                worst = max(worst, _check_spec(sp, want, mode))
                assert ll == pytest.approx(want_lnl, rel=LNL_RTOL[mode])
            # ... and per spectrum through hf_predict
            run.predict(thetas[0])
            want, _ = _restated(nfo, rows, thetas[0])
            got = np.concatenate([s.get_spec() for s in run.spectra])
            worst = max(worst, _check_spec(got, want, mode))
    print(f'hyperfine {mode}: worst relative Tb error {worst:.2e}')
    assert worst < TIGHT[mode]


@pytest.mark.parametrize('mode', MODES)
def test_loglikelihood_with_priors_against_the_restatement(engine, nfo, mode, mode_guard):
    engine.set_exp_mode(mode)
    _, three, forty = synthetic_tables(engine)
    rng = np.random.default_rng(78)
    ut = _simple_priors(engine, RANGES)
    rows = [[_axis(three, 512, 20.0), rng.normal(0, 0.2, 512), 0.2, three],
            [_axis(forty, 1024, 55.0), rng.normal(0, 0.2, 1024), 0.2, forty]]
    run = engine.HyperfineRunner.from_data(rows, ut, ncomp=2)
    U = rng.uniform(size=(96, 8))
    theta = U.copy()
    lnl = run.loglikelihood_batch(theta)
    ps = nfo.PriorSet(ut.lower())
    for k in range(0, 96, 4):
        want_theta = U[k].copy()
        ps.transform(want_theta, 2)
        np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
        assert lnl[k] == pytest.approx(_restated(nfo, rows, theta[k])[1], rel=LNL_RTOL[mode])


def test_window_indices_equal_the_restatement(engine, nfo, mode_guard):
    from nestfit_amd import _ffi, hyperfine
    rng = np.random.default_rng(5)
    for tab in synthetic_tables(engine):
        for n in (256, 1024):
            x = _axis(tab, n, 30.0)
            sg = hyperfine.HyperfineSpectrum(x, np.zeros(n), 0.1, tab)
            run = sg._runner(1)
            for _ in range(40):
                voff, sigm = rng.uniform(-25, 25), 10 ** rng.uniform(-2, 0.5)
                lo, hi = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32)
                _ffi.test_check(_ffi.test_engine().nfa_test_windows(run.handle, 0, voff, sigm, lo.ctypes.data_as(_ffi._ip),
                                                                    hi.ctypes.data_as(_ffi._ip)))
                clo, chi = hfr.hf_windows(x, hfr.table_of(tab), voff, sigm)
                skipped = clo < 0
                assert np.array_equal(lo[:tab.n][~skipped], clo[~skipped])
                assert np.array_equal(hi[:tab.n][~skipped], chi[~skipped])
                assert (lo[:tab.n][skipped] == hi[:tab.n][skipped]).all()


@pytest.mark.parametrize('mode', MODES)
def test_the_order_of_a_tables_rows_does_not_matter(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    _, three, forty = synthetic_tables(engine)
    rng = np.random.default_rng(9)
    ut = _simple_priors(engine, RANGES)
    perm3, perm40 = np.array([2, 0, 1]), rng.permutation(40)
    three_p = engine.LineTable(three.nu, three.voff[perm3], three.tau_wts[perm3])
    forty_p = engine.LineTable(forty.nu, forty.voff[perm40], forty.tau_wts[perm40])
    data = [rng.normal(0, 0.2, 512), rng.normal(0, 0.2, 1024)]
    runs = []
    for a, b in ((three, forty), (three_p, forty_p)):
        rows = [[_axis(a, 512, 20.0), data[0], 0.2, a], [_axis(b, 1024, 55.0), data[1], 0.2, b]]
        runs.append(engine.HyperfineRunner.from_data(rows, ut, ncomp=2))
    U = rng.uniform(size=(320, 8))
    Ua, Ub = U.copy(), U.copy()
    la, lb = runs[0].loglikelihood_batch(Ua), runs[1].loglikelihood_batch(Ub)
    assert np.array_equal(Ua, Ub) and np.array_equal(la, lb)
    sa, _ = runs[0].predict_batch(Ua[:32])
    sb, _ = runs[1].predict_batch(Ub[:32])
    assert np.array_equal(sa, sb)
    ua, ub = U[5].copy(), U[5].copy()
    assert runs[0].loglikelihood(ua) == runs[1].loglikelihood(ub) == la[5]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', range(1, 11))
def test_component_counts_one_to_ten(engine, nfo, ncomp, mode, mode_guard):
    engine.set_exp_mode(mode)
    _, three, _ = synthetic_tables(engine)
    rng = np.random.default_rng(300 + ncomp)
    rows = [[_axis(three, 512, 20.0), rng.normal(0, 0.2, 512), 0.2, three]]
    run = engine.HyperfineRunner.from_data(rows, None, ncomp=ncomp)
    thetas = np.stack([draw_params(rng, ncomp) for _ in range(4)])
    spec, lnl = run.predict_batch(thetas)
    worst = 0.0
    for th, sp, ll in zip(thetas, spec, lnl):
        want, want_lnl = _restated(nfo, rows, th)
        worst = max(worst, _check_spec(sp, want, mode))
        assert ll == pytest.approx(want_lnl, rel=LNL_RTOL[mode])
    assert worst < TIGHT[mode]


# ---------------------------------------------------------------------------- what the C ABI refuses
def _create_lines(lib, n_lines, nus, voff, wts, noise='scalar', n=64):
    from nestfit_amd import _ffi
    n_spec = len(n_lines)
    xs = [np.linspace(1e11, 1.0001e11, n) for _ in range(n_spec)]
    xp = (_ffi._dp * n_spec)(*[_ffi.dptr(x) for x in xs])
    sizes = np.full(n_spec, n, dtype=np.int64)
    n_lines = np.asarray(n_lines, dtype=np.int32)
    nus, voff, wts = (np.ascontiguousarray(a, dtype=np.float64) for a in (nus, voff, wts))
    data = np.zeros((1, n * n_spec))
    sc, ch = np.full((1, n_spec), 0.1), np.full((1, n * n_spec), 0.1)
    h = C.c_void_p()
    rc = lib.nfa_specset_create_lines(C.byref(h), n_spec, sizes.ctypes.data_as(_ffi._lp), n_lines.ctypes.data_as(_ffi._ip),
                                      _ffi.dptr(nus), _ffi.dptr(voff), _ffi.dptr(wts), xp, 1, _ffi.dptr(data),
                                      _ffi.dptr(sc) if noise in ('scalar', 'both') else None,
                                      _ffi.dptr(ch) if noise in ('channel', 'both') else None)
    msg = lib.nfa_last_error().decode()
    if rc == 0:
        lib.nfa_specset_destroy(h)
    return rc, msg


def test_the_engine_refuses_invalid_tables_with_a_message(engine):
    from nestfit_amd import _ffi
    lib = _ffi.engine()
    ERR_ARG = 1
    assert _create_lines(lib, [2], [1e11], [0.0, 1.0], [0.5, 0.5])[0] == 0
    assert _create_lines(lib, [2], [1e11], [0.0, 1.0], [0.5, 0.5], noise='channel')[0] == 0
    c = hfr.CKMS
    bad = [
        (([0], [1e11], [0.0], [1.0]), 'lines'),
        (([51], [1e11], np.zeros(51), np.ones(51)), 'lines'),
        (([1], [0.0], [0.0], [1.0]), 'rest frequency'),
        (([1], [-1e11], [0.0], [1.0]), 'rest frequency'),
        (([1], [np.inf], [0.0], [1.0]), 'rest frequency'),
        (([1], [np.nan], [0.0], [1.0]), 'rest frequency'),
        (([2], [1e11], [0.0, np.nan], [1.0, 1.0]), 'velocity offset'),
        (([1], [1e11], [np.inf], [1.0]), 'velocity offset'),
        (([1], [1e11], [c], [1.0]), 'velocity offset'),
        (([1], [1e11], [-c], [1.0]), 'velocity offset'),
        (([2], [1e11], [0.0, 1.0], [1.0, -0.1]), 'weight'),
        (([1], [1e11], [0.0], [np.nan]), 'weight'),
        (([1], [1e11], [0.0], [np.inf]), 'weight'),
        (([2], [1e11], [0.0, 1.0], [0.0, 0.0]), 'all zero'),
        # the second spectrum's table is the bad one
        (([1, 2], [1e11, 1e11], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]), 'all zero'),
    ]
    for args, word in bad:
        rc, msg = _create_lines(lib, *args)
        assert rc == ERR_ARG and word in msg, (args, rc, msg)
    for noise in ('none', 'both'):
        rc, msg = _create_lines(lib, [1], [1e11], [0.0], [1.0], noise=noise)
        assert rc == ERR_ARG and 'exactly one' in msg
    # the existing creators keep refusing model 3: it needs tables
    x = np.linspace(1e11, 1.0001e11, 64)
    xp = (_ffi._dp * 1)(_ffi.dptr(x))
    sizes, trans = np.array([64], dtype=np.int64), np.array([1], dtype=np.int32)
    data, noise, nu = np.zeros((1, 64)), np.full((1, 1), 0.1), np.array([1e11])
    h = C.c_void_p()
    for create, sig in ((lib.nfa_specset_create_model, noise), (lib.nfa_specset_create_channel_noise, np.full((1, 64), 0.1))):
        rc = create(C.byref(h), 3, 1, sizes.ctypes.data_as(_ffi._lp), trans.ctypes.data_as(_ffi._ip), _ffi.dptr(nu), xp, 1,
                    _ffi.dptr(data), _ffi.dptr(sig))
        assert rc == ERR_ARG and 'nfa_specset_create_lines' in lib.nfa_last_error().decode()
    rc = lib.nfa_specset_create_model(C.byref(h), 4, 1, sizes.ctypes.data_as(_ffi._lp), trans.ctypes.data_as(_ffi._ip),
                                      _ffi.dptr(nu), xp, 1, _ffi.dptr(data), _ffi.dptr(noise))
    assert rc == ERR_ARG and 'unknown model' in lib.nfa_last_error().decode()
    # the Python route: the prior program must cover four parameters; a cube runner wants its tables
    tab = engine.LineTable(1e11, [0.0], [1.0])
    s = engine.hyperfine.HyperfineSpectrum(x, np.zeros(64), 0.1, tab)
    with pytest.raises(engine.EngineError, match='prior program'):
        engine.HyperfineRunner([s], engine.get_irdc_priors(), ncomp=1)
    from nestfit_amd.cube import CubeRunner
    with pytest.raises(ValueError, match='LineTable'):
        CubeRunner([x], [1], data, noise, None, model=3)
    with pytest.raises(ValueError, match='LineTable'):
        CubeRunner([x], [1], data, noise, None, model=1, lines=[tab])


# ---------------------------------------------------------------------------- the cube route
def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube of one-component truths over two cubes with different tables: fit_cube, the store, the map products."""
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    _, three, forty = synthetic_tables(engine)
    rng = np.random.default_rng(31)
    n_side, n_chan, noise = 4, 256, 0.1
    truths = np.stack([rng.uniform(-2, 2, 16), rng.uniform(8, 12, 16), rng.uniform(0.0, 0.4, 16), rng.uniform(0.4, 0.9, 16)], axis=1)
    cubes = []
    for tab, vhalf in ((three, 20.0), (forty, 55.0)):
        x = _axis(tab, n_chan, vhalf)
        tbg = hfr.tbg_of(nfo, x)
        data = rng.normal(0, noise, (n_chan, n_side, n_side))
        for k, th in enumerate(truths):
            data[:, k // n_side, k % n_side] += hfr.hf_predict(nfo, x, tbg, hfr.table_of(tab), th)
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': tab.nu}
        cubes.append(DataCube(SimpleCube(hdr, data), noise, lines=tab))
    stack = CubeStack(cubes)
    ut = _simple_priors(engine, [(-4, 4), (3.0, 20), (-1.0, 1.0), (0.2, 1.5)])
    fitter = CubeFitter(stack, ut, engine.HyperfineRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 60, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'hyperfine' and store.read_model_lines() == [three, forty]
        groups = list(store.iter_pix_groups())
        assert len(groups) == 16 and all(g.attrs['nbest'] == 1 for g in groups)
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])              # (t, m, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                    # (m, p, b, l)
        specs = [np.asarray(store.hdf[f'{store.dpath}/model_spec/spec{k}']) for k in range(2)]     # (m, S, b, l)
        assert peak.shape == (2, 1, 4, 4) and np.isfinite(peak).all() and all(s.shape == (1, n_chan, 4, 4) for s in specs)
        predict = pp._device_predictor(store, stack)                               # table mode, like the products
        rows = [[dc.xarr, np.zeros(n_chan), 1.0, dc.lines] for dc in stack.cubes]
        worst = 0.0
        for l in range(4):
            for b in range(4):
                th = np.ascontiguousarray(pmap[0, :, b, l])
                assert abs(th[0] - truths[b * n_side + l, 0]) < 0.5                # (truth k sits at lat k // 4, lon k % 4)
                got, _, _ = predict(np.array([l]), np.array([b]), th[None, :], True)
                want, _ = _restated(nfo, rows, th)
                worst = max(worst, _check_spec(got[0], want, 'table'))
                for k, sl in enumerate((slice(0, n_chan), slice(n_chan, 2 * n_chan))):
                    assert np.array_equal(specs[k][0, :, b, l], got[0][sl].astype(np.float32))
                    assert peak[k, 0, b, l] == got[0][sl].max()
        assert worst < TIGHT['table']
    # a stack with another table is refused by the device predictor as well
    other = CubeStack([cubes[0], DataCube(SimpleCube(cubes[1].full_header, np.zeros((n_chan, 4, 4))), noise,
                                          lines=engine.LineTable(forty.nu, forty.voff, forty.tau_wts * 2))])
    with HdfStore(path) as store:
        with pytest.raises(ValueError, match='line tables differ'):
            pp._device_predictor(store, other)
