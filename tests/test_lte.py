"""The LTE model on the device (nestfit_amd/lte.py, nfa_specset_create_lte): column density, excitation temperature and a
partition function give every transition of a pixel its own optical depth.

The reference is tests/lte_restatement.py -- the header's formula with `math` in doubles, then the numpy restatement of
c_hf_predict (tests/hf_restatement.py, pinned to the oracle in tests/test_hyperfine_cpu.py) -- at the tolerances
tests/test_hyperfine.py holds the hyperfine model to: zero pattern exact, spectra TIGHT, lnL LNL_RTOL.  The species is a
rigid linear rotor made from closed forms (tests/test_lte_cpu.py: rotor_species)."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import hf_restatement as hfr
import lte_restatement as lr
from test_device_batches import _run_on_device
from test_hyperfine import _through_a_broker
from test_lte_cpu import B_ROT, MU, _trans, rotor_species
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _check_spec, _simple_priors

pytestmark = pytest.mark.gpu

N_CHAN, N_ROWS, NOISE = 160, 200, 0.2          # 200 rows: three whole set-up groups of 64 and one of 8
RANGES = [(-6, 6), (2.8, 60), (12.0, 14.0), (0.1, 1.5)]


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    engine.set_exp_mode('fast')


def wide_transition(mol):
    """3-2 with a made-up structure of 30 lines at distinct offsets over +-25 km/s: more than 26, the wide forms."""
    rng = np.random.default_rng(4321)
    voff = np.sort(rng.uniform(-25, 25, 30))
    assert np.unique(voff).size == 30
    rng.shuffle(voff)
    return mol.transition(*lr.rotor_transition(B_ROT, MU, 2), voff=voff, tau_wts=rng.uniform(0.01, 0.06, 30), name='3-2 wide',
                          normalise=True)


def _axis(t):
    return lr.axis(t.nu, N_CHAN, 45.0 if t.n > 26 else 20.0)


def _rows(tables, seed):
    rng = np.random.default_rng(seed)
    return [[_axis(t), rng.normal(0, NOISE, N_CHAN), NOISE, t] for t in tables]


def draw_params(rng, ncomp, mol, row):
    """tex below the table's first temperature, above its last, exactly on a node and in between, in turn by row and
    component; the other parameters over the ranges a fit would use."""
    tex = np.empty(ncomp)
    for c in range(ncomp):
        kind = (row + c) % 4
        tex[c] = (rng.uniform(2.8, mol.q_temp[0]) if kind == 0 else rng.uniform(mol.q_temp[-1], 1.5 * mol.q_temp[-1]) if kind == 1
                  else mol.q_temp[rng.integers(0, mol.n)] if kind == 2 else rng.uniform(mol.q_temp[0], mol.q_temp[-1]))
    return np.concatenate([rng.uniform(-6, 6, ncomp), tex, rng.uniform(12.0, 14.0, ncomp), 10 ** rng.uniform(-1.0, 0.2, ncomp)])


def _restated(nfo, rows, theta, tbgs=None):
    tbgs = tbgs or [hfr.tbg_of(nfo, x) for x, *_ in rows]
    preds = [lr.lte_predict(nfo, x, tbg, tab, theta) for (x, _, _, tab), tbg in zip(rows, tbgs)]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl


@functools.lru_cache(maxsize=None)
def _reference(n_spec, ncomp, n_q):
    """(rows, thetas, spectra, lnL) of the restatement, computed once for both modes."""
    import nestfit_amd as na
    from oracle import nfo
    mol, t10, t21, t32 = rotor_species(na, n_q=n_q)
    rows = _rows((t10, t21, t32)[:n_spec], seed=10 * n_spec + ncomp)
    rng = np.random.default_rng(1000 + 10 * n_spec + ncomp + n_q)
    thetas = np.stack([draw_params(rng, ncomp, mol, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    want = [_restated(nfo, rows, th, tbgs) for th in thetas]
    spec, lnl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    spec.setflags(write=False), lnl.setflags(write=False), thetas.setflags(write=False)
    return rows, thetas, spec, lnl


def _against_the_reference(engine, mode, n_spec, ncomp, n_q):
    engine.set_exp_mode(mode)
    rows, thetas, want_spec, want_lnl = _reference(n_spec, ncomp, n_q)
    mol = rows[0][3].molecule
    tex = thetas[:, ncomp:2 * ncomp]
    assert (tex < mol.q_temp[0]).any() and (tex > mol.q_temp[-1]).any() and np.isin(tex, mol.q_temp).any()
    run = engine.LteRunner.from_data(rows, None, ncomp=ncomp)
    assert (run.ndim, run.n_params, run.n_spec, run.n_chan_tot, run.n_model) == (4 * ncomp, 4 * ncomp, n_spec, n_spec * N_CHAN, 4)
    assert run.null_lnZ == pytest.approx(sum(-np.sum(d ** 2) / (2 * s ** 2) for _, d, s, _ in rows), rel=1e-13)
    spec, lnl = run.predict_batch(np.array(thetas))
    worst, worst_lnl = 0.0, 0.0
    for sp, ll, ws, wl in zip(spec, lnl, want_spec, want_lnl):
        worst = max(worst, _check_spec(sp, ws, mode))
        worst_lnl = max(worst_lnl, abs(ll - wl) / abs(wl))
    print(f'lte {mode} n_spec={n_spec} ncomp={ncomp} n_q={n_q}: worst relative Tb error {worst:.2e}, lnL {worst_lnl:.2e}')
    assert worst < TIGHT[mode]
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    # ... and per spectrum through lte_predict
    run.predict(np.array(thetas[1]))
    got = np.concatenate([s.get_spec() for s in run.spectra])
    assert _check_spec(got, want_spec[1], mode) < TIGHT[mode]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
@pytest.mark.parametrize('n_spec', [1, 2, 3])
def test_spectra_and_lnl_against_the_restatement(engine, n_spec, ncomp, mode, mode_guard):
    _against_the_reference(engine, mode, n_spec, ncomp, 32)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n_q', [2, 64])
def test_the_smallest_and_the_largest_partition_table(engine, n_q, mode, mode_guard):
    _against_the_reference(engine, mode, 2, 2, n_q)


@pytest.mark.parametrize('mode', MODES)
def test_one_spectrum_against_the_hyperfine_runner(engine, nfo, mode, mode_guard):
    """The hyperfine model fed ltau = log10(tau_main) of the restatement runs the same kernels on the same lines."""
    engine.set_exp_mode(mode)
    mol, t10, _, _ = rotor_species(engine)
    rng = np.random.default_rng(61)
    worst = 0.0
    for ncomp in (1, 3):
        rows = _rows((t10,), seed=5)
        plain = [[rows[0][0], rows[0][1], NOISE, engine.LineTable(t10.nu, t10.voff, t10.tau_wts)]]
        lte = engine.LteRunner.from_data(rows, None, ncomp=ncomp)
        hyp = engine.HyperfineRunner.from_data(plain, None, ncomp=ncomp)
        thetas = np.stack([draw_params(rng, ncomp, mol, k) for k in range(64)])
        as_ltau = np.stack([lr.ltau_params(_trans(t10), mol.q_temp, mol.q_val, th) for th in thetas])
        got, lnl = lte.predict_batch(thetas)
        want, want_lnl = hyp.predict_batch(as_ltau)
        for g, w in zip(got, want):
            worst = max(worst, _check_spec(g, w, mode))
        np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    assert worst < TIGHT[mode]


# ---------------------------------------------------------------------------- the same bits on every route
def _routes(engine, run, rng, n_rows=513, point=True):
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
    for k in (0, 7, 150):                                   # single points (narrow sets: the point kernel)
        u = U[k].copy()
        assert run.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k])
    few = U[20:31].copy()                                   # a broker's handful
    assert np.array_equal(run.loglikelihood_batch(few), lnl[20:31]) and np.array_equal(few, theta[20:31])
    return U, theta, lnl


@pytest.mark.parametrize('mode', MODES)
def test_the_same_bits_on_every_route(engine, nfo, mode, mode_guard):
    engine.set_exp_mode(mode)
    mol, t10, t21, _ = rotor_species(engine)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((t10, t21), seed=3)
    run = engine.LteRunner.from_data(rows, ut, ncomp=2)
    U, theta, lnl = _routes(engine, run, rng)
    lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
    assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
    # predict_batch: whatever the batch, and lte_predict per spectrum
    spec, pl = run.predict_batch(theta[:40])
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]
    np.testing.assert_allclose(pl, lnl[:40], rtol=LNL_RTOL[mode])
    run.predict(theta[3])
    assert np.array_equal(np.concatenate([s.get_spec() for s in run.spectra]), spec[3])
    assert _check_spec(spec[3], _restated(nfo, rows, theta[3])[0], mode) < TIGHT[mode]
    # a noise per channel, with masked channels
    chan = [rng.uniform(0.1, 0.3, N_CHAN) for _ in rows]
    for s in chan:
        s[rng.integers(0, N_CHAN, 5)] = np.inf
    rows_c = [[x, d, s, t] for (x, d, _, t), s in zip(rows, chan)]
    run_c = engine.LteRunner.from_data(rows_c, ut, ncomp=2)
    _, theta_c, lnl_c = _routes(engine, run_c, rng, n_rows=256)
    for k in (0, 100, 255):
        pred = _restated(nfo, rows, theta_c[k])[0]
        want = sum(-np.sum(((d - pred[i * N_CHAN:(i + 1) * N_CHAN]) / s)[np.isfinite(s)] ** 2) / 2 for i, (_, d, s, _) in enumerate(rows_c))
        assert lnl_c[k] == pytest.approx(want, rel=LNL_RTOL[mode])
    # a baseline of order 1: the same bits on every route, and never a worse fit than without one
    run_b = engine.LteRunner.from_data(rows, ut, ncomp=2, baseline_order=1)
    Ub, _, lnl_b = _routes(engine, run_b, rng, n_rows=256)
    plain = run.loglikelihood_batch(Ub.copy())
    assert (lnl_b >= plain - 1e-9 * np.abs(plain)).all() and (lnl_b > plain).any()
    # the 30-line table: the wide forms, whose single points take the batch path
    wide = wide_transition(mol)
    rows_w = _rows((t10, wide), seed=4)
    run_w = engine.LteRunner.from_data(rows_w, ut, ncomp=2)
    _, theta_w, lnl_w = _routes(engine, run_w, rng, n_rows=256)
    for k in (0, 100, 255):
        assert lnl_w[k] == pytest.approx(_restated(nfo, rows_w, theta_w[k])[1], rel=LNL_RTOL[mode])
    spec_w, _ = run_w.predict_batch(theta_w[:8])
    assert max(_check_spec(sp, _restated(nfo, rows_w, th)[0], mode) for sp, th in zip(spec_w, theta_w[:8])) < TIGHT[mode]


@pytest.mark.parametrize('mode', MODES)
def test_unit_cube_in_lnl_out(engine, nfo, mode, mode_guard):
    """A PriorTransformer over the four parameters: theta against the priors' host transform, lnL against the
    restatement at the engine's theta."""
    engine.set_exp_mode(mode)
    _, t10, t21, t32 = rotor_species(engine)
    rng = np.random.default_rng(78)
    ut = _simple_priors(engine, RANGES)
    ps = nfo.PriorSet(ut.lower())
    rows = _rows((t10, t21, t32), seed=6)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    for ncomp in (1, 2):
        run = engine.LteRunner.from_data(rows, ut, ncomp=ncomp)
        U = rng.uniform(size=(N_ROWS, 4 * ncomp))
        theta = U.copy()
        lnl = run.loglikelihood_batch(theta)
        for k in range(0, N_ROWS, 5):
            want_theta = U[k].copy()
            ps.transform(want_theta, ncomp)
            np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
            assert lnl[k] == pytest.approx(_restated(nfo, rows, theta[k], tbgs)[1], rel=LNL_RTOL[mode])


@pytest.mark.parametrize('mode', MODES)
def test_the_resident_kernel_serves_a_narrow_lte_runner(engine, mode, mode_guard):
    """nfa_ring_serve_device on an LTE runner: one call serves a client's points with the batch path's bits."""
    import os
    from nestfit_amd.ring import RingClient, RingServer
    engine.set_exp_mode(mode)
    _, t10, t21, _ = rotor_species(engine)
    run = engine.LteRunner.from_data(_rows((t10, t21), seed=8), _simple_priors(engine, RANGES), ncomp=2)
    U = np.random.default_rng(12).uniform(size=(24, run.ndim))
    want_theta = U.copy()
    want = run.loglikelihood_batch(want_theta)
    name = f'nfa_test_ring_lte_{os.getpid()}_{mode}'
    errors = []
    with RingServer(name, n_slots=1, runner=run) as server:
        def serve():
            try:
                server.serve_device(lifetime_ms=20, idle_ms=10000)
            except Exception as e:                                    # pragma: no cover
                errors.append(e)
        th = threading.Thread(target=serve)
        th.start()
        client = RingClient(name, wait_ms=10000)
        theta = U.copy()
        lnl = np.array([client.loglikelihood(row) for row in theta])
        client.close()
        server.stop()
        th.join(timeout=30)
        assert not th.is_alive() and not errors
        assert server.stats['evals'] == 24
    assert np.array_equal(lnl, want) and np.array_equal(theta, want_theta)


# ---------------------------------------------------------------------------- what the C ABI refuses
def _create_lte(lib, n_lines=(1,), nus=(1e11,), voff=(0.0,), wts=(1.0,), e_up=(4.0,), g_up=(3.0,), a_ul=(1e-5,),
                q_temp=(5.0, 10.0, 20.0), q_val=(2.0, 4.0, 9.0), n_q=None, noise='scalar', n=64):
    from nestfit_amd import _ffi
    n_spec = len(n_lines)
    xs = [np.linspace(1e11, 1.0001e11, n) for _ in range(n_spec)]
    xp = (_ffi._dp * n_spec)(*[_ffi.dptr(x) for x in xs])
    sizes = np.full(n_spec, n, dtype=np.int64)
    n_lines = np.asarray(n_lines, dtype=np.int32)
    nus, voff, wts, e_up, g_up, a_ul, q_temp, q_val = (np.ascontiguousarray(a, dtype=np.float64)
                                                       for a in (nus, voff, wts, e_up, g_up, a_ul, q_temp, q_val))
    data = np.zeros((1, n * n_spec))
    sc, ch = np.full((1, n_spec), 0.1), np.full((1, n * n_spec), 0.1)
    h = C.c_void_p()
    rc = lib.nfa_specset_create_lte(C.byref(h), n_spec, sizes.ctypes.data_as(_ffi._lp), n_lines.ctypes.data_as(_ffi._ip),
                                    _ffi.dptr(nus), _ffi.dptr(voff), _ffi.dptr(wts), _ffi.dptr(e_up), _ffi.dptr(g_up), _ffi.dptr(a_ul),
                                    q_temp.size if n_q is None else n_q, _ffi.dptr(q_temp), _ffi.dptr(q_val), xp, 1, _ffi.dptr(data),
                                    _ffi.dptr(sc) if noise in ('scalar', 'both') else None,
                                    _ffi.dptr(ch) if noise in ('channel', 'both') else None)
    msg = lib.nfa_last_error().decode()
    if rc == 0:
        lib.nfa_specset_destroy(h)
    return rc, msg


def test_the_engine_refuses_invalid_arguments_with_a_message(engine):
    from nestfit_amd import _ffi
    lib = _ffi.engine()
    ERR_ARG = 1
    assert _create_lte(lib)[0] == 0 and _create_lte(lib, noise='channel')[0] == 0
    assert _create_lte(lib, e_up=(0.0,))[0] == 0                                       # the ground state's own energy
    assert _create_lte(lib, q_temp=(5.0, 10.0), q_val=(2.0, 4.0))[0] == 0
    assert _create_lte(lib, q_temp=np.linspace(1, 64, 64), q_val=np.linspace(1, 64, 64))[0] == 0
    assert _create_lte(lib, n_lines=(2,), voff=(0.0, 1.0), wts=(0.5, 0.5 + 5e-7))[0] == 0
    two = dict(n_lines=(1, 2), nus=(1e11, 1e11), voff=(0.0, 0.0, 1.0), wts=(1.0, 0.5, 0.5), e_up=(4.0, 9.0), g_up=(3.0, 5.0),
               a_ul=(1e-5, 2e-5))
    assert _create_lte(lib, **two)[0] == 0
    bad = [
        (dict(e_up=(-0.1,)), 'energy'), (dict(e_up=(np.nan,)), 'energy'), (dict(e_up=(np.inf,)), 'energy'),
        (dict(g_up=(0.0,)), 'weight'), (dict(g_up=(-1.0,)), 'weight'), (dict(g_up=(np.nan,)), 'weight'), (dict(g_up=(np.inf,)), 'weight'),
        (dict(a_ul=(0.0,)), 'Einstein'), (dict(a_ul=(-1e-5,)), 'Einstein'), (dict(a_ul=(np.nan,)), 'Einstein'),
        (dict(a_ul=(np.inf,)), 'Einstein'),
        (dict(n_lines=(2,), voff=(0.0, 1.0), wts=(0.5, 0.4)), 'sum to 1'),
        (dict(n_lines=(2,), voff=(0.0, 1.0), wts=(0.5, 0.5 + 3e-6)), 'sum to 1'),
        (dict(wts=(2.0,)), 'sum to 1'),
        ({**two, 'wts': (1.0, 0.5, 0.6)}, 'spectrum 1'), ({**two, 'e_up': (4.0, -9.0)}, 'spectrum 1'),
        (dict(n_q=1), '2..64'), (dict(n_q=65, q_temp=np.linspace(1, 65, 65), q_val=np.linspace(1, 65, 65)), '2..64'), (dict(n_q=0), '2..64'),
        (dict(q_temp=(5.0, 5.0, 20.0)), 'ascending'), (dict(q_temp=(5.0, 30.0, 20.0)), 'ascending'), (dict(q_temp=(0.0, 10.0, 20.0)), 'ascending'),
        (dict(q_temp=(-5.0, 10.0, 20.0)), 'ascending'), (dict(q_temp=(5.0, np.nan, 20.0)), 'ascending'), (dict(q_temp=(5.0, 10.0, np.inf)), 'ascending'),
        (dict(q_val=(2.0, 0.0, 9.0)), 'partition function'), (dict(q_val=(2.0, -4.0, 9.0)), 'partition function'),
        (dict(q_val=(np.nan, 4.0, 9.0)), 'partition function'), (dict(q_val=(2.0, 4.0, np.inf)), 'partition function'),
        # every check of nfa_specset_create_lines
        (dict(n_lines=(0,)), 'lines'), (dict(nus=(0.0,)), 'rest frequency'), (dict(voff=(np.nan,)), 'velocity offset'),
        (dict(wts=(-1.0,)), 'weight'), (dict(n_lines=(2,), voff=(0.0, 1.0), wts=(0.0, 0.0)), 'all zero'),
        (dict(noise='none'), 'exactly one'), (dict(noise='both'), 'exactly one'),
    ]
    for kw, word in bad:
        rc, msg = _create_lte(lib, **kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)
    # the other creators refuse model 4, as they refuse model 3: it needs its tables
    x = np.linspace(1e11, 1.0001e11, 64)
    xp = (_ffi._dp * 1)(_ffi.dptr(x))
    sizes, trans = np.array([64], dtype=np.int64), np.array([1], dtype=np.int32)
    data, noise, nu = np.zeros((1, 64)), np.full((1, 1), 0.1), np.array([1e11])
    h = C.c_void_p()
    for create, sig in ((lib.nfa_specset_create_model, noise), (lib.nfa_specset_create_channel_noise, np.full((1, 64), 0.1))):
        rc = create(C.byref(h), 4, 1, sizes.ctypes.data_as(_ffi._lp), trans.ctypes.data_as(_ffi._ip), _ffi.dptr(nu), xp, 1,
                    _ffi.dptr(data), _ffi.dptr(sig))
        assert rc == ERR_ARG and 'nfa_specset_create_lte' in lib.nfa_last_error().decode()
    rc = lib.nfa_specset_create_model(C.byref(h), 5, 1, sizes.ctypes.data_as(_ffi._lp), trans.ctypes.data_as(_ffi._ip),
                                      _ffi.dptr(nu), xp, 1, _ffi.dptr(data), _ffi.dptr(noise))
    assert rc == ERR_ARG and 'unknown model' in lib.nfa_last_error().decode()
    # the Python route: the prior program must cover four parameters; a cube runner wants its tables
    mol, t10, _, _ = rotor_species(engine)
    s = engine.LteSpectrum(_axis(t10), np.zeros(N_CHAN), 0.1, t10)
    with pytest.raises(engine.EngineError, match='prior program'):
        engine.LteRunner([s], engine.get_irdc_priors(), ncomp=1)
    from nestfit_amd.cube import CubeRunner
    with pytest.raises(ValueError, match='LineTable'):
        CubeRunner([x], [1], data, noise, None, model=4)
    with pytest.raises(ValueError, match='LteLines'):
        CubeRunner([x], [1], data, noise, None, model=4, lines=[engine.LineTable(1e11, [0.0], [1.0])])


# ---------------------------------------------------------------------------- sampling
B_FIT, MU_FIT = 150e9, 2e-18            # 1-0 at 300 GHz: at 5 K the 2-1 line is thin where 1-0 is thick
TRUTH_FIT = np.array([0.3, 5.0, 13.1, 0.5])
FIT_RANGES = [(-3, 3), (3.0, 12.0), (12.0, 14.5), (0.2, 1.2)]


def _fit_species(engine):
    mol, t10, t21, _ = rotor_species(engine, B=B_FIT, mu=MU_FIT, t_lo=3.0, t_hi=30.0, name='fit rotor')
    return mol, t10, t21


def test_run_multinest_recovers_column_density_and_tex(engine, nfo, mode_guard):
    """One component over 1-0 (optically thick: tex) and 2-1 (thin: the column density), 128 channels each."""
    from nestfit_amd import sampler
    mol, t10, t21 = _fit_species(engine)
    tau = [float(t.tau_main(*TRUTH_FIT[1:])) for t in (t10, t21)]
    assert tau[0] > 3.0 and tau[1] < 0.6
    rng = np.random.default_rng(17)
    noise = 0.01
    rows = []
    for t in (t10, t21):
        x = lr.axis(t.nu, 128, 16.0)
        rows.append([x, lr.lte_predict(nfo, x, hfr.tbg_of(nfo, x), t, TRUTH_FIT) + rng.normal(0, noise, 128), noise, t])
    run = engine.LteRunner.from_data(rows, _simple_priors(engine, FIT_RANGES), ncomp=1)
    res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=5)
    mean, std = res.param_constr[0], res.param_constr[1]
    print(f'lnZ - null_lnZ = {res.lnZ - run.null_lnZ:.1f}; mean {mean}, std {std}, truth {TRUTH_FIT}; tau {tau}')
    assert res.lnZ - run.null_lnZ > 11                              # the fitter's default lnZ_thresh
    for k in (1, 2):
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])
    assert std[1] < 1.0 and std[2] < 0.3                            # both are constrained, not the priors' widths


def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube over the two transitions: fit_cube, the store with its tables, the map products."""
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    mol, t10, t21 = _fit_species(engine)
    rng = np.random.default_rng(31)
    n_side, n_chan, noise = 4, 128, 0.02
    truths = np.stack([rng.uniform(-1, 1, 16), rng.uniform(4.5, 6.0, 16), rng.uniform(13.0, 13.3, 16), rng.uniform(0.4, 0.7, 16)], axis=1)

    def cubes_of(tables):
        out = []
        for tab in tables:
            x = lr.axis(tab.nu, n_chan, 16.0)
            tbg = hfr.tbg_of(nfo, x)
            data = np.random.default_rng(int(tab.g_up)).normal(0, noise, (n_chan, n_side, n_side))
            for k, th in enumerate(truths):
                data[:, k // n_side, k % n_side] += lr.lte_predict(nfo, x, tbg, tab, th)
            hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': n_chan,
                   'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
                   'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': tab.nu}
            out.append(DataCube(SimpleCube(hdr, data), noise, lines=tab))
        return out
    stack = CubeStack(cubes_of((t10, t21)))
    fitter = CubeFitter(stack, _simple_priors(engine, FIT_RANGES), engine.LteRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 60, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (4, 4, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'lte' and store.read_model_lines() == [t10, t21]
        part = store.hdf['/model_partition']
        assert part.attrs['name'] == mol.name and np.array_equal(np.asarray(part['temp'][...]), mol.q_temp)
        assert np.array_equal(np.asarray(part['q'][...]), mol.q_val)
        for k, t in enumerate((t10, t21)):
            attrs = store.hdf[f'/model_lines/spec{k}'].attrs
            assert (attrs['e_up'], attrs['g_up'], attrs['a_ul'], attrs['nu']) == (t.e_up, t.g_up, t.a_ul, t.nu)
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
                truth = truths[b * n_side + l]                                     # (truth k sits at lat k // 4, lon k % 4)
                assert abs(th[0] - truth[0]) < 0.3 and abs(th[1] - truth[1]) < 1.5 and abs(th[2] - truth[2]) < 0.5
                got, _, _ = predict(np.array([l]), np.array([b]), th[None, :], True)
                worst = max(worst, _check_spec(got[0], _restated(nfo, rows, th)[0], 'table'))
                for k, sl in enumerate((slice(0, n_chan), slice(n_chan, 2 * n_chan))):
                    assert np.array_equal(specs[k][0, :, b, l], got[0][sl].astype(np.float32))
                    assert peak[k, 0, b, l] == got[0][sl].max()
        assert worst < TIGHT['table']
    # a stack with a different e_up, or another partition table, is refused: by the check and by the device predictor
    nu, e, g, a = _trans(t21)
    hotter = mol.transition(nu, e * 1.01, g, a, name='2-1')
    mol2, u10, u21, _ = rotor_species(engine, B=B_FIT, mu=MU_FIT, t_lo=3.0, t_hi=31.0, name='fit rotor')
    with HdfStore(path) as store:
        for tables in ((t10, hotter), (u10, u21)):
            other = CubeStack(cubes_of(tables))
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp._device_predictor(store, other)
