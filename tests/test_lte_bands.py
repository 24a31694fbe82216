"""LTE bands on the device (nfa_specset_create_lte_bands): several transitions of the species inside one
spectrum, every line at the optical depth of its own transition.

The reference is tests/band_restatement.py -- tau_main per transition from tests/lte_restatement.py, then the loop of
c_hf_predict's restatement over all the lines -- at the tolerances the hyperfine and the LTE model are held to
(tests/test_lte.py): zero pattern exact, spectra TIGHT, lnL LNL_RTOL.  The species is the symmetric top of
tests/test_lte_bands_cpu.py: K = 0..3 on 300 channels, K = 0 and 1 blended at the larger widths drawn, K = 0 with three
lines of which one lies beyond K = 1."""
import ctypes as C
import functools
import os
import threading

import numpy as np
import pytest

import band_restatement as br
import hf_restatement as hfr
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands_cpu import K0_VOFF, K0_WTS, N_CHAN, _trans, band_axis, top_species
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _check_spec, _simple_priors

pytestmark = pytest.mark.gpu

N_ROWS, NOISE = 200, 0.2                       # 200 rows: three whole set-up groups of 64 and one of 8
RANGES = [(-6, 6), (2.8, 90), (13.0, 15.5), (0.1, 1.5)]
COLD = (0.03, 0.055)                           # tex at which exp(-E_u / tex) of K >= 2 underflows and K = 0, 1 do not


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _rows(tables, seed):
    rng = np.random.default_rng(seed)
    return [[band_axis(t.nu), rng.normal(0, NOISE, N_CHAN), NOISE, t] for t in tables]


def draw_params(rng, ncomp, mol, row):
    """tex below the table's first temperature, above its last, exactly on a node, in between, and so cold that the
    upper transitions of the band underflow, in turn by row and component; sigm over 0.1..1.58 km/s (K = 0 and 1, 2.5 km/s
    apart, blend above 1.25)."""
    tex = np.empty(ncomp)
    for c in range(ncomp):
        kind = (row + c) % 5
        tex[c] = (rng.uniform(2.8, mol.q_temp[0]) if kind == 0 else rng.uniform(mol.q_temp[-1], 1.5 * mol.q_temp[-1]) if kind == 1
                  else mol.q_temp[rng.integers(0, mol.n)] if kind == 2 else rng.uniform(mol.q_temp[0], mol.q_temp[-1]) if kind == 3
                  else rng.uniform(*COLD))
    return np.concatenate([rng.uniform(-6, 6, ncomp), tex, rng.uniform(13.0, 15.5, ncomp), 10 ** rng.uniform(-1.0, 0.2, ncomp)])


def _tables(engine, n_spec):
    """A band alone, or a band and an ordinary spectrum of one transition."""
    mol, ks = top_species(engine)
    return mol, ks, (mol.band(ks), ks[2])[:n_spec]


@functools.lru_cache(maxsize=None)
def _reference(n_spec, ncomp):
    """(rows, thetas, spectra, lnL) of the restatement, computed once for both modes."""
    import nestfit_amd as na
    from oracle import nfo
    mol, ks, tables = _tables(na, n_spec)
    rows = _rows(tables, seed=10 * n_spec + ncomp)
    rng = np.random.default_rng(2000 + 10 * n_spec + ncomp)
    thetas = np.stack([draw_params(rng, ncomp, mol, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    want = [br.restated(nfo, rows, th, tbgs) for th in thetas]
    spec, lnl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    spec.setflags(write=False), lnl.setflags(write=False), thetas.setflags(write=False)
    return rows, thetas, spec, lnl


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
@pytest.mark.parametrize('n_spec', [1, 2])
def test_spectra_and_lnl_against_the_restatement(engine, n_spec, ncomp, mode, mode_guard):
    engine.set_exp_mode(mode)
    rows, thetas, want_spec, want_lnl = _reference(n_spec, ncomp)
    mol, ks = top_species(engine)
    tex, sigm = thetas[:, ncomp:2 * ncomp], thetas[:, 3 * ncomp:]
    assert (tex < mol.q_temp[0]).any() and (tex > mol.q_temp[-1]).any() and np.isin(tex, mol.q_temp).any()
    cold = tex < COLD[1]
    assert cold.any() and all(float(ks[2].tau_main(t, 15.5, 0.1)) == 0.0 < float(ks[1].tau_main(t, 13.0, 1.6)) for t in tex[cold])
    assert (2 * sigm > (1 - ks[1].nu / ks[0].nu) * br.CKMS).any()                 # K = 0 and 1 closer than two widths: blended
    run = engine.LteRunner.from_data(rows, None, ncomp=ncomp)
    assert (run.ndim, run.n_params, run.n_spec, run.n_chan_tot, run.n_model) == (4 * ncomp, 4 * ncomp, n_spec, n_spec * N_CHAN, 4)
    spec, lnl = run.predict_batch(np.array(thetas))
    worst, worst_lnl = 0.0, 0.0
    for sp, ll, ws, wl in zip(spec, lnl, want_spec, want_lnl):
        worst = max(worst, _check_spec(sp, ws, mode))
        worst_lnl = max(worst_lnl, abs(ll - wl) / abs(wl))
    print(f'bands {mode} n_spec={n_spec} ncomp={ncomp}: worst relative Tb error {worst:.2e}, lnL {worst_lnl:.2e}')
    assert worst < TIGHT[mode]
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    assert np.abs(want_spec).max() > 1.0                                          # (lines that matter beside the noise)
    # ... and per spectrum through lte_predict
    run.predict(np.array(thetas[1]))
    got = np.concatenate([s.get_spec() for s in run.spectra])
    assert _check_spec(got, want_spec[1], mode) < TIGHT[mode]


def wide_band(mol, ks):
    """K = 0 with a made-up structure of 27 lines, and K = 1..3: 30 lines, more than 26 -- the wide forms."""
    rng = np.random.default_rng(4321)
    voff = np.sort(rng.uniform(-8, 8, 27))
    assert np.unique(voff).size == 27
    rng.shuffle(voff)
    k0 = mol.transition(*_trans(ks[0]), voff=voff, tau_wts=rng.uniform(0.01, 0.06, 27), name='K=0 wide', normalise=True)
    return mol.band([k0] + ks[1:])


@pytest.mark.parametrize('mode', MODES)
def test_a_band_of_thirty_lines(engine, nfo, mode, mode_guard):
    engine.set_exp_mode(mode)
    mol, ks = top_species(engine)
    band = wide_band(mol, ks)
    assert band.n_lines == 30
    rows = _rows((band, ks[1]), seed=4)
    ut = _simple_priors(engine, RANGES)
    run = engine.LteRunner.from_data(rows, ut, ncomp=2)
    _, theta, lnl = _routes(engine, run, np.random.default_rng(5), n_rows=256)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    for k in (0, 100, 255):
        assert lnl[k] == pytest.approx(br.restated(nfo, rows, theta[k], tbgs)[1], rel=LNL_RTOL[mode])
    spec, _ = run.predict_batch(theta[:12])
    assert max(_check_spec(sp, br.restated(nfo, rows, th, tbgs)[0], mode) for sp, th in zip(spec, theta[:12])) < TIGHT[mode]


def _served_by_the_ring(run, U, name):
    """theta and lnL of the rows of U through nfa_ring_serve_device, one client."""
    from nestfit_amd.ring import RingClient, RingServer
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
        assert server.stats['evals'] == len(U)
    return theta, lnl


@pytest.mark.parametrize('mode', MODES)
def test_a_band_of_one_transition_is_the_lte_model(engine, mode, mode_guard):
    """The bits of LteRunner on the same LteLines, and its routes: the resident ring still serves it."""
    engine.set_exp_mode(mode)
    mol, ks = top_species(engine)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((ks[0], ks[3]), seed=8)
    as_bands = [[x, d, s, mol.band([t])] for x, d, s, t in rows]
    plain = engine.LteRunner.from_data(rows, ut, ncomp=2)
    banded = engine.LteRunner.from_data(as_bands, ut, ncomp=2)
    rng = np.random.default_rng(12)
    U = rng.uniform(size=(200, plain.ndim))
    want_theta = U.copy()
    want = plain.loglikelihood_batch(want_theta)
    theta = U.copy()
    assert np.array_equal(banded.loglikelihood_batch(theta), want) and np.array_equal(theta, want_theta)
    spec_p, lnl_p = plain.predict_batch(want_theta[:50])
    spec_b, lnl_b = banded.predict_batch(want_theta[:50])
    assert np.array_equal(spec_b, spec_p) and np.array_equal(lnl_b, lnl_p)
    got_theta, got = _served_by_the_ring(banded, U[:24], f'nfa_test_ring_band1_{os.getpid()}_{mode}')
    assert np.array_equal(got, want[:24]) and np.array_equal(got_theta, want_theta[:24])


@pytest.mark.parametrize('mode', MODES)
def test_the_order_of_the_transitions_does_not_matter(engine, mode, mode_guard):
    engine.set_exp_mode(mode)
    mol, ks = top_species(engine)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((mol.band(ks), ks[2]), seed=9)
    U = np.random.default_rng(13).uniform(size=(200, 8))
    want_theta = U.copy()
    run = engine.LteRunner.from_data(rows, ut, ncomp=2)
    want = run.loglikelihood_batch(want_theta)
    want_spec, _ = run.predict_batch(want_theta[:40])
    assert np.isfinite(want).all()
    for order in ((3, 2, 1, 0), (2, 0, 3, 1), (1, 3, 0, 2)):                   # the reference transition, K = 0, not first
        other = [[rows[0][0], rows[0][1], NOISE, mol.band([ks[k] for k in order])], rows[1]]
        run_o = engine.LteRunner.from_data(other, ut, ncomp=2)
        theta = U.copy()
        assert np.array_equal(run_o.loglikelihood_batch(theta), want) and np.array_equal(theta, want_theta), order
        assert np.array_equal(run_o.predict_batch(want_theta[:40])[0], want_spec), order


@pytest.mark.parametrize('mode', MODES)
def test_the_same_bits_on_every_route(engine, nfo, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    mol, ks = top_species(engine)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((mol.band(ks), ks[2]), seed=3)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    run = engine.LteRunner.from_data(rows, ut, ncomp=2)
    # host and device batches, coalescing on and off, single points and a handful: these take the batch path
    U, theta, lnl = _routes(engine, run, rng)
    for split in (4, 1):                                                        # ... whatever the row split of a small launch
        _ffi.set_option('lnl_split', split)
        run_s = engine.LteRunner.from_data(rows, ut, ncomp=2)                   # (a runner reads the option when it is made)
        for k in (0, 7, 150):
            u = U[k].copy()
            assert run_s.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k]), split
        few = U[20:31].copy()
        assert np.array_equal(run_s.loglikelihood_batch(few), lnl[20:31]), split
    _ffi.set_option('lnl_split', 0)
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
    assert _check_spec(spec[3], br.restated(nfo, rows, theta[3], tbgs)[0], mode) < TIGHT[mode]
    # a noise per channel, with masked channels
    chan = [rng.uniform(0.1, 0.3, N_CHAN) for _ in rows]
    for s in chan:
        s[rng.integers(0, N_CHAN, 5)] = np.inf
    rows_c = [[x, d, s, t] for (x, d, _, t), s in zip(rows, chan)]
    run_c = engine.LteRunner.from_data(rows_c, ut, ncomp=2)
    _, theta_c, lnl_c = _routes(engine, run_c, rng, n_rows=256)
    for k in (0, 100, 255):
        pred = br.restated(nfo, rows, theta_c[k], tbgs)[0]
        want = sum(-np.sum(((d - pred[i * N_CHAN:(i + 1) * N_CHAN]) / s)[np.isfinite(s)] ** 2) / 2 for i, (_, d, s, _) in enumerate(rows_c))
        assert lnl_c[k] == pytest.approx(want, rel=LNL_RTOL[mode])
    # a baseline of order 1: the same bits on every route, and never a worse fit than without one
    run_b = engine.LteRunner.from_data(rows, ut, ncomp=2, baseline_order=1)
    Ub, _, lnl_b = _routes(engine, run_b, rng, n_rows=256)
    plain = run.loglikelihood_batch(Ub.copy())
    assert (lnl_b >= plain - 1e-9 * np.abs(plain)).all() and (lnl_b > plain).any()


@pytest.mark.parametrize('mode', MODES)
def test_unit_cube_in_lnl_out(engine, nfo, mode, mode_guard):
    """A PriorTransformer over the four parameters: theta against the priors' host transform, lnL against the
    restatement at the engine's theta."""
    engine.set_exp_mode(mode)
    mol, ks = top_species(engine)
    rng = np.random.default_rng(78)
    ut = _simple_priors(engine, RANGES)
    ps = nfo.PriorSet(ut.lower())
    rows = _rows((mol.band(ks), ks[1]), seed=6)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    for ncomp in (1, 2):
        run = engine.LteRunner.from_data(rows, ut, ncomp=ncomp)
        U = rng.uniform(size=(N_ROWS, 4 * ncomp))
        theta = U.copy()
        lnl = run.loglikelihood_batch(theta)
        for k in range(0, N_ROWS, 8):
            want_theta = U[k].copy()
            ps.transform(want_theta, ncomp)
            np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
            assert lnl[k] == pytest.approx(br.restated(nfo, rows, theta[k], tbgs)[1], rel=LNL_RTOL[mode])


# ---------------------------------------------------------------------------- refusals
def test_the_resident_kernel_refuses_a_banded_runner(engine, mode_guard):
    from nestfit_amd.ring import RingServer
    mol, ks = top_species(engine)
    run = engine.LteRunner.from_data(_rows((mol.band(ks),), seed=2), _simple_priors(engine, RANGES), ncomp=1)
    with RingServer(f'nfa_test_ring_band_{os.getpid()}', n_slots=1, runner=run) as server:
        with pytest.raises(engine.EngineError, match='no form for LTE bands: use nfa_ring_serve'):
            server.serve_device(lifetime_ms=20, idle_ms=100)
    u = np.full(4, 0.5)                                               # ... and a single point takes the batch path
    assert np.isfinite(run.loglikelihood(u))


def _create_bands(lib, n_trans=(2,), n_lines=(1, 1), nus=(1e11, 1.00001e11), voff=(0.0, 0.0), wts=(1.0, 1.0), e_up=(4.0, 9.0),
                  g_up=(3.0, 5.0), a_ul=(1e-5, 2e-5), q_temp=(5.0, 10.0, 20.0), q_val=(2.0, 4.0, 9.0), noise='scalar', n=64):
    from nestfit_amd import _ffi
    n_spec = len(n_trans)
    xs = [np.linspace(1e11, 1.0001e11, n) for _ in range(n_spec)]
    xp = (_ffi._dp * n_spec)(*[_ffi.dptr(x) for x in xs])
    sizes = np.full(n_spec, n, dtype=np.int64)
    n_trans, n_lines = np.asarray(n_trans, dtype=np.int32), np.asarray(n_lines, dtype=np.int32)
    nus, voff, wts, e_up, g_up, a_ul, q_temp, q_val = (np.ascontiguousarray(a, dtype=np.float64)
                                                       for a in (nus, voff, wts, e_up, g_up, a_ul, q_temp, q_val))
    data = np.zeros((1, n * n_spec))
    sc, ch = np.full((1, n_spec), 0.1), np.full((1, n * n_spec), 0.1)
    h = C.c_void_p()
    rc = lib.nfa_specset_create_lte_bands(C.byref(h), n_spec, sizes.ctypes.data_as(_ffi._lp), n_trans.ctypes.data_as(_ffi._ip),
                                          n_lines.ctypes.data_as(_ffi._ip), _ffi.dptr(nus), _ffi.dptr(voff), _ffi.dptr(wts),
                                          _ffi.dptr(e_up), _ffi.dptr(g_up), _ffi.dptr(a_ul), q_temp.size, _ffi.dptr(q_temp),
                                          _ffi.dptr(q_val), xp, 1, _ffi.dptr(data),
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
    assert _create_bands(lib)[0] == 0 and _create_bands(lib, noise='channel')[0] == 0
    one = dict(n_trans=(1,), n_lines=(1,), nus=(1e11,), voff=(0.0,), wts=(1.0,), e_up=(4.0,), g_up=(3.0,), a_ul=(1e-5,))
    assert _create_bands(lib, **one)[0] == 0                                               # nfa_specset_create_lte's set
    eight = dict(n_trans=(8,), n_lines=(1,) * 8, nus=1e11 + 1e5 * np.arange(8), voff=(0.0,) * 8, wts=(1.0,) * 8,
                 e_up=4.0 + np.arange(8), g_up=(3.0,) * 8, a_ul=(1e-5,) * 8)
    assert _create_bands(lib, **eight)[0] == 0
    fifty = dict(n_lines=(25, 25), voff=np.tile(np.linspace(-3, 3, 25), 2), wts=np.full(50, 1 / 25))
    assert _create_bands(lib, **fifty)[0] == 0
    mixed = dict(n_trans=(2, 1), n_lines=(1, 1, 1), nus=(1e11, 1.00001e11, 1e11), voff=(0.0,) * 3, wts=(1.0,) * 3, e_up=(4.0, 9.0, 4.0),
                 g_up=(3.0, 5.0, 3.0), a_ul=(1e-5, 2e-5, 1e-5))
    assert _create_bands(lib, **mixed)[0] == 0                                             # the same transition in two spectra
    nine = {k: (np.append(v, v[-1] + 1) if k in ('nus', 'e_up') else tuple(v) + (v[-1],)) for k, v in eight.items() if k != 'n_trans'}
    bad = [
        (dict(n_trans=(0,)), '1..8 transitions'), ({**nine, 'n_trans': (9,)}, '1..8 transitions'), (dict(n_trans=(-1,)), '1..8 transitions'),
        (dict(n_lines=(26, 25), voff=np.zeros(51), wts=np.concatenate([np.full(26, 1 / 26), np.full(25, 1 / 25)])), 'at most 50 lines'),
        (dict(nus=(1e11, 1e11), e_up=(4.0, 4.0), g_up=(3.0, 3.0), a_ul=(1e-5, 1e-5)), 'same transition twice'),
        ({**mixed, 'n_trans': (1, 2), 'nus': (1e11, 1.2e11, 1.2e11), 'e_up': (4.0, 9.0, 9.0), 'g_up': (3.0, 5.0, 5.0),
          'a_ul': (1e-5, 2e-5, 2e-5)}, 'spectrum 1, transition 1'),
        # every check of nfa_specset_create_lte, per transition
        (dict(e_up=(4.0, -9.0)), 'energy'), (dict(e_up=(np.nan, 9.0)), 'spectrum 0, transition 0'), (dict(g_up=(3.0, 0.0)), 'weight'),
        (dict(a_ul=(1e-5, np.inf)), 'Einstein'), (dict(wts=(1.0, 0.9)), 'sum to 1'), (dict(wts=(1.0, 0.9)), 'transition 1'),
        (dict(n_lines=(1, 0), voff=(0.0,), wts=(1.0,)), 'lines'), (dict(nus=(1e11, 0.0)), 'rest frequency'),
        (dict(voff=(0.0, np.nan)), 'velocity offset'), (dict(wts=(1.0, -1.0)), 'weight'),
        (dict(n_lines=(1, 2), voff=(0.0, 0.0, 1.0), wts=(1.0, 0.0, 0.0)), 'all zero'),
        (dict(q_temp=(5.0, 5.0, 20.0)), 'ascending'), (dict(q_val=(2.0, 0.0, 9.0)), 'partition function'),
        (dict(q_temp=(5.0,), q_val=(2.0,)), '2..64'),
        (dict(noise='none'), 'exactly one'), (dict(noise='both'), 'exactly one'),
    ]
    for kw, word in bad:
        rc, msg = _create_bands(lib, **kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)


# ---------------------------------------------------------------------------- sampling
TRUTH_FIT = np.array([0.4, 22.0, 14.6, 0.6])
FIT_RANGES = [(-3, 3), (6.0, 60.0), (13.0, 15.5), (0.2, 1.5)]


def test_run_multinest_recovers_tex_and_column_density_from_the_ladder(engine, nfo, mode_guard):
    """One component on ONE banded spectrum: the ratios of the K components are the thermometer."""
    from nestfit_amd import sampler
    mol, ks = top_species(engine)
    band = mol.band(ks)
    tau = band.tau_main(*TRUTH_FIT[1:])
    assert 0.02 < tau.min() and tau.max() < 3.0                         # every component seen, none saturated
    rng = np.random.default_rng(17)
    noise = 0.02
    x = band_axis(band.nu)
    data = br.band_predict(nfo, x, hfr.tbg_of(nfo, x), band, TRUTH_FIT) + rng.normal(0, noise, N_CHAN)
    run = engine.LteRunner.from_data([[x, data, noise, band]], _simple_priors(engine, FIT_RANGES), ncomp=1)
    res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=5)
    mean, std = res.param_constr[0], res.param_constr[1]
    print(f'lnZ - null_lnZ = {res.lnZ - run.null_lnZ:.1f}; mean {mean}, std {std}, truth {TRUTH_FIT}; tau {tau}')
    assert res.lnZ - run.null_lnZ > 11
    for k in (1, 2):
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])
    assert std[1] < 5.0 and std[2] < 0.3                                # both are constrained, not the priors' widths


def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube of one banded spectrum: fit_cube, the store with its bands, the map products."""
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    mol, ks = top_species(engine)
    band = mol.band(ks, name='J=5-4')
    rng = np.random.default_rng(31)
    n_side, noise = 4, 0.02
    truths = np.stack([rng.uniform(-1, 1, 16), rng.uniform(15.0, 30.0, 16), rng.uniform(14.4, 14.8, 16), rng.uniform(0.4, 0.8, 16)], axis=1)

    def cube_of(lines, seed=1):
        x = band_axis(lines.nu)
        tbg = hfr.tbg_of(nfo, x)
        data = np.random.default_rng(seed).normal(0, noise, (N_CHAN, n_side, n_side))
        for k, th in enumerate(truths):
            data[:, k // n_side, k % n_side] += br.band_predict(nfo, x, tbg, band, th)
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': N_CHAN,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': lines.nu}
        return DataCube(SimpleCube(hdr, data), noise, lines=lines)
    stack = CubeStack([cube_of(band)])
    fitter = CubeFitter(stack, _simple_priors(engine, FIT_RANGES), engine.LteRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 60, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (4, 4, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'lte' and store.read_model_lines() == [band]
        assert int(store.hdf['/model_lines/spec0'].attrs['n_trans']) == 4
        groups = list(store.iter_pix_groups())
        assert len(groups) == 16 and all(g.attrs['nbest'] == 1 for g in groups)
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])              # (t, m, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                    # (m, p, b, l)
        spec = np.asarray(store.hdf[f'{store.dpath}/model_spec/spec0'])            # (m, S, b, l)
        assert peak.shape == (1, 1, 4, 4) and np.isfinite(peak).all() and spec.shape == (1, N_CHAN, 4, 4)
        predict = pp._device_predictor(store, stack)                               # table mode, like the products
        rows = [[stack.cubes[0].xarr, np.zeros(N_CHAN), 1.0, band]]
        worst = 0.0
        for l in range(4):
            for b in range(4):
                th = np.ascontiguousarray(pmap[0, :, b, l])
                truth = truths[b * n_side + l]                                     # (truth k sits at lat k // 4, lon k % 4)
                assert abs(th[0] - truth[0]) < 0.3 and abs(th[1] - truth[1]) < 8.0 and abs(th[2] - truth[2]) < 0.3
                got, _, _ = predict(np.array([l]), np.array([b]), th[None, :], True)
                worst = max(worst, _check_spec(got[0], br.restated(nfo, rows, th)[0], 'table'))
                assert np.array_equal(spec[0, :, b, l], got[0].astype(np.float32)) and peak[0, 0, b, l] == got[0].max()
        assert worst < TIGHT['table']
    # a stack whose band differs from the store's is refused: by the check and by the device predictor
    with HdfStore(path) as store:
        for lines in (mol.band(ks[:3]), mol.band(ks[::-1]), ks[0]):
            other = CubeStack([cube_of(lines)])
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp._device_predictor(store, other)
