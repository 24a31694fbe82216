"""A beam filling factor per component of the LTE models on the device (nfa_specset_create_lte_filled): the last
parameter of a component is lnff = log10 f, and its Tb is multiplied by f.

The reference is tests/fill_restatement.py -- the mix's restatement with the component's term multiplied by 10.0 ** lnff
before it is added -- at the sizes and tolerances of tests/test_lte_mix.py, imported and not restated: zero pattern exact,
spectra TIGHT, lnL LNL_RTOL, the fast mode's floor as that file derives it (f <= 1 here: the floor only shrinks)."""
import functools
import os

import numpy as np
import pytest

import band_restatement as br
import fill_restatement as fr
import hf_restatement as hfr
import mix_restatement as mr
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands import wide_band
from test_lte_bands_cpu import N_CHAN, band_axis
from test_lte_mix import COLD, FIT_RANGES as MIX_FIT_RANGES, N_ROWS, NOISE, RANGES as MIX_RANGES, TRUTH_FIT as MIX_TRUTH_FIT
from test_lte_mix import _check_spec, _rows, draw_params as draw_mix
from test_sibling_models import LNL_RTOL, MODES, TIGHT, _simple_priors

pytestmark = pytest.mark.gpu

LNFF = (-2.0, 0.0)
RANGES = MIX_RANGES + [LNFF]                    # voff, tex, lncol, sigm, lncol2, lnff


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def draw_params(rng, ncomp, mol, iso, row, n_species=2):
    """The mix test's draw -- tex of every kind in turn by row and component, the further column densities -3..+3 about the
    first -- and lnff over -2..0, one value per component: the components of a row in the ncomp equal parts of the range, in
    an order drawn per row, each inside the middle nine tenths of its part -- every component sees the whole range over the
    rows, and two components of a row differ by 0.2 / ncomp at the least."""
    theta = draw_mix(rng, ncomp, mol, iso, row, n_species=n_species)
    lnff = LNFF[0] + (LNFF[1] - LNFF[0]) * (rng.permutation(ncomp) + rng.uniform(0.05, 0.95, ncomp)) / ncomp
    return np.concatenate([theta, lnff])


def _tex_of(theta, n_species):
    ncomp = theta.size // (4 + n_species)
    return theta[ncomp:2 * ncomp]


def _tables(engine, n_spec):
    """A blend of both ladders alone, or beside a spectrum of one transition of species 1 only."""
    mol, ks, iso, isos = mr.test_species(engine)
    return mol, iso, (engine.LteBlend(ks + isos), isos[1])[:n_spec]


@functools.lru_cache(maxsize=None)
def _reference(n_spec, ncomp):
    """(rows, thetas, spectra, lnL) of the restatement, computed once for both modes."""
    import nestfit_amd as na
    from oracle import nfo
    mol, iso, tables = _tables(na, n_spec)
    rows = _rows(tables, seed=10 * n_spec + ncomp)
    rng = np.random.default_rng(7000 + 10 * n_spec + ncomp)
    thetas = np.stack([draw_params(rng, ncomp, mol, iso, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    want = [fr.restated(nfo, rows, (mol, iso), th, tbgs) for th in thetas]
    spec, lnl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    spec.setflags(write=False), lnl.setflags(write=False), thetas.setflags(write=False)
    return rows, thetas, spec, lnl


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3, 4])
@pytest.mark.parametrize('n_spec', [1, 2])
def test_spectra_and_lnl_against_the_restatement(engine, n_spec, ncomp, mode, mode_guard):
    """1..4 components: a filled set takes the general component form at every count."""
    engine.set_exp_mode(mode)
    rows, thetas, want_spec, want_lnl = _reference(n_spec, ncomp)
    mol, ks, iso, isos = mr.test_species(engine)
    tex, sigm = thetas[:, ncomp:2 * ncomp], thetas[:, 3 * ncomp:4 * ncomp]
    dcol = thetas[:, 4 * ncomp:5 * ncomp] - thetas[:, 2 * ncomp:3 * ncomp]
    lnff = thetas[:, 5 * ncomp:]
    # the draws contain what they are meant to contain (tests/test_lte_mix.py) ...
    assert (tex[tex > 1] < iso.q_temp[0]).any() and (tex > iso.q_temp[-1]).any()
    assert np.isin(tex, mol.q_temp).any() and np.isin(tex, iso.q_temp).any()
    assert ((tex > iso.q_temp[0]) & (tex < mol.q_temp[0])).any() and ((tex > mol.q_temp[0]) & (tex < mol.q_temp[-1]) & ~np.isin(tex, mol.q_temp)).any()
    cold = tex < COLD[1]
    assert cold.any() and all(float(ks[2].tau_main(t, 15.5, 0.1)) == 0.0 < float(ks[1].tau_main(t, 13.0, 1.6)) for t in tex[cold])
    assert dcol.min() < -2.5 and dcol.max() > 2.5 and (np.abs(dcol) < 0.5).any()
    assert (2 * sigm > (ks[1].nu - isos[0].nu) / ks[0].nu * br.CKMS).any()         # the two ladders closer than two widths: blended
    # ... and filling factors over the two decades that differ between the components of every row: a component-index slip shows
    assert lnff.shape == (N_ROWS, ncomp) and lnff.min() < -1.85 and lnff.max() > -0.15
    assert ncomp == 1 or np.abs(np.diff(np.sort(lnff, axis=1), axis=1)).min() > 0.19 / ncomp
    mix = engine.LteMix([mol, iso], fill=True)
    run = mix.Runner.from_data(rows, None, ncomp=ncomp)
    assert (run.ndim, run.n_params, run.n_spec, run.n_chan_tot, run.n_model) == (6 * ncomp, 6 * ncomp, n_spec, n_spec * N_CHAN, 6)
    spec, lnl = run.predict_batch(np.array(thetas))
    worst, worst_lnl = 0.0, 0.0
    for sp, ll, ws, wl, th in zip(spec, lnl, want_spec, want_lnl, thetas):
        worst = max(worst, _check_spec(sp, ws, mode, _tex_of(th, 2)))
        worst_lnl = max(worst_lnl, abs(ll - wl) / abs(wl))
    print(f'fill {mode} n_spec={n_spec} ncomp={ncomp}: worst relative Tb error {worst:.2e}, lnL {worst_lnl:.2e}')
    assert worst < TIGHT[mode]
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    assert np.abs(want_spec).max() > 1.0                                           # (lines that matter beside the noise)
    # ... and per spectrum through the mix's predict: a Spectrum's own rows of the parameter vector include the lnff row
    run.predict(np.array(thetas[1]))
    got = np.concatenate([s.get_spec() for s in run.spectra])
    assert _check_spec(got, want_spec[1], mode, _tex_of(thetas[1], 2)) < TIGHT[mode]
    assert [s._rows for s in run.spectra] == [[0, 1, 2, 3, 4, 5], [0, 1, 4, 3, 5]][:n_spec]


@pytest.mark.parametrize('mode', MODES)
def test_one_species_on_one_single_line_transition(engine, nfo, mode, mode_guard):
    """The smallest filled set: its band and mix records exist only for the factor."""
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    assert ks[1].n == 1
    rows = _rows((ks[1],), seed=71)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    mix = engine.LteMix([mol], fill=True)
    rng = np.random.default_rng(72)
    for ncomp in (1, 2):
        run = mix.Runner.from_data(rows, None, ncomp=ncomp)
        assert (run.n_model, run.ndim) == (5, 5 * ncomp)
        thetas = np.stack([draw_params(rng, ncomp, mol, iso, k, n_species=1) for k in range(40)])
        spec, lnl = run.predict_batch(thetas)
        worst = 0.0
        for sp, ll, th in zip(spec, lnl, thetas):
            ws, wl = fr.restated(nfo, rows, (mol,), th, tbgs)
            worst = max(worst, _check_spec(sp, ws, mode, _tex_of(th, 1)))
            assert ll == pytest.approx(wl, rel=LNL_RTOL[mode])
        assert worst < TIGHT[mode] and np.abs(spec).max() > 1.0


@pytest.mark.parametrize('mode', MODES)
def test_against_the_unfilled_mix(engine, mode, mode_guard):
    """lnff == 0 everywhere: the unfilled mix runner's spectra and lnL on the same rows and parameters, to TIGHT (another
    form is taken below four components: bits are not promised).  One component at lnff = -1: a tenth of its spectrum at 0."""
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    rows = _rows((engine.LteBlend(ks + isos), isos[1]), seed=75)
    rng = np.random.default_rng(76)
    for ncomp in (1, 2, 3, 4):
        theta5 = np.stack([draw_mix(rng, ncomp, mol, iso, k) for k in range(64)])
        want_spec, want_lnl = engine.LteMix([mol, iso]).Runner.from_data(rows, None, ncomp=ncomp).predict_batch(theta5)
        filled = engine.LteMix([mol, iso], fill=True).Runner.from_data(rows, None, ncomp=ncomp)
        spec, lnl = filled.predict_batch(np.concatenate([theta5, np.zeros((64, ncomp))], axis=1))
        worst = max(_check_spec(sp, ws, mode, th[ncomp:2 * ncomp]) for sp, ws, th in zip(spec, want_spec, theta5))
        print(f'fill {mode} ncomp={ncomp}: lnff = 0 against the unfilled mix: worst relative Tb difference {worst:.2e}, '
              f'same bits: {np.array_equal(spec, want_spec)}')
        assert worst < TIGHT[mode] and np.abs(want_spec).max() > 1.0
        np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
        if ncomp == 1:
            tenth, _ = filled.predict_batch(np.concatenate([theta5, np.full((64, 1), -1.0)], axis=1))
            assert max(_check_spec(sp, 0.1 * ws, mode, th[1:2]) for sp, ws, th in zip(tenth, spec, theta5)) < TIGHT[mode]


# ---------------------------------------------------------------------------- routes
@pytest.mark.parametrize('mode', MODES)
def test_the_same_bits_on_every_route(engine, nfo, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    species = (mol, iso)
    mix = engine.LteMix(species, fill=True)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((engine.LteBlend(ks + isos), isos[1]), seed=3)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    run = mix.Runner.from_data(rows, ut, ncomp=2)
    # host and device batches, coalescing on and off, single points and a handful: these take the batch path
    U, theta, lnl = _routes(engine, run, rng)
    for k in (0, 100, 512):
        assert lnl[k] == pytest.approx(fr.restated(nfo, rows, species, theta[k], tbgs)[1], rel=LNL_RTOL[mode])
    for split in (4, 1):                                                        # ... whatever the row split of a small launch
        _ffi.set_option('lnl_split', split)
        run_s = mix.Runner.from_data(rows, ut, ncomp=2)                         # (a runner reads the option when it is made)
        for k in (0, 7, 150):
            u = U[k].copy()
            assert run_s.loglikelihood(u) == lnl[k] and np.array_equal(u, theta[k]), split
        few = U[20:31].copy()
        assert np.array_equal(run_s.loglikelihood_batch(few), lnl[20:31]), split
    _ffi.set_option('lnl_split', 0)
    lb, tb = _through_a_broker(engine, run, U[:64].reshape(8, 8, -1))
    assert np.array_equal(lb.ravel(), lnl[:64]) and np.array_equal(tb.reshape(64, -1), theta[:64])
    # predict_batch: whatever the batch
    spec, pl = run.predict_batch(theta[:40])
    for k in (0, 13, 39):
        s1, l1 = run.predict_batch(theta[k:k + 1])
        assert np.array_equal(s1[0], spec[k]) and l1[0] == pl[k]
    np.testing.assert_allclose(pl, lnl[:40], rtol=LNL_RTOL[mode])
    assert _check_spec(spec[3], fr.restated(nfo, rows, species, theta[3], tbgs)[0], mode, theta[3][2:4]) < TIGHT[mode]
    # a noise per channel, with masked channels
    chan = [rng.uniform(0.1, 0.3, N_CHAN) for _ in rows]
    for s in chan:
        s[rng.integers(0, N_CHAN, 5)] = np.inf
    rows_c = [[x, d, s, t] for (x, d, _, t), s in zip(rows, chan)]
    run_c = mix.Runner.from_data(rows_c, ut, ncomp=2)
    _, theta_c, lnl_c = _routes(engine, run_c, rng, n_rows=256)
    for k in (0, 100, 255):
        pred = fr.restated(nfo, rows, species, theta_c[k], tbgs)[0]
        want = sum(-np.sum(((d - pred[i * N_CHAN:(i + 1) * N_CHAN]) / s)[np.isfinite(s)] ** 2) / 2 for i, (_, d, s, _) in enumerate(rows_c))
        assert lnl_c[k] == pytest.approx(want, rel=LNL_RTOL[mode])
    # a baseline of order 1: the same bits on every route, and never a worse fit than without one
    run_b = mix.Runner.from_data(rows, ut, ncomp=2, baseline_order=1)
    Ub, _, lnl_b = _routes(engine, run_b, rng, n_rows=256)
    plain = run.loglikelihood_batch(Ub.copy())
    assert (lnl_b >= plain - 1e-9 * np.abs(plain)).all() and (lnl_b > plain).any()
    # a blend of 33 lines: the wide instances
    wide = engine.LteBlend(list(wide_band(mol, ks)) + isos)
    assert wide.n_lines == 33
    rows_w = _rows((wide, isos[1]), seed=4)
    run_w = mix.Runner.from_data(rows_w, ut, ncomp=2)
    _, theta_w, lnl_w = _routes(engine, run_w, rng, n_rows=256)
    for k in (0, 100, 255):
        assert lnl_w[k] == pytest.approx(fr.restated(nfo, rows_w, species, theta_w[k], tbgs)[1], rel=LNL_RTOL[mode])
    spec_w, _ = run_w.predict_batch(theta_w[:8])
    assert max(_check_spec(spec_w[k], fr.restated(nfo, rows_w, species, theta_w[k], tbgs)[0], mode, theta_w[k][2:4]) for k in range(8)) < TIGHT[mode]


@pytest.mark.parametrize('mode', MODES)
def test_every_batch_of_a_coalesced_group_reads_its_own_theta(engine, mode, mode_guard):
    """lte_fill_kernel takes lnff of item b from grp.U[group_of(b)] at row b - c each: the one thing in it that depends on the
    route.  Device batches of ONE shape (whole set-up groups: held and launched together at coalesce 8, one by one at 1), each
    with its lnff in another part of the prior, and EVERY batch against the host call on the same rows, theta and lnL bit
    for bit.  Two pixels of a cube runner as well, so that the pixel arrays of the group are in play."""
    from nestfit_amd import _ffi
    from nestfit_amd.cube import CubeRunner
    from test_device_batches import _run_on_device
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    mix = engine.LteMix((mol, iso), fill=True)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((engine.LteBlend(ks + isos), isos[1]), seed=61)
    rng = np.random.default_rng(62)
    for ncomp, each, n_batch in ((2, 256, 5), (1, 64, 8), (3, 128, 3)):
        run = mix.Runner.from_data(rows, ut, ncomp=ncomp)
        batches = []
        for k in range(n_batch):
            U = rng.uniform(size=(each, run.ndim))
            U[:, 5 * ncomp:] = (k + rng.uniform(size=(each, ncomp))) / n_batch      # lnff: the k-th part of its prior's range
            batches.append((None, U))
        want = []
        for _, U in batches:
            theta = U.copy()
            want.append((theta, run.loglikelihood_batch(theta)))
        assert len({w[1].tobytes() for w in want}) == n_batch and all(np.isfinite(w[1]).all() for w in want)
        # the factor matters: batch 1's rows with batch 0's lnff have another lnL
        crossed = batches[1][1].copy()
        crossed[:, 5 * ncomp:] = batches[0][1][:, 5 * ncomp:]
        assert not np.array_equal(run.loglikelihood_batch(crossed), want[1][1])
        for coalesce in (8, 1):
            _ffi.set_option('coalesce', coalesce)
            got = _run_on_device(_ffi, run._run.handle, batches)
            for k, ((theta, lnl), (want_theta, want_lnl)) in enumerate(zip(got, want)):
                assert np.array_equal(theta, want_theta) and np.array_equal(lnl, want_lnl), (ncomp, coalesce, k)
        _ffi.set_option('coalesce', 8)
    # a cube runner: every batch with pixel indices of its own
    x = rows[0][0]
    data = np.stack([np.concatenate([rng.normal(0, NOISE, N_CHAN) for _ in rows]) for _ in range(2)])
    cube = CubeRunner([x, x], None, data, np.full((2, 2), NOISE), ut, ncomp=2, model=4, lines=[r[3] for r in rows], species=mix.species, fill=True)
    assert (cube.n_model, cube.ndim) == (6, 12)
    batches = []
    for k in range(4):
        U = rng.uniform(size=(128, cube.ndim))
        U[:, 10:] = (k + rng.uniform(size=(128, 2))) / 4
        batches.append((rng.integers(0, 2, 128).astype(np.int32), U))
    want = []
    for pix, U in batches:
        theta = U.copy()
        want.append((theta, cube.loglikelihood_batch(pix, theta)))
    for coalesce in (8, 1):
        _ffi.set_option('coalesce', coalesce)
        got = _run_on_device(_ffi, cube._run.handle, batches)
        for k, ((theta, lnl), (want_theta, want_lnl)) in enumerate(zip(got, want)):
            assert np.array_equal(theta, want_theta) and np.array_equal(lnl, want_lnl), ('cube', coalesce, k)


@pytest.mark.parametrize('mode', MODES)
def test_unit_cube_in_lnl_out(engine, nfo, mode, mode_guard):
    """A PriorTransformer over the 4 + K parameters: theta against the priors' host transform, lnL against the restatement
    at the engine's theta."""
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    rng = np.random.default_rng(78)
    ut = _simple_priors(engine, RANGES)
    ps = nfo.PriorSet(ut.lower())
    rows = _rows((engine.LteBlend(ks + isos), isos[0]), seed=6)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    mix = engine.LteMix((mol, iso), fill=True)
    for ncomp in (1, 2):
        run = mix.Runner.from_data(rows, ut, ncomp=ncomp)
        U = rng.uniform(size=(N_ROWS, 6 * ncomp))
        theta = U.copy()
        lnl = run.loglikelihood_batch(theta)
        for k in range(0, N_ROWS, 8):
            want_theta = U[k].copy()
            ps.transform(want_theta, ncomp)
            np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
            assert lnl[k] == pytest.approx(fr.restated(nfo, rows, (mol, iso), theta[k], tbgs)[1], rel=LNL_RTOL[mode])


@pytest.mark.parametrize('mode', MODES)
def test_edge_values_of_the_factor(engine, mode, mode_guard):
    """lnff = -inf: exactly the other components' spectrum.  A NaN lnff: NaN lnL for that row only."""
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    rows = _rows((engine.LteBlend(ks + isos), isos[1]), seed=91)
    mix = engine.LteMix((mol, iso), fill=True)
    rng = np.random.default_rng(92)
    two = mix.Runner.from_data(rows, None, ncomp=2)
    one = mix.Runner.from_data(rows, None, ncomp=1)
    thetas = np.stack([draw_params(rng, 2, mol, iso, 4) for _ in range(64)])      # (tex inside both tables: lines everywhere)
    thetas[:, 1::2][:, :5] = thetas[:, 0::2][:, :5] + [[0.7, 3.0, 0.1, 0.05, 0.1]]   # the second component on top of the first
    gone = thetas.copy()
    gone[:, 10] = -np.inf                                                      # the first component fills nothing
    spec, lnl = two.predict_batch(gone)
    want_spec, want_lnl = one.predict_batch(np.ascontiguousarray(thetas[:, 1::2]))
    assert np.array_equal(spec, want_spec) and np.abs(want_spec).max() > 0.05
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    full, lnl_full = two.predict_batch(thetas)
    assert not np.array_equal(full, want_spec) and np.isfinite(lnl_full).all()
    bad = thetas.copy()
    bad[(5, 17, 63), (10, 11, 10)] = np.nan
    spec, lnl = two.predict_batch(bad)
    assert np.array_equal(np.isnan(lnl), np.isin(np.arange(64), (5, 17, 63)))
    keep = ~np.isnan(lnl)
    assert np.array_equal(lnl[keep], lnl_full[keep]) and np.array_equal(spec[keep], full[keep]) and np.isnan(spec[5]).any()


# ---------------------------------------------------------------------------- refusals
def test_the_resident_kernel_refuses_a_filled_runner(engine, mode_guard):
    from nestfit_amd.ring import RingServer
    mol, ks, iso, isos = mr.test_species(engine)
    for species, tables, ranges in (((mol, iso), (engine.LteBlend(ks + isos),), RANGES), ((mol,), (ks[1],), RANGES[:4] + [LNFF])):
        run = engine.LteMix(species, fill=True).Runner.from_data(_rows(tables, seed=2), _simple_priors(engine, ranges), ncomp=1)
        with RingServer(f'nfa_test_ring_fill_{os.getpid()}', n_slots=1, runner=run) as server:
            with pytest.raises(engine.EngineError, match='no form for a filling factor: use nfa_ring_serve'):
                server.serve_device(lifetime_ms=20, idle_ms=100)
        u = np.full(run.ndim, 0.5)                                        # ... and a single point takes the batch path
        assert np.isfinite(run.loglikelihood(u))


def test_a_prior_of_the_wrong_length_and_what_does_not_fit_the_sampler_are_refused(engine, mode_guard):
    """Five priors for six parameters, and the unfilled mix's message names the filling factor; eight parameters and eight
    components: the batch kernels take the 64 dimensions, the device sampler holds 60."""
    mol, ks, iso, isos = mr.test_species(engine)
    rows = _rows((engine.LteBlend(ks + isos),), seed=1)
    with pytest.raises(engine.EngineError, match='prior program.*filling factor'):
        engine.LteMix((mol, iso), fill=True).Runner.from_data(rows, _simple_priors(engine, RANGES[:5]), ncomp=1)
    with pytest.raises(engine.EngineError, match='prior program'):
        engine.LteMix((mol, iso)).Runner.from_data(rows, _simple_priors(engine, RANGES), ncomp=1)
    (m3, t3), (m4, t4) = mr.made_up_species(engine, ks[0].nu)
    rows = _rows((engine.LteBlend([ks[0], isos[0], t3, t4]),), seed=1)
    ut8 = _simple_priors(engine, MIX_RANGES + [(11.0, 15.0), (11.0, 15.0), LNFF])
    big = engine.LteMix((mol, iso, m3, m4), fill=True).Runner.from_data(rows, ut8, ncomp=8)
    assert big.ndim == 64 and np.isfinite(big.loglikelihood_batch(np.full((3, 64), 0.5))).all()
    from nestfit_amd import sampler
    with pytest.raises(engine.EngineError, match='too many dimensions'):
        sampler.run_multinest(big, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=1)


# ---------------------------------------------------------------------------- sampling
TRUTH_FIT = np.concatenate([MIX_TRUTH_FIT, [np.log10(0.3)]])       # voff, tex, lncol, sigm, lncol2, lnff: f = 0.3
FIT_RANGES = MIX_FIT_RANGES + [(-1.5, 0.0)]


def test_run_multinest_recovers_the_filling_factor(engine, nfo, mode_guard):
    """One component on ONE blended spectrum, main ladder thick, isotopologue thin, f = 0.3: the thick lines measure
    f J(tex), the thin ladder's K ratios tex, the thin intensities f N.

    The truths are the mix test's with lnff = log10 0.3.  Checked on the CPU with tests/fill_restatement.py before they were
    fixed: the Fisher matrix of (tex, lncol, lncol2, lnff) at the truth, by central finite differences (steps of 1e-4 of
    the prior ranges) at the noise of 0.02 K used here, with the parameters in units of their prior ranges, has condition
    number 141 (Cramer-Rao standard deviations 0.035 K, 0.0014, 0.0046 and 0.0008 dex).  At a column density 1.5 dex lower,
    where every line is thin (tau <= 0.15) and f and N are degenerate by construction, it is 1.5e4."""
    from nestfit_amd import sampler
    mol, ks, iso, isos = mr.test_species(engine)
    mix = engine.LteMix((mol, iso), fill=True)
    blend = engine.LteBlend(ks + isos)
    tau = engine.LteMix((mol, iso)).tau_main(blend, TRUTH_FIT[1], [TRUTH_FIT[2], TRUTH_FIT[4]], TRUTH_FIT[3])
    assert tau[:2].min() > 3.0 and 0.02 < tau[4:].min() and tau[4:].max() < 0.5        # main K = 0, 1 thick, the isotopologue thin
    rng = np.random.default_rng(17)
    noise = 0.02
    x = band_axis(ks[0].nu)
    data = fr.fill_predict(nfo, x, hfr.tbg_of(nfo, x), blend, (mol, iso), TRUTH_FIT) + rng.normal(0, noise, N_CHAN)
    run = mix.Runner.from_data([[x, data, noise, blend]], _simple_priors(engine, FIT_RANGES), ncomp=1)
    res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=5)
    mean, std = res.param_constr[0], res.param_constr[1]
    print(f'lnZ - null_lnZ = {res.lnZ - run.null_lnZ:.1f}; mean {mean}, std {std}, truth {TRUTH_FIT}')
    assert res.lnZ - run.null_lnZ > 11
    for k in range(6):
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])
    assert std[1] < 5.0 and std[2] < 0.3 and std[4] < 0.3 and std[5] < 0.15   # constrained, not the priors' widths


def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube of one blended spectrum: fit_cube, the store with its species and `fill`, the map products -- predict
    batches of a filled runner, so a pixel's model spectrum is the restatement's at its MAP parameters, factor included."""
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    mol, ks, iso, isos = mr.test_species(engine)
    mix = engine.LteMix((mol, iso), fill=True)
    blend = engine.LteBlend(ks + isos, name='J=5-4')
    rng = np.random.default_rng(31)
    n_side, noise = 4, 0.02
    truths = np.stack([rng.uniform(-1, 1, 16), rng.uniform(18.0, 30.0, 16), rng.uniform(15.2, 15.6, 16), rng.uniform(0.4, 0.8, 16),
                       rng.uniform(13.6, 14.0, 16), rng.uniform(-0.7, -0.3, 16)], axis=1)
    x = band_axis(ks[0].nu)
    tbg = hfr.tbg_of(nfo, x)
    data = np.random.default_rng(1).normal(0, noise, (N_CHAN, n_side, n_side))
    for k, th in enumerate(truths):
        data[:, k // n_side, k % n_side] += fr.fill_predict(nfo, x, tbg, blend, (mol, iso), th)
    hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': N_CHAN,
           'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
           'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': ks[0].nu}
    stack = CubeStack([DataCube(SimpleCube(hdr, data), noise, lines=blend)])
    fitter = CubeFitter(stack, _simple_priors(engine, FIT_RANGES), mix.Runner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 60, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs, fitter.fill) == (4, 6, {}, True)
    runner, _, _ = stack.to_device(None, ncomp=1, model=4, species=mix.species, fill=True)
    assert (runner.n_model, runner.ndim) == (6, 6)
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'lte_mix' and int(store.hdf.attrs['n_params']) == 6 and store.read_model_fill() is True
        assert store.read_model_lines(with_species=True) == ([blend], (mol, iso))
        groups = list(store.iter_pix_groups())
        assert len(groups) == 16 and all(g.attrs['nbest'] == 1 for g in groups)
        with pytest.raises(ValueError, match='fitted with a filling factor'):      # before any product is written
            pp.postprocess_run(store, stack, runner=engine.LteMix((mol, iso)).Runner)
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])              # (t, m, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                    # (m, p, b, l)
        spec = np.asarray(store.hdf[f'{store.dpath}/model_spec/spec0'])            # (m, S, b, l)
        assert peak.shape == (1, 1, 4, 4) and np.isfinite(peak).all() and spec.shape == (1, N_CHAN, 4, 4) and pmap.shape[1] == 6
        predict = pp._device_predictor(store, stack)                               # table mode, like the products: a filled runner
        xs = stack.cubes[0].xarr                                                   # the axis the header gives: not x to the bit
        rows, tbgs = [[xs, np.zeros(N_CHAN), 1.0, blend]], [hfr.tbg_of(nfo, xs)]
        worst = 0.0
        for l in range(4):
            for b in range(4):
                th = np.ascontiguousarray(pmap[0, :, b, l])
                truth = truths[b * n_side + l]                                     # (truth k sits at lat k // 4, lon k % 4)
                assert abs(th[0] - truth[0]) < 0.3 and abs(th[1] - truth[1]) < 8.0 and abs(th[2] - truth[2]) < 0.5 and abs(th[4] - truth[4]) < 0.3
                assert abs(th[5] - truth[5]) < 0.3
                got, _, _ = predict(np.array([l]), np.array([b]), th[None, :], True)
                worst = max(worst, _check_spec(got[0], fr.restated(nfo, rows, (mol, iso), th, tbgs)[0], 'table', th[1:2]))
                assert np.array_equal(spec[0, :, b, l], got[0].astype(np.float32)) and peak[0, 0, b, l] == got[0].max()
                # the factor is in the products: one component, so the peak is f times the unfilled model's
                unfilled = mr.restated(nfo, rows, (mol, iso), th[:5], tbgs)[0]
                assert th[5] < -0.1 and peak[0, 0, b, l] == pytest.approx(10.0 ** th[5] * unfilled.max(), rel=1e-9)
        assert worst < TIGHT['table']
