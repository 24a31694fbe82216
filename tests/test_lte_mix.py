"""LTE mixes on the device (nfa_specset_create_lte_mix): the transitions of a spectrum belong to several species
that share voff, tex and sigm, each with a column density and a partition table of its own.

The reference is tests/mix_restatement.py -- tau_main per transition by the direct formula on its own species' table and
column, then the loop of c_hf_predict's restatement over all the lines -- at the tolerances the hyperfine and the LTE
models are held to: zero pattern exact, spectra TIGHT, lnL LNL_RTOL.  The species: the symmetric top of
tests/test_lte_bands_cpu.py (K = 0..3) and its "isotopologue" (K = 0..2, 4.2 km/s to the red, another table)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import band_restatement as br
import hf_restatement as hfr
import mix_restatement as mr
from test_hyperfine import _through_a_broker
from test_lte import _routes
from test_lte_bands import wide_band
from test_lte_bands_cpu import N_CHAN, _trans, band_axis
from test_sibling_models import LNL_RTOL, MODES, TB_ATOL_K, TB_RTOL, TIGHT, _simple_priors

pytestmark = pytest.mark.gpu

N_ROWS, NOISE = 200, 0.2                       # 200 rows: three whole set-up groups of 64 and one of 8
RANGES = [(-6, 6), (2.8, 90), (13.0, 15.5), (0.1, 1.5), (11.0, 15.0)]          # voff, tex, lncol, sigm, lncol2
COLD = (0.03, 0.055)                           # tex at which the upper transitions of both ladders underflow


@pytest.fixture
def mode_guard(engine):
    from nestfit_amd import _ffi
    yield
    _ffi.set_option('coalesce', 8)
    _ffi.set_option('lnl_split', 0)
    engine.set_exp_mode('fast')


def _check_spec(pg, pc, mode, tex):
    """test_sibling_models._check_spec -- zero pattern exact, every channel within 1e-6 of the reference's value plus a
    floor, the worst relative deviation of the channels above 1e-6 K returned for TIGHT -- with the fast mode's floor
    worked out for the temperatures drawn here instead of its 4e-15 K.  Where the optical depth q of a channel is below 1e-8
    the reference evaluates 1 - (1 - q), a multiple of 2^-53, and the fast mode repeats that rounding on ITS q, an fp32 sum
    6e-8 off: the two can land one step apart, which is 2^-53 T0 (y - tbg) < 2^-53 tex in kelvin per component (T0 y < tex
    for every x = T0 / tex, since 1 / expm1(x) < 1 / x) -- 4e-15 K at the 36 K the other models' tests stay below, 1.2e-14 K
    at the 112 K drawn here above both partition tables.  `tex`: the excitation temperatures of the row's components.  The
    table mode repeats the reference's operations on an optical depth that differs in its last bits: no floor.
    A DELIBERATE DEPARTURE from the shared helper, whose file is not this change's to edit: its 4e-15 K was the one figure of
    the sibling tolerances that the first fast-mode case missed on the device (blend alone, one component).  TIGHT, LNL_RTOL,
    the 1e-6 per channel and the exact zero pattern are the helper's."""
    assert np.array_equal(pg == 0, pc == 0)
    floor = max(TB_ATOL_K[mode], 2.0 ** -53 * float(np.sum(tex))) if mode == 'fast' else TB_ATOL_K[mode]
    scale = np.abs(pc)
    worst = 0.0
    if (pc != 0).any():
        assert (np.abs(pg - pc) <= TB_RTOL * scale + floor).all()
        big = scale > 1e-6
        if big.any():
            worst = float(np.max(np.abs(pg[big] - pc[big]) / scale[big]))
    return worst


def _tex_of(theta, n_species):
    ncomp = theta.size // (3 + n_species)
    return theta[ncomp:2 * ncomp]


def _rows(tables, seed):
    rng = np.random.default_rng(seed)
    nu0 = mr.test_species(__import__('nestfit_amd'))[1][0].nu               # every axis about the main K = 0
    return [[band_axis(nu0), rng.normal(0, NOISE, N_CHAN), NOISE, t] for t in tables]


def _tex_kind(rng, kind, mol, iso):
    if kind == 0:
        return rng.uniform(2.8, iso.q_temp[0])                               # below both tables
    if kind == 1:
        return rng.uniform(iso.q_temp[-1], 1.5 * iso.q_temp[-1])             # above both
    if kind == 2:
        return mol.q_temp[rng.integers(0, mol.n)]                            # on a node of species 0's
    if kind == 3:
        return iso.q_temp[rng.integers(0, iso.n)]                            # on a node of species 1's
    if kind == 4:
        return rng.uniform(mol.q_temp[0], mol.q_temp[-1])                    # between the nodes of both
    if kind == 5:
        return rng.uniform(*COLD)
    return rng.uniform(iso.q_temp[0], mol.q_temp[0])                         # inside one table, below the other


def draw_params(rng, ncomp, mol, iso, row, n_species=2):
    """tex of every kind in turn by row and component; the further column densities -3..+3 about the first; sigm over
    0.1..1.58 km/s (the main K = 1 and the iso K = 0, 1.7 km/s apart, blend above 0.85)."""
    tex = np.array([_tex_kind(rng, (row + c) % 7, mol, iso) for c in range(ncomp)])
    lncol = rng.uniform(13.0, 15.5, ncomp)
    more = [lncol + rng.uniform(-3.0, 3.0, ncomp) for _ in range(n_species - 1)]
    return np.concatenate([rng.uniform(-6, 6, ncomp), tex, lncol, 10 ** rng.uniform(-1.0, 0.2, ncomp)] + more)


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
    rng = np.random.default_rng(3000 + 10 * n_spec + ncomp)
    thetas = np.stack([draw_params(rng, ncomp, mol, iso, k) for k in range(N_ROWS)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    want = [mr.restated(nfo, rows, (mol, iso), th, tbgs) for th in thetas]
    spec, lnl = np.stack([w[0] for w in want]), np.array([w[1] for w in want])
    spec.setflags(write=False), lnl.setflags(write=False), thetas.setflags(write=False)
    return rows, thetas, spec, lnl


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ncomp', [1, 2, 3])
@pytest.mark.parametrize('n_spec', [1, 2])
def test_spectra_and_lnl_against_the_restatement(engine, n_spec, ncomp, mode, mode_guard):
    engine.set_exp_mode(mode)
    rows, thetas, want_spec, want_lnl = _reference(n_spec, ncomp)
    mol, ks, iso, isos = mr.test_species(engine)
    tex, sigm = thetas[:, ncomp:2 * ncomp], thetas[:, 3 * ncomp:4 * ncomp]
    dcol = thetas[:, 4 * ncomp:] - thetas[:, 2 * ncomp:3 * ncomp]
    assert (tex[tex > 1] < iso.q_temp[0]).any() and (tex > iso.q_temp[-1]).any()
    assert np.isin(tex, mol.q_temp).any() and np.isin(tex, iso.q_temp).any()
    assert ((tex > iso.q_temp[0]) & (tex < mol.q_temp[0])).any() and ((tex > mol.q_temp[0]) & (tex < mol.q_temp[-1]) & ~np.isin(tex, mol.q_temp)).any()
    cold = tex < COLD[1]
    assert cold.any() and all(float(ks[2].tau_main(t, 15.5, 0.1)) == 0.0 < float(ks[1].tau_main(t, 13.0, 1.6)) for t in tex[cold])
    assert dcol.min() < -2.5 and dcol.max() > 2.5 and (np.abs(dcol) < 0.5).any()
    assert (2 * sigm > (ks[1].nu - isos[0].nu) / ks[0].nu * br.CKMS).any()         # the two ladders closer than two widths: blended
    mix = engine.LteMix([mol, iso])
    run = mix.Runner.from_data(rows, None, ncomp=ncomp)
    assert (run.ndim, run.n_params, run.n_spec, run.n_chan_tot, run.n_model) == (5 * ncomp, 5 * ncomp, n_spec, n_spec * N_CHAN, 5)
    spec, lnl = run.predict_batch(np.array(thetas))
    worst, worst_lnl = 0.0, 0.0
    for sp, ll, ws, wl, th in zip(spec, lnl, want_spec, want_lnl, thetas):
        worst = max(worst, _check_spec(sp, ws, mode, _tex_of(th, 2)))
        worst_lnl = max(worst_lnl, abs(ll - wl) / abs(wl))
    print(f'mix {mode} n_spec={n_spec} ncomp={ncomp}: worst relative Tb error {worst:.2e}, lnL {worst_lnl:.2e}')
    assert worst < TIGHT[mode]
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])
    assert np.abs(want_spec).max() > 1.0                                           # (lines that matter beside the noise)
    # ... and per spectrum through the mix's predict (a set of the spectrum alone, with the species it has)
    run.predict(np.array(thetas[1]))
    got = np.concatenate([s.get_spec() for s in run.spectra])
    assert _check_spec(got, want_spec[1], mode, _tex_of(thetas[1], 2)) < TIGHT[mode]


# ---------------------------------------------------------------------------- identity to the single-species code
@pytest.mark.parametrize('mode', MODES)
def test_equal_columns_and_one_table_are_the_band_bit_for_bit(engine, mode, mode_guard):
    """Species 1 is species 0's table under another name and holds K = 2, 3.  With lncol_1 == lncol_0 the factor is 1 . 1:
    the bits of LteRunner on the band.  With lncol_1 = lncol_0 + 1 it is the band whose K = 2, 3 have ten times the a_ul."""
    engine.set_exp_mode(mode)
    mol, ks, iso, _ = mr.test_species(engine)
    twin = engine.Molecule('twin', mol.q_temp, mol.q_val)
    as_twin = [twin.transition(*_trans(t), name=t.name) for t in ks[2:]]
    rows = _rows((mol.band(ks), ks[1]), seed=21)
    rows_mix = [[rows[0][0], rows[0][1], NOISE, engine.LteBlend(ks[:2] + as_twin)], rows[1]]
    plain = engine.LteRunner.from_data(rows, None, ncomp=2)
    mixed = engine.LteMix([mol, twin]).Runner.from_data(rows_mix, None, ncomp=2)
    rng = np.random.default_rng(22)
    from test_lte_bands import draw_params as draw4
    theta4 = np.stack([draw4(rng, 2, mol, k) for k in range(N_ROWS)])
    theta5 = np.concatenate([theta4, theta4[:, 4:6]], axis=1)
    want_spec, want_lnl = plain.predict_batch(theta4)
    spec, lnl = mixed.predict_batch(theta5)
    assert np.array_equal(spec, want_spec) and np.array_equal(lnl, want_lnl) and np.abs(want_spec).max() > 1.0
    tenfold = [mol.transition(t.nu, t.e_up, t.g_up, 10.0 * t.a_ul, name=t.name) for t in ks[2:]]
    rows_ten = [[rows[0][0], rows[0][1], NOISE, mol.band(ks[:2] + tenfold)], rows[1]]
    want_spec, want_lnl = engine.LteRunner.from_data(rows_ten, None, ncomp=2).predict_batch(theta4)
    theta5[:, 8:] += 1.0
    spec, lnl = mixed.predict_batch(theta5)
    assert max(_check_spec(sp, ws, mode, th[2:4]) for sp, ws, th in zip(spec, want_spec, theta4)) < TIGHT[mode]
    np.testing.assert_allclose(lnl, want_lnl, rtol=LNL_RTOL[mode])


# ---------------------------------------------------------------------------- other configurations
def _compare(engine, nfo, mode, species, tables, ncomp, seed, n=40):
    """predict_batch of a mix runner on `tables` against the restatement for n drawn parameter rows; (runner, rows, thetas, spectra, lnL)."""
    mol, ks, iso, isos = mr.test_species(engine)
    rows = _rows(tables, seed=seed)
    rng = np.random.default_rng(seed + 1)
    thetas = np.stack([draw_params(rng, ncomp, mol, iso, k, n_species=len(species)) for k in range(n)])
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    run = engine.LteMix(species).Runner.from_data(rows, None, ncomp=ncomp)
    assert run.n_model == 3 + len(species) and run.ndim == run.n_model * ncomp
    spec, lnl = run.predict_batch(thetas)
    worst = 0.0
    for sp, ll, th in zip(spec, lnl, thetas):
        ws, wl = mr.restated(nfo, rows, species, th, tbgs)
        worst = max(worst, _check_spec(sp, ws, mode, _tex_of(th, len(species))))
        assert ll == pytest.approx(wl, rel=LNL_RTOL[mode])
    assert worst < TIGHT[mode] and np.abs(spec).max() > 1.0
    return run, rows, thetas, spec, lnl


@pytest.mark.parametrize('mode', MODES)
def test_four_species_on_one_spectrum(engine, nfo, mode, mode_guard):
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    (m3, t3), (m4, t4) = mr.made_up_species(engine, ks[0].nu)
    _compare(engine, nfo, mode, (mol, iso, m3, m4), (engine.LteBlend([ks[0], t4, isos[0], ks[1], t3, isos[1], ks[2]]),), 2, seed=31)
    # ... and over two spectra, of which neither has all four
    _compare(engine, nfo, mode, (mol, iso, m3, m4), (engine.LteBlend([ks[0], t3, ks[3]]), engine.LteBlend([t4, isos[0], isos[2]])), 1, seed=33)


@pytest.mark.parametrize('mode', MODES)
def test_the_reference_transition_of_either_species_and_the_species_in_either_order(engine, nfo, mode, mode_guard):
    """The window's lowest lower level is the iso K = 0's.  With the species listed (top, iso) the reference transition g = 0
    is of species 1 and takes the factor; listed (iso, top) it is of species 0.  The two orders with the column densities
    permuted are one model but not one sequence of operations -- the set-up stage forms the reference optical depth from
    another column and table, and the factor lands on the other ladder -- so they agree to TIGHT, not to the bit."""
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    tables = (engine.LteBlend(ks + isos), ks[3])
    run, rows, thetas, spec, lnl = _compare(engine, nfo, mode, (mol, iso), tables, 2, seed=41)
    other, _, _, _, _ = _compare(engine, nfo, mode, (iso, mol), tables, 2, seed=41, n=4)
    swapped = np.concatenate([thetas[:, :4], thetas[:, 8:10], thetas[:, 6:8], thetas[:, 4:6]], axis=1)
    spec_o, lnl_o = other.predict_batch(swapped)
    assert max(_check_spec(a, b, mode, th[2:4]) for a, b, th in zip(spec_o, spec, thetas)) < TIGHT[mode]
    np.testing.assert_allclose(lnl_o, lnl, rtol=LNL_RTOL[mode])
    # the transitions of the window in three other orders: the engine sorts them, the same bits
    for order in ((6, 5, 4, 3, 2, 1, 0), (2, 0, 5, 3, 6, 1, 4), (4, 1, 3, 0, 6, 2, 5)):
        blend = engine.LteBlend([(ks + isos)[k] for k in order])
        rows_o = [[rows[0][0], rows[0][1], NOISE, blend], rows[1]]
        spec_p, lnl_p = engine.LteMix((mol, iso)).Runner.from_data(rows_o, None, ncomp=2).predict_batch(thetas)
        assert np.array_equal(spec_p, spec) and np.array_equal(lnl_p, lnl), order


@pytest.mark.parametrize('mode', MODES)
def test_a_blend_of_thirty_three_lines_and_four_components(engine, nfo, mode, mode_guard):
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    wide = engine.LteBlend(list(wide_band(mol, ks)) + isos)                        # more than 26 lines: the wide forms
    assert wide.n_lines == 33
    _compare(engine, nfo, mode, (mol, iso), (wide, isos[1]), 2, seed=51, n=16)
    _compare(engine, nfo, mode, (mol, iso), (engine.LteBlend(ks + isos),), 4, seed=53, n=24)      # the general NCOMP form


# ---------------------------------------------------------------------------- routes
@pytest.mark.parametrize('mode', MODES)
def test_the_same_bits_on_every_route(engine, nfo, mode, mode_guard):
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    species = (mol, iso)
    mix = engine.LteMix(species)
    rng = np.random.default_rng(83)
    ut = _simple_priors(engine, RANGES)
    rows = _rows((engine.LteBlend(ks + isos), isos[1]), seed=3)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    run = mix.Runner.from_data(rows, ut, ncomp=2)
    # host and device batches, coalescing on and off, single points and a handful: these take the batch path
    U, theta, lnl = _routes(engine, run, rng)
    for k in (0, 100, 512):
        assert lnl[k] == pytest.approx(mr.restated(nfo, rows, species, theta[k], tbgs)[1], rel=LNL_RTOL[mode])
    plan_split = run.loglikelihood(U[7].copy())
    assert plan_split == lnl[7]
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
    assert _check_spec(spec[3], mr.restated(nfo, rows, species, theta[3], tbgs)[0], mode, theta[3][2:4]) < TIGHT[mode]
    # a noise per channel, with masked channels
    chan = [rng.uniform(0.1, 0.3, N_CHAN) for _ in rows]
    for s in chan:
        s[rng.integers(0, N_CHAN, 5)] = np.inf
    rows_c = [[x, d, s, t] for (x, d, _, t), s in zip(rows, chan)]
    run_c = mix.Runner.from_data(rows_c, ut, ncomp=2)
    _, theta_c, lnl_c = _routes(engine, run_c, rng, n_rows=256)
    for k in (0, 100, 255):
        pred = mr.restated(nfo, rows, species, theta_c[k], tbgs)[0]
        want = sum(-np.sum(((d - pred[i * N_CHAN:(i + 1) * N_CHAN]) / s)[np.isfinite(s)] ** 2) / 2 for i, (_, d, s, _) in enumerate(rows_c))
        assert lnl_c[k] == pytest.approx(want, rel=LNL_RTOL[mode])
    # a baseline of order 1: the same bits on every route, and never a worse fit than without one
    run_b = mix.Runner.from_data(rows, ut, ncomp=2, baseline_order=1)
    Ub, _, lnl_b = _routes(engine, run_b, rng, n_rows=256)
    plain = run.loglikelihood_batch(Ub.copy())
    assert (lnl_b >= plain - 1e-9 * np.abs(plain)).all() and (lnl_b > plain).any()


@pytest.mark.parametrize('mode', MODES)
def test_every_batch_of_a_coalesced_group_reads_its_own_theta(engine, mode, mode_guard):
    """lte_mix_kernel takes the column densities of item b from grp.U[group_of(b)] at row b - c each: the one thing in it that
    depends on the route.  Device batches of ONE shape (whole set-up groups: they are held and launched together at
    coalesce 8, one by one at 1), each with its lncol2 in another part of the prior -- a kernel that read batch 0's theta for
    everybody, or row b of a later batch, would give other bits -- and EVERY batch against the host call on the same rows,
    theta and lnL bit for bit.  Two pixels of a cube runner as well, so that the pixel arrays of the group are in play."""
    from nestfit_amd import _ffi
    from nestfit_amd.cube import CubeRunner
    from test_device_batches import _run_on_device
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    mix = engine.LteMix((mol, iso))
    ut = _simple_priors(engine, RANGES)
    rows = _rows((engine.LteBlend(ks + isos), isos[1]), seed=61)
    rng = np.random.default_rng(62)
    for ncomp, each, n_batch in ((2, 256, 5), (1, 64, 8), (3, 128, 3)):
        run = mix.Runner.from_data(rows, ut, ncomp=ncomp)
        batches = []
        for k in range(n_batch):
            U = rng.uniform(size=(each, run.ndim))
            U[:, 4 * ncomp:] = (k + rng.uniform(size=(each, ncomp))) / n_batch      # lncol2: the k-th part of its prior's range
            batches.append((None, U))
        want = []
        for _, U in batches:
            theta = U.copy()
            want.append((theta, run.loglikelihood_batch(theta)))
        assert len({w[1].tobytes() for w in want}) == n_batch and all(np.isfinite(w[1]).all() for w in want)
        # the column density matters: batch 1's rows with batch 0's lncol2 have another lnL
        crossed = batches[1][1].copy()
        crossed[:, 4 * ncomp:] = batches[0][1][:, 4 * ncomp:]
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
    cube = CubeRunner([x, x], None, data, np.full((2, 2), NOISE), ut, ncomp=2, model=4, lines=[r[3] for r in rows], species=mix.species)
    batches = []
    for k in range(4):
        U = rng.uniform(size=(128, cube.ndim))
        U[:, 8:] = (k + rng.uniform(size=(128, 2))) / 4
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
    """A PriorTransformer over the 3 + K parameters: theta against the priors' host transform, lnL against the restatement
    at the engine's theta."""
    engine.set_exp_mode(mode)
    mol, ks, iso, isos = mr.test_species(engine)
    rng = np.random.default_rng(78)
    ut = _simple_priors(engine, RANGES)
    ps = nfo.PriorSet(ut.lower())
    rows = _rows((engine.LteBlend(ks + isos), isos[0]), seed=6)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    for ncomp in (1, 2):
        run = engine.LteMix((mol, iso)).Runner.from_data(rows, ut, ncomp=ncomp)
        U = rng.uniform(size=(N_ROWS, 5 * ncomp))
        theta = U.copy()
        lnl = run.loglikelihood_batch(theta)
        for k in range(0, N_ROWS, 8):
            want_theta = U[k].copy()
            ps.transform(want_theta, ncomp)
            np.testing.assert_allclose(theta[k], want_theta, rtol=1e-12, atol=1e-13)
            assert lnl[k] == pytest.approx(mr.restated(nfo, rows, (mol, iso), theta[k], tbgs)[1], rel=LNL_RTOL[mode])
    with pytest.raises(engine.EngineError, match='prior program'):                 # four priors for five parameters
        engine.LteMix((mol, iso)).Runner.from_data(rows, _simple_priors(engine, RANGES[:4]), ncomp=1)


# ---------------------------------------------------------------------------- refusals
def test_the_resident_kernel_refuses_a_mix_runner(engine, mode_guard):
    from nestfit_amd.ring import RingServer
    mol, ks, iso, isos = mr.test_species(engine)
    run = engine.LteMix((mol, iso)).Runner.from_data(_rows((engine.LteBlend(ks + isos),), seed=2), _simple_priors(engine, RANGES), ncomp=1)
    with RingServer(f'nfa_test_ring_mix_{os.getpid()}', n_slots=1, runner=run) as server:
        with pytest.raises(engine.EngineError, match='no form for LTE bands: use nfa_ring_serve'):
            server.serve_device(lifetime_ms=20, idle_ms=100)
    u = np.full(5, 0.5)                                               # ... and a single point takes the batch path
    assert np.isfinite(run.loglikelihood(u))


def _create_mix(lib, n_trans=(2,), n_lines=(1, 1), nus=(1e11, 1.00001e11), voff=(0.0, 0.0), wts=(1.0, 1.0), e_up=(4.0, 9.0),
                g_up=(3.0, 5.0), a_ul=(1e-5, 2e-5), n_species=2, species=(0, 1), n_q=(3, 2), q_temp=(5.0, 10.0, 20.0, 6.0, 30.0),
                q_val=(2.0, 4.0, 9.0, 3.0, 20.0), noise='scalar', n=64):
    from nestfit_amd import _ffi
    n_spec = len(n_trans)
    xs = [np.linspace(1e11, 1.0001e11, n) for _ in range(n_spec)]
    xp = (_ffi._dp * n_spec)(*[_ffi.dptr(x) for x in xs])
    sizes = np.full(n_spec, n, dtype=np.int64)
    n_trans, n_lines, species, n_q = (np.asarray(a, dtype=np.int32) for a in (n_trans, n_lines, species, n_q))
    nus, voff, wts, e_up, g_up, a_ul, q_temp, q_val = (np.ascontiguousarray(a, dtype=np.float64)
                                                       for a in (nus, voff, wts, e_up, g_up, a_ul, q_temp, q_val))
    data = np.zeros((1, n * n_spec))
    sc, ch = np.full((1, n_spec), 0.1), np.full((1, n * n_spec), 0.1)
    h = C.c_void_p()
    ip = lambda a: a.ctypes.data_as(_ffi._ip)
    rc = lib.nfa_specset_create_lte_mix(C.byref(h), n_spec, sizes.ctypes.data_as(_ffi._lp), ip(n_trans), ip(n_lines), _ffi.dptr(nus),
                                        _ffi.dptr(voff), _ffi.dptr(wts), _ffi.dptr(e_up), _ffi.dptr(g_up), _ffi.dptr(a_ul),
                                        n_species, ip(species), ip(n_q), _ffi.dptr(q_temp), _ffi.dptr(q_val), xp, 1, _ffi.dptr(data),
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
    assert _create_mix(lib)[0] == 0 and _create_mix(lib, noise='channel')[0] == 0
    one = dict(n_species=1, species=(0, 0), n_q=(3,), q_temp=(5.0, 10.0, 20.0), q_val=(2.0, 4.0, 9.0))
    assert _create_mix(lib, **one)[0] == 0                                                 # nfa_specset_create_lte_bands' set
    same = dict(nus=(1e11, 1e11), e_up=(4.0, 4.0), g_up=(3.0, 3.0), a_ul=(1e-5, 1e-5))
    assert _create_mix(lib, **same)[0] == 0                                                # the same numbers, two species
    four = dict(n_trans=(4,), n_lines=(1,) * 4, nus=1e11 + 1e5 * np.arange(4), voff=(0.0,) * 4, wts=(1.0,) * 4, e_up=4.0 + np.arange(4),
                g_up=(3.0,) * 4, a_ul=(1e-5,) * 4, n_species=4, species=(3, 1, 0, 2), n_q=(2, 2, 2, 2),
                q_temp=(5.0, 10.0) * 4, q_val=(2.0, 4.0) * 4)
    assert _create_mix(lib, **four)[0] == 0
    two_spectra = dict(n_trans=(1, 1))                                                     # a species per spectrum: one transition each
    assert _create_mix(lib, **two_spectra)[0] == 0
    bad = [
        (dict(n_species=0), 'n_species must be in 1..4'), (dict(n_species=5), 'n_species must be in 1..4'),
        (dict(species=(0, 2)), 'species index'), (dict(species=(-1, 1)), 'species index'),
        (dict(species=(0, 0)), 'species 1'), (dict(species=(1, 1)), 'without a transition'),
        ({**four, 'species': (3, 1, 0, 1)}, 'species 2'),
        ({**same, 'species': (1, 1), 'n_trans': (2, 1), 'n_lines': (1, 1, 1), 'nus': (1e11, 1e11, 1e11), 'voff': (0.0,) * 3, 'wts': (1.0,) * 3,
          'e_up': (4.0,) * 3, 'g_up': (3.0,) * 3, 'a_ul': (1e-5,) * 3, 'species': (1, 1, 0)}, 'twice'),
        (dict(n_q=(3, 1)), '2..64 entries (species 1)'), (dict(n_q=(65, 2)), '2..64 entries (species 0)'),
        (dict(q_temp=(5.0, 10.0, 20.0, 30.0, 30.0)), 'ascending (species 1)'), (dict(q_val=(2.0, 0.0, 9.0, 3.0, 20.0)), 'positive (species 0)'),
        (dict(q_val=(2.0, 4.0, 9.0, 3.0, np.nan)), 'species 1'),
        # the bands creator's checks, per transition
        (dict(n_trans=(0,)), '1..8 transitions'), (dict(n_trans=(9,)), '1..8 transitions'),
        (dict(n_lines=(26, 25), voff=np.zeros(51), wts=np.concatenate([np.full(26, 1 / 26), np.full(25, 1 / 25)])), 'at most 50 lines'),
        (dict(e_up=(4.0, -9.0)), 'energy'), (dict(e_up=(np.nan, 9.0)), 'spectrum 0, transition 0'), (dict(g_up=(3.0, 0.0)), 'weight'),
        (dict(a_ul=(1e-5, np.inf)), 'Einstein'), (dict(wts=(1.0, 0.9)), 'sum to 1'), (dict(wts=(1.0, 0.9)), 'transition 1'),
        (dict(n_lines=(1, 0), voff=(0.0,), wts=(1.0,)), 'lines'), (dict(nus=(1e11, 0.0)), 'rest frequency'),
        (dict(voff=(0.0, np.nan)), 'velocity offset'), (dict(wts=(1.0, -1.0)), 'weight'),
        (dict(noise='none'), 'exactly one'), (dict(noise='both'), 'exactly one'),
    ]
    for kw, word in bad:
        rc, msg = _create_mix(lib, **kw)
        assert rc == ERR_ARG and word in msg, (kw, rc, msg)


def test_what_does_not_fit_the_sampler_is_refused_with_a_message(engine, mode_guard):
    """Seven parameters and ten components: the batch kernels take the 70 dimensions, the device sampler holds 60."""
    mol, ks, iso, isos = mr.test_species(engine)
    (m3, t3), (m4, t4) = mr.made_up_species(engine, ks[0].nu)
    rows = _rows((engine.LteBlend([ks[0], isos[0], t3, t4]),), seed=1)
    ut7 = _simple_priors(engine, RANGES + [(11.0, 15.0), (11.0, 15.0)])
    big = engine.LteMix((mol, iso, m3, m4)).Runner.from_data(rows, ut7, ncomp=10)
    assert big.ndim == 70 and np.isfinite(big.loglikelihood_batch(np.full((3, 70), 0.5))).all()
    from nestfit_amd import sampler
    with pytest.raises(engine.EngineError, match='too many dimensions'):
        sampler.run_multinest(big, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=1)      # (more live points than dimensions)


# ---------------------------------------------------------------------------- sampling
TRUTH_FIT = np.array([0.4, 24.0, 15.5, 0.6, 13.9])                  # voff, tex, lncol, sigm, lncol2
FIT_RANGES = [(-3, 3), (6.0, 60.0), (13.5, 16.5), (0.2, 1.5), (12.0, 15.0)]


def test_run_multinest_recovers_tex_and_both_column_densities(engine, nfo, mode_guard):
    """One component on ONE blended spectrum: the main ladder thick, the isotopologue thin -- the thin ladder fixes the
    optical depth the thick one cannot."""
    from nestfit_amd import sampler
    mol, ks, iso, isos = mr.test_species(engine)
    mix = engine.LteMix((mol, iso))
    blend = engine.LteBlend(ks + isos)
    tau = mix.tau_main(blend, TRUTH_FIT[1], [TRUTH_FIT[2], TRUTH_FIT[4]], TRUTH_FIT[3])
    print(f'tau_main of the transitions: {tau}')
    assert tau[:2].min() > 3.0 and 0.02 < tau[4:].min() and tau[4:].max() < 0.5        # main K = 0, 1 thick, the isotopologue thin
    rng = np.random.default_rng(17)
    noise = 0.02
    x = band_axis(ks[0].nu)
    data = mr.mix_predict(nfo, x, hfr.tbg_of(nfo, x), blend, (mol, iso), TRUTH_FIT) + rng.normal(0, noise, N_CHAN)
    run = mix.Runner.from_data([[x, data, noise, blend]], _simple_priors(engine, FIT_RANGES), ncomp=1)
    res = sampler.run_multinest(run, sampler.Dumper(sampler.MemoryGroup()), nlive=100, seed=5)
    mean, std = res.param_constr[0], res.param_constr[1]
    print(f'lnZ - null_lnZ = {res.lnZ - run.null_lnZ:.1f}; mean {mean}, std {std}, truth {TRUTH_FIT}')
    assert res.lnZ - run.null_lnZ > 11
    for k in (1, 2, 4):
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])
    assert std[1] < 5.0 and std[2] < 0.3 and std[4] < 0.3               # all three are constrained, not the priors' widths


def test_cube_route_on_the_device(engine, nfo, tmp_path, mode_guard):
    """A 4 x 4 cube of one blended spectrum: fit_cube, the store with its species, the map products."""
    from nestfit_amd import postprocess as pp
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    mol, ks, iso, isos = mr.test_species(engine)
    mix = engine.LteMix((mol, iso))
    blend = engine.LteBlend(ks + isos, name='J=5-4')
    rng = np.random.default_rng(31)
    n_side, noise = 4, 0.02
    truths = np.stack([rng.uniform(-1, 1, 16), rng.uniform(18.0, 30.0, 16), rng.uniform(15.2, 15.6, 16), rng.uniform(0.4, 0.8, 16),
                       rng.uniform(13.6, 14.0, 16)], axis=1)
    x = band_axis(ks[0].nu)
    tbg = hfr.tbg_of(nfo, x)

    def cube_of(lines, seed=1):
        data = np.random.default_rng(seed).normal(0, noise, (N_CHAN, n_side, n_side))
        for k, th in enumerate(truths):
            data[:, k // n_side, k % n_side] += mr.mix_predict(nfo, x, tbg, blend, (mol, iso), th)
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n_side, 'NAXIS2': n_side, 'NAXIS3': N_CHAN,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': ks[0].nu}
        return DataCube(SimpleCube(hdr, data), noise, lines=lines)
    stack = CubeStack([cube_of(blend)])
    fitter = CubeFitter(stack, _simple_priors(engine, FIT_RANGES), mix.Runner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 60, 'tol': 1.0, 'seed': 5}, nlive_snr_fact=0)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (4, 5, {})
    runner, _, _ = stack.to_device(None, ncomp=1, model=4, species=mix.species)
    assert (runner.n_model, runner.ndim) == (5, 5)
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'lte_mix' and int(store.hdf.attrs['n_params']) == 5
        assert store.read_model_lines(with_species=True) == ([blend], (mol, iso))
        groups = list(store.iter_pix_groups())
        assert len(groups) == 16 and all(g.attrs['nbest'] == 1 for g in groups)
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6))
        peak = np.asarray(store.hdf[f'{store.dpath}/peak_intensity'])              # (t, m, b, l)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])                    # (m, p, b, l)
        spec = np.asarray(store.hdf[f'{store.dpath}/model_spec/spec0'])            # (m, S, b, l)
        assert peak.shape == (1, 1, 4, 4) and np.isfinite(peak).all() and spec.shape == (1, N_CHAN, 4, 4) and pmap.shape[1] == 5
        predict = pp._device_predictor(store, stack)                               # table mode, like the products
        xs = stack.cubes[0].xarr                                                   # the axis the header gives: not x to the bit
        rows, tbgs = [[xs, np.zeros(N_CHAN), 1.0, blend]], [hfr.tbg_of(nfo, xs)]
        worst = 0.0
        for l in range(4):
            for b in range(4):
                th = np.ascontiguousarray(pmap[0, :, b, l])
                truth = truths[b * n_side + l]                                     # (truth k sits at lat k // 4, lon k % 4)
                assert abs(th[0] - truth[0]) < 0.3 and abs(th[1] - truth[1]) < 8.0 and abs(th[2] - truth[2]) < 0.5 and abs(th[4] - truth[4]) < 0.3
                got, _, _ = predict(np.array([l]), np.array([b]), th[None, :], True)
                worst = max(worst, _check_spec(got[0], mr.restated(nfo, rows, (mol, iso), th, tbgs)[0], 'table', th[1:2]))
                assert np.array_equal(spec[0, :, b, l], got[0].astype(np.float32)) and peak[0, 0, b, l] == got[0].max()
        assert worst < TIGHT['table']
    # a stack whose transitions differ from the store's is refused: by the check and by the device predictor
    with HdfStore(path) as store:
        swapped = engine.LteBlend([iso.transition(*_trans(t)) for t in ks] + [mol.transition(*_trans(t)) for t in isos])
        for lines in (engine.LteBlend(ks + isos[:2]), engine.LteBlend(isos + ks), swapped, mol.band(ks)):
            other = CubeStack([cube_of(lines)])
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp._device_predictor(store, other)
