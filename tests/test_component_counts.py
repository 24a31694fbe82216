"""Component counts up to MAXCOMP = 10 (nfa_runner_create: 1..10) against the CPU oracle, and the engine's launch forms
against each other bit for bit.  Counts 1-3 are compiled with the component loop unrolled; every other count takes the
general form (NCOMP == 0) of the likelihood, point and queue kernels.  In the table mode the set-up stage of a runner
with 500-point irdc tables needs more than 160 KiB of LDS from 8 components on, and reads its prior tables from global
memory there (nfa_launch_plan.h: setup_staged).

Safety: at high counts the minimum separations of the placement prior overflow a narrow velocity axis and the
reference's draw is an artefact (NaN centroids among them).  Every unit-cube row is screened on the CPU with the closed
forms (prior_closed_forms.transform must not raise Degenerate) before it reaches a likelihood, predict or sampler
launch; the sampler draws its own rows and runs on a prior set whose draws are never degenerate."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import prior_closed_forms as pcf
from device_buffers import DeviceArrays
from test_closed_forms import irdc_wide_axis
from test_gpu_parity import LNL_RTOL, MODES, TB_ATOL_K, TB_RTOL, TIGHT, _draw_params
from test_sibling_models import CKMS, _simple_priors, n2hp_axis

from nestfit_amd.synth import freq_axis

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
THETA_TOL = dict(rtol=1e-9, atol=1e-10)          # the prior transform's tolerance (test_gpu_parity, test_closed_forms)
N2HP_RANGES = [(-6, 6), (2.8, 20), (-1.5, 1.0), (0.1, 1.5)]
GAUSS_RANGES = [(-20, 20), (0.2, 3.0), (0.0, 5.0)]


@pytest.fixture(autouse=True)
def _options_restored(engine):
    """Every test leaves the engine's defaults behind: fast mode, lnl_queue 1, lnl_split 0, prior_stage 1."""
    from nestfit_amd import _ffi
    try:
        yield
    finally:
        for key, value in (('lnl_queue', 1), ('lnl_split', 0), ('prior_stage', 1)):
            _ffi.set_option(key, value)
        engine.set_exp_mode('fast')


def _wide(engine):
    """irdc-shaped priors with 500-point tables (the same 10 tables staged as get_irdc_priors()) on +-40 km/s, sigma <=
    1 km/s: a fresh transformer, so that its device program is created under the options of the moment."""
    return engine.PriorTransformer(np.array(irdc_wide_axis(engine, size=500), dtype=object))


def usable_rows(ut, ncomp, n, seed, n_draw=None):
    """Up to n unit-cube rows whose prior transform is not Degenerate (checked on the CPU, row by row)."""
    rng = np.random.default_rng(seed)
    priors = list(ut.priors)
    U = rng.uniform(size=(n_draw or 2 * n, 6 * ncomp))
    keep = []
    for k, u in enumerate(U):
        try:
            th = pcf.transform(priors, u, ncomp)
        except pcf.Degenerate:
            continue
        if np.all(np.isfinite(th)):
            keep.append(k)
        if len(keep) == n:
            break
    return U[keep]


def _nh3_pair(engine, nfo, ut, trans, n, ncomp, seed, noise=0.2):
    rng = np.random.default_rng(seed)
    spec_data = [[freq_axis(t, n), rng.normal(0, noise, n), noise, t] for t in trans]
    gpu = engine.AmmoniaRunner.from_data(spec_data, ut, ncomp=ncomp)
    cpu = nfo.AmmoniaRunner([nfo.AmmoniaSpectrum(*sd) for sd in spec_data], nfo.PriorSet(ut.lower()), ncomp=ncomp)
    return gpu, cpu, spec_data


def _check_spec(pg, pc, mode, scale=None):
    """Zero pattern exact, Tb within TB_RTOL of `scale` (default: the oracle's value) + TB_ATOL_K; returns the worst
    relative error over the channels above 1e-6 K."""
    assert np.array_equal(pg == 0, pc == 0)
    scale = np.abs(pc) if scale is None else scale
    assert (np.abs(pg - pc) <= TB_RTOL * scale + TB_ATOL_K[mode]).all()
    big = scale > 1e-6
    return float(np.max(np.abs(pg[big] - pc[big]) / scale[big])) if big.any() else 0.0


def _against_oracle(gpu, cpu, U, mode, what):
    """loglikelihood_batch of both on copies of U: theta to THETA_TOL, and lnL to LNL_RTOL against the oracle's
    likelihood at the engine's own theta.  (At 7 and more components a centroid's 1e-10 km/s -- the placement CDF from
    prefix moments -- moves lnL by up to 3e-9 relative where many narrow lines sit in the band: that is the prior's
    deviation, not the likelihood's.)  Returns the engine's (lnL, theta)."""
    Ug, Uc = U.copy(), U.copy()
    lg, lc = gpu.loglikelihood_batch(Ug), cpu.loglikelihood_batch(Uc)
    assert np.all(np.isfinite(lc)), what
    np.testing.assert_allclose(Ug, Uc, **THETA_TOL, err_msg=f'{what}: theta')
    np.testing.assert_allclose(lg, lc, rtol=10 * LNL_RTOL[mode], err_msg=f'{what}: lnL at the oracle theta')
    np.testing.assert_allclose(lg, _oracle_lnl_at(cpu, Ug), rtol=LNL_RTOL[mode], err_msg=f'{what}: lnL')
    return lg, Ug


def _oracle_lnl_at(cpu, theta):
    """The oracle's lnL at given physical parameters: the sum of its spectra's likelihoods after predict."""
    out = np.empty(len(theta))
    for k, th in enumerate(theta):
        cpu.predict(np.ascontiguousarray(th))
        out[k] = sum(s.loglikelihood for s in cpu.spectra)
    return out


# ------------------------------------------------------------------------------------------------------ a. predict grid
@pytest.mark.parametrize('mode', MODES)
def test_predict_grid_four_to_ten_components(engine, nfo, mode):
    """amm_predict / nnhp_predict / gauss_predict at 4..10 components (the general form of every kernel): zero pattern
    exact, Tb to TB_RTOL, lnL to LNL_RTOL, the worst relative Tb below TIGHT.  NH3 (1,1), (2,2) and (3,3) (26 lines:
    the narrow form's limit), cold / lte; N2H+ 1-0, and 2-1 and 3-2 (the WIDE kernels); 1024 and 2048 channels."""
    from nestfit_amd import gaussian
    engine.set_exp_mode(mode)
    rng = np.random.default_rng(101)
    worst = 0.0
    for n in (1024, 2048):
        for trans in (1, 2, 3):
            x = freq_axis(trans, n, 40.0 if n == 2048 else 30.0)
            data = rng.normal(0, 0.3, n)
            sg, sc = engine.AmmoniaSpectrum(x, data, 0.3, trans), nfo.AmmoniaSpectrum(x, data, 0.3, trans)
            for ncomp in range(4, 11):
                for cold, lte in ((False, False), (True, False), (False, True), (True, True)):
                    th = _draw_params(rng, ncomp)
                    engine.amm_predict(sg, th, cold=cold, lte=lte)
                    nfo.amm_predict(sc, th, cold=cold, lte=lte)
                    worst = max(worst, _check_spec(sg.get_spec(), sc.get_spec(), mode))
                    assert sg.loglikelihood == pytest.approx(sc.loglikelihood, rel=LNL_RTOL[mode]), (trans, n, ncomp)
        for trans in (1, 2, 3):
            x = n2hp_axis(trans, n, 30.0 if n == 2048 else 20.0)
            data = rng.normal(0, 0.2, n)
            sg, sc = engine.DiazenyliumSpectrum(x, data, 0.2, trans), nfo.DiazenyliumSpectrum(x, data, 0.2, trans)
            for ncomp in range(4, 11):
                for _ in range(2):
                    th = np.concatenate([rng.uniform(-8, 8, ncomp), rng.uniform(2.8, 25, ncomp),
                                         rng.uniform(-2, 1.5, ncomp), 10 ** rng.uniform(-1.3, 0.3, ncomp)])
                    engine.nnhp_predict(sg, th)
                    nfo.nnhp_predict(sc, th)
                    worst = max(worst, _check_spec(sg.get_spec(), sc.get_spec(), mode))
                    assert sg.loglikelihood == pytest.approx(sc.loglikelihood, rel=LNL_RTOL[mode]), (trans, n, ncomp)
        nu0 = 110.201354e9
        x = nu0 * (1.0 - np.linspace(40, -40, n) / CKMS)
        data = rng.normal(0, 0.5, n)
        sg, sc = gaussian.Spectrum(x, data, 0.5, rest_freq=nu0), nfo.Spectrum(x, data, 0.5, rest_freq=nu0)
        for ncomp in range(4, 11):
            for _ in range(3):
                th = np.concatenate([rng.uniform(-45, 45, ncomp), 10 ** rng.uniform(-1.5, 1.0, ncomp),
                                     rng.uniform(-2, 8, ncomp)])
                nfo.gauss_predict(sc, np.concatenate([th[:2 * ncomp], np.abs(th[2 * ncomp:])]))
                scale = sc.get_spec()                # components of opposite sign cancel (test_gauss_predict_grid)
                engine.gauss_predict(sg, th)
                nfo.gauss_predict(sc, th)
                worst = max(worst, _check_spec(sg.get_spec(), sc.get_spec(), mode, scale))
                assert sg.loglikelihood == pytest.approx(sc.loglikelihood, rel=LNL_RTOL[mode]), (n, ncomp)
    print(f'{mode}: worst relative Tb error at 4..10 components {worst:.2e}')
    assert worst < TIGHT[mode], worst


# ------------------------------------------------------------------------------------ b. runners through the set-up stage
@pytest.mark.parametrize('ncomp', range(1, 11))
@pytest.mark.parametrize('mode', MODES)
def test_runner_through_the_setup_stage(engine, nfo, mode, ncomp):
    """loglikelihood_batch (the fused set-up stage, then the likelihood) against nfo.AmmoniaRunner at every count:
    theta and lnL, with the irdc shape on a wide axis (500-point tables, the 10 tables of get_irdc_priors() staged) and
    get_irdc_priors() itself where its draws are usable.  In the table mode 8..10 components do not fit the staged
    layout in LDS (they failed with "too many parameters for the set-up kernel")."""
    engine.set_exp_mode(mode)
    cases = [('wide', _wide(engine), (1, 2, 3), 300)]
    irdc = engine.get_irdc_priors()
    U_irdc = usable_rows(irdc, ncomp, 160, seed=10 + ncomp, n_draw=1500)
    if len(U_irdc) >= 16:                            # (at 10 components about 2 % of the draws fit its 8 km/s axis)
        cases.append(('irdc', irdc, (1, 2), 256))
    for name, ut, trans, n in cases:
        U = usable_rows(ut, ncomp, 160, seed=20 + ncomp) if name == 'wide' else U_irdc
        gpu, cpu, _ = _nh3_pair(engine, nfo, ut, trans, n, ncomp, seed=ncomp)
        lg, Ug = _against_oracle(gpu, cpu, U, mode, f'{mode} {name} ncomp={ncomp}')
        # one row: the point kernel up to ndim 24, the batch kernels beyond -- the batch's bits
        u = U[3].copy()
        assert gpu.loglikelihood(u) == lg[3] and np.array_equal(u, Ug[3]), (name, ncomp)


# ---------------------------------------------------------------------------------------- c. launch forms, bit for bit
def _tiled(U, B):
    return np.ascontiguousarray(np.resize(U, (B, U.shape[1])))


@pytest.mark.parametrize('ncomp', [4, 7, 10])
def test_unit_queue_matches_one_unit_per_wave(engine, nfo, ncomp):
    """Table mode, lnl_kernel_queue<WS, 0> (lnl_queue 1) against one wave per unit (lnl_queue 0): the same bits, theta
    included; a sample against the oracle.  Sized like test_row_split's: 2 * 512 workgroups * 16 waves of units."""
    from nestfit_amd import _ffi
    engine.set_exp_mode('table')
    ut = _wide(engine)
    trans, n = (1, 2), 512
    B = 16384 // len(trans) + 16 * 40 + 1
    U = _tiled(usable_rows(ut, ncomp, 1024, seed=30 + ncomp), B)
    out = {}
    for q in (0, 1):
        _ffi.set_option('lnl_queue', q)
        gpu, cpu, _ = _nh3_pair(engine, nfo, ut, trans, n, ncomp, seed=3)
        Us = U.copy()
        out[q] = (gpu.loglikelihood_batch(Us), Us)
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1])
    pick = np.random.default_rng(3).choice(1024, 200, replace=False)
    Uc = U[pick].copy()
    np.testing.assert_allclose(out[1][1][pick], _copy_transform(cpu, Uc), **THETA_TOL)
    np.testing.assert_allclose(out[1][0][pick], cpu.loglikelihood_batch(U[pick].copy()), rtol=LNL_RTOL['table'])


def _copy_transform(cpu, U):
    cpu.loglikelihood_batch(U)
    return U


@pytest.mark.parametrize('ncomp', [4, 7, 10])
@pytest.mark.parametrize('mode', MODES)
def test_row_split_matches_one_wave_per_unit(engine, nfo, mode, ncomp):
    """lnl_split 2, 4 and 0 (automatic) against 1 at small batches: lnL, theta, predict_batch and one point."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    ut = _wide(engine)
    U = usable_rows(ut, ncomp, 300, seed=40 + ncomp)
    out = {}
    for split in (1, 2, 4, 0):
        _ffi.set_option('lnl_split', split)
        gpu, cpu, _ = _nh3_pair(engine, nfo, ut, (1, 2), 1024, ncomp, seed=4)
        Us = U.copy()
        lnl = gpu.loglikelihood_batch(Us)
        spec, lp = gpu.predict_batch(Us[:32])
        out[split] = (lnl, Us, spec, lp, gpu.loglikelihood(U[0].copy()))
    base = out[1]
    for split in (2, 4, 0):
        lnl, Us, spec, lp, one = out[split]
        assert np.array_equal(Us, base[1]) and np.array_equal(spec, base[2]), (mode, ncomp, split)
        assert np.array_equal(lnl, base[0]) and np.array_equal(lp, base[3]), (mode, ncomp, split)
        assert one == base[4] == lnl[0], (mode, ncomp, split)
    np.testing.assert_allclose(out[4][0], cpu.loglikelihood_batch(U.copy()), rtol=LNL_RTOL[mode])


@pytest.mark.parametrize('ncomp', [4, 7, 10])
@pytest.mark.parametrize('mode', MODES)
def test_prior_stage_zero_gives_the_staged_bits(engine, nfo, mode, ncomp):
    """Priors created under option prior_stage 0 (tables in global memory) against prior_stage 1 (staged in LDS where
    the layout fits): identical theta and lnL, one launch of a few rows and one of two workgroup rounds."""
    from nestfit_amd import _ffi
    engine.set_exp_mode(mode)
    U = usable_rows(_wide(engine), ncomp, 600, seed=50 + ncomp)
    U = np.concatenate([U, _tiled(U, 40000)])
    out = {}
    for stage in (0, 1):
        _ffi.set_option('prior_stage', stage)
        ut = _wide(engine)
        gpu, cpu, _ = _nh3_pair(engine, nfo, ut, (1, 2), 512, ncomp, seed=5)
        res = []
        for rows in (U[:40], U):
            Us = rows.copy()
            res.append((gpu.loglikelihood_batch(Us), Us))
        out[stage] = res
    for (l0, t0), (l1, t1) in zip(out[0], out[1]):
        assert np.array_equal(l0, l1) and np.array_equal(t0, t1), (mode, ncomp)
    np.testing.assert_allclose(out[1][0][0], cpu.loglikelihood_batch(U[:40].copy()), rtol=LNL_RTOL[mode])


@pytest.mark.parametrize('ncomp', [4, 7, 10])
@pytest.mark.parametrize('mode', MODES)
def test_predict_batch_and_coalesced_device_groups(engine, nfo, mode, ncomp):
    """predict_batch of a CubeRunner against three nfa_runner_predict_batch_dev calls, coalesced into one group (the
    engine's default): spectra
    and lnL bit for bit, theta untouched; spectra of a subset against the oracle's amm_predict."""
    from nestfit_amd import _ffi
    from nestfit_amd.cube import CubeRunner
    engine.set_exp_mode(mode)
    ut = _wide(engine)
    trans, n, rows, n_batch = (1, 2), 512, 256, 3
    axes = [freq_axis(t, n) for t in trans]
    rng = np.random.default_rng(60 + ncomp)
    data = rng.normal(0, 0.2, (2, len(trans) * n))
    cube = CubeRunner(axes, trans, data, np.full((2, len(trans)), 0.2), ut, ncomp=ncomp)
    U = usable_rows(ut, ncomp, n_batch * rows, seed=61 + ncomp)
    assert len(U) == n_batch * rows
    batches = []
    for k in range(n_batch):
        pix = rng.integers(0, 2, rows).astype(np.int32)
        theta = U[k * rows:(k + 1) * rows].copy()
        cube.loglikelihood_batch(pix, theta)                 # unit cube -> physical parameters
        batches.append((pix, theta))
    lib = _ffi.load()
    dev = DeviceArrays(lib, _ffi.check)
    try:
        calls = [(dev.upload(pix), dev.upload(theta), dev.empty(8 * rows * cube.n_chan_tot), dev.empty(8 * rows))
                 for pix, theta in batches]
        for d_p, d_t, d_s, d_l in calls:
            _ffi.check(lib.nfa_runner_predict_batch_dev(cube._run.handle, d_p, d_t, rows, d_s, d_l))
        _ffi.check(lib.nfa_runner_synchronize(cube._run.handle))
        got = [(dev.download(d_s, np.empty((rows, cube.n_chan_tot))), dev.download(d_l, np.empty(rows)),
                dev.download(d_t, theta)) for (d_p, d_t, d_s, d_l), (_, theta) in zip(calls, batches)]
    finally:
        dev.free()
    oracle = [[nfo.AmmoniaSpectrum(x, data[p, k * n:(k + 1) * n], 0.2, t) for k, (x, t) in enumerate(zip(axes, trans))]
              for p in range(2)]
    worst = 0.0
    for k, ((pix, theta), (spec, lnl, th_back)) in enumerate(zip(batches, got)):
        want_spec, want_lnl = cube.predict_batch(pix, theta)
        assert np.array_equal(spec, want_spec) and np.array_equal(lnl, want_lnl), (mode, ncomp, k)
        assert np.array_equal(th_back, theta), (mode, ncomp, k)
        for b in range(0, rows, 32):
            tot = 0.0
            for s, sc in enumerate(oracle[pix[b]]):
                nfo.amm_predict(sc, theta[b])
                worst = max(worst, _check_spec(spec[b, s * n:(s + 1) * n], sc.get_spec(), mode))
                tot += sc.loglikelihood
            assert lnl[b] == pytest.approx(tot, rel=LNL_RTOL[mode]), (mode, ncomp, k, b)
    assert worst < TIGHT[mode], worst


def test_the_queue_kernel_runs_at_high_counts(engine):
    """lnl_kernel_queue<WS, 0> is what served the launches of test_unit_queue_matches_one_unit_per_wave at 4, 7 and
    10 components (the test library's queue trace, in a child process of its own)."""
    lib_path = ROOT / 'nestfit_amd' / 'lib' / 'libnestfit_amd_test.so'
    assert lib_path.exists()
    env = dict(os.environ, NFA_ENGINE_LIB=str(lib_path))
    res = subprocess.run([sys.executable, str(ROOT / 'tests' / 'component_queue_worker.py')], env=env, cwd=str(ROOT),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    for ncomp in ('4', '7', '10'):
        assert out[ncomp]['queue'] and out[ncomp]['units_recorded'] > 0, (ncomp, out[ncomp])


# ------------------------------------------------------------------------------------- d. the point kernel's boundary
def _point_cases(engine, nfo):
    from nestfit_amd import gaussian
    rng = np.random.default_rng(70)
    ut = _wide(engine)
    args = [[freq_axis(t, 256), rng.normal(0, 0.2, 256), 0.2, t] for t in (1, 2)]
    yield ('NH3', 4, engine.AmmoniaRunner.from_data(args, ut, ncomp=4),
           nfo.AmmoniaRunner([nfo.AmmoniaSpectrum(*a) for a in args], nfo.PriorSet(ut.lower()), ncomp=4), ut)
    utn = _simple_priors(engine, N2HP_RANGES)
    x = n2hp_axis(1, 400)
    argn = [[x, rng.normal(0, 0.15, 400), 0.15, 1]]
    for ncomp in (6, 7):
        yield ('N2H+ 1-0', ncomp, engine.DiazenyliumRunner.from_data(argn, utn, ncomp=ncomp),
               nfo.DiazenyliumRunner([nfo.DiazenyliumSpectrum(*a) for a in argn], nfo.PriorSet(utn.lower()), ncomp=ncomp),
               None)
    utg = _simple_priors(engine, GAUSS_RANGES)
    nu0 = 110.201354e9
    xg = nu0 * (1.0 - np.linspace(30, -30, 600) / CKMS)
    dg = rng.normal(0, 0.3, 600)
    for ncomp in (8, 9):
        yield ('Gaussian', ncomp, gaussian.GaussianRunner.from_data([xg, dg, 0.3, nu0], utg, ncomp=ncomp),
               nfo.GaussianRunner(nfo.Spectrum(xg, dg, 0.3, rest_freq=nu0), nfo.PriorSet(utg.lower()), ncomp=ncomp), None)


@pytest.mark.parametrize('mode', MODES)
def test_single_points_at_the_point_kernel_boundary(engine, nfo, mode):
    """ndim 24 (NH3 x 4, N2H+ x 6, Gaussian x 8: the point kernel's NFA_POINT_MAXDIM) and just past it (N2H+ x 7,
    Gaussian x 9: the batch path): loglikelihood(u), from the third call on a graph replay, gives the bits of
    loglikelihood_batch, theta included, and both match the oracle."""
    engine.set_exp_mode(mode)
    for name, ncomp, gpu, cpu, ut in _point_cases(engine, nfo):
        assert gpu.ndim == (24 if ncomp in (4, 6, 8) else 28 if name.startswith('N2H+') else 27), (name, gpu.ndim)
        U = usable_rows(ut, ncomp, 12, seed=71) if ut is not None else np.random.default_rng(71).uniform(size=(12, gpu.ndim))
        lg, Ug = _against_oracle(gpu, cpu, U, mode, f'{mode} {name} x {ncomp}')
        for k in range(8):
            u = U[k].copy()
            assert gpu.loglikelihood(u) == lg[k], (mode, name, ncomp, k)
            assert np.array_equal(u, Ug[k]), (mode, name, ncomp, k)


# ------------------------------------------------------------------------------------------ e. channel noise at ten
@pytest.mark.parametrize('mode', MODES)
def test_constant_channel_noise_gives_the_scalar_bits_at_ten_components(engine, mode):
    """A noise array of one constant value per spectrum (the weighted kind, general form) against the scalar noise: theta,
    lnL and predict_batch bit for bit at 10 components."""
    engine.set_exp_mode(mode)
    ut = _wide(engine)
    rng = np.random.default_rng(80)
    trans, n = (1, 2), 512
    axes = [freq_axis(t, n) for t in trans]
    data = [rng.normal(0, 0.2, n) for _ in trans]
    scalar = engine.AmmoniaRunner.from_data([[x, d, 0.2, t] for x, d, t in zip(axes, data, trans)], ut, ncomp=10)
    chan = engine.AmmoniaRunner.from_data([[x, d, np.full(n, 0.2), t] for x, d, t in zip(axes, data, trans)], ut, ncomp=10)
    assert chan.null_lnZ == scalar.null_lnZ
    U = usable_rows(ut, 10, 300, seed=81)
    ts, tc = U.copy(), U.copy()
    ls, lc = scalar.loglikelihood_batch(ts), chan.loglikelihood_batch(tc)
    assert np.all(np.isfinite(ls))
    assert np.array_equal(tc, ts) and np.array_equal(lc, ls)
    ss, lss = scalar.predict_batch(ts[:32])
    sc, lsc = chan.predict_batch(ts[:32])
    assert np.array_equal(sc, ss) and np.array_equal(lsc, lss)
    assert np.array_equal(lsc, ls[:32])


# ----------------------------------------------------------------------------- f. the device sampler's general form
@pytest.mark.parametrize('ncomp', [4, 10])
def test_device_sampler_matches_its_twin_outside_the_specialised_dimensions(engine, nfo, ncomp):
    """ns_propose_kernel<0>: 20 and 50 free dimensions (NS_MAXD at 10 components) on the device against the host
    twin with the same seed, table mode: equal n_iter and n_evals, lnZ to 1e-10, posterior allclose.  The prior set's
    draws are never degenerate (sigma <= 1 km/s on +-40 km/s), and the set-up stage of 10 components reads its prior
    tables from global memory."""
    from nestfit_amd import sampler
    from nestfit_amd.cube import CubeRunner
    engine.set_exp_mode('table')
    ut = _wide(engine)
    assert int(ut.free_mask(ncomp).sum()) == 5 * ncomp
    n_pix, n, noise = 2, 256, 0.15
    axes = [freq_axis(1, n), freq_axis(2, n)]
    rng = np.random.default_rng(90)
    v = np.linspace(-3.0 * ncomp, 3.0 * ncomp, ncomp)
    truths = np.tile(np.concatenate([v, np.full(ncomp, 14.0), np.full(ncomp, 6.0), np.full(ncomp, 14.4),
                                     np.full(ncomp, 0.4), np.zeros(ncomp)]), (n_pix, 1))
    probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * n)), np.full((1, 2), noise), ut, ncomp=ncomp)
    model, _ = probe.predict_batch(np.zeros(n_pix, dtype=np.int32), truths)
    cube = CubeRunner(axes, (1, 2), model + rng.normal(0, noise, model.shape), np.full((n_pix, 2), noise), ut, ncomp=ncomp)
    kw = dict(nlive=100 if ncomp == 4 else 160, tol=0.5, efr=0.3, seed=13, method='reject', maxiter=300)
    dev = sampler.fit_pixels(cube, np.arange(n_pix), device=True, **kw)
    twin = sampler.fit_pixels(cube, np.arange(n_pix), device=False, **kw)
    for d, t in zip(dev, twin):
        assert (d.n_iter, d.n_evals) == (t.n_iter, t.n_evals), (ncomp, d.n_iter, t.n_iter, d.n_evals, t.n_evals)
        assert d.n_evals > 0 and np.isfinite(d.lnZ)
        assert d.lnZ == pytest.approx(t.lnZ, rel=1e-10)
        np.testing.assert_allclose(d.posterior, t.posterior, rtol=1e-8, atol=1e-12)
