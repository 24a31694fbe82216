"""The set-up stage's overlapped flow (setup_body, nfa_setup.h; option "setup_overlap"): the velocities of a resolved
prior run beside the partition sums and the derived records instead of before them.  The flow moves no operation to
other operands, so everything the stage hands on -- theta, and through the derived records lnL and the spectra -- must
have the bits of the flow with the phases in sequence (option 0), on every path: whole and partial groups of 64 rows,
one row through the point kernel, the table mode's two-group instance, coalesced device-pointer batches, the predict
path (no priors), the sibling models' records, and a prior program that must keep the old flow.

Shapes are small: two NH3 spectra, (1,1) and (2,2), of 128 channels, one pixel."""
import contextlib
import ctypes as C

import numpy as np
import pytest
from scipy import stats

from device_buffers import DeviceArrays
from nestfit_amd.synth import freq_axis

pytestmark = pytest.mark.gpu

MODES = ['table', 'fast']
LNL_RTOL = {'table': 1e-9, 'fast': 1e-6}             # test_gpu_parity.LNL_RTOL
N_CHAN = 128
ROWS = [192, 100, 1]      # three whole groups of 64; a partial group; the point kernel
CKMS = 299792.458


@contextlib.contextmanager
def engine_state(engine, mode):
    """Exp mode `mode` for the block; afterwards the mode before it and the option's default."""
    from nestfit_amd import _ffi
    before = _ffi.load().nfa_get_exp_mode()
    try:
        engine.set_exp_mode(mode)
        yield
    finally:
        _ffi.set_option('setup_overlap', 1)
        engine.set_exp_mode(before)


def on_against_off(call):
    """`call()` -> arrays, with the option 0 and then 1; asserts the same bits and returns those of 1."""
    from nestfit_amd import _ffi
    _ffi.set_option('setup_overlap', 0)
    off = call()
    _ffi.set_option('setup_overlap', 1)
    on = call()
    for k, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f'output {k} differs between setup_overlap 1 and 0'
    return on


def loglike_and_predict(run, U):
    """theta, lnL of unit-cube rows U, and the spectra and lnL predict_batch makes of that theta (no priors there)."""
    theta = U.copy()
    lnl = run.loglikelihood_batch(theta)
    spec, lnl_p = run.predict_batch(theta)
    return theta, lnl, spec, lnl_p


def nh3_args(rng):
    return [[freq_axis(t, N_CHAN), rng.normal(0, 0.2, N_CHAN), 0.2, t] for t in (1, 2)]


_NH3 = {}


def nh3_runner(engine, kind, ncomp):
    """AmmoniaRunner over the two spectra: 'irdc' (placement), 'synth' (resolved centre and separation, duplicate; cold,
    lte) or 'shared' (placement in a program whose priors share a slot: not parallel, so the old flow)."""
    key = (kind, ncomp)
    if key not in _NH3:
        args = nh3_args(np.random.default_rng(7))
        if kind == 'irdc':
            run = engine.AmmoniaRunner.from_data(args, engine.get_irdc_priors(size=200), ncomp=ncomp)
        elif kind == 'synth':
            run = engine.AmmoniaRunner.from_data(args, engine.get_synth_priors(size=200), ncomp=ncomp, cold=True, lte=True)
        else:
            u = np.linspace(0, 1, 200)
            d_v = engine.Distribution(8 * u - 4, stats.beta(5, 5).pdf(u))
            d_s = engine.Distribution(2 * u + 0.067, stats.beta(1.5, 5).pdf(u))
            d_t = engine.Distribution(23 * u + 7, stats.beta(3, 6.7).pdf(u))
            d_x = engine.Distribution(9.26 * u + 2.8, stats.beta(1, 2.5).pdf(u))
            # slot 3 is written twice (the later constant stands); slot 5, orth, keeps its unit-cube value
            ut = engine.PriorTransformer(np.array([
                engine.ResolvedPlacementPrior(engine.Prior(d_v, 0), engine.Prior(d_s, 4), scale=1.2),
                engine.Prior(d_t, 1), engine.Prior(d_x, 2), engine.ConstantPrior(13.5, 3), engine.ConstantPrior(14.5, 3)],
                dtype=object))
            assert ut.n_param == 6
            run = engine.AmmoniaRunner.from_data(args, ut, ncomp=ncomp)
        _NH3[key] = run
    return _NH3[key]


@pytest.fixture(scope='module', autouse=True)
def _release_runners():
    yield
    _NH3.clear()


def unit_rows(B, ndim, seed=3):
    U = np.random.default_rng(seed).uniform(size=(B, ndim))
    if B > 2:                                    # the corners of the unit cube, as test_gpu_parity draws them, in the last
        U[-2] = 0.0                              # two rows (three components placed at the upper corner: not a number, in
        U[-1] = np.nextafter(1.0, 0)             # the reference too; the bits are compared all the same)
    return U


def finite(*arrays):
    """Whether the rows drawn inside the unit cube (all but unit_rows' two corners) are finite in every array."""
    return all(np.isfinite(a if a.shape[0] <= 2 else a[:-2]).all() for a in arrays)


# (the smallest case stands first: one row, one component, through the point kernel)
@pytest.mark.parametrize('B', sorted(ROWS))
@pytest.mark.parametrize('ncomp', [1, 2, 3])
@pytest.mark.parametrize('mode', MODES)
def test_placement_prior(engine, mode, ncomp, B):
    """get_irdc_priors: ResolvedPlacementPrior on the velocities with the widths as its sub-prior."""
    run = nh3_runner(engine, 'irdc', ncomp)
    U = unit_rows(B, run.ndim)
    with engine_state(engine, mode):
        theta, lnl, spec, lnl_p = on_against_off(lambda: loglike_and_predict(run, U))
    assert finite(theta, lnl)
    assert np.array_equal(lnl, lnl_p, equal_nan=True)
    # the program did run: velocities inside the prior's range and in ascending order of component
    v = theta[:-2, :ncomp] if B > 2 else theta[:, :ncomp]
    assert (v >= -4).all() and (v <= 4).all() and (np.diff(v, axis=1) >= 0).all()


@pytest.mark.parametrize('B', sorted(ROWS))
@pytest.mark.parametrize('ncomp', [1, 2])
@pytest.mark.parametrize('mode', MODES)
def test_resolved_censep_and_duplicate_priors(engine, mode, ncomp, B):
    """get_synth_priors with cold and lte: ResolvedCenSepPrior (defined for one and two components), DuplicatePrior."""
    run = nh3_runner(engine, 'synth', ncomp)
    U = unit_rows(B, run.ndim, seed=5)
    with engine_state(engine, mode):
        theta, lnl, spec, lnl_p = on_against_off(lambda: loglike_and_predict(run, U))
    assert finite(theta, lnl)
    assert np.array_equal(lnl, lnl_p, equal_nan=True)
    assert np.array_equal(theta[:, ncomp:2 * ncomp], theta[:, 2 * ncomp:3 * ncomp], equal_nan=True)       # the duplicate


@pytest.mark.parametrize('B', sorted(ROWS))
@pytest.mark.parametrize('mode', MODES)
def test_program_that_is_not_parallel_keeps_the_old_flow(engine, mode, B):
    """Two priors write slot 3: the priors of such a program run one after the other in one lane per row, and the
    option changes nothing."""
    run = nh3_runner(engine, 'shared', 2)
    U = unit_rows(B, run.ndim, seed=9)
    with engine_state(engine, mode):
        theta, lnl, spec, lnl_p = on_against_off(lambda: loglike_and_predict(run, U))
    assert (theta[:, 6:8] == 14.5).all()                          # the later prior of slot 3 stands
    assert np.array_equal(theta[:, 10:12], U[:, 10:12])           # no prior on slot 5
    assert finite(lnl) and np.array_equal(lnl, lnl_p, equal_nan=True)


@pytest.mark.parametrize('mode', MODES)
def test_predict_path_without_priors(engine, mode):
    """has_prior 0: parameters in, spectra and lnL out, the same whatever the option says."""
    run = nh3_runner(engine, 'irdc', 2)
    rng = np.random.default_rng(13)
    theta = np.concatenate([rng.uniform(-4, 4, (100, 2)), rng.uniform(7, 30, (100, 2)), rng.uniform(2.8, 12, (100, 2)),
                            rng.uniform(12.5, 16.5, (100, 2)), rng.uniform(0.067, 2.067, (100, 2)),
                            rng.uniform(0, 0.5, (100, 2))], axis=1)
    with engine_state(engine, mode):
        spec, lnl = on_against_off(lambda: run.predict_batch(theta))
    assert spec.shape == (100, 2 * N_CHAN) and spec.any() and np.isfinite(lnl).all()


def _sibling_runner(engine, model):
    """N2H+ (voff, tex, ltau, sigm) and Gaussian (voff, sigm, peak) runners whose velocities are placed by a resolved
    prior over the widths: the records of derive_simple_lane."""
    u = np.linspace(0, 1, 200)
    flat = np.ones_like(u) / u.size
    d_v = engine.Distribution(12 * u - 6, stats.beta(5, 5).pdf(u))
    d_s = engine.Distribution(1.4 * u + 0.1, stats.beta(1.5, 5).pdf(u))
    rng = np.random.default_rng(17)
    if model == 'n2hp':
        d_tex = engine.Distribution(17.2 * u + 2.8, flat.copy())
        d_tau = engine.Distribution(2.5 * u - 1.5, flat.copy())
        ut = engine.PriorTransformer(np.array([
            engine.ResolvedPlacementPrior(engine.Prior(d_v, 0), engine.Prior(d_s, 3), scale=1.2),
            engine.Prior(d_tex, 1), engine.Prior(d_tau, 2)], dtype=object))
        v = np.linspace(20.0, -20.0, N_CHAN)
        args = [[nu * (1.0 - v / CKMS), rng.normal(0, 0.15, N_CHAN), 0.15, t]
                for t, nu in ((1, 93173.7637e6), (2, 186344.8420e6))]
        return engine.DiazenyliumRunner.from_data(args, ut, ncomp=2)
    from nestfit_amd import gaussian
    d_pk = engine.Distribution(5.0 * u, flat.copy())
    ut = engine.PriorTransformer(np.array([
        engine.ResolvedPlacementPrior(engine.Prior(d_v, 0), engine.Prior(d_s, 1), scale=1.2),
        engine.Prior(d_pk, 2)], dtype=object))
    nu0 = 110.201354e9
    x = nu0 * (1.0 - np.linspace(30, -30, N_CHAN) / CKMS)
    return gaussian.GaussianRunner.from_data([x, rng.normal(0, 0.3, N_CHAN), 0.3, nu0], ut, ncomp=3)


@pytest.mark.parametrize('model', ['n2hp', 'gauss'])
@pytest.mark.parametrize('mode', MODES)
def test_sibling_models(engine, mode, model):
    run = _sibling_runner(engine, model)
    with engine_state(engine, mode):
        for B in sorted(ROWS):
            U = unit_rows(B, run.ndim, seed=19)
            theta, lnl, spec, lnl_p = on_against_off(lambda: loglike_and_predict(run, U))
            assert finite(theta, lnl) and np.array_equal(lnl, lnl_p, equal_nan=True)
            assert (np.diff(theta[:-2, :run.ncomp] if B > 2 else theta[:, :run.ncomp], axis=1) >= 0).all()


def _loglike_dev(run, batches):
    """The batches (unit-cube rows each) through nfa_runner_loglike_batch_dev one after the other, then one synchronise:
    [theta], [lnL]."""
    from nestfit_amd import _ffi
    lib = _ffi.load()
    dev = DeviceArrays(lib, _ffi.check)
    try:
        d_u = [dev.upload(U) for U in batches]
        d_l = [dev.upload(np.full(U.shape[0], np.nan)) for U in batches]
        for U, pu, pl in zip(batches, d_u, d_l):
            _ffi.check(lib.nfa_runner_loglike_batch_dev(run._run.handle, None, pu, pl, U.shape[0]))
        _ffi.check(lib.nfa_runner_synchronize(run._run.handle))
        return [dev.download(p, U) for p, U in zip(d_u, batches)] + [dev.download(p, U[:, 0].copy()) for p, U in zip(d_l, batches)]
    finally:
        dev.free()


@pytest.mark.parametrize('mode', MODES)
def test_three_coalesced_device_batches(engine, mode):
    """Three device-pointer batches of 192 rows held and launched as one group (BatchGroup.n = 3): on against off, and
    the bits of the host call of each batch alone."""
    run = nh3_runner(engine, 'irdc', 2)
    batches = [unit_rows(192, run.ndim, seed=23 + k) for k in range(3)]
    with engine_state(engine, mode):
        got = on_against_off(lambda: _loglike_dev(run, batches))
        for k, U in enumerate(batches):
            theta = U.copy()
            lnl = run.loglikelihood_batch(theta)
            assert np.array_equal(got[k], theta, equal_nan=True) and np.array_equal(got[3 + k], lnl, equal_nan=True)


def test_two_group_table_instance(engine):
    """128 n_cu + 64 rows in one device-pointer call, table mode: more than 64 n_cu rows, so the set-up launch is the
    two-group instance (plan_setup), its last workgroup with one group of 64 rows and one of none.  On against off,
    and a sample of rows against the host call of those rows alone (the one-group instance)."""
    from nestfit_amd import _ffi
    name = C.create_string_buffer(256)
    _ffi.check(_ffi.engine().nfa_device_name(name, 256))
    n_cu = int(name.value.decode().split(',')[-1].split()[0])
    run = nh3_runner(engine, 'irdc', 2)
    B = 128 * n_cu + 64
    U = unit_rows(B, run.ndim, seed=29)
    with engine_state(engine, 'table'):
        theta, lnl = on_against_off(lambda: _loglike_dev(run, [U]))
        sel = np.r_[0:64, B - 100:B]
        sub = U[sel].copy()
        lnl_sub = run.loglikelihood_batch(sub)
    assert np.array_equal(theta[sel], sub, equal_nan=True) and np.array_equal(lnl[sel], lnl_sub, equal_nan=True)
    assert finite(lnl)


@pytest.mark.parametrize('mode', MODES)
def test_overlapped_flow_against_the_oracle(engine, nfo, mode):
    """64 rows of the irdc case with the option on, against the CPU oracle at test_gpu_parity's tolerances."""
    from nestfit_amd import _ffi
    ut = engine.get_irdc_priors()
    args = nh3_args(np.random.default_rng(7))
    gpu = engine.AmmoniaRunner.from_data(args, ut, ncomp=2)
    cpu = nfo.AmmoniaRunner([nfo.AmmoniaSpectrum(*a) for a in args], nfo.PriorSet(ut.lower()), ncomp=2)
    U = unit_rows(64, 12, seed=31)
    Ug, Uc = U.copy(), U.copy()
    with engine_state(engine, mode):
        _ffi.set_option('setup_overlap', 1)
        lg = gpu.loglikelihood_batch(Ug)
    lc = cpu.loglikelihood_batch(Uc)
    np.testing.assert_allclose(Ug, Uc, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(lg, lc, rtol=LNL_RTOL[mode])
