"""The ensemble sampler on the device (nfa_ensemble_*) against its numpy twin, decision for decision, and
against the nested sampler, statistically.

Fed by the device's own likelihood the twin sees the very lnL the device sees, so the two runs are equal to the bit unless
the device's `log` and numpy's differ in a decision: only one whose margin |log r_2 - rhs| is of the size of an ulp.  Each
case asserts the twin's smallest margin first; its seed is the first seed >= 1 for which that holds."""
import numpy as np
import pytest

from nestfit_amd import ensemble
from test_sibling_models import MODES, mode_guard          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
N_CHAN, NOISE = 96, 0.15
LD = np.longdouble
U = 2.0 ** -53


def _data(engine, ncomp, n_pix, seed):
    """Synthetic ammonia (1,1)+(2,2) on 2 x 96 channels: (axes, data, utrans)."""
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import TRUTH_1COMP, TRUTH_2COMP, freq_axis
    rng = np.random.default_rng(seed)
    axes = [freq_axis(1, N_CHAN), freq_axis(2, N_CHAN)]
    ut = engine.get_irdc_priors(size=300, vsys=0.0)
    truth = np.repeat((TRUTH_1COMP if ncomp == 1 else TRUTH_2COMP)[None], n_pix, axis=0).copy()
    truth[:, :ncomp] += rng.uniform(-0.5, 0.5, (n_pix, ncomp))
    before = engine.get_exp_mode()
    engine.set_exp_mode('table')
    try:
        probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * N_CHAN)), np.full((1, 2), NOISE), ut, ncomp=ncomp)
        model, _ = probe.predict_batch(np.zeros(n_pix, np.int32), truth)
    finally:
        engine.set_exp_mode(before)
    return axes, model + rng.normal(0, NOISE, model.shape), ut


def _runner(engine, ncomp, n_pix, seed=4, **options):
    from nestfit_amd.cube import CubeRunner
    axes, data, ut = _data(engine, ncomp, n_pix, seed)
    return CubeRunner(axes, (1, 2), data, np.full((n_pix, 2), NOISE), ut, ncomp=ncomp, **options)


def _both(runner, pix, W, u0, n_steps, n_burn, thin, seed, free_mask=None, a=2.0):
    """(twin fed by the runner's loglikelihood_batch, device ensemble after its run)."""
    pix = np.asarray(pix, dtype=np.int32)
    twin = ensemble.run_twin(lambda px, T: runner.loglikelihood_batch(px, T), runner.ndim, pix.size, W, u0, n_steps, n_burn, thin,
                             a=a, seed=seed, free_mask=free_mask, pix=pix)
    dev = ensemble.DeviceEnsemble(runner, pix, W, u0, free_mask)
    dev.run(n_steps, n_burn, thin, a, seed)
    return twin, dev


def _assert_equal_runs(twin, dev, what=''):
    u, theta, lnL = dev.state()
    chain_theta, chain_lnL = dev.chain()
    accepted, outside, evaluated = dev.counts()
    for name, got, ref in (('u', u, twin.u), ('theta', theta, twin.theta), ('lnL', lnL, twin.lnL),
                           ('chain_theta', chain_theta, twin.chain_theta), ('chain_lnL', chain_lnL, twin.chain_lnL),
                           ('trace', dev.trace(), twin.trace), ('accepted', accepted, twin.accepted),
                           ('outside', outside, twin.outside), ('evaluated', evaluated, twin.evaluated)):
        assert np.array_equal(got, ref), (what, name)


# (P, W, ncomp, masked, seed): 24 rows, nothing a multiple of 64; a half of 80 over two waves; D = 10 < ndim = 12
SHAPES = [(3, 16, 1, False, 1), (2, 160, 1, False, 1), (2, 32, 2, True, 1)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('P,W,ncomp,masked,seed', SHAPES)
def test_device_equals_twin_fed_by_the_device(engine, mode, P, W, ncomp, masked, seed):
    runner = _runner(engine, ncomp, P)
    runner.set_exp_mode(mode)
    mask = runner.utrans.free_mask(ncomp) if masked else None
    if masked:
        assert int(np.count_nonzero(mask)) < runner.ndim
    pix = np.arange(P, dtype=np.int32)[::-1].copy()           # (the cube pixel, not the position, is in the stream)
    u0 = ensemble.starts(runner, pix, W, n_init=512, seed=3)
    twin, dev = _both(runner, pix, W, u0, 30, 6, 4, seed, mask)
    print(f'ensemble {mode} P={P} W={W} ncomp={ncomp}: margin {twin.margin:.3e}, accepted {twin.accepted}, outside {twin.outside}')
    assert twin.margin >= 1e-9
    assert twin.accepted.min() > 0 and twin.chain_theta.shape == (P, 6, W, runner.ndim)
    assert twin.evaluated.tolist() == [30 * W] * P
    _assert_equal_runs(twin, dev, (mode, P, W))
    if masked:
        assert (dev.state()[0][:, :, mask == 0] == 0.5).all() and dev.trace().shape == (P, 30, 11)


def test_device_equals_twin_fed_by_the_oracle(engine, nfo):
    """Table mode, as test_sampler_on_gpu_matches_the_same_sampler_on_the_oracle: u and the counters to the bit, lnL and theta
    to that test's tolerances.  The seed: the first >= 1 whose oracle-fed twin has a margin >= 1e-6 (found on the CPU)."""
    from test_sampler import _cube
    n_pix, W, seed = 2, 16, 1
    cube, cpu_runners, _, _, _ = _cube(engine, nfo, n_pix, seed=21)

    def cpu_loglike(pix, T):
        out = np.empty(T.shape[0])
        for p in np.unique(pix):
            m = pix == p
            sub = T[m]
            out[m] = cpu_runners[p].loglikelihood_batch(sub)
            T[m] = sub
        return out
    mask = cube.utrans.free_mask(1)
    rng = np.random.default_rng(6)
    u0 = 0.5 + 0.1 * rng.uniform(-1, 1, (n_pix, W, cube.ndim))
    pix = np.arange(n_pix, dtype=np.int32)
    ref = ensemble.run_twin(cpu_loglike, cube.ndim, n_pix, W, u0, 20, 0, 1, seed=seed, free_mask=mask, pix=pix)
    assert ref.margin >= 1e-6, ref.margin
    cube.set_exp_mode('table')
    dev = ensemble.DeviceEnsemble(cube, pix, W, u0, mask)
    dev.run(20, 0, 1, 2.0, seed)
    u, theta, lnL = dev.state()
    assert np.array_equal(u, ref.u)
    for got, want in zip(dev.counts(), (ref.accepted, ref.outside, ref.evaluated)):
        assert np.array_equal(got, want)
    np.testing.assert_allclose(lnL, ref.lnL, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(theta, ref.theta, rtol=1e-8, atol=1e-12)
    chain_theta, chain_lnL = dev.chain()
    np.testing.assert_allclose(chain_lnL, ref.chain_lnL, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(chain_theta, ref.chain_theta, rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize('mode', MODES)
def test_outside_proposals_leave_their_walkers_alone(engine, mode):
    runner = _runner(engine, 1, 2)
    runner.set_exp_mode(mode)
    P, W, seed = 2, 16, 1
    pix = np.arange(P, dtype=np.int32)
    rng = np.random.default_rng(12)
    u0 = rng.uniform(0.2, 0.8, (P, W, 6))
    u0[:, ::2, 1] = rng.uniform(1e-4, 1e-3, (P, W // 2))      # every other walker within 1e-3 of a face
    u0[:, 1::2, 3] = 1.0 - rng.uniform(1e-4, 1e-3, (P, W // 2))
    twin, dev = _both(runner, pix, W, u0, 1, 0, 1, seed)
    assert twin.margin >= 1e-9
    _assert_equal_runs(twin, dev, mode)
    outside = dev.counts()[1]
    assert outside.min() > 0 and np.array_equal(outside, twin.outside)
    # one step: every walker moved at most once, and the walker of an outside proposal not at all
    S = ensemble._create(lambda px, T: runner.loglikelihood_batch(px, T), 6, pix, W, u0, None, 1 << 18)
    S.lnL = np.where(np.isfinite(S.lnL), S.lnL, ensemble.LOG_ZERO)
    u, theta, lnL = dev.state()
    n_out = 0
    for h in (0, 1):
        ensemble._propose(S, np.uint64(seed), 1, h, 2.0)
        k = h * (W // 2) + np.arange(W // 2)
        out = ~S.inside
        n_out += int(out.sum())
        assert np.array_equal(u[:, k][out], u0[:, k][out]) and np.array_equal(theta[:, k][out], S.theta[:, k][out])
        assert np.array_equal(lnL[:, k][out], S.lnL[:, k][out])
        ensemble._accept(S, np.uint64(seed), 1, h, 2.0)
    assert n_out == int(outside.sum())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('options', [dict(baseline_order=1, noise_uncertainty=0.2), dict(robust=4)], ids=['baseline+noise', 'robust'])
def test_every_likelihood_option_goes_through(engine, mode, options):
    runner = _runner(engine, 1, 2, **options)
    runner.set_exp_mode(mode)
    pix = np.arange(2, dtype=np.int32)
    u0 = ensemble.starts(runner, pix, 16, n_init=256, seed=5)
    twin, dev = _both(runner, pix, 16, u0, 20, 0, 2, 1)
    assert twin.margin >= 1e-9 and twin.accepted.min() > 0
    _assert_equal_runs(twin, dev, (mode, options))


def _check_summary(dev, levels):
    theta, lnL = dev.chain()
    P, n_keep, W, ndim = theta.shape
    N = n_keep * W
    mean, std, best, best_lnL, quant = dev.summary(levels)
    t_mean, t_std, t_best, t_best_lnL, t_quant = ensemble.summarize(theta, lnL, levels)
    assert np.array_equal(best, t_best) and np.array_equal(best_lnL, t_best_lnL)
    assert np.array_equal(quant, t_quant) and quant.shape == (P, ndim, len(levels))
    d = theta.reshape(P, N, ndim).astype(LD) - best[:, None, :].astype(LD)
    m = d.mean(axis=1)
    ref_mean, ref_var = best.astype(LD) + m, (d * d).mean(axis=1) - m * m
    dmax = np.abs(d).max(axis=1)
    err_mean, err_var = np.abs(mean.astype(LD) - ref_mean), np.abs(std.astype(LD) ** 2 - ref_var)
    live = dmax > 0                                            # (a constant parameter: every difference 0, and the error too)
    print(f'summary N={N}: mean off by {float(np.max(err_mean / (8 * N * U * dmax + U * np.abs(ref_mean) + LD(1e-300)))):.3f} of its bound, '
          f'variance by {float(np.max((err_var / np.where(live, 8 * N * U * dmax ** 2, 1))[live], initial=0.0)):.3f}')
    assert np.all(err_mean <= 8 * N * U * dmax + U * np.abs(ref_mean))     # (the sum's error and the result's rounding)
    assert np.all(err_var <= 8 * N * U * dmax ** 2)


@pytest.mark.parametrize('mode', MODES)
def test_summary(engine, mode):
    runner = _runner(engine, 1, 3)
    runner.set_exp_mode(mode)
    pix = np.arange(3, dtype=np.int32)
    dev = ensemble.DeviceEnsemble(runner, pix, 16, ensemble.starts(runner, pix, 16, n_init=256, seed=5))
    with pytest.raises(engine.EngineError, match='no run yet'):
        dev.summary((0.5,))
    dev.run(30, 6, 4, 2.0, 1)
    assert dev.n_keep == 6
    _check_summary(dev, (0.16, 0.5, 0.84))
    _check_summary(dev, (0.0, 1.0, 0.25, 0.5, 0.5, 0.75, 0.999, 0.001))
    a, b = dev.summary((0.16, 0.5, 0.84)), dev.summary((0.16, 0.5, 0.84))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], dev.summary(())[:4]))      # the moments do not depend on the quantiles asked for
    # the cap: 64 x 128 = 8192 samples sorted in 64 KB of LDS; one kept step more and the quantiles are refused, the rest served
    cap = ensemble.DeviceEnsemble(runner, pix[:1], 64, ensemble.starts(runner, pix[:1], 64, n_init=256, seed=5))
    cap.run(128, 0, 1, 2.0, 2)
    _check_summary(cap, (0.16, 0.5, 0.84))
    cap.run(129, 0, 1, 2.0, 3)
    with pytest.raises(engine.EngineError, match='NFA_ENS_MAX_SORT'):
        cap.summary((0.5,))
    _check_summary(cap, ())
    with pytest.raises(engine.EngineError, match='NFA_ENS_MAX_Q'):
        dev.summary(np.linspace(0, 1, 9))
    with pytest.raises(engine.EngineError, match=r'outside \[0, 1\]'):
        dev.summary((0.5, 1.5))


@pytest.mark.parametrize('mode', MODES)
def test_same_arguments_same_bits_and_a_second_run_continues(engine, mode):
    runner = _runner(engine, 1, 2)
    runner.set_exp_mode(mode)
    pix = np.arange(2, dtype=np.int32)
    u0 = ensemble.starts(runner, pix, 16, n_init=256, seed=5)
    loglike = lambda px, T: runner.loglikelihood_batch(px, T)
    runs = []
    for _ in range(2):
        dev = ensemble.DeviceEnsemble(runner, pix, 16, u0)
        dev.run(12, 2, 2, 2.0, 1)
        runs.append((dev, dev.state() + dev.chain() + dev.counts() + (dev.trace(),) + dev.summary((0.16, 0.5, 0.84))))
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1], runs[1][1]))
    # run again: from the state, steps numbered from 1, with the caller's new seed; chain, trace and counters are replaced
    dev = runs[0][0]
    dev.run(10, 0, 1, 2.0, 2)
    first = ensemble.run_twin(loglike, 6, 2, 16, u0, 12, 2, 2, seed=1, pix=pix)
    cont = ensemble.run_twin(loglike, 6, 2, 16, None, 10, 0, 1, seed=2, pix=pix, state=first.state)
    assert first.margin >= 1e-9 and cont.margin >= 1e-9
    _assert_equal_runs(cont, dev, mode)
    assert dev.trace().shape == (2, 10, 7) and dev.counts()[2].tolist() == [160, 160]


def test_errors_leave_the_runner_usable(engine):
    runner = _runner(engine, 1, 2)
    pix = np.arange(2, dtype=np.int32)
    rng = np.random.default_rng(2)
    probe = rng.uniform(size=(40, 6))
    before = runner.loglikelihood_batch(np.repeat(pix, 20), probe.copy())
    u0 = rng.uniform(0.3, 0.7, (2, 16, 6))
    E = engine.EngineError
    with pytest.raises(E, match='even'):
        ensemble.DeviceEnsemble(runner, pix, 15, u0[:, :15])
    with pytest.raises(E, match=r'sampled dimensions \+ 1'):
        ensemble.DeviceEnsemble(runner, pix, 12, u0[:, :12])
    with pytest.raises(E, match='NFA_ENS_MAX_WALKERS'):
        ensemble.DeviceEnsemble(runner, pix, 514, rng.uniform(0.3, 0.7, (2, 514, 6)))
    with pytest.raises(E, match='pixel index out of range'):
        ensemble.DeviceEnsemble(runner, np.array([0, 2], dtype=np.int32), 16, u0)
    for edge in (0.0, 1.0, np.nan):
        bad = u0.copy()
        bad[1, 3, 2] = edge
        with pytest.raises(E, match=r'inside \(0, 1\)'):
            ensemble.DeviceEnsemble(runner, pix, 16, bad)
    bad = u0.copy()
    bad[1, 3, 5] = 0.0                                         # ... but not at a slot that is not sampled
    ensemble.DeviceEnsemble(runner, pix, 16, bad, runner.utrans.free_mask(1)).close()
    dev = ensemble.DeviceEnsemble(runner, pix, 16, u0)
    for args, word in (((10, 0, 1, 1.0, 1), 'stretch scale'), ((10, 0, 1, 17.0, 1), 'stretch scale'), ((10, 0, 0, 2.0, 1), 'thin'),
                       ((10, 10, 1, 2.0, 1), 'n_burn'), ((10, 5, 6, 2.0, 1), 'no step is kept')):
        with pytest.raises(E, match=word):
            dev.run(*args)
    with pytest.raises(E, match='no run yet'):
        dev.chain()
    dev.run(4, 0, 1, 2.0, 1)                                   # and the ensemble itself is usable after its refusals
    assert np.array_equal(runner.loglikelihood_batch(np.repeat(pix, 20), probe.copy()), before)
    dev.close()
    assert np.array_equal(runner.loglikelihood_batch(np.repeat(pix, 20), probe.copy()), before)


def test_agreement_with_the_nested_sampler(engine, mode_guard):
    """GaussianRunner, one component, 128 channels, four pixels at peak S/N 10: posterior mean and std of every parameter
    against `sampler.run_multinest`'s weighted ones (deviations observed on an MI355X: DESIGN 4.24)."""
    from nestfit_amd import gaussian, sampler
    from nestfit_amd.synth import CKMS
    from test_sibling_models import _simple_priors
    engine.set_exp_mode('table')
    rng = np.random.default_rng(8)
    nu0, n, noise, W, n_steps, ndim = 110.201354e9, 128, 0.3, 32, 600, 3
    x = nu0 * (1.0 - np.linspace(15, -15, n) / CKMS)
    ut = _simple_priors(engine, [(-10, 10), (0.2, 3.0), (0.0, 8.0)])
    for p in range(4):
        truth = np.array([rng.uniform(-3, 3), rng.uniform(0.8, 1.5), 10 * noise])
        probe = gaussian.GaussianRunner.from_data([x, np.zeros(n), noise, nu0], ut, ncomp=1)
        model, _ = probe.predict_batch(truth[None])
        runner = gaussian.GaussianRunner.from_data([x, model[0] + rng.normal(0, noise, n), noise, nu0], ut, ncomp=1)
        res = runner.sample_posterior(n_walkers=W, n_steps=n_steps, seed=1 + p, keep_chain=True)
        nested = sampler.run_multinest(runner, sampler.Dumper(None, no_dump=True), nlive=400, tol=0.5, efr=0.3, seed=5 + p)
        post = nested.posterior
        w = post[:, -1] / post[:, -1].sum()
        n_eff_ns = 1.0 / np.sum(w * w)
        ns_mean = (w[:, None] * post[:, :ndim]).sum(axis=0)
        ns_std = np.sqrt((w[:, None] * (post[:, :ndim] - ns_mean) ** 2).sum(axis=0))
        # the ensemble's standard error: batch means of the per-step walker means of theta, computed here
        step_mean = res.theta[0].mean(axis=1)                  # [n_keep, ndim]
        nb = 10
        batches = step_mean[:step_mean.shape[0] // nb * nb].reshape(nb, -1, ndim).mean(axis=1)
        se = np.sqrt(batches.var(axis=0, ddof=1) / nb + ns_std ** 2 / n_eff_ns)
        n_eff_ens = float(np.min(res.n_eff[0]))
        rel = 5 * np.sqrt(1 / (2 * n_eff_ens) + 1 / (2 * n_eff_ns))
        dm, ds = np.abs(res.mean[0] - ns_mean) / se, np.abs(res.std[0] / ns_std - 1)
        print(f'pixel {p}: mean off by {np.round(dm, 2)} combined standard errors (5 allowed), std by {np.round(ds, 3)} relative '
              f'({rel:.3f} allowed); n_eff {n_eff_ens:.0f} / {n_eff_ns:.0f}, tau {np.round(res.tau[0], 1)}, acceptance {res.acceptance[0]:.2f}')
        assert res.theta.shape == (1, res.theta.shape[1], W, ndim) and np.isfinite(n_eff_ens)
        assert np.all(dm < 5) and np.all(ds < rel)
        res.close()


def _stack(axes, data, side, noise):
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.synth import NU0
    cubes = []
    for k, t in enumerate((1, 2)):
        f = axes[k]
        hdr = {'BUNIT': 'K', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz', 'CRVAL3': float(f[0]), 'CDELT3': float((f[-1] - f[0]) / (N_CHAN - 1)),
               'CRPIX3': 1.0, 'RESTFRQ': NU0[t], 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CRVAL1': 270.0, 'CRVAL2': -20.0,
               'CDELT1': -1e-3, 'CDELT2': 1e-3, 'CRPIX1': 1.0, 'CRPIX2': 1.0, 'CUNIT1': 'deg', 'CUNIT2': 'deg',
               'NAXIS1': side, 'NAXIS2': side, 'NAXIS3': N_CHAN, 'NAXIS': 3}
        arr = data[:, k * N_CHAN:(k + 1) * N_CHAN].reshape(side, side, N_CHAN).transpose(2, 1, 0)     # (chan, lat, lon)
        cubes.append(DataCube(SimpleCube(hdr, arr), noise, trans_id=t))
    return CubeStack(cubes)


def test_sample_cube(engine):
    axes, data, ut = _data(engine, 1, 9, seed=4)
    data[4, 10] = np.nan                                       # the middle pixel is not good
    engine.set_exp_mode('table')
    kw = dict(n_walkers=16, n_steps=40, n_burn=8, thin=4, seed=2, n_init=256, free_mask=ut.free_mask(1))
    one = ensemble.sample_cube(_stack(axes, data, 3, NOISE), ut, engine.AmmoniaRunner, 1, **kw)
    per_pixel = engine._ffi.load().nfa_ensemble_bytes(1, 16, 6, 5, 40, 8)
    three = ensemble.sample_cube(_stack(axes, data, 3, NOISE), ut, engine.AmmoniaRunner, 1, memory_budget=3 * per_pixel + 1, **kw)
    assert one.n_groups == 1 and three.n_groups == 3
    shapes = dict(mean=(6, 3, 3), std=(6, 3, 3), best=(6, 3, 3), best_lnL=(3, 3), quantiles=(6, 3, 3, 3), acceptance=(3, 3),
                  outside=(3, 3), n_evals=(3, 3), tau=(5, 3, 3), n_eff=(5, 3, 3))
    bad = np.zeros((3, 3), dtype=bool)
    bad[1, 1] = True                                           # pixel 4 = lon 1, lat 1
    for name, shape in shapes.items():
        a, b = getattr(one, name), getattr(three, name)
        assert a.shape == shape, name
        assert np.array_equal(a, b, equal_nan=True), name      # the grouping does not change a pixel's run
        if name == 'n_evals':
            assert (a[bad] == -1).all() and (a[~bad] == 40 * 16).all()
        else:
            assert np.isnan(a[..., bad]).all() and (name in ('tau', 'n_eff') or np.isfinite(a[..., ~bad]).all()), name
    assert np.all(one.acceptance[~bad] > 0) and np.all(one.quantiles[:, 0] <= one.quantiles[:, 2], where=~bad)
