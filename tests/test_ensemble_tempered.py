"""Tempered ensembles on the device (nfa_ensemble_create_tempered and what follows it) against the numpy twin,
decision for decision; against the untempered ensemble, bit for bit where the two must agree; the evidence kernel against a
longdouble evaluation; and the evidence itself against the nested sampler's.

As in test_ensemble.py the twin is fed by the device's own likelihood, so the two runs are equal to the bit unless the device's
`log` and numpy's differ in a decision: each case asserts the twin's smallest margins, of the moves and of the swaps, first."""
import numpy as np
import pytest

from nestfit_amd import ensemble
from test_ensemble import NOISE, _assert_equal_runs, _data, _runner, _stack
from test_sibling_models import MODES, _simple_priors, mode_guard          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
N_STEPS = 12


def _gauss_runner(engine, seed=8, n=128, noise=0.3):
    """A one-pixel GaussianRunner, one component at peak S/N 10 on n channels (the setting of DESIGN 4.24's comparison)."""
    from nestfit_amd import gaussian
    from nestfit_amd.synth import CKMS
    rng = np.random.default_rng(seed)
    nu0 = 110.201354e9
    x = nu0 * (1.0 - np.linspace(15, -15, n) / CKMS)
    ut = _simple_priors(engine, [(-10, 10), (0.2, 3.0), (0.0, 8.0)])
    truth = np.array([rng.uniform(-3, 3), rng.uniform(0.8, 1.5), 10 * noise])
    probe = gaussian.GaussianRunner.from_data([x, np.zeros(n), noise, nu0], ut, ncomp=1)
    model, _ = probe.predict_batch(truth[None])
    return gaussian.GaussianRunner.from_data([x, model[0] + rng.normal(0, noise, n), noise, nu0], ut, ncomp=1)


_CACHE = {}


def _shape(engine, kind):
    """(runner, pix for the device, pix for the twin, loglike, free_mask) of a shape, built once."""
    if kind not in _CACHE:
        if kind == 'gauss':
            runner = _gauss_runner(engine)
            _CACHE[kind] = (runner, None, np.zeros(1, dtype=np.int32), lambda px, T: runner.loglikelihood_batch(T), None)
        else:
            runner = _runner(engine, 2, 3)
            mask = runner.utrans.free_mask(2)
            assert runner.ndim - int(np.count_nonzero(mask)) == 2                 # two slots are not sampled
            pix = np.array([2, 0], dtype=np.int32)                                # (the cube pixel, not the position, is in the stream)
            _CACHE[kind] = (runner, pix, pix, lambda px, T: runner.loglikelihood_batch(px, T), mask)
    return _CACHE[kind]


def _start(runner, pix, W, T, mask, seed=3):
    """u0[P, T, W, ndim] around the best of a few prior draws: every rung its own start."""
    rng = np.random.default_rng(seed)
    P = 1 if pix is None else pix.size
    best = ensemble.starts(runner, pix, 2, n_init=512, seed=seed)[:, :1]          # [P, 1, ndim]
    return np.clip(best[:, None] + 0.02 * rng.uniform(-1, 1, (P, T, W, runner.ndim)), 0.01, 0.99)


def _assert_equal_rungs(twin, dev, what=''):
    u, theta, lnL = dev.rung_state()
    accepted, outside, evaluated, s_acc, s_prop = dev.rung_counts()
    for name, got, ref in (('rung_u', u, twin.rung_u), ('rung_theta', theta, twin.rung_theta), ('rung_lnL_state', lnL, twin.rung_lnL_state),
                           ('rung_lnL', dev.rung_lnL(), twin.rung_lnL), ('rung_trace', dev.rung_trace(), twin.rung_trace),
                           ('rung_accepted', accepted, twin.rung_accepted), ('rung_outside', outside, twin.rung_outside),
                           ('rung_evaluated', evaluated, twin.rung_evaluated), ('swaps_accepted', s_acc, twin.swaps_accepted),
                           ('swaps_proposed', s_prop, twin.swaps_proposed)):
        assert got.shape == ref.shape and np.array_equal(got, ref), (what, name)


# W = 130: a half of 65, so a second wave of the moves holds one lane, and the swap kernel runs three waves.  The
# two-component shape samples D = 10 of its 12 slots, so W / 2 >= D + 1 asks for 22 walkers at least: 22 is its small W.
CASES = [('gauss', 8), ('gauss', 130), ('cube2', 22), ('cube2', 130)]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('swap_every', [1, 3])
@pytest.mark.parametrize('T', [2, 3, 5])
@pytest.mark.parametrize('kind,W', CASES)
def test_device_equals_twin_fed_by_the_device(engine, mode_guard, kind, W, T, swap_every, mode):
    runner, pix, twin_pix, loglike, mask = _shape(engine, kind)
    runner.set_exp_mode(mode)
    betas = ensemble.ladder(T, 1e-2)
    u0 = _start(runner, pix, W, T, mask)
    twin = ensemble.run_twin(loglike, runner.ndim, twin_pix.size, W, u0, N_STEPS, 2, 2, seed=1, free_mask=mask, pix=twin_pix, betas=betas,
                             swap_every=swap_every)
    print(f'tempered {kind} {mode} W={W} T={T} swap_every={swap_every}: margin {twin.margin:.3e}, swap margin {twin.swap_margin:.3e}, '
          f'swaps {twin.swaps_accepted.sum()} of {twin.swaps_proposed.sum()}')
    assert twin.margin >= 1e-9 and twin.swap_margin >= 1e-9
    dev = ensemble.DeviceEnsemble(runner, pix, W, u0, mask, betas=betas, swap_every=swap_every)
    dev.run(N_STEPS, 2, 2, 2.0, 1)
    _assert_equal_runs(twin, dev, (kind, mode, W, T))            # the cold chain, through the calls of an untempered ensemble
    _assert_equal_rungs(twin, dev, (kind, mode, W, T))
    assert twin.rung_accepted.min() > 0 and twin.chain_theta.shape == (twin_pix.size, 5, W, runner.ndim)
    sweeps = N_STEPS // swap_every
    want = [W * len(range(t % 2, sweeps, 2)) for t in range(T - 1)]          # pair t is active on the sweeps of its parity
    assert dev.rung_counts()[4].tolist() == [want] * twin_pix.size
    if T == 2:
        assert want == [W * ((sweeps + 1) // 2)]                 # one pair, on the even sweeps only
    dev.close()


@pytest.mark.parametrize('mode', MODES)
def test_rung_0_without_swaps_is_the_untempered_ensemble(engine, mode_guard, mode):
    runner, pix, twin_pix, loglike, mask = _shape(engine, 'cube2')
    runner.set_exp_mode(mode)
    W, T = 32, 3
    u0 = _start(runner, pix, W, T, mask)
    hot = ensemble.DeviceEnsemble(runner, pix, W, u0, mask, betas=[1.0, 0.25, 0.0], swap_every=0)
    cold = ensemble.DeviceEnsemble(runner, pix, W, u0[:, 0], mask)
    hot.run(20, 4, 2, 2.0, 5)
    cold.run(20, 4, 2, 2.0, 5)
    for name, a, b in (('state', hot.state(), cold.state()), ('chain', hot.chain(), cold.chain()), ('counts', hot.counts(), cold.counts()),
                       ('trace', (hot.trace(),), (cold.trace(),))):
        assert all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b)), name
    assert not hot.rung_counts()[4].any() and np.array_equal(hot.rung_state()[0][:, 0], cold.state()[0])
    # the products of a tempered ensemble are those of an untempered one that holds the same cold chain
    edges = ensemble.bin_edges(runner.utrans, 2, 7)
    for name, a, b in (('summary', hot.summary((0.16, 0.5, 0.84)), cold.summary((0.16, 0.5, 0.84))),
                       ('histogram', hot.histogram(edges), cold.histogram(edges)), ('covariance', (hot.covariance(),), (cold.covariance(),))):
        assert all(x.shape == y.shape and np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b)), name
    ma, mb = hot.moments(), cold.moments()
    for field in ('mean', 'std', 'peak_mean', 'peak_std', 'total_mean', 'total_std'):
        assert np.array_equal(getattr(ma, field), getattr(mb, field)), field
    hot.close()
    cold.close()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('W,n_keep,blocks', [(8, 6, (1, 4)), (16, 70, (1, 8, 16))])
def test_evidence_kernel_against_longdouble(engine, mode_guard, W, n_keep, blocks, mode):
    """n = n_keep W = 48 and 1120 values a set at most; B = 4 does not divide 6, nor 8 and 16 divide 70.  The bounds are DESIGN
    4.26's; the shares of them observed on an MI355X stand there."""
    runner, pix, _, _, mask = _shape(engine, 'gauss')
    runner.set_exp_mode(mode)
    T = 5
    betas = ensemble.ladder(T, 1e-3)
    dev = ensemble.DeviceEnsemble(runner, pix, W, _start(runner, pix, W, T, mask), mask, betas=betas, swap_every=1)
    dev.run(2 * n_keep, n_keep, 1, 2.0, 3)
    x = dev.rung_lnL()
    assert x.shape == (1, T, n_keep, W) and np.isfinite(x).all()
    for B in blocks:
        ev = dev.evidence(B)
        got, ref = ev.sets, ensemble.evidence_sets(x, betas, B, dtype=LD)
        assert got.shape == (1, T, B + 1, 3)
        blk = n_keep // B
        share = np.zeros(3)
        for j in range(B + 1):
            first, steps = (0, n_keep) if j == 0 else ((j - 1) * blk, blk)
            v = x[:, :, first:first + steps].reshape(1, T, -1).astype(LD)
            n = v.shape[2]
            d = np.abs(v - v[:, :, :1]).max(axis=2)
            err = np.abs(got[:, :, j].astype(LD) - ref[:, :, j])
            bound = np.stack([8 * n * U * d + U * np.abs(ref[:, :, j, 0]), 8 * n * U * d * d, 8 * n * U + 2 * U * np.abs(ref[:, :, j, 2])], axis=2)
            share = np.maximum(share, (err / bound).max(axis=(0, 1)).astype(np.float64))
            assert np.all(err <= bound), (B, j)
        print(f'evidence {mode} n_keep W = {n_keep * W} B = {B}: mean, var, r off by {np.round(share, 3)} of their bounds')
        assert (got[:, 0, :, 2] == 0).all()
        again = dev.evidence(B)
        assert np.array_equal(again.sets, got) and np.array_equal(again.lnZ, ev.lnZ)
        twin = ensemble.evidence_of(x, betas, B)
        np.testing.assert_allclose(ev.lnZ, twin.lnZ, rtol=0, atol=T * 16 * n_keep * W * U + 4 * U * np.abs(twin.sets[..., 0, 2]).sum())
    dev.close()


def test_refusals_leave_the_runner_usable(engine, mode_guard):
    runner, pix, _, _, mask = _shape(engine, 'gauss')
    rng = np.random.default_rng(2)
    probe = rng.uniform(size=(40, 3))
    before = runner.loglikelihood_batch(probe.copy())
    W = 8
    u0 = rng.uniform(0.3, 0.7, (1, W, 3))
    E = engine.EngineError
    for betas, word in (([1.0], 'NFA_ENS_MAX_TEMPS'), (ensemble.ladder(33), 'NFA_ENS_MAX_TEMPS'), ([0.9, 0.5, 0.0], r'betas\[0\] must be 1'),
                        ([1.0, 0.5, 0.5, 0.0], 'decrease strictly'), ([1.0, 0.5, 0.6, 0.0], 'decrease strictly'),
                        ([1.0, 0.5, -1e-9], 'must not be negative'), ([1.0, np.nan, 0.0], 'not finite')):
        with pytest.raises(E, match=word):
            ensemble.DeviceEnsemble(runner, pix, W, u0, betas=betas)
    with pytest.raises(E, match='swap_every'):
        ensemble.DeviceEnsemble(runner, pix, W, u0, betas=[1.0, 0.0], swap_every=-1)
    with pytest.raises(E, match='even'):                        # the rules for W hold for every rung
        ensemble.DeviceEnsemble(runner, pix, 7, u0[:, :7], betas=[1.0, 0.0])
    dev = ensemble.DeviceEnsemble(runner, pix, W, u0, betas=[1.0, 0.1, 0.0])
    with pytest.raises(E, match='no run yet'):
        dev.evidence(2)
    with pytest.raises(E, match='no run yet'):
        dev.rung_lnL()
    dev.run(6, 2, 1, 2.0, 1)
    for B, word in ((5, 'no more blocks than kept steps'), (0, 'NFA_ENS_MAX_BLOCKS'), (17, 'NFA_ENS_MAX_BLOCKS')):
        with pytest.raises(E, match=word):
            dev.evidence(B)
    assert np.isfinite(dev.evidence(4).lnZ).all()               # and the ensemble itself is usable after its refusals
    cold = ensemble.DeviceEnsemble(runner, pix, W, u0)
    cold.run(6, 2, 1, 2.0, 1)
    with pytest.raises(E, match='not a tempered ensemble'):
        cold.evidence(2)
    with pytest.raises(E, match='not a tempered ensemble'):
        cold.rung_state()
    assert np.array_equal(runner.loglikelihood_batch(probe.copy()), before)
    dev.close()
    cold.close()
    assert np.array_equal(runner.loglikelihood_batch(probe.copy()), before)


def test_evidence_agrees_with_the_nested_sampler(engine, mode_guard):
    """GaussianRunner, one component, 128 channels, four pixels at peak S/N 10, W = 16, `ladder(16, 1e-4)`, 600 steps: the
    stepping-stone lnZ within 5 combined error bars of `sampler.run_multinest`'s, and the cold chain's means within 5 combined
    standard errors of the nested ones, as test_ensemble.py asserts for the untempered run.  The values observed on an MI355X
    stand in DESIGN 4.26."""
    from nestfit_amd import sampler
    engine.set_exp_mode('table')
    W, n_steps, ndim = 16, 600, 3
    betas = ensemble.ladder(16, 1e-4)
    for p in range(4):
        runner = _gauss_runner(engine, seed=80 + p)
        res = runner.sample_posterior(n_walkers=W, n_steps=n_steps, seed=1 + p, keep_chain=True, betas=betas)
        nested = sampler.run_multinest(runner, sampler.Dumper(None, no_dump=True), nlive=400, tol=0.5, efr=0.3, seed=5 + p)
        post = nested.posterior
        w = post[:, -1] / post[:, -1].sum()
        n_eff_ns = 1.0 / np.sum(w * w)
        ns_mean = (w[:, None] * post[:, :ndim]).sum(axis=0)
        ns_std = np.sqrt((w[:, None] * (post[:, :ndim] - ns_mean) ** 2).sum(axis=0))
        step_mean = res.theta[0].mean(axis=1)                  # [n_keep, ndim]
        nb = 10
        batches = step_mean[:step_mean.shape[0] // nb * nb].reshape(nb, -1, ndim).mean(axis=1)
        se = np.sqrt(batches.var(axis=0, ddof=1) / nb + ns_std ** 2 / n_eff_ns)
        dm = np.abs(res.mean[0] - ns_mean) / se
        dz, sz = abs(res.lnZ[0] - nested.lnZ), np.sqrt(res.lnZ_err[0] ** 2 + nested.lnZ_err ** 2)
        print(f'pixel {p}: lnZ {res.lnZ[0]:.3f} +- {res.lnZ_err[0]:.3f} against the nested {nested.lnZ:.3f} +- {nested.lnZ_err:.3f}: |dlnZ| = '
              f'{dz:.3f} = {dz / sz:.2f} combined errors (5 allowed); lnZ_ti {res.lnZ_ti[0]:.3f}; means off by {np.round(dm, 2)} combined '
              f'standard errors (5 allowed); swap rates {np.round(res.swap_rate[0], 2)}, rung acceptance {np.round(res.rung_acceptance[0], 2)}')
        assert res.theta.shape == (1, res.theta.shape[1], W, ndim) and res.mean_lnL.shape == (1, 16) and res.swap_rate.shape == (1, 15)
        assert res.swap_rate.min() >= 0.1                       # (below that the ladder would be too coarse for this target)
        assert dz <= 5 * sz
        assert np.all(dm < 5)
        res.close()


def test_sample_cube_with_a_ladder(engine, mode_guard):
    axes, data, ut = _data(engine, 1, 4, seed=4)
    engine.set_exp_mode('table')
    betas = ensemble.ladder(4, 1e-2)
    kw = dict(n_walkers=16, n_steps=40, n_burn=8, thin=4, seed=2, n_init=256, free_mask=ut.free_mask(1))
    one = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, betas=betas, **kw)
    per_pixel = engine._ffi.load().nfa_ensemble_tempered_bytes(1, 16, 4, 6, 5, 40, 8)
    assert per_pixel > engine._ffi.load().nfa_ensemble_bytes(1, 16, 6, 5, 40, 8)
    two = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, betas=betas, memory_budget=2 * per_pixel + 1, **kw)
    assert one.n_groups == 1 and two.n_groups == 2
    shapes = dict(lnZ=(2, 2), lnZ_err=(2, 2), lnZ_ti=(2, 2), mean_lnL=(4, 2, 2), swap_rate=(3, 2, 2), rung_acceptance=(4, 2, 2))
    for name in ensemble.MAP_FIELDS + ensemble.TEMPERED_FIELDS:
        a, b = getattr(one, name), getattr(two, name)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name          # the grouping does not change a pixel's run
        if name in shapes:
            assert a.shape == shapes[name] and np.isfinite(a).all(), name
    assert (one.n_evals == 40 * 16).all() and np.all(one.swap_rate > 0)
    # betas=None is the call as it was: no evidence among its maps, and they are the cold maps of a ladder that never swaps --
    # a start [P, W, ndim] goes to every rung, rung 0 moves on the untempered streams, and beta_0 = 1 multiplies exactly
    cold = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, **kw)
    same = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, betas=None, **kw)
    still = ensemble.sample_cube(_stack(axes, data, 2, NOISE), ut, engine.AmmoniaRunner, 1, betas=betas, swap_every=0, **kw)
    assert not hasattr(cold, 'lnZ') and np.isnan(still.swap_rate).all()
    for name in ensemble.MAP_FIELDS:
        assert np.array_equal(getattr(cold, name), getattr(same, name), equal_nan=True), name
        assert np.array_equal(getattr(cold, name), getattr(still, name), equal_nan=True), name
        assert name in ('n_evals', 'outside') or not np.array_equal(getattr(cold, name), getattr(one, name), equal_nan=True), name
