"""Device = twin, decision for decision, at the sampled dimensions that are not 5, 10 or 15: everything there runs the
general proposal kernel (`ns_propose_kernel<0>`), the cluster fits `ns_refit_multi<1..4, 6>` or the general refit, and
rows of up to 60 entries through the update wave -- the Gaussian, hyperfine, LTE and LTE-band models, NH3 from four
components on, any free mask that is not NH3's.  And at 10 dimensions the named settings precision='speed' / 'evidence'.

As tests/test_sampler.py::test_box_vetoes_on_the_device_follow_the_twin does it: `fit_pixels(device=True)` against
`fit_pixels(device=False)` (numpy rounds, the GPU's table-mode likelihood), same seed: iteration and evaluation counts
equal, lnZ to 1e-10, the table to rtol 1e-8.  Two pixels of 128 channels (per spectrum), a model at a truth plus noise,
independent uniform priors, at least 6 nlive iterations; every case asserts from the twin's own rounds (the `detail`
hook of `run_nested`) that the phase it is there for happened."""
import functools

import numpy as np
import pytest

from nestfit_amd import nested, sampler
from nestfit_amd.synth import CKMS, freq_axis
from test_sibling_models import _simple_priors

pytestmark = pytest.mark.gpu

N_CHAN, N_PIX = 128, 2


class Rounds:
    """The twin's rounds, as `run_nested(progress=...)` reports them: which pixels ever walked, left the unit cube for
    an ellipsoid bound, had more than one ellipsoid; how often a pixel's bound changed (refits)."""

    def __init__(self):
        self.rounds, self.walked, self.left_cube, self.max_ell, self.refits, self._lnvol = 0, None, None, None, None, None

    def __call__(self, n_active, n_iter):
        pass

    @property
    def split(self):
        return self.max_ell > 1

    def detail(self, d):
        lnvol = np.array(d['lnvol'], dtype=np.float64)
        if self._lnvol is None:
            P = lnvol.size
            self.walked, self.left_cube = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
            self.max_ell, self.refits = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
        else:
            self.refits += lnvol != self._lnvol
        self._lnvol = lnvol
        self.rounds = int(d['rnd'])
        self.walked |= np.asarray(d['walk'], dtype=bool)
        self.left_cube |= ~np.asarray(d['use_cube'], dtype=bool)
        self.max_ell = np.maximum(self.max_ell, d['nell'])


def _cube(engine, model_kw, xarrs, ranges, ncomp, truth, noise, seed, priors=None):
    """Two pixels of the model at `truth` (parameter-major, the second pixel's velocities shifted a little) plus noise."""
    from nestfit_amd.cube import CubeRunner
    rng = np.random.default_rng(seed)
    ut = priors or _simple_priors(engine, ranges)
    n_tot = sum(len(x) for x in xarrs)
    truths = np.tile(np.asarray(truth, dtype=np.float64), (N_PIX, 1))
    truths[1, :ncomp] += 0.3
    trans = model_kw.pop('trans_ids', [1] * len(xarrs))
    probe = CubeRunner(xarrs, trans, np.zeros((1, n_tot)), np.full((1, len(xarrs)), noise), ut, ncomp=ncomp, **model_kw)
    model, _ = probe.predict_batch(np.zeros(N_PIX, dtype=np.int32), truths)
    assert np.isfinite(model).all() and model.max() > 5 * noise
    return CubeRunner(xarrs, trans, model + rng.normal(0, noise, model.shape), np.full((N_PIX, len(xarrs)), noise), ut, ncomp=ncomp, **model_kw)


def _spread(lo, hi, k):
    return np.linspace(lo, hi, k) if k > 1 else np.array([0.5 * (lo + hi) - 2.0])


def gaussian_cube(engine, ncomp):
    nu0 = 110.201354e9
    x = nu0 * (1.0 - np.linspace(20, -20, N_CHAN) / CKMS)
    truth = np.concatenate([_spread(-9, 9, ncomp), 0.8 + 0.15 * np.arange(ncomp), 2.0 + 0.3 * np.arange(ncomp)])
    return _cube(engine, dict(model=2, rest_freqs=[nu0]), [x], [(-15, 15), (0.2, 3.0), (0.0, 5.0)], ncomp, truth, 0.1, 40 + ncomp)


def hyperfine_cube(engine, ncomp):
    """A made-up three-line table; `ncomp` components spread over a band of +-40 km/s."""
    table = engine.LineTable(88.6318e9, [-7.1, 0.0, 4.9], [0.2, 0.5, 0.3], name='three')
    x = table.nu * (1.0 - np.linspace(40, -40, N_CHAN) / CKMS)
    truth = np.concatenate([_spread(-27, 27, ncomp), 6.0 + 0.5 * np.arange(ncomp), np.full(ncomp, 0.2), 0.8 + 0.05 * np.arange(ncomp)])
    return _cube(engine, dict(model=3, lines=[table]), [x], [(-30, 30), (3.0, 15.0), (-1.0, 1.0), (0.4, 2.0)], ncomp, truth, 0.1, 50 + ncomp)


def lte_cube(engine):
    """Two components over the 1-0 and 2-1 lines of tests/test_lte.py's rotor."""
    import lte_restatement as lr
    from test_lte_cpu import rotor_species
    mol, t10, t21, _ = rotor_species(engine, B=150e9, mu=2e-18, t_lo=3.0, t_hi=30.0, name='fit rotor')
    xarrs = [lr.axis(t.nu, N_CHAN, 16.0) for t in (t10, t21)]
    truth = [-1.5, 1.5, 5.0, 7.0, 13.1, 13.3, 0.5, 0.7]
    return _cube(engine, dict(model=4, lines=[t10, t21]), xarrs, [(-3, 3), (3.0, 12.0), (12.0, 14.5), (0.2, 1.2)], 2, truth, 0.02, 61)


def band_cube(engine):
    """Two components on one banded spectrum: K = 0..3 of tests/test_lte_bands_cpu.py's symmetric top."""
    from test_lte_bands_cpu import band_axis, top_species
    mol, ks = top_species(engine)
    band = mol.band(ks, name='J=5-4')
    truth = [-1.2, 1.0, 22.0, 30.0, 14.6, 14.4, 0.6, 0.5]
    return _cube(engine, dict(model=4, lines=[band]), [band_axis(band.nu, n=N_CHAN)], [(-3, 3), (6.0, 60.0), (13.0, 15.5), (0.2, 1.5)], 2, truth, 0.02, 62)


def ammonia_cube(engine, ncomp, ranges=((-12, 12), (8.0, 25.0), (3.0, 10.0), (13.5, 15.5), (0.2, 1.5))):
    """NH3 (1,1)+(2,2), `ncomp` components, uniform ranges and the constant orth slot: 5 ncomp of 6 ncomp sampled."""
    x = np.linspace(0, 1, 200)
    base = _simple_priors(engine, ranges)
    ut = engine.PriorTransformer(list(base.priors) + [engine.ConstantPrior(0, 5)])
    assert ut.free_mask(ncomp).tolist() == [1] * (5 * ncomp) + [0] * ncomp
    truth = np.concatenate([_spread(-10, 10, ncomp), 12.0 + 0.5 * np.arange(ncomp), 5.0 + 0.2 * np.arange(ncomp), np.full(ncomp, 14.5),
                            0.35 + 0.02 * np.arange(ncomp), np.zeros(ncomp)])
    return _cube(engine, dict(trans_ids=(1, 2)), [freq_axis(1, N_CHAN), freq_axis(2, N_CHAN)], None, ncomp, truth, 0.1, 70 + ncomp, priors=ut)


# name: (sampled dimensions, cube, options of the run, what the plan must say, phases that must happen in every pixel beside
# three refits: 'left_cube' = an ellipsoid bound smaller than the unit cube, 'split' = more than one ellipsoid, 'walked')
CASES = {
    'gauss 3': (3, lambda e: gaussian_cube(e, 1), dict(nlive=100, maxiter=600), dict(multi=1), 'left_cube split'),
    'gauss 3, one ellipsoid': (3, lambda e: gaussian_cube(e, 1), dict(nlive=100, maxiter=600, ellipsoids=1), dict(multi=0), 'left_cube'),
    'gauss 6': (6, lambda e: gaussian_cube(e, 2), dict(nlive=100, maxiter=700), dict(multi=1, walk_factor=64), 'left_cube split'),
    'gauss 6, one ellipsoid': (6, lambda e: gaussian_cube(e, 2), dict(nlive=100, maxiter=700, ellipsoids=1), dict(multi=0), ''),
    'hyperfine 4': (4, lambda e: hyperfine_cube(e, 1), dict(nlive=100, maxiter=600), dict(multi=1), 'left_cube split'),
    # (a prior fixes a parameter of every component: a mask of 7 of 8 slots pins ONE slot, the second width, at u = 0.5)
    'lte 7 of 8': (7, lte_cube, dict(nlive=110, maxiter=700, free_mask=[1, 1, 1, 1, 1, 1, 1, 0]), dict(multi=0, walk_factor=2), ''),
    'band 8': (8, band_cube, dict(nlive=110, maxiter=700), dict(multi=0, walk_factor=2), ''),
    'gauss 12, auto': (12, lambda e: gaussian_cube(e, 4), dict(nlive=120, maxiter=800, n_steps=30), dict(multi=0, shear=0), ''),
    'gauss 12, walk': (12, lambda e: gaussian_cube(e, 4), dict(nlive=120, maxiter=800, n_steps=30, method='walk'), dict(multi=0), 'walked'),
    'nh3 20': (20, lambda e: ammonia_cube(e, 4), dict(nlive=130, maxiter=800, n_steps=40), dict(shear=0, boxes=0, stage_live=1), ''),
    'hyperfine 40, staged': (40, lambda e: hyperfine_cube(e, 10), dict(nlive=100, maxiter=800, n_steps=40), dict(stage_live=1, shear=0), ''),
    'hyperfine 40, unstaged': (40, lambda e: hyperfine_cube(e, 10), dict(nlive=320, maxiter=2400, n_steps=40), dict(stage_live=0, shear=0), ''),
    'nh3 50, walk': (50, lambda e: ammonia_cube(e, 10), dict(nlive=80, maxiter=480, n_steps=25, method='walk'), dict(stage_live=1, shear=0), 'walked'),
}


def _follow(engine, cube, nd, opts, plan, phases, name):
    fm = np.asarray(opts.get('free_mask', cube.utrans.free_mask(cube.ncomp)))
    assert int(fm.sum()) == nd and nd not in (5, 10, 15)
    nl = opts['nlive']
    assert opts['maxiter'] >= 6 * nl
    pl = nested._plan(nd, cube.ndim, nl, np.flatnonzero(fm), ellipsoids=opts.get('ellipsoids'))
    for k, v in plan.items():
        assert getattr(pl, k) == v, (name, k, getattr(pl, k), v)
    kw = dict(tol=0.5, efr=0.3, seed=7, batch_target=2048, **opts)
    seen = Rounds()
    pix = np.arange(N_PIX)
    dev = sampler.fit_pixels(cube, pix, device=True, time_limit=60, **kw)
    twin = sampler.fit_pixels(cube, pix, device=False, progress=seen, **kw)
    print(f'\n{name}: n_iter {[t.n_iter for t in twin]}, n_evals {[t.n_evals for t in twin]}, rounds {seen.rounds}, refits {seen.refits.tolist()}, '
          f'left the cube {seen.left_cube.tolist()}, walked {seen.walked.tolist()}, ellipsoids {seen.max_ell.tolist()}')
    for d, t in zip(dev, twin):
        assert (d.n_iter, d.n_evals) == (t.n_iter, t.n_evals), (name, d.n_iter, t.n_iter, d.n_evals, t.n_evals)
        assert d.lnZ == pytest.approx(t.lnZ, rel=1e-10)
        np.testing.assert_allclose(d.posterior, t.posterior, rtol=1e-8, atol=1e-12)
    assert (seen.refits >= 3).all(), (name, seen.refits)
    for phase in phases.split():
        assert getattr(seen, phase).all(), (name, phase)


@pytest.mark.parametrize('name', list(CASES))
def test_the_device_follows_the_twin_off_the_compiled_dimensions(engine, name):
    nd, make, opts, plan, phases = CASES[name]
    try:
        engine.set_exp_mode('table')
        _follow(engine, make(engine), nd, dict(opts), plan, phases, name)
    finally:
        engine.set_exp_mode('fast')


@pytest.mark.parametrize('precision', ['speed', 'evidence'])
def test_named_precision_settings_follow_the_twin(engine, precision):
    """Ten sampled dimensions (the two-component cube of test_shear_on_the_device_follows_the_twin), the knobs taken from
    `nested.PRECISION`: shear, box margin and pair ellipses at their named values, 'evidence' without walks."""
    from nestfit_amd.cube import CubeRunner
    n_pix, noise = 3, 0.1
    rng = np.random.default_rng(3)
    axes = [freq_axis(1, N_CHAN), freq_axis(2, N_CHAN)]
    ut = engine.get_irdc_priors(size=500, vsys=0.0)
    truths = np.tile(np.array([-0.5, 1.0, 12.0, 15.0, 5.0, 6.0, 14.4, 14.6, 0.4, 0.4, 0.0, 0.0]), (n_pix, 1))
    truths[:, 6] += np.array([0.0, -0.4, 0.2])
    knobs = nested.PRECISION[precision]
    margin, pairs, method, shear = nested.resolve_precision(precision)
    assert (margin, pairs, shear) == (knobs['margin'], knobs['pairs'], knobs['shear']) and method == knobs.get('method', 'auto')
    try:
        engine.set_exp_mode('table')
        probe = CubeRunner(axes, (1, 2), np.zeros((1, 2 * N_CHAN)), np.full((1, 2), noise), ut, ncomp=2)
        model, _ = probe.predict_batch(np.zeros(n_pix, dtype=np.int32), truths)
        cube = CubeRunner(axes, (1, 2), model + rng.normal(0, noise, model.shape), np.full((n_pix, 2), noise), ut, ncomp=2)
        kw = dict(nlive=150, tol=0.5, efr=0.3, seed=7, maxiter=900, batch_target=2048, precision=precision)
        seen = Rounds()
        dev = sampler.fit_pixels(cube, np.arange(n_pix), device=True, **kw)
        twin = sampler.fit_pixels(cube, np.arange(n_pix), device=False, progress=seen, **kw)
        print(f'\n{precision}: n_iter {[t.n_iter for t in twin]}, n_evals {[t.n_evals for t in twin]}, refits {seen.refits.tolist()}, walked {seen.walked.tolist()}')
        for d, t in zip(dev, twin):
            assert (d.n_iter, d.n_evals) == (t.n_iter, t.n_evals), (precision, d.n_iter, t.n_iter, d.n_evals, t.n_evals)
            assert d.lnZ == pytest.approx(t.lnZ, rel=1e-10)
            np.testing.assert_allclose(d.posterior, t.posterior, rtol=1e-8, atol=1e-12)
        assert (seen.refits >= 3).all()
        if precision == 'evidence':
            assert not seen.walked.any()
    finally:
        engine.set_exp_mode('fast')
