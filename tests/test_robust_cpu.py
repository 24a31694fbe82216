"""A robust likelihood (Student-t channel noise, `robust=`, nfa_specset_set_robust) without a device: the
argument checks and every refused combination on the host, `_model`'s numpy twin of the device's difference form against the
direct sum of tests/robust_restatement.py, the Gaussian limit, the outlier diagnostic, `estimate_tails`, the store's
attribute, the fused kernels' refusal through the compiled launch plan, and the science case on a grid.

The science case (robust_restatement.spiked_line: N = 300, sigma = 0.2, a line of peak 1.0 and sigma = 3 channels at channel
150, spikes of +12 and +9 sigma at channels 153 and 155, noise seeds 0..7, peaks 0.5..1.5 by 0.01 and centres 148..152 by
0.05), the restatement's own figures:

    likelihood          fitted peak        |peak - 1| over the seeds   fitted centre   |centre - 150| over the seeds
    Gaussian (nu = 0)   1.47 +- 0.03       0.43 .. 0.50                151.99          1.90 .. 2.00 (the grid's edge)
    Student-t, nu = 4   1.01 +- 0.05       0.01 .. 0.08                150.04          0.00 .. 0.65

and on the same data without the spikes the width 1 / sqrt(-d^2 lnL / d peak^2) at the optimum is 0.0867 under the Gaussian
likelihood and 0.084 .. 0.108 under the t (ratios 0.97 .. 1.25: the t likelihood of Gaussian data has the Fisher information
(nu + 1) / (nu + 3) = 5 / 7 in expectation, a width 1.18 times the Gaussian one).  The thresholds below lie between the two
likelihoods' figures: 0.3 and 0.15 in the peak, 1.5 and 1.0 channels in the centre, 0.9 .. 1.35 for the widths' ratio.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import robust_restatement as rr
from test_launch_plan import FusedPlan, ROOT, knobs, shape


# ---------------------------------------------------------------------------- the argument checks
def test_the_argument_checks():
    from nestfit_amd._model import check_robust
    assert check_robust(None) is None and check_robust(0, 2) is None and check_robust([0.0, 0.0], 2) is None
    assert np.array_equal(check_robust(4, 2), [4.0, 4.0]) and check_robust(4, 2).dtype == np.float64
    assert np.array_equal(check_robust([4, 0], 2), [4.0, 0.0]) and np.array_equal(check_robust(np.array([2.0, 10.0])), [2.0, 10.0])
    assert np.array_equal(check_robust([1, 1e6], 2), [1.0, 1e6])                # the ends of the domain
    for bad, why in ((0.5, 'robust must be'), (-4, 'robust must be'), (1e6 + 1, 'robust must be'), (np.nan, 'robust must be'),
                     (np.inf, 'robust must be'), ([4.0, np.nan], 'robust must be'), ([4.0, 0.99], 'robust must be'),
                     ([4, 4, 4], '3 values for 2 spectra'), ('heavy', 'robust must be'), (True, 'robust must be'), ([], 'robust must be'),
                     (np.ones((2, 2)), 'robust must be')):
        with pytest.raises(ValueError, match=why):
            check_robust(bad, 2)
    # every refused combination, and their neutral values, which pass
    for kw in ({'baseline_order': 1}, {'calibration': 0.1}, {'correlation': (0.5, 0.25)}, {'response': (0.25, 0.5, 0.25)},
               {'templates': [np.ones((1, 8)), None]}, {'noise_uncertainty': 0.1}, {'continuum': [3.0, 0.0]}):
        with pytest.raises(ValueError, match='a robust likelihood'):
            check_robust(4, 2, **kw)
        assert check_robust(0, 2, **kw) is None                                  # no robust likelihood: nothing to refuse
    assert check_robust(4, 2, baseline_order=None, calibration=0.0, correlation=(0, 0), response=(0, 1, 0), templates=[None, None],
                        noise_uncertainty=0.0, continuum=np.zeros(2)) is not None


def test_the_runners_refuse_before_any_device_call():
    """`from_data`, `CubeRunner` and `CubeFitter` raise ValueError on the host -- this machine has no device to ask."""
    import nestfit_amd as na
    from nestfit_amd.cube import CubeRunner
    x = np.linspace(1.0e11, 1.0001e11, 32)
    rows = [[x, np.zeros(32), 0.1, 1], [x, np.zeros(32), 0.1, 2]]
    cases = (({'robust': 0.5}, 'robust must be'), ({'robust': [4.0]}, '1 values for 2 spectra'),
             ({'robust': 4, 'baseline_order': 0}, 'a robust likelihood'), ({'robust': 4, 'calibration': 0.1}, 'a robust likelihood'),
             ({'robust': 4, 'correlation': na.HANNING}, 'a robust likelihood'), ({'robust': 4, 'response': na.HANNING_RESPONSE}, 'a robust likelihood'),
             ({'robust': 4, 'templates': [na.ripple(32, 9.3), None]}, 'a robust likelihood'),
             ({'robust': 4, 'noise_uncertainty': 0.1}, 'a robust likelihood'), ({'robust': 4, 'continuum': 3.0}, 'a robust likelihood'))
    for kw, why in cases:
        with pytest.raises(ValueError, match=why):
            na.AmmoniaRunner.from_data(rows, None, **kw)
        with pytest.raises(ValueError, match=why):
            CubeRunner([x, x], (1, 2), np.zeros((1, 64)), np.full((1, 2), 0.1), None, **kw)
    with pytest.raises(ValueError, match='robust must be'):
        na.GaussianRunner.from_data([x, np.zeros(32), 0.1, 1.00005e11], None, robust=-1)
    with pytest.raises(ValueError, match='a robust likelihood'):
        na.GaussianRunner.from_data([x, np.zeros(32), 0.1, 1.00005e11], None, robust=4, baseline_order=1)


def test_the_fitter_checks_robust_before_any_pixel():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    from test_continuum_cpu import _stack
    stack = _stack((None, None))
    assert np.array_equal(CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'robust': 4}).robust, [4.0, 4.0])
    assert CubeFitter(stack, None, na.AmmoniaRunner).robust is None
    CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'robust': (4, 0), 'layered': True})
    for kw in ({'calibration': 0.1}, {'correlation': na.HANNING}, {'response': na.HANNING_RESPONSE}, {'baseline_order': 1},
               {'templates': [na.ripple(48, 9.3), None]}, {'noise_uncertainty': 0.1}):
        with pytest.raises(ValueError, match='a robust likelihood'):
            CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'robust': 4, **kw})
    with pytest.raises(ValueError, match='a robust likelihood'):
        CubeFitter(_stack((3.0, None)), None, na.AmmoniaRunner, runner_kwargs={'robust': 4})
    with pytest.raises(ValueError, match='robust must be'):
        CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'robust': 0.2})


def test_the_new_entry_points_are_declared():
    text = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert 'int nfa_specset_set_robust(nfa_specset *ss, const double *nu);' in text
    assert 'int nfa_specset_robust(const nfa_specset *ss, double *out);' in text
    from nestfit_amd import _ffi
    assert 'nfa_specset_set_robust' in _ffi.SIGNATURES and 'nfa_specset_robust' in _ffi.SIGNATURES


# ---------------------------------------------------------------------------- the difference form
def _random_case(rng, it):
    nu = (1, 2, 4, 10, 100)[it % 5]
    n = int(rng.integers(5, 300))
    noise = rng.uniform(0.1, 0.3, n) if it % 2 else 0.2
    if it % 4 == 1:
        noise[rng.integers(0, n, 3)] = np.inf
    j = np.arange(n)
    p = rng.uniform(0.2, 3.0) * np.exp(-0.5 * ((j - rng.integers(0, n)) / 2.0) ** 2)
    d = p * rng.uniform(0.0, 1.2) + rng.normal(0, 0.2, n)
    k = int(rng.integers(0, n))
    d[k] += rng.uniform(5.0, 40.0) * 0.2                                        # a spike of 5 .. 40 sigma
    if it % 3 == 0:
        p[k] += d[k]                                                            # ... that the model matches
    d = np.where(np.isfinite(np.broadcast_to(noise, (n,))), d, 0.0)
    return d, p, noise, nu


def test_the_twin_of_the_difference_form_against_the_direct_sum():
    """-(nu + 1) / 2 (sum log1p(a d^2) + sum log1p(p (g p - 2 g d))) in fp64 against the direct sum in longdouble: within
    1e-14 M over 200 cases -- nu of 1 .. 100, weights, masks, spikes of 5 .. 40 sigma, models that match a spike."""
    from nestfit_amd._model import robust_lnl
    rng = np.random.default_rng(1)
    worst = 0.0
    for it in range(200):
        d, p, noise, nu = _random_case(rng, it)
        want, M = float(rr.lnl_spectrum(d, p, noise, nu)[0]), float(rr.magnitude_spectrum(d, p, noise, nu)[0])
        worst = max(worst, abs(robust_lnl(d, p, noise, nu) - want) / M)
    print(f'the twin against the direct sum: worst |got - want| / M {worst:.2e} (bound 1e-14)')
    assert worst <= 1e-14
    # nu = 0 is the Gaussian half chi^2, and the restatement says the same
    d, p, noise, _ = _random_case(rng, 1)
    assert robust_lnl(d, p, noise, 0) == pytest.approx(float(rr.lnl_spectrum(d, p, noise, 0)[0]), rel=1e-13)


def test_the_gaussian_limit():
    """nu = 1e6 against half_chi2.  log1p(x) lies in [x - x^2 / 2, x], so with z = r / sigma the value is -(1 + 1 / nu) h times a
    factor in [1 - max z^2 / (2 nu), 1]: |lnL + h| <= h (1 / nu + (1 + 1 / nu) max z^2 / (2 nu))."""
    from nestfit_amd._model import half_chi2, robust_lnl
    rng = np.random.default_rng(3)
    n, nu = 200, 1e6
    p = np.exp(-0.5 * ((np.arange(n) - 100) / 3.0) ** 2)
    for noise in (0.2, rng.uniform(0.1, 0.3, n)):
        d = p + rng.normal(0, 1, n) * noise
        h = half_chi2(d, p, noise)[0]
        z2 = np.max(((d - p) / noise) ** 2)
        dev = abs(robust_lnl(d, p, noise, nu) + h) / h
        assert 0 < dev <= 1 / nu + (1 + 1 / nu) * z2 / (2 * nu) and dev < 2e-5, (dev, z2)
        assert abs(float(rr.lnl_spectrum(d, p, noise, nu)[0]) + h) / h <= 1 / nu + (1 + 1 / nu) * z2 / (2 * nu)


def test_the_prefactor_is_the_t_normalisation():
    """exp(prefactor + lnL) integrates to 1 over one channel's datum, scalar noise and a noise per channel with a mask."""
    import nestfit_amd as na
    from nestfit_amd._model import robust_lnl
    x = np.linspace(1.0e11, 1.0001e11, 3)
    for noise, live in ((0.3, 3), (np.array([0.2, np.inf, 0.5]), 2)):
        s = na.core.Spectrum(x, np.zeros(3), noise, rest_freq=1.00005e11)
        white = s.prefactor
        s.set_robust(4)
        per_channel = []
        for k in range(3):
            sig = np.broadcast_to(noise, (3,))[k]
            if not np.isfinite(sig):
                continue
            grid = np.linspace(-400 * sig, 400 * sig, 400001)
            dens = np.exp(-2.5 * np.log1p(grid ** 2 / (4 * sig ** 2)))          # exp(lnL) of one channel at p = 0
            per_channel.append(np.log(np.sum(dens) * (grid[1] - grid[0])))
        assert len(per_channel) == live and s.prefactor == pytest.approx(-sum(per_channel), rel=1e-5) and s.robust == 4.0
        assert robust_lnl(np.zeros(3), np.zeros(3), noise, 4) == 0.0
        s.set_robust(None)
        assert s.prefactor == white and s.robust is None


# ---------------------------------------------------------------------------- diagnostics
def test_the_outlier_factors_on_a_spiked_spectrum():
    from nestfit_amd._model import robust_outliers
    j, data, clean = rr.spiked_line(0)
    w = robust_outliers(data, clean, 0.2, 4)
    # (nu + 1) / (nu + z^2) with z = 12 and 9 give or take three sigma of noise: below 5 / (4 + 81) and 5 / (4 + 36)
    assert w.shape == data.shape and w[153] < 0.059 and w[155] < 0.125
    rest = np.delete(w, [153, 155])
    assert rest.min() > 0.25 and 0.9 < np.median(rest) <= 1.25 and rest.max() <= 1.25
    assert np.array_equal(np.argsort(w)[:2], [153, 155])
    # a noise per channel with a mask; a Gaussian spectrum trusts every channel alike
    noise = np.full(300, 0.2)
    noise[10] = np.inf
    wm = robust_outliers(data, clean, noise, 4)
    assert np.isnan(wm[10]) and np.array_equal(np.delete(wm, 10), np.delete(w, 10))
    assert np.array_equal(robust_outliers(data, clean, 0.2, 0), np.ones(300))


def test_estimate_tails():
    from nestfit_amd.cubeio import estimate_tails
    rng = np.random.default_rng(5)
    free = np.r_[0:100, 200:300]
    gauss = rng.normal(0, 0.3, (6, 8, 300))
    gauss[..., 100:200] += 5.0                                                  # a line outside the line-free channels
    assert estimate_tails(gauss, free) is None
    heavy = 0.3 * rng.standard_t(6, (6, 8, 300))
    nu = estimate_tails(heavy, free)
    assert nu is not None and 4.0 < nu < 12.0                                   # kappa = 3 for nu = 6, a noisy statistic
    assert 4.0 < estimate_tails(0.3 * rng.standard_t(3, (6, 8, 300)), free) < 6.0       # no fourth moment: a little above 4
    spiked = rng.normal(0, 0.3, (6, 8, 300))
    spiked[:, :, 7] += 4.0                                                      # one bad channel in every pixel
    assert 4.0 < estimate_tails(spiked, slice(0, 100)) < 8.0
    # pixels with a NaN are left out; too few channels is an error
    heavy[0, 0, 5] = np.nan
    assert estimate_tails(heavy, free) is not None
    with pytest.raises(ValueError, match='8 line-free channels'):
        estimate_tails(gauss, slice(0, 5))


# ---------------------------------------------------------------------------- the store
class _Fitter:
    """What insert_fitter_pars reads of a fitter."""
    lnZ_thresh, ncomp_max, nlive_snr_fact, nlive_quantum = 11, 2, 5, 1
    mn_kwargs = {'nlive': 100, 'tol': 1.0, 'seed': 5}

    def __init__(self, stack, runner_kwargs):
        self.stack, self.runner_kwargs = stack, runner_kwargs


@pytest.mark.parametrize('form', ['npz', 'hdf5'])
def test_the_store_carries_the_degrees_of_freedom(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import store as st
    from test_continuum_cpu import _stack
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    stack = _stack((None, None))
    for name, kw, want in (('all', {'robust': 4}, [4.0, 4.0]), ('one', {'robust': (0, 2.5)}, [0.0, 2.5]), ('none', {}, None),
                           ('zeros', {'robust': 0}, None)):
        path = str(tmp_path / f'{name}_{form}')
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter(stack, kw))
        with st.HdfStore(path) as store:
            got = store.read_model_robust()
            assert ('robust_dof' in store.hdf.attrs) == (want is not None)
            if want is None:
                assert got is None
            else:
                assert got.dtype == np.float64 and np.array_equal(got, want)


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void fused13(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, int templates, int continuum, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0,
                      templates != 0, continuum != 0);
}
void fused14(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, int templates, int continuum, int robust, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0,
                      templates != 0, continuum != 0, robust != 0);
}
int size_of(int i) {
    const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan), (int)LNL_KINDS, (int)LNL_INSTANCES};
    return s[i];
}
}
'''


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('plan_rob')
    src, so = tmp / 'plan_rob.cpp', tmp / 'libplan_rob.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return C.CDLL(str(so))


def test_the_table_and_the_structures_are_what_they_were(plan):
    from test_launch_plan import LnlPlan, LpLaunch
    assert [plan.size_of(i) for i in range(5)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan), 32, 1024]


def test_the_fused_kernels_refuse_a_robust_set_first_of_all(plan):
    """A robust set is weighted to its kernels: without a reason of its own the refusal would speak of a noise per channel,
    and a point that reached a kernel which sums t would be given a chi^2.  Whatever else the set is -- layered, filled, wide
    -- the reason is the robust likelihood's.  Without the argument, and with it false, the plan is what it was."""
    s, k = shape(n_spec=2, size=300, ncomp=2), knobs()
    reason = b'the resident kernel has no form for a robust likelihood: use nfa_ring_serve'
    for mode in (0, 2):
        #        bl wt banded filled layered calibrated correlated response templates continuum
        for flags in ((0, 1, 0, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 1, 0, 0, 0, 0, 0), (0, 1, 0, 1, 1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0, 0, 0, 0, 0),
                      (0, 0, 0, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 1, 1, 1, 1, 1)):
            with_r, without, thirteen = FusedPlan(), FusedPlan(), FusedPlan()
            plan.fused14(C.byref(s), C.byref(k), mode, *flags, 1, C.byref(with_r))
            plan.fused14(C.byref(s), C.byref(k), mode, *flags, 0, C.byref(without))
            plan.fused13(C.byref(s), C.byref(k), mode, *flags, C.byref(thirteen))
            assert with_r.refusal == reason and with_r.ring_error == reason
            assert bytes(without) == bytes(thirteen) and without.refusal != reason
        plain = FusedPlan()
        plan.fused14(C.byref(s), C.byref(k), mode, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, C.byref(plain))
        assert plain.refusal is None


# ---------------------------------------------------------------------------- the science case
PEAKS, CENTRES = np.linspace(0.5, 1.5, 101), np.linspace(148.0, 152.0, 81)
SEEDS = range(8)


def _width(lnl):
    """1 / sqrt(-d^2 lnL / d peak^2) at the grid's optimum, by the second difference."""
    b = int(np.argmax(lnl.max(axis=0)))
    a = min(max(int(np.argmax(lnl[:, b])), 1), len(PEAKS) - 2)
    h = PEAKS[1] - PEAKS[0]
    return 1.0 / np.sqrt(-(lnl[a + 1, b] - 2.0 * lnl[a, b] + lnl[a - 1, b]) / (h * h))


def test_spikes_drag_the_gaussian_fit_and_not_the_robust_one():
    """The figures of the module's docstring, seed by seed."""
    fits = {0: [], 4: []}
    for seed in SEEDS:
        _, data, _ = rr.spiked_line(seed)
        assert data[153] > 9 * 0.2 and data[155] > 6 * 0.2
        for nu in fits:
            fits[nu].append(rr.grid_fit(data, 0.2, nu, PEAKS, CENTRES)[:2])
    g, t = np.array(fits[0]), np.array(fits[4])
    print(f'spiked: Gaussian peak {g[:, 0].mean():.2f} +- {g[:, 0].std():.2f} centre {g[:, 1].mean():.2f}; '
          f't(4) peak {t[:, 0].mean():.2f} +- {t[:, 0].std():.2f} centre {t[:, 1].mean():.2f}')
    assert (np.abs(g[:, 0] - 1.0) > np.abs(t[:, 0] - 1.0)).all() and (np.abs(g[:, 1] - 150.0) > np.abs(t[:, 1] - 150.0)).all()
    assert (np.abs(g[:, 0] - 1.0) > 0.3).all() and (np.abs(t[:, 0] - 1.0) < 0.15).all()
    assert (np.abs(g[:, 1] - 150.0) > 1.5).all() and (np.abs(t[:, 1] - 150.0) < 1.0).all()


def test_robustness_costs_little_on_clean_data():
    for seed in SEEDS:
        _, data, _ = rr.spiked_line(seed, spikes=())
        pg, cg, lg = rr.grid_fit(data, 0.2, 0, PEAKS, CENTRES)
        pt, ct, lt = rr.grid_fit(data, 0.2, 4, PEAKS, CENTRES)
        assert abs(pg - pt) < 0.17 and abs(cg - ct) < 0.5, seed                 # within two Gaussian widths (0.087) of each other
        ratio = _width(lt) / _width(lg)
        assert 0.9 < ratio < 1.35, (seed, ratio)
