"""Channel noise correlated along the spectral axis: what can be checked without a GPU.

The closed-form pentadiagonal inverse and determinant of the AR(2) correlation matrix against dense numpy; Yule-Walker;
`check_correlation`; `estimate_correlation` on true AR(2) noise; the calibration of the likelihood with the restatement
(tests/corr_restatement.py); the store's attribute; the fused kernels' refusal through a compiled shim of csrc/nfa_launch_plan.h.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import corr_restatement as cs
from test_launch_plan import FusedPlan, ROOT, knobs, shape

RHOS = {'hanning': (2.0 / 3.0, 1.0 / 6.0), 'ar1': (0.5, 0.25), 'mixed': (0.3, -0.2), 'negative': (-0.4, 0.3), 'strong': (0.9, 0.7)}
SIZES = (4, 5, 63, 130)


# ---------------------------------------------------------------------------- the closed forms
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', list(RHOS))
def test_the_closed_form_bands_against_the_dense_inverse(name, n):
    """Q = diag(u) R^-1 diag(u) with unequal sigma_c: the three bands from `corr_bands`, every other entry of the dense inverse
    zero, and ln det R."""
    import nestfit_amd as na
    from nestfit_amd._model import corr_bands, corr_lndet
    assert na.HANNING == RHOS['hanning'] and na.ar1(0.5) == RHOS['ar1']
    rho = RHOS[name]
    sigma = np.random.default_rng(n).uniform(0.1, 0.4, n)
    u = sigma.min() / sigma
    dense = sigma.min() ** 2 * np.linalg.inv(cs.covariance(sigma, rho, n))
    d0, d1, d2 = corr_bands(*rho, n)
    Q = np.diag(u * u * d0) + np.diag(u[:-1] * u[1:] * d1, 1) + np.diag(u[:-1] * u[1:] * d1, -1) \
        + np.diag(u[:-2] * u[2:] * d2, 2) + np.diag(u[:-2] * u[2:] * d2, -2)
    scale = np.abs(dense).max()
    cond = np.linalg.cond(cs.corr_matrix(rho, n))
    assert np.abs(Q - dense).max() <= 8 * cond * np.finfo(float).eps * scale, (np.abs(Q - dense).max() / scale, cond)
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    assert np.abs(dense[idx > 2]).max(initial=0.0) <= 8 * cond * np.finfo(float).eps * scale
    sign, lndet = np.linalg.slogdet(cs.corr_matrix(rho, n))
    assert sign == 1.0 and corr_lndet(*rho, n) == pytest.approx(lndet, abs=1e-11 * n)


@pytest.mark.parametrize('name', list(RHOS))
def test_yule_walker_returns_the_two_autocorrelations(name):
    """The AR(2) process of (phi_1, phi_2, v) has rho_1 = phi_1 / (1 - phi_2), rho_2 = phi_1 rho_1 + phi_2 and variance
    v / (1 - phi_1 rho_1 - phi_2 rho_2) = 1; and 100 000 simulated samples of the recursion show them."""
    from nestfit_amd._model import yule_walker
    r1, r2 = RHOS[name]
    phi1, phi2, v = yule_walker(r1, r2)
    assert phi1 / (1.0 - phi2) == pytest.approx(r1, abs=1e-14) and phi1 * r1 + phi2 == pytest.approx(r2, abs=1e-14)
    assert v / (1.0 - phi1 * r1 - phi2 * r2) == pytest.approx(1.0, abs=1e-14) and v > 0
    rng = np.random.default_rng(9)
    e = rng.normal(0, np.sqrt(v), 101000)
    x = np.zeros_like(e)
    for k in range(2, e.size):
        x[k] = phi1 * x[k - 1] + phi2 * x[k - 2] + e[k]
    x = x[1000:]
    for k, want in ((1, r1), (2, r2)):
        assert float(np.mean(x[:-k] * x[k:]) / np.mean(x * x)) == pytest.approx(want, abs=5 * cs.bartlett_se((r1, r2), k, x.size))
    assert float(np.var(x)) == pytest.approx(1.0, rel=0.1)


# ---------------------------------------------------------------------------- the argument
def test_check_correlation_refuses_before_any_device_call(monkeypatch):
    """(No library is loaded here: `_ffi.load` and `_ffi.engine` fail if anything reaches them.)"""
    import nestfit_amd as na
    from nestfit_amd import _ffi
    from nestfit_amd._model import check_correlation
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import freq_axis

    def no_library(*a, **k):
        raise AssertionError('a device call')
    monkeypatch.setattr(_ffi, 'load', no_library)
    monkeypatch.setattr(_ffi, 'engine', no_library)
    assert check_correlation(None) is None and check_correlation((0, 0), 2) is None and check_correlation(np.zeros((2, 2)), 2) is None
    out = check_correlation(na.HANNING, 3)
    assert out.dtype == np.float64 and out.shape == (3, 2) and np.array_equal(out, np.tile(na.HANNING, (3, 1)))
    # a one-dimensional value is one pair, never one number per spectrum
    assert np.array_equal(check_correlation([0.5, 0.25], 2), [[0.5, 0.25], [0.5, 0.25]])
    assert np.array_equal(check_correlation(np.array([0.5, 0.25])), [[0.5, 0.25]])
    assert np.array_equal(check_correlation([na.HANNING, (0, 0)], 2), [na.HANNING, (0.0, 0.0)])
    for value in ('a', 0.5, [0.5], [0.5, 0.25, 0.1], [[0.5, 0.25, 0.1]], np.zeros((2, 2, 2)), {'a': 1}, [0.5, None], np.array([True, False]), []):
        with pytest.raises(ValueError, match='correlation must be'):
            check_correlation(value, 2)
    with pytest.raises(ValueError, match='3 pairs for 2 spectra'):
        check_correlation(np.tile(na.HANNING, (3, 1)), 2)
    for value, why in (((np.nan, 0.1), 'finite'), ((0.5, np.inf), 'finite'), ((1.0, 0.5), r'\|rho_1\| < 1'), ((-1.2, 0.5), r'\|rho_1\| < 1'),
                       ((0.9, 0.6), 'positive definite'), ((0.5, 1.0), 'positive definite'), ((0.5, -0.5), 'positive definite'),
                       ((0.99, 0.965), 'innovations variance'), ([na.HANNING, (0.995, 0.985)], 'innovations variance')):
        with pytest.raises(ValueError, match=why):
            check_correlation(value, 2)
    # what a correlation does not go with
    with pytest.raises(ValueError, match='masked channels'):
        check_correlation(na.HANNING, 1, masked=True)
    with pytest.raises(ValueError, match='baseline'):
        check_correlation(na.HANNING, 1, baseline_order=0)
    with pytest.raises(ValueError, match='calibration'):
        check_correlation(na.HANNING, 1, calibration=[0.1])
    with pytest.raises(ValueError, match='4 channels'):
        check_correlation(na.HANNING, 2, sizes=[64, 3])
    assert check_correlation((0, 0), 1, masked=True, baseline_order=2, calibration=[0.1], sizes=[2]) is None      # no correlation: nothing to refuse
    assert check_correlation(na.HANNING, 1, baseline_order=-1, calibration=[0.0], sizes=[4]) is not None
    # every runner's from_data and the cube runner: before the spectra are made
    from mix_restatement import test_species as species
    from test_lte_bands_cpu import band_axis
    mol, ks, iso, isos = species(na)
    x, xa = band_axis(ks[0].nu, 64), freq_axis(1, 64)
    line = na.LineTable(1e11, [0.0], [1.0])
    rows = {
        na.AmmoniaRunner: [[xa, np.zeros(64), 0.1, 1]],
        na.DiazenyliumRunner: [[xa, np.zeros(64), 0.1, 1]],
        na.HyperfineRunner: [[x, np.zeros(64), 0.1, line]],
        na.LteRunner: [[x, np.zeros(64), 0.1, ks[0]]],
        na.LteMix([mol, iso]).Runner: [[x, np.zeros(64), 0.1, na.LteBlend(ks + isos)]],
        na.LteMix([mol], fill=True).Runner: [[x, np.zeros(64), 0.1, ks[0]]],
    }
    for cls, spec_data in rows.items():
        for value in ('a', 0.5, (1.0, 0.5), (0.9, 0.6), (np.nan, 0.0)):
            with pytest.raises(ValueError, match='correlation'):
                cls.from_data(spec_data, None, correlation=value)
        with pytest.raises(ValueError, match='baseline'):
            cls.from_data(spec_data, None, correlation=na.HANNING, baseline_order=1)
        with pytest.raises(ValueError, match='calibration'):
            cls.from_data(spec_data, None, correlation=na.HANNING, calibration=0.1)
        holed = np.full(64, 0.1)
        holed[9] = np.inf
        with pytest.raises(ValueError, match='masked channels'):                 # (before the spectra and their device sets are made)
            cls.from_data([[spec_data[0][0], np.zeros(64), holed, spec_data[0][3]]], None, correlation=na.HANNING)
        with pytest.raises(ValueError, match='4 channels'):
            cls.from_data([[spec_data[0][0][:3], np.zeros(3), 0.1, spec_data[0][3]]], None, correlation=na.HANNING)
    for value in ('a', (1.0, 0.5)):
        with pytest.raises(ValueError, match='correlation'):
            na.GaussianRunner.from_data([xa, np.zeros(64), 0.1, 2.3e10], None, correlation=value)
        with pytest.raises(ValueError, match='masked channels'):
            na.GaussianRunner.from_data([xa, np.zeros(64), np.where(np.arange(64) == 5, np.inf, 0.1), 2.3e10], None, correlation=na.HANNING)
        with pytest.raises(ValueError, match='correlation'):
            CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, correlation=value)
    noise = np.full((1, 64), 0.1)
    noise[0, 5] = np.inf
    with pytest.raises(ValueError, match='masked channels'):
        CubeRunner([xa], [1], np.zeros((1, 64)), noise, None, correlation=na.HANNING)
    with pytest.raises(ValueError, match='baseline'):
        CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, correlation=na.HANNING, baseline_order=0)
    with pytest.raises(ValueError, match='calibration'):
        CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, correlation=na.HANNING, calibration=0.1)
    for name in ('nfa_specset_set_correlation', 'nfa_specset_correlation'):
        assert name in _ffi.SIGNATURES


def test_the_cube_fitter_checks_the_keyword():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    from mix_restatement import test_species as species
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = species(na)
    stack = _stack(na, [na.LteBlend(ks + isos), isos[1]])
    mix = na.LteMix([mol, iso])
    assert CubeFitter(stack, None, mix.Runner).correlation is None
    assert CubeFitter(stack, None, mix.Runner, runner_kwargs={'correlation': (0, 0)}).correlation is None
    assert np.array_equal(CubeFitter(stack, None, mix.Runner, runner_kwargs={'correlation': na.HANNING}).correlation, [na.HANNING] * 2)
    for kw in ({'correlation': 0.5}, {'correlation': (1.0, 0.2)}, {'correlation': na.HANNING, 'baseline_order': 1},
               {'correlation': na.HANNING, 'calibration': 0.1}):
        with pytest.raises(ValueError, match='correlation'):
            CubeFitter(stack, None, mix.Runner, runner_kwargs=kw)


def test_the_spectrum_prefactor_gains_the_determinant():
    import nestfit_amd as na
    from nestfit_amd.core import Spectrum
    x = np.linspace(1e10, 1.0001e10, 50)
    for noise in (0.3, np.random.default_rng(1).uniform(0.1, 0.5, 50)):
        s = Spectrum(x, np.zeros(50), noise)
        white = s.prefactor
        s.set_correlation(na.HANNING)
        C = cs.covariance(noise, na.HANNING, 50)
        assert s.prefactor == pytest.approx(-0.5 * np.linalg.slogdet(2 * np.pi * C)[1], rel=1e-12) and s.correlation == na.HANNING
        s.set_correlation((0.0, 0.0))
        assert s.prefactor == white and s.correlation is None
        s.set_correlation(na.ar1(0.5)), s.set_correlation(None)
        assert s.prefactor == white


# ---------------------------------------------------------------------------- estimate_correlation
@pytest.mark.parametrize('name', ['hanning', 'mixed', 'negative'])
def test_estimate_correlation_recovers_the_pair(name):
    """Seeded true AR(2) noise, 12 x 10 pixels of 200 channels of which the middle 60 hold a line: both estimates within five
    standard errors (Bartlett's formula from the true autocorrelations, the number of products that were averaged)."""
    from nestfit_amd.cubeio import estimate_correlation
    rho = RHOS[name]
    rng = np.random.default_rng(17)
    cube = 0.3 * cs.ar2_noise(rng, rho, (12, 10, 200)) + rng.normal(0, 1, (12, 10, 1))          # an offset per pixel
    cube[..., 70:130] += 5.0 * np.exp(-0.5 * ((np.arange(60) - 30) / 8.0) ** 2)
    line_free = np.ones(200, dtype=bool)
    line_free[70:130] = False
    got = estimate_correlation(cube, line_free)
    again = estimate_correlation(cube, np.flatnonzero(line_free))
    assert got == again and len(got) == 2
    for k, want in ((1, rho[0]), (2, rho[1])):
        n_pairs = 120 * int((line_free[:-k] & line_free[k:]).sum())
        se = cs.bartlett_se(rho, k, n_pairs)
        print(f'{name} rho_{k}: {got[k - 1]:+.4f} (true {want:+.4f}, standard error {se:.4f})')
        assert abs(got[k - 1] - want) <= 5 * se
    with pytest.raises(ValueError, match='8 line-free channels'):
        estimate_correlation(cube, slice(0, 5))


# ---------------------------------------------------------------------------- the calibration of the likelihood, on the CPU
def test_the_likelihood_is_calibrated_with_the_correlation_and_not_without():
    """512 pixels of true AR(2) noise with Hanning's pair, N = 256: -2 lnL at p = 0 by the restatement.  With the correlation its
    mean is N within four standard errors and its variance 2N within [0.75, 1.25] (four standard errors of sqrt(2 / 511)); the
    white likelihood's variance is 2N sum_k rho_k^2 ~ 2.2 times 2N."""
    rho = RHOS['hanning']
    data = cs.calibration_pixels(rho)
    zero = np.zeros(cs.CAL_N)
    with_corr = [-2.0 * cs.lnl(d, zero, cs.CAL_SIGMA, rho) for d in data]
    white = [-2.0 * cs.lnl(d, zero, cs.CAL_SIGMA, (0.0, 0.0)) for d in data]
    mean, z, ratio = cs.calibration_figures(with_corr)
    wmean, wz, wratio = cs.calibration_figures(white)
    print(f'with the correlation: mean {mean:.2f} ({z:+.2f} standard errors from {cs.CAL_N}), variance / 2N {ratio:.3f}; '
          f'white: mean {wmean:.2f}, variance / 2N {wratio:.3f}')
    assert abs(z) <= 4.0 and 0.75 <= ratio <= 1.25
    assert wratio > 1.6


# ---------------------------------------------------------------------------- the store
class _Fitter:
    """What insert_fitter_pars reads of a fitter."""
    lnZ_thresh, ncomp_max, nlive_snr_fact, nlive_quantum = 11, 2, 5, 1
    mn_kwargs = {'nlive': 100, 'tol': 1.0, 'seed': 5}

    class stack:
        cubes = [None, None, None]

    def __init__(self, runner_kwargs):
        self.runner_kwargs = runner_kwargs


@pytest.mark.parametrize('form', ['npz', 'hdf5'])
def test_the_store_carries_the_correlation(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import store as st
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    h = RHOS['hanning']
    cases = {'pair': (h, [h, h, h]), 'each': ([h, (0, 0), (0.3, -0.2)], [h, (0.0, 0.0), (0.3, -0.2)]), 'zeros': ((0, 0), None), 'none': (None, None),
             'absent': ('absent', None)}
    for name, (value, want) in cases.items():
        path = str(tmp_path / f'{name}_{form}')
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'layered': False} if value == 'absent' else {'correlation': value}))
        with st.HdfStore(path) as store:
            got = store.read_model_correlation()
            assert ('noise_correlation' in store.hdf.attrs) == (want is not None)
            if want is None:
                assert got is None
            else:
                assert got.dtype == np.float64 and got.shape == (3, 2) and np.array_equal(got, np.array(want))     # to the bit, in both forms
    with pytest.raises(ValueError, match='2 pairs for 3 spectra'):
        with st.HdfStore(str(tmp_path / f'bad_{form}'), nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'correlation': [h, h]}))


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void fused9(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0);
}
void fused10(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0);
}
int size_of(int i) { const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan), (int)LNL_KINDS, (int)LNL_INSTANCES}; return s[i]; }
}
'''


def test_the_fused_kernels_refuse_a_correlated_set_with_a_reason_of_its_own(tmp_path):
    from test_launch_plan import LnlPlan, LpLaunch
    src, so = tmp_path / 'plan.cpp', tmp_path / 'libplan.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    # the structures and the table of kinds are what they were
    assert [lib.size_of(i) for i in range(5)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan), 32, 1024]
    s, k = shape(n_spec=2, size=300, ncomp=2), knobs()
    for mode in (0, 2):
        for flags in ((0, 1, 0, 0, 0, 0), (0, 1, 0, 1, 1, 0), (0, 1, 1, 0, 0, 0)):
            with_corr, without = FusedPlan(), FusedPlan()
            lib.fused10(C.byref(s), C.byref(k), mode, *flags, 1, C.byref(with_corr))
            lib.fused10(C.byref(s), C.byref(k), mode, *flags, 0, C.byref(without))
            assert with_corr.refusal == b'the resident kernel has no form for correlated channel noise: use nfa_ring_serve'
            assert with_corr.ring_error == with_corr.refusal
            nine = FusedPlan()
            lib.fused9(C.byref(s), C.byref(k), mode, *flags, C.byref(nine))
            assert nine.refusal == without.refusal and nine.refusal is not None and b'correlated' not in nine.refusal


def test_the_new_entry_points_are_declared():
    text = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert 'int nfa_specset_set_correlation(nfa_specset *ss, const double *rho);' in text
    assert 'int nfa_specset_correlation(const nfa_specset *ss, double *out);' in text
