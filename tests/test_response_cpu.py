"""A channel response: what can be checked without a GPU.

`check_response` and where it is called; `correlation_of_response`; the restatement (tests/resp_restatement.py) against
numpy's convolution; the width bias that the response removes; the fused kernels' refusal through a compiled shim of
csrc/nfa_launch_plan.h; the store's attribute.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import resp_restatement as rr
from test_launch_plan import FusedPlan, ROOT, knobs, shape

BINOMIAL = tuple(np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0)
SKEW = (0.1, 0.2, 0.4, 0.25, 0.05)
IDENTITY5 = [0.0, 0.0, 1.0, 0.0, 0.0]


# ---------------------------------------------------------------------------- the argument
def test_check_response_refuses_before_any_device_call(monkeypatch):
    """(No library is loaded here: `_ffi.load` and `_ffi.engine` fail if anything reaches them.)"""
    import nestfit_amd as na
    from nestfit_amd import _ffi
    from nestfit_amd._model import check_response
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import freq_axis

    def no_library(*a, **k):
        raise AssertionError('a device call')
    monkeypatch.setattr(_ffi, 'load', no_library)
    monkeypatch.setattr(_ffi, 'engine', no_library)
    assert na.HANNING_RESPONSE == (0.25, 0.5, 0.25)
    # none, and the identity in every spelling
    assert check_response(None) is None and check_response((0, 1, 0), 2) is None and check_response(IDENTITY5, 2) is None
    assert check_response(np.tile(IDENTITY5, (2, 1)), 2) is None and check_response([(0, 1, 0), (0, 1, 0)], 2) is None
    # three taps are stored as five, with zero ends
    out = check_response(na.HANNING_RESPONSE, 3)
    assert out.dtype == np.float64 and out.shape == (3, 5) and out.flags.c_contiguous
    assert np.array_equal(out, np.tile([0.0, 0.25, 0.5, 0.25, 0.0], (3, 1)))
    assert np.array_equal(check_response(BINOMIAL, 2), np.tile(BINOMIAL, (2, 1)))
    assert np.array_equal(check_response(np.array(SKEW)), [SKEW])
    # a one-dimensional value is one response; an array gives one per spectrum, the identity beside real ones unfiltered
    assert np.array_equal(check_response([na.HANNING_RESPONSE, (0, 1, 0)], 2), [[0.0, 0.25, 0.5, 0.25, 0.0], IDENTITY5])
    assert np.array_equal(check_response(np.array([BINOMIAL, IDENTITY5]), 2), [BINOMIAL, IDENTITY5])
    for value in ('a', 0.5, [1.0], [0.5, 0.5], [0.25, 0.25, 0.25, 0.25], [0.1] * 7, [[0.2] * 4], np.zeros((2, 2, 3)), {'a': 1}, [0.5, None, 0.5],
                  np.array([False, True, False]), []):
        with pytest.raises(ValueError, match='response must be'):
            check_response(value, 2)
    with pytest.raises(ValueError, match='3 responses for 2 spectra'):
        check_response(np.tile(na.HANNING_RESPONSE, (3, 1)), 2)
    for value, why in (((np.nan, 0.5, 0.25), 'finite'), ((0.25, np.inf, 0.25), 'finite'), ((0.25, 0.5, 0.3), 'sum to 1'),
                       ((0.25, 0.5, 0.25 + 3e-9), 'sum to 1'), ((0.5, 0.0, 0.5), 'central tap'), ((0.6, -0.2, 0.6), 'central tap'),
                       ([na.HANNING_RESPONSE, (0.2, 0.5, 0.2)], 'sum to 1'), ((0.0, 0.5, 0.0, 0.5, 0.0), 'central tap')):
        with pytest.raises(ValueError, match=why):
            check_response(value, 2)
    assert check_response((0.25, 0.5, 0.25 + 5e-10), 1) is not None                         # within 1e-9 of 1
    # what a response does not go with: the messages name the channel response, never a correlation
    for kw, why in (({'masked': True}, 'masked channels'), ({'baseline_order': 0}, 'baseline'), ({'calibration': [0.1]}, 'calibration'),
                    ({'sizes': [64, 3]}, '4 channels')):
        with pytest.raises(ValueError, match=why) as err:
            check_response(na.HANNING_RESPONSE, 2 if 'sizes' in kw else 1, **kw)
        assert 'channel response' in str(err.value) and 'correlat' not in str(err.value)
    assert check_response((0, 1, 0), 1, masked=True, baseline_order=2, calibration=[0.1], sizes=[2]) is None      # no response: nothing to refuse
    assert check_response(na.HANNING_RESPONSE, 1, baseline_order=-1, calibration=[0.0], sizes=[4]) is not None
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
        for value in ('a', 0.5, (0.5, 0.5), (0.3, 0.5, 0.3), (0.5, 0.0, 0.5), (np.nan, 1.0, 0.0)):
            with pytest.raises(ValueError, match='response'):
                cls.from_data(spec_data, None, response=value)
        with pytest.raises(ValueError, match='channel response does not go with a baseline'):
            cls.from_data(spec_data, None, response=na.HANNING_RESPONSE, baseline_order=1)
        with pytest.raises(ValueError, match='channel response does not go with a calibration'):
            cls.from_data(spec_data, None, response=na.HANNING_RESPONSE, calibration=0.1)
        holed = np.full(64, 0.1)
        holed[9] = np.inf
        with pytest.raises(ValueError, match='channel response does not go with masked channels'):
            cls.from_data([[spec_data[0][0], np.zeros(64), holed, spec_data[0][3]]], None, response=na.HANNING_RESPONSE)
        with pytest.raises(ValueError, match='channel response needs spectra of 4 channels'):
            cls.from_data([[spec_data[0][0][:3], np.zeros(3), 0.1, spec_data[0][3]]], None, response=na.HANNING_RESPONSE)
    for value in ('a', (0.5, 0.0, 0.5)):
        with pytest.raises(ValueError, match='response'):
            na.GaussianRunner.from_data([xa, np.zeros(64), 0.1, 2.3e10], None, response=value)
        with pytest.raises(ValueError, match='masked channels'):
            na.GaussianRunner.from_data([xa, np.zeros(64), np.where(np.arange(64) == 5, np.inf, 0.1), 2.3e10], None, response=na.HANNING_RESPONSE)
        with pytest.raises(ValueError, match='response'):
            CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, response=value)
    noise = np.full((1, 64), 0.1)
    noise[0, 5] = np.inf
    with pytest.raises(ValueError, match='channel response does not go with masked channels'):
        CubeRunner([xa], [1], np.zeros((1, 64)), noise, None, response=na.HANNING_RESPONSE)
    with pytest.raises(ValueError, match='channel response does not go with a baseline'):
        CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, response=na.HANNING_RESPONSE, baseline_order=0)
    with pytest.raises(ValueError, match='channel response does not go with a calibration'):
        CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, response=na.HANNING_RESPONSE, calibration=0.1)
    for name in ('nfa_specset_set_response', 'nfa_specset_response'):
        assert name in _ffi.SIGNATURES


def test_the_cube_fitter_checks_the_keyword():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    from mix_restatement import test_species as species
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = species(na)
    stack = _stack(na, [na.LteBlend(ks + isos), isos[1]])
    mix = na.LteMix([mol, iso])
    assert CubeFitter(stack, None, mix.Runner).response is None
    assert CubeFitter(stack, None, mix.Runner, runner_kwargs={'response': (0, 1, 0)}).response is None
    fitter = CubeFitter(stack, None, mix.Runner, runner_kwargs=na.smoothed(na.HANNING_RESPONSE))
    assert np.array_equal(fitter.response, [[0.0, 0.25, 0.5, 0.25, 0.0]] * 2) and np.array_equal(fitter.correlation, [na.HANNING] * 2)
    for kw in ({'response': 0.5}, {'response': (0.5, 0.0, 0.5)}, {'response': na.HANNING_RESPONSE, 'baseline_order': 1},
               {'response': na.HANNING_RESPONSE, 'calibration': 0.1}):
        with pytest.raises(ValueError, match='response'):
            CubeFitter(stack, None, mix.Runner, runner_kwargs=kw)


# ---------------------------------------------------------------------------- the pair that a response gives white noise
def test_the_correlation_of_a_response():
    import nestfit_amd as na
    got = na.correlation_of_response(na.HANNING_RESPONSE)
    assert isinstance(got, tuple) and len(got) == 2
    for g, w in zip(got, na.HANNING):
        assert abs(g - w) <= np.spacing(w)                                                  # to 1 ulp
    assert na.correlation_of_response(BINOMIAL) == pytest.approx((0.8, 0.4), abs=1e-15)
    assert na.correlation_of_response((0, 1, 0)) == (0.0, 0.0)
    assert na.correlation_of_response((0, 0.25, 0.5, 0.25, 0)) == got
    both = na.smoothed(na.HANNING_RESPONSE)
    assert set(both) == {'response', 'correlation'} and both['response'] == na.HANNING_RESPONSE and both['correlation'] == got
    for bad in (0.5, (0.5, 0.5), [[0.25, 0.5, 0.25]]):
        with pytest.raises(ValueError, match='3 or 5 taps'):
            na.correlation_of_response(bad)
    # ... which is what smoothing white noise does: 400 000 samples, five standard errors of 1 / sqrt(n) times a few
    x = np.convolve(np.random.default_rng(3).normal(size=400000), SKEW, 'valid')
    want = na.correlation_of_response(SKEW)
    for k in (1, 2):
        assert float(np.mean(x[:-k] * x[k:]) / np.mean(x * x)) == pytest.approx(want[k - 1], abs=5 * 2.0 / np.sqrt(x.size))


# ---------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('n', [4, 5, 58, 59, 300])
def test_the_restatement_against_numpy_convolve(n):
    """p~_j = sum_k h_k p_{j+k} is numpy's convolution with the taps REVERSED, `same` keeping the zero-beyond-the-ends rule."""
    import nestfit_amd as na
    from nestfit_amd._model import check_response
    assert na.HANNING_RESPONSE == rr.HANNING_RESPONSE
    rng = np.random.default_rng(n)
    p = rng.normal(size=n)
    for taps in (rr.HANNING_RESPONSE, BINOMIAL, SKEW, rr.IDENTITY, (0.3, 0.6, 0.1)):
        got = rr.filtered(p, taps)
        # (the restatement pads three taps as the package stores them)
        assert taps == rr.IDENTITY or np.array_equal(check_response(taps)[0], np.asarray(rr.taps5(taps), dtype=np.float64))
        assert got.dtype == np.longdouble and got.shape == (n,)
        g = np.asarray(taps, dtype=np.float64)[::-1]
        # ('same' keeps the LONGER argument's length: for a spectrum shorter than the taps, the middle of 'full' by hand)
        want = np.convolve(p, g, 'same') if n >= g.size else np.convolve(p, g, 'full')[g.size // 2:g.size // 2 + n]
        scale = np.asarray(rr.filtered_scale(p, taps), dtype=np.float64)
        assert (np.abs(np.asarray(got, dtype=np.float64) - want) <= 8 * np.finfo(float).eps * scale).all(), taps
    assert np.array_equal(np.asarray(rr.filtered(p, rr.IDENTITY), dtype=np.float64), p)
    # the ends by hand: the skewed taps on a spectrum of ones
    ends = np.asarray(rr.filtered(np.ones(n), SKEW), dtype=np.float64)
    assert ends[0] == pytest.approx(0.4 + 0.25 + 0.05) and ends[1] == pytest.approx(0.2 + 0.4 + 0.25 + 0.05)
    assert ends[-1] == pytest.approx(0.1 + 0.2 + 0.4) and ends[-2] == pytest.approx(0.1 + 0.2 + 0.4 + 0.25)
    # rows at once, and the likelihood: white noise, chi^2 by hand
    rows = rng.normal(size=(3, n))
    assert np.array_equal(rr.filtered(rows, SKEW)[1], rr.filtered(rows[1], SKEW))
    d = rng.normal(size=n)
    lnl, M = rr.lnl(d, p, 0.5, SKEW)
    r = d - np.asarray(rr.filtered(p, SKEW), dtype=np.float64)
    assert float(lnl) == pytest.approx(-np.sum(r * r) / (2 * 0.25), rel=1e-13) and float(M) >= abs(float(lnl))
    many, Ms = rr.lnl_rows(d, np.stack([p, rows[0]]), 0.5, SKEW, (0.5, 0.25))
    one, M1 = rr.lnl(d, p, 0.5, SKEW, (0.5, 0.25))
    assert float(many[0]) == pytest.approx(float(one), rel=1e-13) and float(Ms[0]) == pytest.approx(float(M1), rel=1e-13)


# ---------------------------------------------------------------------------- the width bias
def test_the_response_removes_the_width_bias():
    """A Gaussian of sigma = 1 channel, Hanning-smoothed, no noise: chi^2 over a (peak, sigm) grid of step 0.02.  With the
    response the minimum is the truth; without it the best unsmoothed model is wider and lower -- numpy gives 1.24 and 0.81
    times the truth; asserted: sigm >= 1.15, peak <= 0.9."""
    assert rr.BIAS_STEP <= 0.02 and rr.BIAS_PEAKS[rr.BIAS_TRUE[0]] == rr.BIAS_PEAK and rr.BIAS_SIGMS[rr.BIAS_TRUE[1]] == rr.BIAS_SIGM
    assert np.diff(rr.BIAS_PEAKS).max() <= 0.02 * rr.BIAS_PEAK * (1 + 1e-12) and np.diff(rr.BIAS_SIGMS).max() <= 0.02 * rr.BIAS_SIGM * (1 + 1e-12)
    import nestfit_amd as na
    assert na.HANNING_RESPONSE == rr.HANNING_RESPONSE
    d = rr.bias_data()
    models = np.stack([[rr.gaussian(pk, sg) for sg in rr.BIAS_SIGMS] for pk in rr.BIAS_PEAKS]).reshape(-1, rr.BIAS_N)
    shape2 = (rr.BIAS_PEAKS.size, rr.BIAS_SIGMS.size)
    with_resp = -2.0 * np.asarray(rr.lnl_rows(d, models, 1.0, rr.HANNING_RESPONSE)[0], dtype=np.float64).reshape(shape2)
    without = -2.0 * np.asarray(rr.lnl_rows(d, models, 1.0, rr.IDENTITY)[0], dtype=np.float64).reshape(shape2)
    assert rr.bias_argmin(with_resp) == rr.BIAS_TRUE and with_resp[rr.BIAS_TRUE] <= 1e-28
    ip, isg = rr.bias_argmin(without)
    peak, sigm = rr.BIAS_PEAKS[ip] / rr.BIAS_PEAK, rr.BIAS_SIGMS[isg] / rr.BIAS_SIGM
    print(f'without the response the best model has {sigm:.2f} times the width and {peak:.2f} times the peak')
    assert sigm >= 1.15 and peak <= 0.9
    assert 0 < ip < shape2[0] - 1 and 0 < isg < shape2[1] - 1                               # a minimum inside the grid
    # with the correlation that goes with the smoothing it is no different: Q changes the metric, not the model
    corr = -2.0 * np.asarray(rr.lnl_rows(d, models, 1.0, na.HANNING_RESPONSE, na.correlation_of_response(na.HANNING_RESPONSE))[0],
                             dtype=np.float64).reshape(shape2)
    assert rr.bias_argmin(corr) == rr.BIAS_TRUE


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void fused10(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0);
}
void fused11(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0);
}
int size_of(int i) { const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan), (int)LNL_KINDS, (int)LNL_INSTANCES}; return s[i]; }
}
'''


def test_the_fused_kernels_refuse_a_response_with_a_reason_of_its_own(tmp_path):
    from test_launch_plan import LnlPlan, LpLaunch
    src, so = tmp_path / 'plan_resp.cpp', tmp_path / 'libplan_resp.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    # the structures and the table of kinds are what they were
    assert [lib.size_of(i) for i in range(5)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan), 32, 1024]
    s, k = shape(n_spec=2, size=300, ncomp=2), knobs()
    reason = b'the resident kernel has no form for a channel response: use nfa_ring_serve'
    for mode in (0, 2):
        for flags in ((0, 1, 0, 0, 0, 0), (0, 1, 0, 1, 1, 0), (0, 1, 1, 0, 0, 0)):
            for correlated in (0, 1):                       # a response-only set, and one with a correlation: the response comes first
                with_resp, without, ten = FusedPlan(), FusedPlan(), FusedPlan()
                lib.fused11(C.byref(s), C.byref(k), mode, *flags, correlated, 1, C.byref(with_resp))
                lib.fused11(C.byref(s), C.byref(k), mode, *flags, correlated, 0, C.byref(without))
                lib.fused10(C.byref(s), C.byref(k), mode, *flags, correlated, C.byref(ten))
                assert with_resp.refusal == reason and with_resp.ring_error == reason and b'correlated' not in with_resp.refusal
                assert ten.refusal == without.refusal and b'response' not in (without.refusal or b'')
                assert (b'correlated' in (without.refusal or b'')) == bool(correlated)


def test_the_new_entry_points_are_declared():
    text = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert 'int nfa_specset_set_response(nfa_specset *ss, const double *taps);' in text
    assert 'int nfa_specset_response(const nfa_specset *ss, double *out);' in text


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
def test_the_store_carries_the_response(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import store as st
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    h3, h5 = rr.HANNING_RESPONSE, [0.0, 0.25, 0.5, 0.25, 0.0]
    cases = {'one': (h3, [h5, h5, h5]), 'each': ([BINOMIAL, IDENTITY5, SKEW], [BINOMIAL, IDENTITY5, SKEW]), 'identity': ((0, 1, 0), None),
             'none': (None, None), 'absent': ('absent', None)}
    for name, (value, want) in cases.items():
        path = str(tmp_path / f'{name}_{form}')
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'layered': False} if value == 'absent' else {'response': value}))
        with st.HdfStore(path) as store:
            got = store.read_model_response()
            assert ('channel_response' in store.hdf.attrs) == (want is not None)
            if want is None:
                assert got is None
            else:
                assert got.dtype == np.float64 and got.shape == (3, 5) and np.array_equal(got, np.array(want))     # to the bit, in both forms
    with pytest.raises(ValueError, match='2 responses for 3 spectra'):
        with st.HdfStore(str(tmp_path / f'bad_{form}'), nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'response': [h3, h3]}))
