"""A continuum background behind the components, without a GPU: the restatement of tests/cont_restatement.py
against the sibling restatements (Tc = 0) and by an independent route (the background term shifted by Tc / T0), what the GPU
test's draws exercise, the argument checks, the signed peak, `DataCube` and `CubeStack` with continuum maps, the store's
dataset in both formats, the fitter's and the post-processing's checks, and the resident kernel's refusal through the
HIP-free launch-plan header compiled into a small program."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import cont_cases as cc
import cont_restatement as cr
import fill_restatement as fr
import hf_restatement as hfr
import layer_restatement as lay
from test_launch_plan import FusedPlan, ROOT, knobs, shape

N_CHECK = 24                      # rows of a case the restatement's own checks walk


def _vectors(name, ncomp):
    axes, thetas, _ = cc.reference(name, ncomp)
    return axes, thetas[:N_CHECK]


# ---------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('name,ncomp', [('ammonia', 3), ('n2hp', 2)])
def test_the_oracle_models_without_a_continuum_are_the_sibling_restatements(nfo, name, ncomp):
    """Tc = 0: layered, tests/layer_restatement.py to the bit; summed, the oracle's own prediction of all components."""
    axes, thetas = _vectors(name, ncomp)
    make = {'ammonia': (cr.amm_terms, lay.amm_layered, nfo.AmmoniaSpectrum, nfo.amm_predict),
            'n2hp': (cr.nnhp_terms, lay.nnhp_layered, nfo.DiazenyliumSpectrum, nfo.nnhp_predict)}[name]
    for x, trans in axes:
        for th in thetas:
            terms, _ = make[0](nfo, x, trans, th)
            got, S = cr.through_oracle(terms, 0.0, True)
            want, want_S = make[1](nfo, x, trans, th)
            assert np.array_equal(got, want) and np.array_equal(S, want_S)
            s = make[2](x, np.zeros(x.size), 1.0, trans)
            make[3](s, th)
            summed, S2 = cr.through_oracle(terms, 0.0, False)
            assert np.allclose(summed, s.get_spec(), rtol=0, atol=4 * 2.0 ** -53 * S2.max()) and np.array_equal(S2, S)
            assert np.array_equal(summed == 0, s.get_spec() == 0)


def test_the_table_models_without_a_continuum_are_the_sibling_restatements(nfo):
    """Tc = 0: the line table against hf_restatement.hf_predict and layer_restatement.hf_layered to the bit; the filled mix
    against layer_restatement.mix_layered to the bit and fill_restatement.fill_predict, whose product is associated
    f (g a) where the kernel's is (g f) a, within four roundings of S."""
    import test_layered as tl
    axes, thetas = _vectors('lines', 3)
    x, table = axes[0]
    tbg = hfr.tbg_of(nfo, x)
    for th in thetas:
        layers = cr.hf_layers(nfo, x, hfr.table_of(table), th)
        assert np.array_equal(cr.through(nfo, x, tbg, layers, 0.0, False)[0], hfr.hf_predict(nfo, x, tbg, hfr.table_of(table), th))
        got, S = cr.through(nfo, x, tbg, layers, 0.0, True)
        want, want_S = lay.hf_layered(nfo, x, tbg, hfr.table_of(table), th)
        assert np.array_equal(got, want) and np.array_equal(S, want_S)
    axes, thetas = _vectors('filled', 2)
    mol, ks, iso, isos = tl._species()
    for x, what in axes:
        tbg = hfr.tbg_of(nfo, x)
        for th in thetas:
            layers = cr.mix_layers(nfo, x, what, (mol, iso), th, fill=True)
            got, S = cr.through(nfo, x, tbg, layers, 0.0, True)
            want, want_S = lay.mix_layered(nfo, x, tbg, what, (mol, iso), th, fill=True)
            assert np.array_equal(got, want) and np.allclose(S, want_S, rtol=2.0 ** -50, atol=0)     # (S: |g| |f a| here, |(g f) a| there)
            summed = cr.through(nfo, x, tbg, layers, 0.0, False)[0]
            assert np.allclose(summed, fr.fill_predict(nfo, x, tbg, what, (mol, iso), th), rtol=0, atol=4 * 2.0 ** -53 * max(S.max(), 1e-300))


@pytest.mark.parametrize('name,ncomp', [('ammonia', 2), ('n2hp', 2), ('lines', 3), ('filled', 2)])
def test_a_continuum_is_a_shifted_background_term(nfo, name, ncomp):
    """The independent route: T0 (y - (tbg + Tc / T0)) = g - Tc, so the restatements WITHOUT a continuum -- layer_restatement's
    `through_the_layers` and, summed, the same components added -- given tbg + Tc / T0 give the model with one, within
    1e-12 S.  For ammonia and N2H+ the layers are the oracle's own optical depths (`tarr`) and tex."""
    import test_layered as tl
    axes, thetas = _vectors(name, ncomp)
    worst = 0.0
    for k, (x, what) in enumerate(axes):
        for which in ('high', 'low'):
            tc = cc.pairs(name)[which][k]
            for th in thetas:
                if name in ('ammonia', 'n2hp'):
                    terms, tbg = (cr.amm_terms if name == 'ammonia' else cr.nnhp_terms)(nfo, x, what, th)
                    layers = [(tau, tex, None) for _, _, tau, tex in terms]
                    ours = {lay_: cr.through_oracle(terms, tc, lay_) for lay_ in (False, True)}
                else:
                    tbg = hfr.tbg_of(nfo, x)
                    if name == 'lines':
                        layers = cr.hf_layers(nfo, x, hfr.table_of(what), th)
                    else:
                        mol, _, iso, _ = tl._species()
                        layers = cr.mix_layers(nfo, x, what, (mol, iso), th, fill=True)
                    ours = {lay_: cr.through(nfo, x, tbg, layers, tc, lay_) for lay_ in (False, True)}
                shifted = cr.shifted_background(x, tbg, tc)
                want_layered = lay.through_the_layers(nfo, x, shifted, layers)[0]
                want_summed = sum(lay.through_the_layers(nfo, x, shifted, [one])[0] for one in layers)
                for lay_, want in ((True, want_layered), (False, want_summed)):
                    got, S = ours[lay_]
                    assert np.array_equal(got == 0, S == 0)
                    assert (np.abs(got - want) <= 1e-12 * S).all(), (name, which, lay_, float(np.max(np.abs(got - want) / np.maximum(S, 1e-300))))
                    live = S > 0
                    worst = max(worst, float(np.max(np.abs(got - want)[live] / S[live])) if live.any() else 0.0)
    print(f'{name}: the two routes agree within {worst:.1e} S')


@pytest.mark.parametrize('name,ncomp', cc.CASES)
def test_the_draws_exercise_what_the_gpu_test_says(name, ncomp):
    """Of the restatement's own spectra: before 35 K every row with a non-zero channel is negative there, and the spectrum with
    Tc = 0 beside it emits; before the model's low Tc each sign occurs in at least a tenth of the rows."""
    for layered in (False, True):
        n_abs, _ = cc.check_draws(name, ncomp, 'high', layered)
        absorb, emit = cc.check_draws(name, ncomp, 'low', layered)
        print(f'{name} ncomp={ncomp} layered={layered}: {n_abs} rows absorb before 35 K; before {cc.TC_LOW[name]} K {absorb} absorb, {emit} emit')
    # what a continuum is for: the summed model can be far below zero
    assert cc.evaluate(name, ncomp, 'high', False)[0].min() < -5.0


# ---------------------------------------------------------------------------- the argument checks
def test_the_argument_checks():
    from nestfit_amd._model import check_continuum
    assert check_continuum(None) is None and check_continuum(0.0, 2) is None and check_continuum([0, 0], 2) is None
    assert np.array_equal(check_continuum(3, 2), [3.0, 3.0]) and check_continuum(3, 2).dtype == np.float64
    assert np.array_equal(check_continuum([30.0, 0.0], 2), [30.0, 0.0])
    assert np.array_equal(check_continuum(np.array([1.5, 2.5])), [1.5, 2.5])
    # a cube: a number, a row, or one row per pixel -- always [n_pix, n_spec]
    assert np.array_equal(check_continuum(2.0, 2, 3), np.full((3, 2), 2.0))
    assert np.array_equal(check_continuum([1.0, 0.0], 2, 3), np.tile([1.0, 0.0], (3, 1)))
    maps = np.arange(6.0).reshape(3, 2)
    got = check_continuum(maps, 2, 3)
    assert np.array_equal(got, maps) and got is not maps and got.flags.c_contiguous
    assert check_continuum(np.zeros((3, 2)), 2, 3) is None
    for bad, kw, why in ((-1.0, {}, 'finite and >= 0'), ([1.0, np.nan], {}, 'finite and >= 0'), ([1.0, np.inf], {}, 'finite and >= 0'),
                         ([1.0, 2.0, 3.0], {}, '3 values for 2 spectra'), ('warm', {}, 'continuum must be'), (True, {}, 'continuum must be'),
                         ([], {}, 'continuum must be'), (np.ones((3, 2)), {}, 'shape'), (np.ones((2, 2, 2)), {'n_pix': 2}, 'shape'),
                         (np.ones((4, 2)), {'n_pix': 3}, 'for 3 pixels'), (np.ones((3, 3)), {'n_pix': 3}, 'for 3 pixels')):
        with pytest.raises(ValueError, match=why):
            check_continuum(bad, 2, **kw)
    # not with the Gaussian model, a calibration, a correlation, a response or templates; their neutral values pass
    for kw in ({'model': 2}, {'calibration': 0.1}, {'correlation': (0.5, 0.25)}, {'response': (0.25, 0.5, 0.25)},
               {'templates': [np.ones((1, 8)), None]}):
        with pytest.raises(ValueError, match='continuum'):
            check_continuum([3.0, 0.0], 2, **kw)
        assert check_continuum([0.0, 0.0], 2, **kw) is None                      # no continuum: nothing to refuse
    assert check_continuum(3.0, 2, model=0, calibration=0.0, correlation=(0, 0), response=(0, 1, 0), templates=[None, None]) is not None


def test_the_runners_refuse_before_any_device_call():
    """`from_data` raises ValueError on the host -- this machine has no device to ask."""
    import nestfit_amd as na
    x = np.linspace(1.0e11, 1.0001e11, 32)
    with pytest.raises(ValueError, match='Gaussian model has no optical depth'):
        na.GaussianRunner.from_data([x, np.zeros(32), 0.1, 1.00005e11], None, continuum=3.0)
    rows = [[x, np.zeros(32), 0.1, 1], [x, np.zeros(32), 0.1, 2]]
    for kw, why in (({'continuum': -1.0}, 'finite and >= 0'), ({'continuum': [1.0]}, '1 values for 2 spectra'),
                    ({'continuum': np.ones((1, 2))}, 'shape'), ({'continuum': 3.0, 'calibration': 0.1}, 'calibration'),
                    ({'continuum': 3.0, 'correlation': na.HANNING}, 'correlation'), ({'continuum': 3.0, 'response': na.HANNING_RESPONSE}, 'response'),
                    ({'continuum': 3.0, 'templates': [na.ripple(32, 9.3), None]}, 'templates')):
        with pytest.raises(ValueError, match=why):
            na.AmmoniaRunner.from_data(rows, None, **kw)


def test_the_signed_peak():
    from nestfit_amd._model import signed_peak
    a = np.array([[0.0, -3.0, 2.0, np.nan], [1.0, -0.5, 0.0, 0.0], [np.nan] * 4, [0.0, 0.0, 0.0, 0.0], [2.0, -2.0, 1.0, 0.0]])
    got = signed_peak(a, axis=1)
    assert np.array_equal(got[[0, 1, 3, 4]], [-3.0, 1.0, 0.0, 2.0]) and np.isnan(got[2])
    emit = np.abs(np.random.default_rng(1).normal(size=(5, 9)))
    assert np.array_equal(signed_peak(emit, axis=1), np.nanmax(emit, axis=1))        # nothing changes where a line emits


def test_the_new_entry_points_are_declared():
    text = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert 'int nfa_specset_set_continuum(nfa_specset *ss, const double *tc);' in text
    assert 'int nfa_specset_continuum(const nfa_specset *ss, double *out);' in text
    from nestfit_amd import _ffi
    assert 'nfa_specset_set_continuum' in _ffi.SIGNATURES and 'nfa_specset_continuum' in _ffi.SIGNATURES


# ---------------------------------------------------------------------------- cubes
N_CHAN, NOISE = 48, 0.1


def _stack(tc_maps, absorb=True, seed=0):
    """A 3 x 3 stack of two NH3 cubes: a dip of 0.8 K (absorb) or a peak, noise; tc_maps: per cube None, a number or (lat, lon)."""
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    from nestfit_amd.synth import freq_axis
    rng = np.random.default_rng(seed)
    cubes = []
    for k, (trans, tc) in enumerate(zip((1, 2), tc_maps)):
        x = freq_axis(trans, N_CHAN, 10.0)
        line = 0.8 * np.exp(-0.5 * ((np.arange(N_CHAN) - N_CHAN // 2) / 2.0) ** 2)
        data = rng.normal(0, NOISE, (N_CHAN, 3, 3)) + (-line if absorb else line)[:, None, None]
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': 3, 'NAXIS2': 3, 'NAXIS3': N_CHAN, 'BUNIT': 'K',
               'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz', 'CRVAL3': float(x[0]),
               'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': float(x[N_CHAN // 2])}
        cubes.append(DataCube(SimpleCube(hdr, data), NOISE, trans_id=trans, continuum=tc))
    return CubeStack(cubes)


def _maps():
    """(lat, lon) maps: 30 K with a NaN pixel at (lat 1, lon 2) and Tc = 0 at (lat 0, lon 0); 28 K likewise without the NaN."""
    a, b = np.full((3, 3), 30.0), np.full((3, 3), 28.0)
    a[1, 2] = np.nan
    a[0, 0] = b[0, 0] = 0.0
    a[2, 1] = 12.5                                             # (lat 2, lon 1): the orientation shows
    return a, b


def test_a_data_cube_takes_its_continuum_map():
    from nestfit_amd.cubeio import DataCube
    a, b = _maps()
    stack = _stack((a, b))
    dc = stack.cubes[0]
    assert dc.continuum.shape == (3, 3) and dc.continuum[1, 2] == 12.5 and np.isnan(dc.continuum[2, 1])      # [lon, lat]
    maps = stack.continuum_maps()
    assert maps.shape == (2, 3, 3) and maps[1, 1, 2] == 28.0 and maps[0, 0, 0] == 0.0
    # a number is every pixel's; a stack without any has none; one cube without beside one with: zeros
    assert np.array_equal(_stack((3.0, None)).continuum_maps(), np.stack([np.full((3, 3), 3.0), np.zeros((3, 3))]))
    assert _stack((None, None)).continuum_maps() is None
    # a pixel whose continuum is NaN is no good pixel
    lon, lat = stack.good_pixels()
    assert lon.size == 8 and (2, 1) not in set(zip(lon.tolist(), lat.tolist()))
    assert _stack((None, None)).good_pixels()[0].size == 9
    # the same shape check as a noise map's, and the values a brightness temperature can have
    src = stack.cubes[0]
    from nestfit_amd.cubeio import SimpleCube
    cube = SimpleCube(src.full_header, np.zeros((N_CHAN, 3, 3)))
    with pytest.raises(AssertionError, match='continuum map'):
        DataCube(cube, NOISE, trans_id=1, continuum=np.ones((3, 4)))
    for bad in (-1.0, np.full((3, 3), np.inf)):
        with pytest.raises(ValueError, match='>= 0'):
            DataCube(cube, NOISE, trans_id=1, continuum=bad)


def test_absorption_pixels_get_their_live_points():
    """get_max_snr: max |spec| for a cube with a continuum -- the dip counts like a peak -- and what it was for every other."""
    a, b = _maps()
    plain_abs, plain_emit = _stack((None, None), absorb=True), _stack((None, None), absorb=False)
    cont_abs, cont_emit = _stack((a, b), absorb=True), _stack((a, b), absorb=False)
    for i, j in ((0, 0), (1, 1), (2, 0)):
        assert cont_abs.get_max_snr(i, j) > 6.0 > 4.5 > plain_abs.get_max_snr(i, j)       # 0.8 K deep at 0.1 K noise
        # an emission cube: never fewer than before, and the same wherever the peak is the largest magnitude
        assert cont_emit.get_max_snr(i, j) == plain_emit.get_max_snr(i, j) > 6.0
    # one cube with a continuum beside one without: each by its own rule
    mixed = _stack((a, None), absorb=True)
    want = np.max(np.abs(mixed.cubes[0].data[1, 1])) / NOISE
    assert mixed.get_max_snr(1, 1) == pytest.approx(max(want, np.max(mixed.cubes[1].data[1, 1]) / NOISE))


class _Fitter:
    """What insert_fitter_pars reads of a fitter."""
    lnZ_thresh, ncomp_max, nlive_snr_fact, nlive_quantum = 11, 2, 5, 1
    mn_kwargs = {'nlive': 100, 'tol': 1.0, 'seed': 5}
    runner_kwargs = {}

    def __init__(self, stack):
        self.stack = stack


@pytest.mark.parametrize('form', ['npz', 'hdf5'])
def test_the_store_carries_the_continuum_maps(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import postprocess as pp
    from nestfit_amd import store as st
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    a, b = _maps()
    for name, maps in (('some', (a, b)), ('one', (a, None)), ('none', (None, None))):
        path = str(tmp_path / f'{name}_{form}')
        stack = _stack(maps)
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter(stack))
        with st.HdfStore(path) as store:
            got = store.read_model_continuum()
            assert ('model_continuum' in store.hdf) == (name != 'none')
            if name == 'none':
                assert got is None
                assert pp.check_model_continuum(store, stack) is None
                continue
            want = np.stack([a, b if maps[1] is not None else np.zeros((3, 3))])        # (t, b, l): the maps as they were given
            assert got.dtype == np.float64 and got.shape == (2, 3, 3) and np.array_equal(got, want, equal_nan=True)
            # the post-processing's check: the stack of the fit passes, another one does not, nor does a runner that differs
            assert np.array_equal(pp.check_model_continuum(store, stack), want, equal_nan=True)
            with pytest.raises(ValueError, match="stack's continuum maps differ"):
                pp.check_model_continuum(store, _stack((a, 0.5 * a)))

            class runner:
                continuum = None
            with pytest.raises(ValueError, match='the runner has none'):
                pp.check_model_continuum(store, stack, runner)
            lon, lat = stack.good_pixels()
            runner.continuum = np.nan_to_num(want)[:, lat, lon].T
            pp.check_model_continuum(store, stack, runner)
            runner.continuum = runner.continuum + 1.0
            with pytest.raises(ValueError, match="runner's continuum differs"):
                pp.check_model_continuum(store, stack, runner)
    # a store without maps refuses a runner that has a continuum
    with st.HdfStore(str(tmp_path / f'none_{form}')) as store:
        class runner:
            continuum = np.array([3.0, 0.0])
        with pytest.raises(ValueError, match='fitted without a continuum'):
            pp.check_model_continuum(store, None, runner)


def test_the_fitter_checks_the_continuum_before_any_pixel():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    a, b = _maps()
    stack = _stack((a, b))
    fitter = CubeFitter(stack, None, na.AmmoniaRunner)
    assert fitter.continuum.shape == (2, 3, 3)
    assert CubeFitter(_stack((None, None)), None, na.AmmoniaRunner).continuum is None
    for kw, why in (({'calibration': 0.1}, 'calibration'), ({'correlation': na.HANNING}, 'correlation'),
                    ({'response': na.HANNING_RESPONSE}, 'response'), ({'templates': [na.ripple(N_CHAN, 9.3), None]}, 'templates'),
                    ({'continuum': 3.0}, 'comes from its cubes')):
        with pytest.raises(ValueError, match=why):
            CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs=kw)
    with pytest.raises(ValueError, match='Gaussian model'):
        CubeFitter(stack, None, na.GaussianRunner)
    CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'baseline_order': 0, 'layered': True, 'noise_uncertainty': 0.1})


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void fused12(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, int templates, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0,
                      templates != 0);
}
void fused13(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, int templates, int continuum, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0,
                      templates != 0, continuum != 0);
}
int size_of(int i) {
    const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan), (int)LNL_KINDS, (int)LNL_INSTANCES};
    return s[i];
}
}
'''


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('plan_cont')
    src, so = tmp / 'plan_cont.cpp', tmp / 'libplan_cont.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return C.CDLL(str(so))


def test_the_table_and_the_structures_are_what_they_were(plan):
    from test_launch_plan import LnlPlan, LpLaunch
    assert [plan.size_of(i) for i in range(5)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan), 32, 1024]


def test_the_fused_kernels_refuse_a_continuum_with_a_reason_of_their_own(plan):
    """A set with a continuum is weighted and has the baseline form's record: without a reason of its own the refusal would
    speak of a noise per channel or a baseline.  Without the argument, and with it false, the plan is what it was."""
    s, k = shape(n_spec=2, size=300, ncomp=2), knobs()
    reason = b'the resident kernel has no form for a continuum background: use nfa_ring_serve'
    for mode in (0, 2):
        #        bl wt banded filled layered calibrated correlated response templates
        for flags in ((0, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0, 0, 0, 0)):
            with_c, without, twelve = FusedPlan(), FusedPlan(), FusedPlan()
            plan.fused13(C.byref(s), C.byref(k), mode, *flags, 1, C.byref(with_c))
            plan.fused13(C.byref(s), C.byref(k), mode, *flags, 0, C.byref(without))
            plan.fused12(C.byref(s), C.byref(k), mode, *flags, C.byref(twelve))
            assert with_c.refusal == reason and with_c.ring_error == reason
            assert bytes(without) == bytes(twelve) and without.refusal != reason
        # a plain set is served as before
        plain = FusedPlan()
        plan.fused13(C.byref(s), C.byref(k), mode, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, C.byref(plain))
        assert plain.refusal is None
