"""Layered radiative transfer without a GPU (`layered=True`, nfa_specset_set_layered): the restatement the device
tests compare with (tests/layer_restatement.py) against the product form and in its limits, the host classes' keyword, the
store's attribute, the launch plan's rule for layered sets and the linkage of the two new entry points from C."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import band_restatement as br
import fill_restatement as fr
import hf_restatement as hfr
import layer_restatement as lay
import lte_restatement as lr
import mix_restatement as mr
from test_launch_plan import FusedPlan, LnlPlan, LpLaunch, ROOT, knobs, shape
from test_lte_bands_cpu import N_CHAN, band_axis
from test_lte_fill_cpu import RANGES6, _priors
from test_lte_mix_cpu import _stub_backend

TABLE = (1.0e11, np.array([-7.0, 0.0, 5.5]), np.array([0.25, 0.5, 0.25]))      # a made-up hyperfine pattern
HF_AXIS = lr.axis(TABLE[0], N_CHAN, 25.0)


def _hf_draw(rng, ncomp, ltau=(-1.0, 1.2), spread=1.0):
    """voff, tex, ltau, sigm: components within `spread` km/s of one another -- they overlap."""
    return np.concatenate([rng.uniform(-spread, spread, ncomp), rng.uniform(3.5, 30.0, ncomp), rng.uniform(*ltau, ncomp),
                           rng.uniform(0.3, 1.2, ncomp)])


def _mix_draw(rng, ncomp, fill):
    lncol = rng.uniform(14.0, 15.5, ncomp)
    theta = [rng.uniform(-1, 1, ncomp), rng.uniform(8.0, 50.0, ncomp), lncol, rng.uniform(0.3, 1.2, ncomp), lncol - rng.uniform(0.5, 2.0, ncomp)]
    return np.concatenate(theta + ([rng.uniform(-1.0, 0.0, ncomp)] if fill else []))


def _amm_draw(rng, ncomp):
    """voff, trot, tex, ntot, sigm, orth"""
    return np.concatenate([rng.uniform(-1, 1, ncomp), rng.uniform(10, 25, ncomp), rng.uniform(3.5, 9.0, ncomp), rng.uniform(14.0, 15.3, ncomp),
                           rng.uniform(0.3, 1.0, ncomp), rng.uniform(0.0, 0.5, ncomp)])


def _cases(nfo, na, rng, ncomp):
    """(name, layered function of (params, terms), summed function of params, params) for every model."""
    from nestfit_amd.synth import freq_axis
    mol, ks, iso, isos = mr.test_species(na)
    blend, band = na.LteBlend(ks + isos), mol.band(ks)
    x = band_axis(ks[0].nu)
    tbg, tbg_hf = hfr.tbg_of(nfo, x), hfr.tbg_of(nfo, HF_AXIS)
    xa, xn = freq_axis(1, N_CHAN), __import__('test_sibling_models').n2hp_axis(1, N_CHAN)
    sa, sn = nfo.AmmoniaSpectrum(xa, np.zeros(N_CHAN), 1.0, 1), nfo.DiazenyliumSpectrum(xn, np.zeros(N_CHAN), 1.0, 1)

    def oracle(s, predict):
        def summed(p):
            predict(s, p)
            return s.get_spec()
        return summed
    mixp = _mix_draw(rng, ncomp, False)
    return [
        ('lines', lambda p, t=None: lay.hf_layered(nfo, HF_AXIS, tbg_hf, TABLE, p, t), lambda p: hfr.hf_predict(nfo, HF_AXIS, tbg_hf, TABLE, p),
         _hf_draw(rng, ncomp)),
        ('lte', lambda p, t=None: lay.lte_layered(nfo, x, tbg, ks[1], p, t), lambda p: lr.lte_predict(nfo, x, tbg, ks[1], p), mixp[:4 * ncomp]),
        ('band', lambda p, t=None: lay.band_layered(nfo, x, tbg, band, p, t), lambda p: br.band_predict(nfo, x, tbg, band, p), mixp[:4 * ncomp]),
        ('mix', lambda p, t=None: lay.mix_layered(nfo, x, tbg, blend, (mol, iso), p, terms=t), lambda p: mr.mix_predict(nfo, x, tbg, blend, (mol, iso), p), mixp),
        ('filled', lambda p, t=None: lay.mix_layered(nfo, x, tbg, blend, (mol, iso), p, fill=True, terms=t),
         lambda p: fr.fill_predict(nfo, x, tbg, blend, (mol, iso), p), _mix_draw(rng, ncomp, True)),
        ('ammonia', lambda p, t=None: lay.amm_layered(nfo, xa, 1, p, t), oracle(sa, nfo.amm_predict), _amm_draw(rng, ncomp)),
        ('n2hp', lambda p, t=None: lay.nnhp_layered(nfo, xn, 1, p, t), oracle(sn, nfo.nnhp_predict), _hf_draw(rng, ncomp)),
    ]


def test_the_recurrence_is_the_product_form(nfo):
    """pred <- pred + (g - pred) a over the layers = sum_c g_c a_c prod_{c' > c} (1 - a_c'), to 1e-14 of S."""
    import nestfit_amd as na
    rng = np.random.default_rng(11)
    for ncomp in (1, 2, 3, 4):
        for _ in range(4):
            for name, layered, _, params in _cases(nfo, na, rng, ncomp):
                terms = []
                got, S = layered(params, terms)
                assert len(terms) == ncomp and S.max() > 0.05, name
                assert np.array_equal(got == 0, S == 0), name
                assert (np.abs(got - lay.product_form(terms)) <= 1e-14 * S).all(), (name, ncomp)
                assert (np.abs(got) <= S * (1 + 1e-14)).all(), name


def test_one_component_is_the_summed_model(nfo):
    """g - 0 = g: the summed restatement's bits (filled: the factor multiplies g here as on the device, the product of the
    summed restatement; the two associations differ by roundings, 4 ulp at the most)."""
    import nestfit_amd as na
    rng = np.random.default_rng(12)
    for _ in range(6):
        for name, layered, summed, params in _cases(nfo, na, rng, 1):
            got, S = layered(params)
            want = summed(params)
            assert np.abs(want).max() > 0.05, name
            if name == 'filled':
                assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all() and np.array_equal(got == 0, want == 0)
            else:
                assert np.array_equal(got, want), name
            assert np.array_equal(S, np.abs(got))


def test_components_that_do_not_overlap_are_summed(nfo):
    """Two components 16 km/s apart, windows disjoint: every channel has one layer at the most -- the summed bits."""
    import nestfit_amd as na
    rng = np.random.default_rng(13)
    for _ in range(6):
        for name, layered, summed, params in _cases(nfo, na, rng, 2):
            if name != 'lte':                                                   # (one single-line transition: the others' patterns are wider)
                continue
            params = params.copy()
            params[0:2] = (-12.0, 8.0)
            params[6:8] = np.minimum(params[6:8], 0.6)                          # sigm
            terms = []
            got, S = layered(params, terms)
            assert not ((terms[0][0] != 0) & (terms[1][0] != 0)).any() and all((t[0] != 0).any() for t in terms), name
            assert np.array_equal(got, summed(params)), name


def test_an_opaque_front_layer_hides_what_is_behind_it(nfo):
    """tau >= 32 in front: FastExp is 0, a = 1, and the channel reads the front layer alone (pred + (g - pred): two roundings)."""
    rng = np.random.default_rng(14)
    tbg = hfr.tbg_of(nfo, HF_AXIS)
    assert nfo.fast_expn(np.array([32.0]))[0] == 0.0
    for _ in range(10):
        params = _hf_draw(rng, 2)
        params[5] = 3.0                                                         # ltau of the front component: 250 in the main line
        terms = []
        got, _ = lay.hf_layered(nfo, HF_AXIS, tbg, TABLE, params, terms)
        front = hfr.hf_predict(nfo, HF_AXIS, tbg, TABLE, params[1::2])
        opaque = terms[1][0] >= 32.0
        assert opaque.sum() >= 3 and (terms[0][2][opaque] > 0.01).any()        # the back layer would show there
        assert (np.abs(got[opaque] - front[opaque]) <= 2 * np.spacing(np.abs(front[opaque]))).all()
        summed = hfr.hf_predict(nfo, HF_AXIS, tbg, TABLE, params)
        assert np.abs(summed[opaque] - front[opaque]).max() > 0.05


def test_the_thin_limit_is_the_summed_model_to_second_order(nfo):
    """layered - summed = -sum_{c < c'} g_c a_c a_c' + ...: a tenth of every optical depth, a hundredth of the difference."""
    rng = np.random.default_rng(15)
    tbg = hfr.tbg_of(nfo, HF_AXIS)
    for _ in range(10):
        params = _hf_draw(rng, 3, ltau=(-2.5, -2.0))
        diff = []
        for shift in (0.0, -1.0):
            p = params.copy()
            p[6:9] += shift
            diff.append(np.abs(lay.hf_layered(nfo, HF_AXIS, tbg, TABLE, p)[0] - hfr.hf_predict(nfo, HF_AXIS, tbg, TABLE, p)).max())
        peak = np.abs(hfr.hf_predict(nfo, HF_AXIS, tbg, TABLE, params)).max()
        assert 0 < diff[0] < 0.02 * peak and diff[1] == pytest.approx(0.01 * diff[0], rel=0.05)


def test_the_order_of_overlapping_thick_components_matters(nfo):
    rng = np.random.default_rng(16)
    tbg = hfr.tbg_of(nfo, HF_AXIS)
    for _ in range(10):
        params = _hf_draw(rng, 2, ltau=(0.5, 1.2), spread=0.3)
        params[2:4] = (4.0, 20.0) if rng.uniform() < 0.5 else (20.0, 4.0)
        swapped = params.reshape(4, 2)[:, ::-1].ravel()
        a, S = lay.hf_layered(nfo, HF_AXIS, tbg, TABLE, params)
        b, S2 = lay.hf_layered(nfo, HF_AXIS, tbg, TABLE, swapped)
        assert np.allclose(S, S2, rtol=1e-15, atol=0) and np.abs(a - b).max() > 0.1 * np.abs(a).max()
        # the cold layer in front: a dip the summed model cannot make
        cold_front = a if params[3] < params[2] else b
        assert cold_front.min() >= 0 and cold_front[np.argmax(S)] < 0.8 * cold_front.max()


# ---------------------------------------------------------------------------- the host classes
def test_every_value_error_comes_before_a_device_call():
    """(There is no device here: whatever reached one would fail with another error.)"""
    import nestfit_amd as na
    from nestfit_amd._model import check_layered
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import freq_axis
    mol, ks, iso, isos = mr.test_species(na)
    x = band_axis(ks[0].nu, 64)
    xa = freq_axis(1, 64)
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
        for bad in (1, 0, 'yes', None, 0.5):
            with pytest.raises(ValueError, match='`layered` is True or False'):
                cls.from_data(spec_data, None, layered=bad)
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match='`layered` is True or False'):
            CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, layered=bad)
        with pytest.raises(ValueError, match='`layered` is True or False'):
            na.GaussianRunner.from_data([xa, np.zeros(64), 0.1, 2.3e10], None, layered=bad)
    # the Gaussian model has no optical depth
    with pytest.raises(ValueError, match='Gaussian model has no optical depth'):
        na.GaussianRunner.from_data([xa, np.zeros(64), 0.1, 2.3e10], None, layered=True)
    with pytest.raises(ValueError, match='Gaussian model has no optical depth'):
        CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, model=2, rest_freqs=[2.3e10], layered=True)
    assert check_layered(False, 2) is False and check_layered(np.bool_(True), 0) is True
    from nestfit_amd import _ffi
    for name in ('nfa_specset_set_layered', 'nfa_specset_layered'):
        assert name in _ffi.SIGNATURES and hasattr(_ffi.load(), name)
    assert _ffi.SIGNATURES['nfa_specset_set_layered'] == _ffi.SIGNATURES['nfa_specset_set_baseline']


def test_the_cube_fitter_checks_the_keyword():
    import nestfit_amd as na
    from nestfit_amd import gaussian
    from nestfit_amd.fitter import CubeFitter
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = mr.test_species(na)
    stack = _stack(na, [na.LteBlend(ks + isos)])
    mix = na.LteMix([mol, iso])
    assert CubeFitter(stack, None, mix.Runner, runner_kwargs={'layered': True}).layered is True
    assert CubeFitter(stack, None, mix.Runner).layered is False
    with pytest.raises(ValueError, match='`layered` is True or False'):
        CubeFitter(stack, None, mix.Runner, runner_kwargs={'layered': 1})
    with pytest.raises(ValueError, match='Gaussian model has no optical depth'):
        CubeFitter(stack, None, gaussian.GaussianRunner, runner_kwargs={'layered': True})


# ---------------------------------------------------------------------------- the store and the map products
def _fit(na, tmp_path, name, mix, stack, layered, ncomp_max=2):
    from nestfit_amd.fitter import CubeFitter
    fitter = CubeFitter(stack, _priors(na, RANGES6[:5]), mix.Runner, runner_kwargs={'layered': True} if layered else None, lnZ_thresh=11,
                        ncomp_max=ncomp_max, mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0,
                        fit_backend=_stub_backend)
    path = str(tmp_path / name)
    fitter.fit_cube(path, nproc=1)
    return fitter, path


class _Summed:
    layered = False


class _Layered:
    layered = True


def test_store_round_trip_and_the_total_model_cube(tmp_path):
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.store import HdfStore
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = mr.test_species(na)
    mix = na.LteMix([mol, iso])
    blend = na.LteBlend(ks + isos, name='J=5-4')
    stack = _stack(na, [blend, isos[1]])
    n_chan = [dc.nchan for dc in stack.cubes]
    calls = []

    def backend(lon, lat, theta, want_spectra):
        """spectra: the row's first parameter (layer 0's voff) + 1000 x its number of columns, in every channel"""
        calls.append((theta.shape, want_spectra))
        if not want_spectra:
            return None, np.ones((theta.shape[0], 2)), np.ones((theta.shape[0], 2))
        return np.repeat((theta[:, 0] + 1000.0 * theta.shape[1])[:, None], sum(n_chan), axis=1), None, None
    fitter, path = _fit(na, tmp_path, 'layered', mix, stack, True)
    assert fitter.layered is True and fitter.runner_kwargs == {'layered': True}
    with HdfStore(path) as store:
        assert bool(store.hdf.attrs['layered']) is True and store.read_model_layered() is True
        assert pp.check_model_layered(store) is True and pp.check_model_layered(store, _Layered()) is True
        assert pp.check_model_layered(store, mix.Runner) is True             # a runner class does not say: nothing to compare
        with pytest.raises(ValueError, match='fitted with layered components, the runner is summed'):
            pp.check_model_layered(store, _Summed())
        with pytest.raises(ValueError, match='fitted with layered components'):      # before any product is written
            pp.postprocess_run(store, stack, runner=_Summed(), predict_backend=backend)
        assert not calls
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6), predict_backend=backend)
        pmap = np.asarray(store.hdf[f'{store.dpath}/nbest_MAP'])              # (m, p, b, l)
        n_layers = np.all(np.isfinite(pmap), axis=1).sum(axis=0)
        assert pmap.shape[:2] == (2, 5) and n_layers.max() >= 1
        for k, name in enumerate(('spec0', 'spec1')):
            per_layer = np.asarray(store.hdf[f'{store.dpath}/model_spec/{name}'])
            total = np.asarray(store.hdf[f'{store.dpath}/model_spec_total/{name}'])
            assert per_layer.shape == (2, n_chan[k], 3, 3) and total.shape == (n_chan[k], 3, 3) and total.dtype == np.float32
            for b in range(3):
                for l in range(3):
                    n = n_layers[b, l]
                    if n == 0:
                        assert np.isnan(total[:, b, l]).all()
                    else:       # one call of n layers, parameter-major: 5 n columns, the first of them layer 0's voff
                        assert (total[:, b, l] == np.float32(pmap[0, 0, b, l] + 1000.0 * 5 * n)).all()
                        assert (per_layer[0, :, b, l] == np.float32(pmap[0, 0, b, l] + 5000.0)).all()
        assert {shape[1] for shape, ws in calls if ws} == {5} | {5 * int(n) for n in np.unique(n_layers[n_layers > 0])}
    # an old store -- one without the attribute -- reads as summed, and gets no total cube
    fitter, old = _fit(na, tmp_path, 'summed', mix, stack, False)
    assert fitter.layered is False
    with HdfStore(old) as store:
        assert 'layered' not in store.hdf.attrs and store.read_model_layered() is False
        assert pp.check_model_layered(store) is False and pp.check_model_layered(store, _Summed()) is False
        with pytest.raises(ValueError, match='fitted with summed components, the runner is layered'):
            pp.postprocess_run(store, stack, runner=_Layered(), predict_backend=backend)
        pp.postprocess_run(store, stack, evid_kernel=0.6, post_kernel=pp.gaussian_kernel(0.6), predict_backend=backend)
        assert 'model_spec' in store.hdf[store.dpath] and 'model_spec_total' not in store.hdf[store.dpath]


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void lnl(const LpShape *s, const LpKnobs *k, const LpLaunch *L, int filled, int layered, LnlPlan *out) {
    LpLaunch l = *L;
    l.filled = filled != 0;
    l.layered = layered != 0;
    *out = plan_lnl(*s, *k, l);
}
int plan_filled(const LnlPlan *p) { return p->filled ? 1 : 0; }
int plan_layered(const LnlPlan *p) { return p->layered ? 1 : 0; }
int launch_layered(const LpLaunch *L) { return L->layered ? 1 : 0; }
void fused5(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, FusedPlan *out) { *out = plan_fused(*s, *k, mode, bl != 0, wt != 0); }
void fused6(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0);
}
void fused7(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0);
}
void fused8(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0);
}
int size_of(int i) { const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan)}; return s[i]; }
}
'''
PLAIN, W8, QUEUE, WEIGHTED, BASELINE = range(5)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('layer_plan')
    src, so = tmp / 'plan.cpp', tmp / 'libplan.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    # the mirrors of tests/test_launch_plan.py still have the structures' sizes: the flags sit in padding
    assert [lib.size_of(i) for i in range(3)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan)]
    return lib


def test_a_layered_set_takes_baseline_weighted_or_plain_and_says_so(plan):
    fields = ('form', 'wide', 'waves', 'lds', 'blocks')
    seen = set()
    for mode in (0, 2):
        for B in (1, 11, 64, 4096, 32768):
            for nhf_max, size, model in ((9, 300, 4), (21, 1024, 0), (33, 1024, 1)):
                for ncomp in (1, 2, 3, 4, 8):
                    for write_spec in (False, True):
                        for baseline, weighted in ((False, False), (False, True), (True, True)):
                            s = shape(n_spec=2, size=size, nhf_max=nhf_max, ncomp=ncomp, model=model)
                            L = LpLaunch(B=B, mode=mode, group_n=1, group_each=B, write_spec=write_spec, has_prior=True,
                                         baseline=baseline, weighted=weighted, has_queue=True)
                            assert plan.launch_layered(C.byref(L)) == 0               # the mirror's zero padding: summed
                            k = knobs()
                            p0 = LnlPlan()
                            plan.lnl(C.byref(s), C.byref(k), C.byref(L), 0, 0, C.byref(p0))
                            if p0.error:
                                continue
                            seen.add(p0.form)
                            assert plan.plan_layered(C.byref(p0)) == 0
                            for filled in (0, 1):
                                p1 = LnlPlan()
                                plan.lnl(C.byref(s), C.byref(k), C.byref(L), filled, 1, C.byref(p1))
                                assert not p1.error and plan.plan_layered(C.byref(p1)) == 1 and plan.plan_filled(C.byref(p1)) == filled
                                want = BASELINE if baseline else WEIGHTED if weighted else PLAIN
                                assert p1.form == want and p1.form not in (QUEUE, W8)
                                assert p1.wide == p0.wide == (nhf_max > 26) and p1.G.split == p0.G.split and p1.waves == p0.waves
                                if p0.form == p1.form:
                                    assert all(getattr(p0, f) == getattr(p1, f) for f in fields)
    assert seen == {PLAIN, W8, QUEUE, WEIGHTED, BASELINE}                   # (the summed plans did take the queue and w8)


def test_the_fused_kernels_refuse_a_layered_set_first_of_all(plan):
    why = b'the resident kernel has no form for layered transfer: use nfa_ring_serve'
    same = ('refusal', 'ring_error', 'n_blocks', 'ctl_double', 'staged', 'lds_point', 'lds_ring')
    for ncomp, npar, nhf_max in ((1, 6, 21), (2, 6, 21), (3, 4, 15), (4, 6, 21), (4, 7, 9), (5, 5, 9), (2, 4, 33)):
        for mode in (0, 2):
            for bl, wt in ((0, 0), (0, 1), (1, 1)):
                s, k = shape(n_spec=2, ncomp=ncomp, nhf_max=nhf_max, ndim=npar * ncomp, n_stage=npar, stage_doubles=200 * npar), knobs()
                for banded, filled in ((0, 0), (1, 0), (1, 1)):
                    p = FusedPlan()
                    plan.fused8(C.byref(s), C.byref(k), mode, bl, wt, banded, filled, 1, C.byref(p))
                    assert p.refusal == why and p.ring_error == why, (ncomp, npar, p.refusal)     # ahead of every other refusal
                    # the five-, six- and seven-argument calls: the eight-argument call at false
                    p8, p7 = FusedPlan(), FusedPlan()
                    plan.fused8(C.byref(s), C.byref(k), mode, bl, wt, banded, filled, 0, C.byref(p8))
                    plan.fused7(C.byref(s), C.byref(k), mode, bl, wt, banded, filled, C.byref(p7))
                    assert all(getattr(p8, f) == getattr(p7, f) for f in same) and p8.refusal != why
                    if not filled:
                        p6 = FusedPlan()
                        plan.fused6(C.byref(s), C.byref(k), mode, bl, wt, banded, C.byref(p6))
                        assert all(getattr(p8, f) == getattr(p6, f) for f in same)
                    if not filled and not banded:
                        p5 = FusedPlan()
                        plan.fused5(C.byref(s), C.byref(k), mode, bl, wt, C.byref(p5))
                        assert all(getattr(p8, f) == getattr(p5, f) for f in same)


def test_the_new_entry_points_link_from_c(tmp_path):
    """include/nestfit_amd.h compiles as C99 and a C program that names the two new symbols links against the library."""
    from nestfit_amd.build import OUT, build
    build()
    src = tmp_path / 'use_layered.c'
    src.write_text('#include "nestfit_amd.h"\n'
                   'typedef int (*set_t)(nfa_specset *, int);\n'
                   'typedef int (*get_t)(const nfa_specset *);\n'
                   'int main(void) { set_t f = nfa_specset_set_layered, b = nfa_specset_set_baseline; get_t g = nfa_specset_layered;\n'
                   '                 return f == 0 || b == 0 || g == 0; }\n')
    exe = tmp_path / 'use_layered'
    res = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', f'-I{ROOT / "include"}', str(src), '-o', str(exe),
                          f'-L{OUT.parent}', '-lnestfit_amd', f'-Wl,-rpath,{OUT.parent}', '-Wl,--allow-shlib-undefined'],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
