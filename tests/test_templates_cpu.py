"""Nuisance templates without a GPU: the restatement of tests/tmpl_restatement.py against numpy's dense least
squares, the argument checks, `ripple`, the store, the launch plans of a templated launch (the HIP-free header compiled into a
small program, as tests/test_launch_plan.py does), and the condition of every template set the GPU tests use."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import tmpl_cases as tc
import tmpl_restatement as tr
from test_launch_plan import FusedPlan, LDS_PER_CU, LnlPlan, LpLaunch, ROOT, TABLES, TAIL, knobs, launch, shape, wave_doubles


# ---------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('n', [4, 5, 63, 130])
def test_the_restatement_against_dense_least_squares(n):
    """chi2_min by QR in longdouble against numpy.linalg.lstsq on the weighted design matrix [Legendre | templates]: scalar and
    per-channel noise with masked channels, every order, 1, 2 and 4 templates.  Where the span has more functions than the
    spectrum channels (n = 4, 5) both drop what is left over and chi2_min is 0 within rounding."""
    rng = np.random.default_rng(n)
    for chan in (False, True):
        noise = tc.channel_noise(n, 3 * n) if chan else 0.2
        w, ref = tr.weights(noise, n)
        w64 = np.asarray(w, dtype=np.float64)
        for order in tc.ORDERS:
            for count in tc.COUNTS:
                t = tc.templates(n, count)
                d = rng.normal(0, 1, n)
                preds = rng.normal(0, 1, (3, n))
                got, got_ref = tr.chi2_min(d, preds, noise, order, t)
                assert float(got_ref) == pytest.approx(float(ref))
                V = np.concatenate([np.polynomial.legendre.legvander((2.0 * np.arange(n) - (n - 1)) / (n - 1), order) if order >= 0
                                    else np.zeros((n, 0)), (t / np.abs(t).max(axis=1, keepdims=True)).T], axis=1)
                sw = np.sqrt(w64)
                for p, g in zip(preds, got):
                    r = sw * (np.where(w64 > 0, d, 0.0) - p)
                    coef = np.linalg.lstsq(V * sw[:, None], r, rcond=1e-9)[0]
                    want = float(np.sum((r - (V * sw[:, None]) @ coef) ** 2))
                    assert float(g) == pytest.approx(want, rel=1e-9, abs=1e-12 * float(r @ r)), (chan, order, count)
                    if V.shape[1] >= int((w64 > 0).sum()):
                        assert float(g) <= 1e-20 * float(r @ r)
    # the rank rule: a constant beside order 0, a template twice, P_1 beside order 1 are the smaller span
    d, p = rng.normal(0, 1, n), rng.normal(0, 1, n)
    one = tc.templates(n, 1)
    assert tr.orthonormal(n, np.ones(n), 0, np.ones((1, n))).shape[0] == 1
    assert tr.orthonormal(n, np.ones(n), -1, np.concatenate([one, 3.0 * one])).shape[0] == 1
    assert tr.orthonormal(n, np.ones(n), 1, np.linspace(-2.0, 2.0, n)[None, :]).shape[0] == 2
    assert float(tr.chi2_min(d, p, 0.2, 0, np.ones((1, n)))[0][0]) == pytest.approx(float(tr.chi2_min(d, p, 0.2, 0, None)[0][0]), rel=1e-15)
    # M bounds |lnL|, and lnL without nuisance terms is the plain sum
    rows = [[np.arange(n), d, 0.2]]
    lnl, M = tr.restate(rows, p[None, :], -1, None)
    assert lnl[0] == pytest.approx(-np.sum((d - p) ** 2) / (2 * 0.04), rel=1e-14) and M[0] >= abs(lnl[0])


def test_every_template_set_of_the_gpu_tests_is_well_conditioned():
    """A condition of the inputs: the moment form of the kernel loses about cond x 2e-16 of M against the restatement's QR; with
    cond <= 1e3 that is 2e-13, far inside the table mode's 1e-9."""
    worst = 0.0
    n_sets = 0
    for label, n, noise, order, t in tc.every_set():
        cond = tr.gram_condition(n, noise, order, t)
        assert cond <= tc.COND_MAX, (label, cond)
        worst = max(worst, cond)
        n_sets += 1
    print(f'{n_sets} template sets, worst condition number of the normalised Gram matrix {worst:.1f}')
    assert n_sets > 200
    # periods: 1.5 cycles and more across the spectrum
    assert tc.N_CHAN / 37.3 >= 1.5 and tc.SCI_N / tc.SCI_PERIOD >= 1.5


# ---------------------------------------------------------------------------- ripple and the argument checks
def test_ripple():
    import nestfit_amd as na
    for n, period in ((256, 37.3), (4, 1.74), (300, 300 / 2.3)):
        got = na.ripple(n, period)
        assert got.shape == (2, n) and got.dtype == np.float64 and np.array_equal(got, tc.ripple(n, period))
        j = np.arange(n)
        assert np.allclose(got[0], np.sin(2 * np.pi * j / period), atol=1e-15) and np.allclose(got[1], np.cos(2 * np.pi * j / period), atol=1e-15)
        one = na.ripple(n, period, phase=0.7)
        assert one.shape == (1, n) and np.array_equal(one, tc.ripple(n, period, 0.7))
        # a known phase lies in the span of the pair
        assert np.allclose(one[0], np.cos(0.7) * got[0] + np.sin(0.7) * got[1], atol=1e-14)
    assert np.vstack([na.ripple(64, 20.5), na.ripple(64, 9.1)]).shape == (4, 64)
    for bad in ((0, 10.0), (16, 0.0), (16, -3.0), (16, np.nan), (16, np.inf)):
        with pytest.raises(ValueError, match='ripple'):
            na.ripple(*bad)
    with pytest.raises(ValueError, match='phase'):
        na.ripple(16, 5.0, phase=np.nan)


def test_the_argument_checks():
    from nestfit_amd._model import check_templates
    n = 32
    t2 = tc.ripple(n, 9.3)
    assert check_templates(None) is None and check_templates([None, None], 2) is None and check_templates([np.zeros((0, n))], 1) is None
    out = check_templates([t2, None, t2[0]], 3, [n, 40, n])
    assert out[1] is None and out[0].shape == (2, n) and out[2].shape == (1, n) and out[0].dtype == np.float64
    assert np.array_equal(out[0], t2) and out[0] is not t2                   # the caller's values, a copy
    assert check_templates(t2, 1, [n])[0].shape == (2, n)                     # one spectrum: its array alone
    for bad, why in (([t2], 'entries for 2 spectra'), ([t2, np.ones((5, n))], 'at most 4'), ([t2, np.ones((1, n + 1))], 'channels'),
                     ([t2, np.full((1, n), np.nan)], 'finite'), ([t2, np.full((1, n), np.inf)], 'finite'),
                     ([t2, np.stack([t2[0], np.zeros(n)])], 'zero over its whole spectrum'), ([t2, 'ripple'], 'templates must be'),
                     ('ripple', 'templates must be'), ([], 'templates must be'), ([t2, np.ones((1, 2, n))], 'shape')):
        with pytest.raises(ValueError, match=why):
            check_templates(bad, 2, [n, n])
    # not with a calibration, a correlation or a response -- in words that name the templates; their neutral values pass
    for kw in ({'calibration': 0.1}, {'calibration': [0.0, 0.2]}, {'correlation': (0.5, 0.25)}, {'response': (0.25, 0.5, 0.25)}):
        with pytest.raises(ValueError, match='nuisance templates'):
            check_templates([t2, None], 2, [n, n], **kw)
    assert check_templates([t2, None], 2, [n, n], calibration=0.0, correlation=(0, 0), response=(0, 1, 0)) is not None
    assert check_templates([None, None], 2, [n, n], calibration=0.1) is None  # no template: nothing to refuse


def test_the_fitter_checks_the_templates_before_any_pixel():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter

    class stack:
        cubes = [None, None]
    t2 = tc.ripple(32, 9.3)
    assert CubeFitter(stack, None, na.AmmoniaRunner).templates is None
    fitter = CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs={'templates': [t2, None], 'baseline_order': 1})
    assert fitter.templates[1] is None and np.array_equal(fitter.templates[0], t2)
    for kw, why in (({'templates': [t2]}, 'entries for 2 spectra'), ({'templates': [t2, None], 'calibration': 0.1}, 'nuisance templates'),
                    ({'templates': [t2, None], 'correlation': na.HANNING}, 'nuisance templates'),
                    ({'templates': [t2, None], 'response': na.HANNING_RESPONSE}, 'nuisance templates')):
        with pytest.raises(ValueError, match=why):
            CubeFitter(stack, None, na.AmmoniaRunner, runner_kwargs=kw)


def test_the_new_entry_points_are_declared():
    text = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    assert '#define NFA_TMPL_MAX 4' in text
    assert 'int nfa_specset_set_templates(nfa_specset *ss, const double *t, const int *n_tmpl);' in text
    assert 'int nfa_specset_templates(const nfa_specset *ss, double *out_t, int *out_n);' in text
    from nestfit_amd import _ffi
    assert 'nfa_specset_set_templates' in _ffi.SIGNATURES and 'nfa_specset_templates' in _ffi.SIGNATURES


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
def test_the_store_carries_the_templates(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import store as st
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    a, b = 25.0 * tc.ripple(40, 11.7), 0.3 * tc.ripple(64, 20.1, 0.4)
    cases = {'some': ([a, None, b], [a, None, b]), 'none': (None, None), 'empty': ([None, None, None], None), 'absent': ('absent', None)}
    for name, (value, want) in cases.items():
        path = str(tmp_path / f'{name}_{form}')
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'baseline_order': 1} if value == 'absent' else {'templates': value}))
        with st.HdfStore(path) as store:
            got = store.read_model_templates()
            assert ('nuisance_templates' in store.hdf) == (want is not None)
            if want is None:
                assert got is None
                continue
            assert len(got) == 3 and got[1] is None
            for g, w in zip(got, want):
                assert (g is None) == (w is None)
                assert g is None or (g.dtype == np.float64 and np.array_equal(g, w))     # to the bit, the caller's scaling
    with pytest.raises(ValueError, match='2 entries for 3 spectra'):
        with st.HdfStore(str(tmp_path / f'bad_{form}'), nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'templates': [a, b]}))


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void lnl3(const LpShape *s, const LpKnobs *k, const LpLaunch *L, LnlPlan *out) { *out = plan_lnl(*s, *k, *L); }
void lnl4(const LpShape *s, const LpKnobs *k, const LpLaunch *L, int templates, LnlPlan *out) { *out = plan_lnl(*s, *k, *L, templates != 0); }
int slots2(int baseline, int calibrated) { return lnl_part_slots(baseline != 0, calibrated != 0); }
int slots3(int baseline, int calibrated, int templates) { return lnl_part_slots(baseline != 0, calibrated != 0, templates != 0); }
unsigned long long units_lds(const LpShape *s, int table, int split, int waves, int slots) { return lnl_units_lds(*s, table != 0, split, waves, slots); }
void fused11(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0);
}
void fused12(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, int correlated,
             int response, int templates, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0, correlated != 0, response != 0,
                      templates != 0);
}
int size_of(int i) {
    const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan), (int)LNL_KINDS, (int)LNL_INSTANCES, NFA_TMPL_MAX, NFA_TP_NB};
    return s[i];
}
}
'''
LNL_BASELINE = 4


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('plan_tmpl')
    src, so = tmp / 'plan_tmpl.cpp', tmp / 'libplan_tmpl.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    lib.units_lds.restype = C.c_ulonglong
    return lib


def test_the_table_and_the_structures_are_what_they_were(plan):
    assert [plan.size_of(i) for i in range(7)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan), 32, 1024, 4, 8]
    assert [plan.slots2(b, c) for b, c in ((0, 0), (1, 0), (1, 1))] == [1, 5, 6]
    assert [plan.slots3(b, c, 0) for b, c in ((0, 0), (1, 0), (1, 1))] == [1, 5, 6]
    assert plan.slots3(1, 0, 1) == 9 and plan.slots3(0, 0, 1) == 9


def _plans(plan, s, k, L):
    without, zero, with_t = LnlPlan(), LnlPlan(), LnlPlan()
    plan.lnl3(C.byref(s), C.byref(k), C.byref(L), C.byref(without))
    plan.lnl4(C.byref(s), C.byref(k), C.byref(L), 0, C.byref(zero))
    plan.lnl4(C.byref(s), C.byref(k), C.byref(L), 1, C.byref(with_t))
    return without, zero, with_t


def test_a_templated_launch_plans_the_baseline_form_with_nine_slots(plan):
    """Both modes, lnl_split 0, 1, 2 and 4, from one row to thousands, narrow and wide, few and many components: the form is the
    baseline's, the LDS is that of nine sums per part at the plan's own split and waves and fits a compute unit, the split is the
    asked one unless the nine slots do not fit (then the workgroup takes one unit, then the split halves), and wherever the set
    plans at all with a baseline it plans with templates.  Without the argument, and with it false, the plan is what it was."""
    lowered_waves = lowered_split = n_plans = 0
    for mode in (0, 2):
        table = mode == 0
        for ncomp, nhf_max in ((1, 21), (2, 21), (4, 21), (2, 40), (10, 40), (24, 50), (40, 50), (50, 50)):
            for wpb in (1, 4, 16):
                for split in (0, 1, 2, 4):
                    s = shape(n_spec=2, size=300, ncomp=ncomp, nhf_max=nhf_max, lnl_split=split, wpb=wpb)
                    for B in (1, 8, 200, 4096):
                        for baseline in (False, True):
                            L = launch(B, mode, baseline=baseline, weighted=True)
                            without, zero, with_t = _plans(plan, s, knobs(), L)
                            assert bytes(without) == bytes(zero)
                            base = LnlPlan()
                            plan.lnl3(C.byref(s), C.byref(knobs()), C.byref(launch(B, mode, baseline=True, weighted=True)), C.byref(base))
                            if with_t.error is not None:
                                # (only where the baseline form has no plan either: a line table too large for one unit per
                                # workgroup -- one wave per unit keeps no sums in LDS)
                                assert with_t.error == base.error and base.error is not None
                                continue
                            n_plans += 1
                            assert with_t.form == LNL_BASELINE and with_t.wide == base.wide
                            sp, waves = with_t.G.split, with_t.waves
                            assert sp in (1, 2, 4) and sp <= base.G.split and waves % sp == 0 and waves >= sp
                            lds = plan.units_lds(C.byref(s), int(table), sp, waves, 9)
                            want = 8 * ((TABLES if table else 0) + (wave_doubles(ncomp, nhf_max) + (4 * 64 * 9 if sp > 1 else 0)) * (waves // sp))
                            assert lds == want
                            if table:
                                lds = max(lds, 8 * (TABLES + TAIL))
                            assert with_t.lds >= lds and with_t.lds <= LDS_PER_CU and (table and with_t.lds == lds or not table)
                            assert with_t.blocks == -(-(B * 2) // (waves // sp))
                            # the asked split stays wherever its nine slots fit one unit per workgroup
                            one_unit = plan.units_lds(C.byref(s), int(table), base.G.split, base.G.split, 9)
                            if one_unit <= LDS_PER_CU:
                                assert sp == base.G.split
                            else:
                                lowered_split += 1
                            if sp == base.G.split and waves < base.waves:
                                lowered_waves += 1
    print(f'{n_plans} templated plans; {lowered_waves} took one unit per workgroup, {lowered_split} a smaller split')
    assert n_plans > 500 and lowered_waves > 0 and lowered_split > 0


def test_the_fused_kernels_refuse_templates_with_a_reason_of_their_own(plan):
    s, k = shape(n_spec=2, size=300, ncomp=2), knobs()
    reason = b'the resident kernel has no form for nuisance templates: use nfa_ring_serve'
    for mode in (0, 2):
        for flags in ((0, 1, 0, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0, 0)):
            with_t, without, eleven = FusedPlan(), FusedPlan(), FusedPlan()
            plan.fused12(C.byref(s), C.byref(k), mode, *flags, 1, C.byref(with_t))
            plan.fused12(C.byref(s), C.byref(k), mode, *flags, 0, C.byref(without))
            plan.fused11(C.byref(s), C.byref(k), mode, *flags, C.byref(eleven))
            assert with_t.refusal == reason and with_t.ring_error == reason
            assert eleven.refusal == without.refusal and b'templates' not in without.refusal
