"""A calibration uncertainty per spectrum, integrated out of the likelihood: what can be checked without a GPU.

The restatement (tests/calib_restatement.py) against a numerical integral over the gain and at its limits; `check_calibration`;
the store's attribute; and the launch plans of a calibrated set through a compiled shim of csrc/nfa_launch_plan.h.
"""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import calib_restatement as cr
from test_launch_plan import IN, LDS_PER_CU, TABLES, FusedPlan, LnlPlan, LpLaunch, ROOT, knobs, shape, table_workgroup, wave_doubles

LD = np.longdouble
N_CHAN = 96


# ---------------------------------------------------------------------------- the restatement
def _case(rng, channel_noise, order, bright=1.0):
    """(data, pred, noise): a line of two Gaussians times a gain of 1.12, what the baseline of `order` can take away (nothing, an
    offset, a ramp too), noise; a channel noise masks a stretch."""
    j = np.arange(N_CHAN)
    pred = bright * (3.0 * np.exp(-0.5 * ((j - 40) / 4.0) ** 2) + 1.2 * np.exp(-0.5 * ((j - 61) / 7.0) ** 2))
    sigma = 0.3
    if channel_noise:
        noise = rng.uniform(0.2, 0.5, N_CHAN)
        noise[35:43] = np.inf                                    # a stretch of the brighter line
        noise[[3, 77]] = np.inf
        scatter = np.where(np.isfinite(noise), noise, 0.0)
    else:
        noise, scatter = sigma, sigma
    data = 1.12 * pred + (0.0 if order is None else 0.4) + (0.01 * (j - 50) if order else 0.0) + rng.normal(0, 1, N_CHAN) * scatter
    if channel_noise:
        data[~np.isfinite(noise)] = 1e6                          # what a masked channel holds does not matter
    return data, pred, noise


def _integral(data, pred, noise, cal, order, n=60001):
    """ln of the integral over g in 1 +- 12 s of exp(lnL(g)) N(g; 1, s^2) by the trapezoid rule, in log space.  lnL(g) is the
    plain likelihood of the residual d - g p with the baseline profiled out -- by a weighted fit of a power-basis polynomial
    (numpy.polynomial.polynomial), another route than the restatement's Legendre fit -- evaluated at every g."""
    from numpy.polynomial import polynomial
    w, sigma = cr.weights_of(noise, N_CHAN)
    live = w > 0
    t = np.linspace(-1.0, 1.0, N_CHAN)

    def perp(x):
        x = np.where(live, np.asarray(x, dtype=LD), LD(0))
        if order is None:
            return x
        out = x.copy()
        for _ in range(2):
            coef = polynomial.polyfit(t[live], out[live].astype(np.float64), order, w=np.sqrt(w[live]).astype(np.float64))
            out[live] = out[live] - polynomial.polyvander(t[live], order).astype(LD) @ coef.astype(LD)
        return out
    d, p = perp(data), perp(pred)
    s = LD(cal)
    g = LD(1) + s * np.linspace(LD(-12), LD(12), n, dtype=LD)
    lnf = np.empty(n, dtype=LD)
    for lo in range(0, n, 4096):
        r = d[None, :] - g[lo:lo + 4096, None] * p[None, :]
        lnf[lo:lo + 4096] = -np.sum(w[None, :] * r * r, axis=1) / (2 * sigma * sigma)
    lnf += -((g - 1) / s) ** 2 / 2 - np.log(s * np.sqrt(2 * LD(np.pi)))
    top = lnf.max()
    f = np.exp(lnf - top)
    return top + np.log((np.sum(f) - (f[0] + f[-1]) / 2) * (g[1] - g[0]))


@pytest.mark.parametrize('channel_noise', [False, True])
@pytest.mark.parametrize('order', [None, 0, 3])
def test_the_restatement_against_an_integral_over_the_gain(channel_noise, order):
    rng = np.random.default_rng(11 + 2 * int(channel_noise) + (0 if order is None else order + 1))
    data, pred, noise = _case(rng, channel_noise, order)
    for cal in (0.02, 0.1, 0.5):
        got = cr.marginal_lnl(data, pred, noise, cal, order)
        want = _integral(data, pred, noise, cal, order)
        print(f'channel noise {channel_noise}, baseline {order}, s = {cal}: lnL {float(got):.6f}, integral - closed form {float(want - got):.2e}')
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want))
        plain = cr.marginal_lnl(data, pred, noise, 0, order)
        assert got != plain


def test_the_limits_of_the_restatement():
    rng = np.random.default_rng(5)
    for channel_noise, order in itertools.product((False, True), (None, 0, 3)):
        data, pred, noise = _case(rng, channel_noise, order)
        a, b, c = cr.products(data, pred, noise, order)
        # s = 0: the plain likelihood, exactly -- sum w (d - p)^2 of the projected residual
        w, sigma = cr.weights_of(noise, N_CHAN)
        r = cr.project_out(np.asarray(data, dtype=LD) - np.asarray(pred, dtype=LD), w, order)
        assert cr.marginal_lnl(data, pred, noise, 0, order) == -(c - 2 * b + a) / 2
        assert float(cr.marginal_lnl(data, pred, noise, 0, order)) == pytest.approx(float(-np.sum(w * r * r) / (2 * sigma * sigma)), rel=1e-13)
        # ... and small s goes there: the difference is s^2 (b - a)^2 / 2 to first order (not smaller s: the unsimplified form
        # subtracts terms of size 1 / s^2)
        near = cr.marginal_lnl(data, pred, noise, 1e-4, order)
        assert float(near + (c - 2 * b + a) / 2) == pytest.approx(float(1e-8 * ((b - a) ** 2 - a) / 2), rel=1e-3)
        # p = 0: the null value, whatever s
        for cal in (0, 0.1, 1.0):
            assert cr.marginal_lnl(data, np.zeros(N_CHAN), noise, cal, order) == -c / 2
        assert cr.gain_posterior(data, pred, noise, 0, order) == (1, 0)
        # s = 1 with a bright model (a >> 1): the gain profiled out, c - b^2 / a, and the log term
        data, pred, noise = _case(rng, channel_noise, order, bright=20.0)
        a, b, c = cr.products(data, pred, noise, order)
        assert a > 1e4
        profiled = -(c - b * b / a) / 2 - np.log1p(a) / 2
        assert float(cr.marginal_lnl(data, pred, noise, 1.0, order)) == pytest.approx(float(profiled), rel=0.01)
        # the posterior of the gain: the injected 1.12 within 4 of its standard deviations, far narrower than the prior
        mean, std = cr.gain_posterior(data, pred, noise, 0.3, order)
        assert abs(mean - 1.12) < 4 * std and std < 0.01


# ---------------------------------------------------------------------------- the argument
def test_check_calibration_refuses_before_any_device_call(monkeypatch):
    """(No library is loaded here: `_ffi.load` and `_ffi.engine` fail if anything reaches them.)"""
    import nestfit_amd as na
    from nestfit_amd import _ffi
    from nestfit_amd._model import check_calibration
    from nestfit_amd.cube import CubeRunner
    from nestfit_amd.synth import freq_axis

    def no_library(*a, **k):
        raise AssertionError('a device call')
    monkeypatch.setattr(_ffi, 'load', no_library)
    monkeypatch.setattr(_ffi, 'engine', no_library)
    assert check_calibration(None) is None and check_calibration(None, 3) is None
    assert check_calibration(0) is None and check_calibration(0.0, 2) is None and check_calibration((0, 0.0), 2) is None
    out = check_calibration(0.1, 3)
    assert out.dtype == np.float64 and np.array_equal(out, [0.1, 0.1, 0.1])
    assert np.array_equal(check_calibration([0, 0.2], 2), [0.0, 0.2]) and np.array_equal(check_calibration(np.array([1.0, 0.05])), [1.0, 0.05])
    assert np.array_equal(check_calibration(np.float32(0.5), 1), [0.5]) and np.array_equal(check_calibration(1, 2), [1.0, 1.0])
    bad = ['0.1', b'x', True, [0.1, None], [0.1, '0.2'], {'a': 1}, [[0.1, 0.2]], np.array([[0.1, 0.2]]), [], 1j,
           np.nan, np.inf, [0.1, np.nan], [0.1, -np.inf], -0.01, 1.0001, [0.1, 1.5], [-1e-300, 0.1], np.array([True, False])]
    for value in bad:
        with pytest.raises(ValueError, match='calibration must be'):
            check_calibration(value, 2)
    for value in ([0.1], [0.1, 0.2, 0.3], np.array([0.1])):                  # the wrong number of spectra
        with pytest.raises(ValueError, match='for 2 spectra'):
            check_calibration(value, 2)
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
        for value in ('a', np.nan, 1.5, -0.1, [0.1, 0.2], True):
            with pytest.raises(ValueError, match='calibration must be'):
                cls.from_data(spec_data, None, calibration=value)
    for value in ('a', np.nan, 1.5, [0.1, 0.2]):
        with pytest.raises(ValueError, match='calibration must be'):
            na.GaussianRunner.from_data([xa, np.zeros(64), 0.1, 2.3e10], None, calibration=value)
        with pytest.raises(ValueError, match='calibration must be'):
            CubeRunner([xa], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, calibration=value)
    for name in ('nfa_specset_set_calibration', 'nfa_specset_calibration'):
        assert name in _ffi.SIGNATURES


def test_the_cube_fitter_checks_the_keyword():
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    from mix_restatement import test_species as species
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = species(na)
    stack = _stack(na, [na.LteBlend(ks + isos), isos[1]])
    mix = na.LteMix([mol, iso])
    assert CubeFitter(stack, None, mix.Runner).calibration is None
    assert CubeFitter(stack, None, mix.Runner, runner_kwargs={'calibration': 0}).calibration is None
    assert np.array_equal(CubeFitter(stack, None, mix.Runner, runner_kwargs={'calibration': 0.1}).calibration, [0.1, 0.1])
    for value in ('a', 2, [0.1], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError, match='calibration must be'):
            CubeFitter(stack, None, mix.Runner, runner_kwargs={'calibration': value})


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
def test_the_store_carries_the_calibration(tmp_path, form):
    from nestfit_amd import hdf5
    from nestfit_amd import store as st
    if form == 'hdf5' and not hdf5.available():
        pytest.skip('no HDF5 library on this machine')
    cases = {'number': (0.1, [0.1, 0.1, 0.1]), 'each': ((0.05, 0.0, 0.3), [0.05, 0.0, 0.3]), 'zeros': ((0, 0, 0), None), 'none': (None, None),
             'absent': ('absent', None)}
    for name, (value, want) in cases.items():
        path = str(tmp_path / f'{name}_{form}')
        with st.HdfStore(path, nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'baseline_order': 1} if value == 'absent' else {'calibration': value}))
        with st.HdfStore(path) as store:
            got = store.read_model_calibration()
            assert ('calibration' in store.hdf.attrs) == (want is not None)
            if want is None:
                assert got is None
            else:
                assert got.dtype == np.float64 and np.array_equal(got, np.array(want))     # to the bit, in both forms
    with pytest.raises(ValueError, match='calibration must be'):
        with st.HdfStore(str(tmp_path / f'bad_{form}'), nchunks=1, file_format=form) as store:
            store.insert_fitter_pars(_Fitter({'calibration': (0.1, 0.2)}))                  # two values, three cubes


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void lnl(const LpShape *s, const LpKnobs *k, const LpLaunch *L, int filled, int layered, int calibrated, LnlPlan *out) {
    LpLaunch l = *L;
    l.filled = filled != 0; l.layered = layered != 0; l.calibrated = calibrated != 0;
    *out = plan_lnl(*s, *k, l);
}
int plan_calibrated(const LnlPlan *p) { return p->calibrated ? 1 : 0; }
int launch_calibrated(const LpLaunch *L) { return L->calibrated ? 1 : 0; }
void fused8(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0);
}
void fused9(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, int layered, int calibrated, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0, layered != 0, calibrated != 0);
}
int size_of(int i) { const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan)}; return s[i]; }
int part_slots(int baseline, int calibrated) { return lnl_part_slots(baseline != 0, calibrated != 0); }
// rows of test_launch_plan.IN, each planned with a baseline and then calibrated as well: {error, split, waves, lds, form} twice
void both(long long n, const long long *in, long long *out) {
    for (long long i = 0; i < n; ++i, in += 16, out += 10) {
        LpShape s = {};
        s.nhf_max = (int)in[1]; s.n_spec = (int)in[4]; s.ncomp = (int)in[5]; s.ndim = 6 * s.ncomp; s.model = NFA_MODEL_AMMONIA;
        for (int q = 0; q < s.n_spec; ++q) s.size[q] = (int)(q ? in[3] : in[2]);
        s.lnl_split = (int)in[12]; s.wpb = (int)in[13]; s.lnl_cap = (int)in[14]; s.prog_bytes = 3624; s.line_rec_bytes = 32;
        LpKnobs k = {};
        k.lnl_queue = (int)in[10]; k.n_cu = (int)in[15]; k.coalesce = NFA_GROUP_MAX;
        LpLaunch L = {};
        L.B = in[6]; L.mode = (int)in[0]; L.group_n = 1; L.group_each = in[6];
        L.write_spec = in[7]; L.baseline = in[8]; L.weighted = in[9]; L.has_queue = in[11];
        for (int c = 0; c < 2; ++c) {
            L.calibrated = c != 0;
            const LnlPlan P = plan_lnl(s, k, L);
            long long *o = out + 5 * c;
            o[0] = P.error != nullptr; o[1] = P.G.split; o[2] = P.waves; o[3] = (long long)P.lds; o[4] = P.form;
        }
    }
}
}
'''
PLAIN, W8, QUEUE, WEIGHTED, BASELINE = range(5)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('calib_plan')
    src, so = tmp / 'plan.cpp', tmp / 'libplan.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    # the mirrors of tests/test_launch_plan.py still have the structures' sizes: the flags sit in padding
    assert [lib.size_of(i) for i in range(3)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan)]
    lib.both.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p]
    return lib


def test_a_calibrated_set_takes_the_baseline_form_whatever_else_it_is(plan):
    assert [plan.part_slots(b, c) for b, c in ((0, 0), (1, 0), (1, 1))] == [1, 5, 6]
    seen = set()
    for mode in (0, 2):
        for B in (1, 11, 64, 4096, 32768):
            for nhf_max, size, model in ((9, 300, 4), (21, 1024, 0), (33, 1024, 1)):
                for ncomp, write_spec in itertools.product((1, 2, 3, 4, 8), (False, True)):
                    for baseline, weighted, has_queue in itertools.product((False, True), (False, True), (False, True)):
                        s, k = shape(n_spec=2, size=size, nhf_max=nhf_max, ncomp=ncomp, model=model), knobs()
                        L = LpLaunch(B=B, mode=mode, group_n=1, group_each=B, write_spec=write_spec, has_prior=True,
                                     baseline=baseline, weighted=weighted, has_queue=has_queue)
                        assert plan.launch_calibrated(C.byref(L)) == 0                # the mirror's zero padding: none
                        p0 = LnlPlan()
                        plan.lnl(C.byref(s), C.byref(k), C.byref(L), 0, 0, 0, C.byref(p0))
                        assert plan.plan_calibrated(C.byref(p0)) == 0
                        seen.add(p0.form)
                        for filled, layered in itertools.product((0, 1), (0, 1)):
                            p1 = LnlPlan()
                            plan.lnl(C.byref(s), C.byref(k), C.byref(L), filled, layered, 1, C.byref(p1))
                            assert not p1.error and plan.plan_calibrated(C.byref(p1)) == 1
                            assert p1.form == BASELINE and p1.wide == (nhf_max > 26)
                            # the dynamic LDS: [table mode: the tables][per unit: the line table; split > 1: 1 + 4 + 1 sums of 4
                            # parts x 64 lanes]
                            split, upw = p1.G.split, p1.waves // p1.G.split
                            lds = 8 * ((TABLES if mode == 0 else 0) + (wave_doubles(ncomp, nhf_max) + (6 * 256 if split > 1 else 0)) * upw)
                            assert p1.lds == (max(lds, 8 * (TABLES + 768)) if mode == 0 else lds) and p1.lds <= LDS_PER_CU
                            if p0.form == BASELINE and not p0.error:                  # the slot more, and nothing else
                                assert (p1.G.split, p1.waves, p1.blocks) == (p0.G.split, p0.waves, p0.blocks)
                                assert p1.lds - p0.lds == (8 * 256 * upw if split > 1 else 0)
    assert seen == {PLAIN, W8, QUEUE, WEIGHTED, BASELINE}
    # the extra slot at split 2 and 4 (a single point of the benchmark's set: split 4; eleven: split 4; a few hundred: 2)
    for B, split in ((1, 4), (1500, 2), (4096, 1)):
        s, k, p = shape(), knobs(), LnlPlan()
        plan.lnl(C.byref(s), C.byref(k), C.byref(LpLaunch(B=B, mode=2, group_n=1, group_each=B, baseline=True, weighted=True)), 0, 0, 1, C.byref(p))
        assert p.G.split == split and p.lds == 8 * (wave_doubles(2, 21) + (6 * 256 if split > 1 else 0)) * (p.waves // split)
    # where the sixth slot is what does not fit: one unit per workgroup at the planned split.  N2H+ 2-1 (40 lines), ten
    # components, two waves per unit in the table mode -- the launch of tests/test_calibration.py: a baseline set's eight waves
    # hold four units in 158 KB, four calibrated units would need 166 KB
    s, k = shape(n_spec=1, size=300, nhf_max=40, ncomp=10, model=1, ndim=40, lnl_split=2), knobs()
    L = LpLaunch(B=200, mode=0, group_n=1, group_each=200, baseline=True, weighted=True)
    p0, p1 = LnlPlan(), LnlPlan()
    plan.lnl(C.byref(s), C.byref(k), C.byref(L), 0, 0, 0, C.byref(p0))
    plan.lnl(C.byref(s), C.byref(k), C.byref(L), 0, 0, 1, C.byref(p1))
    assert (p0.error, p0.G.split, p0.waves, p0.lds) == (None, 2, 8, 8 * (TABLES + 4 * (2000 + 5 * 256)))
    assert 8 * (TABLES + 4 * (2000 + 6 * 256)) > LDS_PER_CU
    assert (p1.error, p1.G.split, p1.waves, p1.lds, p1.blocks) == (None, 2, 2, 8 * (TABLES + 2000 + 6 * 256), 200)


def test_whatever_plans_with_a_baseline_plans_calibrated(plan):
    """The shapes of tests/test_launch_plan.py's list, each with a baseline: the calibrated plan exists wherever the baseline's
    does, with the same split and waves unless the sixth slot is what did not fit -- then fewer units per workgroup or a smaller
    split, which the bits do not depend on."""
    n_cu, n, moved = 256, 0, 0
    tw = np.zeros((11, 51, 2), dtype=np.int64)
    for ncomp in (1, 2, 3, 4, 10):
        for nhf in (1, 18, 26, 27, 40, 50):
            tw[ncomp, nhf] = table_workgroup(ncomp, nhf)
    fixed_B = np.array([1, 2, 63, 300, 513, 4096, 32768, 0, 0])
    for mode, nhf, size in itertools.product((0, 2), (1, 18, 26, 27, 40, 50), (128, 256, 511, 512, 1024, 2 ** 22 + 64)):
        blocks = []
        for size_rest, b_ix in ((size, range(9)), (1024, (0, 5, 8))):
            n_spec, ncomp, ws, queue, split, wpb, cap, b = [m.ravel() for m in np.meshgrid(
                (1, 2, 3, 16), (1, 2, 3, 4, 10), (0, 1), (0, 1), (0, 1, 2, 4), (1, 4, 16), (0, 2), b_ix, indexing='ij')]
            edge = -(-2 * n_cu * tw[ncomp, nhf, 1] * tw[ncomp, nhf, 0] // n_spec)
            B = np.where(b < 7, fixed_B[b], edge - (b == 7))
            one = np.ones_like(B)
            blocks.append(np.stack([mode * one, nhf * one, size * one, size_rest * one, n_spec, ncomp, B, ws, one, one,
                                    queue, one, split, wpb, cap, n_cu * one], axis=1)[(n_spec > 1) | (size_rest == size)])
        a = np.ascontiguousarray(np.concatenate(blocks), dtype=np.int64)
        assert a.shape[1] == len(IN)
        out = np.zeros((len(a), 10), dtype=np.int64)
        plan.both(len(a), a.ctypes.data, out.ctypes.data)
        bl, cal = out[:, :5], out[:, 5:]
        ok = bl[:, 0] == 0
        assert ok.any() and np.all(bl[ok, 4] == BASELINE)
        assert np.all(cal[ok, 0] == 0), dict(zip(IN, a[np.flatnonzero(ok & (cal[:, 0] != 0))[0]]))
        assert np.all(cal[ok, 4] == BASELINE) and np.all(cal[ok, 3] <= LDS_PER_CU) and np.all(cal[ok, 2] % cal[ok, 1] == 0)
        same = ok & (cal[:, 1] == bl[:, 1]) & (cal[:, 2] == bl[:, 2])
        # where the geometry moved, the baseline's geometry with six slots would not have fitted
        other = ok & ~same
        upw = bl[:, 2] // bl[:, 1]
        assert np.all((bl[other, 3] + 8 * 256 * upw[other] > LDS_PER_CU) & (bl[other, 1] > 1))
        assert np.all(cal[other, 1] <= bl[other, 1])
        n += int(ok.sum()); moved += int(other.sum())
    print(f'{n} baseline plans, {moved} of them with another geometry when calibrated')
    assert n > 100000


def test_the_fused_kernels_refuse_a_calibrated_set_first_of_all(plan):
    why = b'the resident kernel has no form for a calibration uncertainty: use nfa_ring_serve'
    same = ('refusal', 'ring_error', 'n_blocks', 'ctl_double', 'staged', 'lds_point', 'lds_ring')
    for ncomp, npar, nhf_max in ((1, 6, 21), (2, 6, 21), (3, 4, 15), (4, 7, 9), (2, 4, 33)):
        for mode, (bl, wt), banded, filled, layered in itertools.product((0, 2), ((0, 0), (0, 1), (1, 1)), (0, 1), (0, 1), (0, 1)):
            s, k = shape(n_spec=2, ncomp=ncomp, nhf_max=nhf_max, ndim=npar * ncomp, n_stage=npar, stage_doubles=200 * npar), knobs()
            p = FusedPlan()
            plan.fused9(C.byref(s), C.byref(k), mode, bl, wt, banded, filled, layered, 1, C.byref(p))
            assert p.refusal == why and p.ring_error == why
            p9, p8 = FusedPlan(), FusedPlan()
            plan.fused9(C.byref(s), C.byref(k), mode, bl, wt, banded, filled, layered, 0, C.byref(p9))
            plan.fused8(C.byref(s), C.byref(k), mode, bl, wt, banded, filled, layered, C.byref(p8))
            assert all(getattr(p9, f) == getattr(p8, f) for f in same) and p9.refusal != why


def test_the_new_entry_points_link_from_c(tmp_path):
    """include/nestfit_amd.h compiles as C99 and a C program that names the two new symbols links against the library."""
    from nestfit_amd.build import OUT, build
    build()
    src = tmp_path / 'use_calibration.c'
    src.write_text('#include "nestfit_amd.h"\n'
                   'typedef int (*set_t)(nfa_specset *, const double *);\n'
                   'typedef int (*get_t)(const nfa_specset *, double *);\n'
                   'int main(void) { set_t f = nfa_specset_set_calibration; get_t g = nfa_specset_calibration; return f == 0 || g == 0; }\n')
    exe = tmp_path / 'use_calibration'
    res = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', f'-I{ROOT / "include"}', str(src), '-o', str(exe),
                          f'-L{OUT.parent}', '-lnestfit_amd', f'-Wl,-rpath,{OUT.parent}', '-Wl,--allow-shlib-undefined'],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
