"""A beam filling factor per component of the LTE models without a GPU (`LteMix(species, fill=True)`,
nfa_specset_create_lte_filled): the restatement the device tests compare with, the host class, the store, the
launch plan's rule for filled sets and the new entry point's linkage from C.  The species are tests/mix_restatement.py's."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import fill_restatement as fr
import hf_restatement as hfr
import mix_restatement as mr
from test_launch_plan import FusedPlan, LnlPlan, LpLaunch, ROOT, knobs, shape
from test_lte_bands_cpu import N_CHAN, band_axis
from test_lte_mix_cpu import _stub_backend


def _draw(rng, ncomp, n_species):
    """voff, tex, lncol, sigm, the further column densities (the mix's 3 + K rows)."""
    lncol = rng.uniform(13.0, 15.5, ncomp)
    more = [lncol + rng.uniform(-3.0, 3.0, ncomp) for _ in range(n_species - 1)]
    return np.concatenate([rng.uniform(-6, 6, ncomp), 10 ** rng.uniform(0.5, 1.9, ncomp), lncol, 10 ** rng.uniform(-1.0, 0.2, ncomp)] + more)


def _rows(na, rng):
    mol, ks, iso, isos = mr.test_species(na)
    tables = (na.LteBlend(ks + isos), isos[1])
    return (mol, iso), [[band_axis(ks[0].nu), rng.normal(0, 0.2, N_CHAN), 0.2, t] for t in tables]


def test_a_factor_of_one_restates_the_mix_bit_for_bit(nfo):
    import nestfit_amd as na
    rng = np.random.default_rng(5)
    species, rows = _rows(na, rng)
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    lit = 0
    for k in range(200):
        ncomp = 1 + k % 3
        theta = _draw(rng, ncomp, 2)
        want_spec, want_lnl = mr.restated(nfo, rows, species, theta, tbgs)
        spec, lnl = fr.restated(nfo, rows, species, np.concatenate([theta, np.zeros(ncomp)]), tbgs)
        assert np.array_equal(spec, want_spec) and lnl == want_lnl
        lit += int(np.abs(want_spec).max() > 0.1)
    assert lit > 150                                                    # (spectra with lines in them)


def test_a_tenth_of_the_beam_is_a_tenth_of_the_spectrum(nfo):
    """One component: lnff = -1 against lnff = 0 to 1e-15 relative (10.0 ** -1.0 is the double 0.1: in fact to the bit);
    of two components only the one with the factor scales."""
    import nestfit_amd as na
    rng = np.random.default_rng(6)
    species, rows = _rows(na, rng)
    x, tbg, blend = rows[0][0], hfr.tbg_of(nfo, rows[0][0]), rows[0][3]
    for k in range(20):
        theta = _draw(rng, 1, 2)
        full = fr.fill_predict(nfo, x, tbg, blend, species, np.concatenate([theta, [0.0]]))
        tenth = fr.fill_predict(nfo, x, tbg, blend, species, np.concatenate([theta, [-1.0]]))
        assert np.abs(full).max() > 0 and np.array_equal(tenth == 0, full == 0)
        nz = full != 0
        assert (np.abs(tenth[nz] - 0.1 * full[nz]) <= 1e-15 * np.abs(0.1 * full[nz])).all()
    theta = _draw(rng, 2, 2)
    one = [fr.fill_predict(nfo, x, tbg, blend, species, np.concatenate([theta.reshape(5, 2)[:, c], [0.0]])) for c in (0, 1)]
    both = fr.fill_predict(nfo, x, tbg, blend, species, np.concatenate([theta, [-1.0, 0.0]]))
    np.testing.assert_allclose(both, 0.1 * one[0] + one[1], rtol=1e-14, atol=1e-300)
    # -inf: the component adds nothing, exactly; NaN: NaN where the component has optical depth
    assert np.array_equal(fr.fill_predict(nfo, x, tbg, blend, species, np.concatenate([theta, [-np.inf, 0.0]])), one[1])
    assert np.isnan(fr.fill_predict(nfo, x, tbg, blend, species, np.concatenate([theta, [np.nan, 0.0]]))).any()


def test_the_filled_mix_against_the_unfilled_one():
    import nestfit_amd as na
    mol, ks, iso, isos = mr.test_species(na)
    plain, filled = na.LteMix([mol, iso]), na.LteMix([mol, iso], fill=True)
    assert plain.fill is False and filled.fill is True and na.LteMix([mol, iso], fill=False) == plain
    assert (plain.N, filled.N, filled.NAME, filled.IX_VCEN, filled.IX_SIGM) == (5, 6, 'lte_mix', 0, 3)
    assert filled.PAR_NAMES == plain.PAR_NAMES + ['lnff'] and filled.PAR_NAMES_SHORT == plain.PAR_NAMES_SHORT + ['lf']
    assert filled.TEX_LABELS[:5] == plain.TEX_LABELS and filled.TEX_LABELS_WITH_UNITS[:5] == plain.TEX_LABELS_WITH_UNITS
    assert len(filled.TEX_LABELS) == len(filled.TEX_LABELS_WITH_UNITS) == 6 and 'f' in filled.TEX_LABELS[5]
    assert filled.get_par_names(2)[-4:] == ['lN21', 'lN22', 'lf1', 'lf2']
    assert filled != plain and plain != filled and hash(filled) != hash(plain) and len({plain, filled}) == 2
    twin = na.LteMix((mol, iso), fill=True)
    assert filled == twin and hash(filled) == hash(twin) and filled.Runner is not twin.Runner
    assert repr(plain) == "LteMix('top', 'iso')" and repr(filled) == "LteMix('top', 'iso', fill=True)"
    assert filled.species == plain.species and filled.lncol_row(1) == 4
    assert (filled.Runner.N_MODEL, filled.Runner.FILL, filled.Runner.MODEL_INFO, filled.Runner.MODEL) == (6, True, filled, 4)
    assert plain.Runner.FILL is False and filled.Spectrum.MIX is filled and filled.Spectrum.FILL is True
    one = na.LteMix([mol], fill=True)                                   # one species: the common case
    assert one.N == 5 and one.PAR_NAMES == ['voff', 'tex', 'lncol', 'sigm', 'lnff'] and one != na.LteMix([mol])
    assert na.LteMix([mol, iso, *(m for m, _ in mr.made_up_species(na, ks[0].nu))], fill=True).N == 8
    with pytest.raises(AttributeError):
        filled.fill = False
    # exactly what it was without the keyword
    assert plain.PAR_NAMES == ['voff', 'tex', 'lncol', 'sigm', 'lncol2'] and hash(plain) == hash(('lte_mix', mol, iso))
    from nestfit_amd import _ffi
    assert 'nfa_specset_create_lte_filled' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'nfa_specset_create_lte_filled')
    assert _ffi.SIGNATURES['nfa_specset_create_lte_filled'] == _ffi.SIGNATURES['nfa_specset_create_lte_mix']


def test_every_value_error_comes_before_a_device_call():
    """(There is no device here: whatever reached one would fail with another error.)"""
    import nestfit_amd as na
    from nestfit_amd._model import _SpecSet
    from nestfit_amd.cube import CubeRunner
    mol, ks, iso, isos = mr.test_species(na)
    (m3, t3), _ = mr.made_up_species(na, ks[0].nu)
    for bad in (1, 'yes', None, 0.5):
        with pytest.raises(ValueError, match='`fill` is True or False'):
            na.LteMix([mol, iso], fill=bad)
    with pytest.raises(ValueError):
        na.LteMix([mol, mol], fill=True)
    filled = na.LteMix([mol, iso], fill=True)
    blend = na.LteBlend(ks + isos)
    x = band_axis(ks[0].nu, 64)
    row = lambda t: [x, np.zeros(64), 0.1, t]
    with pytest.raises(ValueError, match="'third', which is no species of the mix"):
        filled.Runner.from_data([row(blend), row(t3)], None)
    with pytest.raises(ValueError, match='no transition in any spectrum.*iso'):
        filled.Runner.from_data([row(mol.band(ks))], None)
    with pytest.raises(ValueError, match='LteBlend per spectrum'):
        filled.Runner.from_data([row(na.LineTable(1e11, [0.0], [1.0]))], None)
    with pytest.raises(ValueError, match='baseline_order'):
        filled.Runner.from_data([row(blend)], None, baseline_order=7)
    with pytest.raises(ValueError, match='no species of the mix'):
        filled.Spectrum(x, np.zeros(64), 0.1, t3)
    with pytest.raises(ValueError, match='Invalid parameter vector length'):
        filled.predict(None, np.zeros(5))                               # six per component
    # a filling factor belongs to a mix: species and lines
    with pytest.raises(ValueError, match='belongs to an LTE mix'):
        _SpecSet([x], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), fill=True)
    with pytest.raises(ValueError, match='belongs to an LTE mix'):
        CubeRunner([x], [1], np.zeros((1, 64)), np.full((1, 1), 0.1), None, fill=True)
    with pytest.raises(ValueError, match='belongs to an LTE mix'):
        CubeRunner([x], None, np.zeros((1, 64)), np.full((1, 1), 0.1), None, model=3, lines=[na.LineTable(1e11, [0.0], [1.0])], fill=True)


# ---------------------------------------------------------------------------- the cube driver and the store
def _priors(na, ranges):
    from scipy import stats
    x = np.linspace(0, 1, 200)
    return na.PriorTransformer([
        na.Prior(na.Distribution(lo + x * (hi - lo), stats.uniform(lo, hi - lo).pdf(lo + x * (hi - lo))), k)
        for k, (lo, hi) in enumerate(ranges)])


RANGES6 = [(-4, 4), (3.0, 20), (12.0, 14.5), (0.2, 1.5), (11.0, 14.0), (-2.0, 0.0)]


def _fit(na, tmp_path, name, mix, stack, ranges):
    from nestfit_amd.fitter import CubeFitter
    fitter = CubeFitter(stack, _priors(na, ranges), mix.Runner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0, fit_backend=_stub_backend)
    path = str(tmp_path / name)
    fitter.fit_cube(path, nproc=1)
    return fitter, path


def test_store_round_trip_of_a_filled_mix(tmp_path):
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.store import HdfStore
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = mr.test_species(na)
    plain, filled = na.LteMix([mol, iso]), na.LteMix([mol, iso], fill=True)
    blend = na.LteBlend(ks + isos, name='J=5-4')
    stack = _stack(na, [blend, isos[1]])
    fitter, path = _fit(na, tmp_path, 'filled', filled, stack, RANGES6)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs, fitter.species, fitter.fill) == (4, 6, {}, (mol, iso), True)
    with HdfStore(path) as store:
        root = store.hdf.attrs
        assert root['model_name'] == 'lte_mix' and int(root['n_params']) == 6 and bool(root['fill']) is True
        assert list(root['par_names']) == filled.PAR_NAMES and list(root['par_names_short']) == filled.PAR_NAMES_SHORT
        assert len(root['tex_labels']) == 6 and store.model.IX_VCEN == 0 and store.model.IX_SIGM == 3
        assert int(store.hdf['/model_partition'].attrs['n_species']) == 2
        back, species = store.read_model_lines(with_species=True)
        assert species == (mol, iso) and back == [blend, na.LteBlend([isos[1]])] and store.read_model_fill() is True
        assert na.LteMix(species, fill=store.read_model_fill()) == filled          # what rebuilds the model
    with HdfStore(path) as store:                                       # reopened
        assert pp.check_model_lines(store, stack) == [blend, isos[1]]
        assert pp.check_model_fill(store) is True and pp.check_model_fill(store, filled.Runner) is True
        with pytest.raises(ValueError, match='fitted with a filling factor'):
            pp.check_model_fill(store, plain.Runner)
        with pytest.raises(ValueError, match='fitted with a filling factor'):
            pp.postprocess_run(store, stack, runner=plain.Runner, predict_backend=lambda *a: None)
    # an old store -- one without the attribute -- reads as unfilled
    fitter, old = _fit(na, tmp_path, 'plain', plain, stack, RANGES6[:5])
    assert fitter.fill is False and fitter.n_model == 5
    with HdfStore(old) as store:
        assert 'fill' not in store.hdf.attrs and store.read_model_fill() is False and int(store.hdf.attrs['n_params']) == 5
        assert pp.check_model_fill(store) is False and pp.check_model_fill(store, plain.Runner) is False
        assert na.LteMix(store.read_model_species(), fill=store.read_model_fill()) == plain
        with pytest.raises(ValueError, match='fitted without a filling factor'):
            pp.check_model_fill(store, filled.Runner)
        with pytest.raises(ValueError, match='fitted without a filling factor'):
            pp.postprocess_run(store, stack, runner=filled.Runner, predict_backend=lambda *a: None)


def test_a_filled_store_of_one_species_keeps_its_species(tmp_path):
    """One species with a filling factor takes the mix's layout: a store in the single-species layout could not say, on
    reading, that its lines are a mix's."""
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.store import HdfStore
    from test_lte_bands_cpu import _stack, top_species
    mol, ks = top_species(na)
    one = na.LteMix([mol], fill=True)
    stack = _stack(na, [mol.band(ks, name='J=5-4'), ks[2]])
    fitter, path = _fit(na, tmp_path, 'one', one, stack, RANGES6[:4] + RANGES6[5:])
    assert (fitter.n_model, fitter.species, fitter.fill) == (5, (mol,), True)
    with HdfStore(path) as store:
        assert int(store.hdf.attrs['n_params']) == 5 and list(store.hdf.attrs['par_names']) == ['voff', 'tex', 'lncol', 'sigm', 'lnff']
        assert store.read_model_species() == (mol,) and store.read_model_fill() is True
        assert store.read_model_lines() == [na.LteBlend(ks, name='J=5-4'), na.LteBlend([ks[2]])]
        assert pp.check_model_lines(store, stack) == [mol.band(ks), ks[2]] and pp.check_model_fill(store, one.Runner) is True
        assert na.LteMix(store.read_model_species(), fill=store.read_model_fill()) == one


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void lnl(const LpShape *s, const LpKnobs *k, const LpLaunch *L, int filled, LnlPlan *out) {
    LpLaunch l = *L;
    l.filled = filled != 0;
    *out = plan_lnl(*s, *k, l);
}
int plan_filled(const LnlPlan *p) { return p->filled ? 1 : 0; }
int launch_filled(const LpLaunch *L) { return L->filled ? 1 : 0; }
void fused5(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, FusedPlan *out) { *out = plan_fused(*s, *k, mode, bl != 0, wt != 0); }
void fused6(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0);
}
void fused7(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, int filled, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0, filled != 0);
}
int size_of(int i) { const int s[] = {(int)sizeof(LpLaunch), (int)sizeof(LnlPlan), (int)sizeof(FusedPlan)}; return s[i]; }
}
'''
PLAIN, W8, QUEUE, WEIGHTED, BASELINE = range(5)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('fill_plan')
    src, so = tmp / 'plan.cpp', tmp / 'libplan.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    # the mirrors of tests/test_launch_plan.py still have the structures' sizes: the flags sit in padding
    assert [lib.size_of(i) for i in range(3)] == [C.sizeof(LpLaunch), C.sizeof(LnlPlan), C.sizeof(FusedPlan)]
    return lib


def test_a_filled_set_takes_baseline_weighted_or_plain_and_says_so(plan):
    fields = ('form', 'wide', 'waves', 'lds', 'blocks')
    seen = set()
    for mode in (0, 2):
        for B in (1, 11, 64, 4096, 32768):
            for nhf_max, size in ((9, 300), (21, 1024), (33, 1024)):
                for ncomp in (1, 2, 3, 4, 8):
                    for write_spec in (False, True):
                        for baseline, weighted in ((False, False), (False, True), (True, True)):
                            s = shape(n_spec=2, size=size, nhf_max=nhf_max, ncomp=ncomp, model=4, ndim=6 * ncomp, n_stage=0, stage_doubles=0)
                            L = LpLaunch(B=B, mode=mode, group_n=1, group_each=B, write_spec=write_spec, has_prior=True,
                                         baseline=baseline, weighted=weighted, has_queue=True)
                            assert plan.launch_filled(C.byref(L)) == 0                # the mirror's zero padding: not filled
                            k = knobs()
                            p0, p1 = LnlPlan(), LnlPlan()
                            plan.lnl(C.byref(s), C.byref(k), C.byref(L), 0, C.byref(p0))
                            plan.lnl(C.byref(s), C.byref(k), C.byref(L), 1, C.byref(p1))
                            assert p0.error == p1.error                             # (a line table too large for the LDS: for both)
                            if p0.error:
                                continue
                            assert plan.plan_filled(C.byref(p0)) == 0 and plan.plan_filled(C.byref(p1)) == 1
                            want = BASELINE if baseline else WEIGHTED if weighted else PLAIN
                            assert p1.form == want and p1.form not in (QUEUE, W8)
                            seen.add(p0.form)
                            # wide and the split are what they are without the factor; where the unfilled set takes the
                            # same form, so is everything else
                            assert p1.wide == p0.wide == (nhf_max > 26) and p1.G.split == p0.G.split and p1.waves == p0.waves
                            if p0.form == p1.form:
                                assert all(getattr(p0, f) == getattr(p1, f) for f in fields)
    assert seen == {PLAIN, W8, QUEUE, WEIGHTED, BASELINE}                   # (the unfilled plans did take the queue and w8)


def test_the_fused_kernels_refuse_a_filled_set(plan):
    why = b'the resident kernel has no form for a filling factor: use nfa_ring_serve'
    bands = b'the resident kernel has no form for LTE bands: use nfa_ring_serve'
    batch = b"this runner's points go through the batch kernels: use nfa_ring_serve"
    same = ('refusal', 'ring_error', 'n_blocks', 'ctl_double', 'staged', 'lds_point', 'lds_ring')
    for ncomp, npar, want in ((1, 5, why), (2, 6, why), (3, 8, why), (4, 6, why), (4, 7, batch), (5, 5, batch)):
        for mode in (0, 2):
            for bl, wt in ((0, 0), (0, 1), (1, 1)):
                s, k = shape(n_spec=2, ncomp=ncomp, nhf_max=9, model=4, ndim=npar * ncomp, n_stage=npar, stage_doubles=200 * npar), knobs()
                p = FusedPlan()
                plan.fused7(C.byref(s), C.byref(k), mode, bl, wt, 1, 1, C.byref(p))
                assert p.refusal == want and p.ring_error == want, (ncomp, npar, p.refusal)
                # the five- and six-argument calls: the seven-argument call at false
                for banded in (0, 1):
                    p7, p6 = FusedPlan(), FusedPlan()
                    plan.fused7(C.byref(s), C.byref(k), mode, bl, wt, banded, 0, C.byref(p7))
                    plan.fused6(C.byref(s), C.byref(k), mode, bl, wt, banded, C.byref(p6))
                    assert all(getattr(p7, f) == getattr(p6, f) for f in same)
                    assert p7.refusal != why and (p7.refusal == bands) == (banded == 1 and want == why and not wt)
                p5 = FusedPlan()
                plan.fused5(C.byref(s), C.byref(k), mode, bl, wt, C.byref(p5))
                plan.fused7(C.byref(s), C.byref(k), mode, bl, wt, 0, 0, C.byref(p7))
                assert all(getattr(p7, f) == getattr(p5, f) for f in same)


def test_the_new_entry_point_links_from_c(tmp_path):
    """include/nestfit_amd.h compiles as C99 and a C program that names nfa_specset_create_lte_filled links against the library;
    the new entry point has nfa_specset_create_lte_mix's type."""
    from nestfit_amd.build import OUT, build
    build()
    src = tmp_path / 'use_fill.c'
    src.write_text('#include "nestfit_amd.h"\n'
                   'typedef int (*fn_t)(nfa_specset **, int, const int64_t *, const int32_t *, const int32_t *, const double *,\n'
                   '                    const double *, const double *, const double *, const double *, const double *, int,\n'
                   '                    const int32_t *, const int32_t *, const double *, const double *, const double *const *,\n'
                   '                    int64_t, const double *, const double *, const double *);\n'
                   'int main(void) { fn_t f = nfa_specset_create_lte_filled, g = nfa_specset_create_lte_mix; return f == 0 || g == 0; }\n')
    exe = tmp_path / 'use_fill'
    res = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', f'-I{ROOT / "include"}', str(src), '-o', str(exe),
                          f'-L{OUT.parent}', '-lnestfit_amd', f'-Wl,-rpath,{OUT.parent}', '-Wl,--allow-shlib-undefined'],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
