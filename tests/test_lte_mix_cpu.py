"""LTE mixes without a GPU (nestfit_amd/lte.py: LteBlend, LteMix): the restatement the device tests compare
with, the host classes, the mixed ratio form the device computes tau_main in, the launch plan's refusal of the fused
kernels and the new entry point's linkage from C.  The species are tests/mix_restatement.py's."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import band_restatement as br
import hf_restatement as hfr
import lte_restatement as lr
import mix_restatement as mr
from test_launch_plan import FusedPlan, ROOT, knobs, shape
from test_lte_bands_cpu import N_CHAN, _trans, band_axis, top_species


def test_the_species_are_what_the_tests_need():
    import nestfit_amd as na
    mol, ks, iso, isos = mr.test_species(na)
    v = [(1.0 - t.nu / ks[0].nu) * lr.CKMS for t in isos]               # km/s from the main K = 0
    assert v[0] == pytest.approx(4.2, abs=0.01) and v[1] == pytest.approx(6.7, abs=0.02) and v[2] == pytest.approx(14.2, abs=0.06)
    assert v[0] - 2.5 < 2 * 10 ** 0.2                                   # the main K = 1 and the iso K = 0 blend at the larger widths
    assert iso.n != mol.n and not np.isin(iso.q_temp, mol.q_temp).any() # another grid of another length
    x = band_axis(ks[0].nu)
    (m3, t3), (m4, t4) = mr.made_up_species(na, ks[0].nu)
    for t in isos + [t3, t4]:
        assert x[0] < t.nu * (1 - 6.0 / lr.CKMS) and t.nu * (1 + 6.0 / lr.CKMS) < x[-1]
    # in the engine's order (lower-level energy) the two ladders interleave, and the reference transition of a window with
    # both is the isotopologue's K = 0 (the smaller B): with the main species listed first, g = 0 is of species 1
    e_low = sorted((t.e_up - lr.H * t.nu / lr.KB, t.molecule.name) for t in ks + isos)
    assert [n for _, n in e_low] == ['iso', 'top', 'iso', 'top', 'iso', 'top', 'top']


def test_a_mix_of_one_species_restates_the_band_bit_for_bit(nfo):
    import nestfit_amd as na
    from test_lte_bands import draw_params
    mol, ks = top_species(na)
    rng = np.random.default_rng(11)
    rows = [[band_axis(t.nu), rng.normal(0, 0.2, N_CHAN), 0.2, t] for t in (mol.band(ks), ks[2])]
    blends = [[x, d, s, na.LteBlend(t.transitions if hasattr(t, 'transitions') else [t])] for x, d, s, t in rows]
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
    for ncomp in (1, 2, 3):
        for k in range(20):
            theta = draw_params(rng, ncomp, mol, k)
            want_spec, want_lnl = br.restated(nfo, rows, theta, tbgs)
            for these in (rows, blends):
                spec, lnl = mr.restated(nfo, these, [mol], theta, tbgs)
                assert np.array_equal(spec, want_spec) and lnl == want_lnl


# The mixed ratio form against the direct formula on each species' own table, held to the band test's 1e-13.
#   1. On the grid the bound was set on -- 8 temperatures from 0.128 to 400 K, column-density differences -1.8, +3.5 and 0,
#      the 7 transitions -- against lte_restatement.tau_main in doubles, wherever that exceeds 1e-300.
#   2. On a finer grid (96 temperatures, the nodes of both tables, 8 column-density pairs) against the same formula in
#      extended precision (mix_restatement.tau_main_extended).  There the doubles' evaluation is itself no reference: at
#      0.165 K, E_u / tex = 550 for the main K = 3, it is 4.9e-14 off the extended value, and the ratio form, 7.7e-14 off the
#      extended value at worst, reads 1.15e-13 against it.  (Most of the 7.7e-14 is the rounding of de = 85 K, half an ulp of
#      which is 7e-15 K, over a tex of 0.14 K: the band record's, lte_band_kernel's too.)
# As in tests/test_lte_bands_cpu.py the cold end is reached with small columns (every factor of the direct formula a
# normal number down to results below 1e-280); the physical columns are checked above 0.2 K.
COARSE_TEX = np.geomspace(0.128, 400.0, 8)
COARSE_PAIRS = ((8.0, -1.8), (4.5, 3.5), (8.0, 0.0), (14.0, -1.8), (12.0, 3.5), (13.5, 0.0))
MIX_TEX = np.concatenate([np.geomspace(0.128, 400.0, 96), [4.0, 5.0, 60.0, 75.0], np.geomspace(4.0, 75.0, 21)[3:6], np.geomspace(5.0, 60.0, 32)[7:9]])
PAIRS = COARSE_PAIRS + ((14.5, -3.0), (12.5, 3.0))     # lncol_0, lncol_1 - lncol_0


def _ratio_form_deviations(mol, ks, isos, texs, pairs, reference):
    """(worst relative deviation of the mixed ratio form from `reference`, smallest reference value, values compared) over
    the window with both ladders (reference transition: the iso K = 0, of species 1) and the one without it (the main K = 0)."""
    worst, smallest, n = 0.0, np.inf, 0
    with np.errstate(under='ignore'):
        for first, window in ((isos[0], ks + isos), (ks[0], ks + isos[1:])):
            ref = _trans(first)
            for lncol0, d in pairs:
                for tex in texs:
                    for t in window:
                        lncol = lncol0 if t.molecule is mol else lncol0 + d
                        direct = lr.tau_main(_trans(t), t.molecule.q_temp, t.molecule.q_val, float(tex), lncol, 0.7)
                        if not direct > 1e-300 or (lncol0 > 9 and tex < 0.2):
                            continue
                        want = direct if reference == 'doubles' else mr.tau_main_extended(_trans(t), t.molecule, tex, lncol, 0.7)
                        got = (direct if reference == 'doubles against extended' else
                               float(mr.mixed_ratio_form(_trans(t), t.molecule, ref, mol, tex, lncol, lncol0, 0.7, is_ref=t is first)))
                        worst = max(worst, float(abs(got - want) / want))
                        smallest = min(smallest, direct)
                        n += 1
    return worst, smallest, n


def test_the_mixed_ratio_form_agrees_with_the_direct_formula():
    import nestfit_amd as na
    mol, ks, iso, isos = mr.test_species(na)
    worst, smallest, n = _ratio_form_deviations(mol, ks, isos, COARSE_TEX, COARSE_PAIRS, 'doubles')
    print(f'mixed ratio form, 8 temperatures, against the doubles: worst relative difference {worst:.2e} over {n} values')
    assert n > 400 and worst < 1e-13
    assert np.finfo(np.longdouble).eps < 2e-19                          # (the extended reference is one)
    worst, smallest, n = _ratio_form_deviations(mol, ks, isos, MIX_TEX, PAIRS, 'extended')
    print(f'mixed ratio form, finer grid, against extended precision: worst relative difference {worst:.2e} over {n} values; '
          f'smallest direct value {smallest:.2e}')
    assert n > 4000 and smallest < 1e-280
    assert worst < 1e-13
    # ... and the argument for the extended reference, checked and not only stated: on that grid the doubles' own
    # evaluation of the direct formula is several 1e-14 off the extended one, so that a form within 1e-13 of the truth can
    # read more than 1e-13 against the doubles (the ratio form does: 1.15e-13)
    off, _, _ = _ratio_form_deviations(mol, ks, isos, MIX_TEX, PAIRS, 'doubles against extended')
    against_doubles, _, _ = _ratio_form_deviations(mol, ks, isos, MIX_TEX, PAIRS, 'doubles')
    print(f'the direct formula in doubles against extended precision: worst {off:.2e}; the ratio form against the doubles: {against_doubles:.2e}')
    assert 3e-14 < off < 1e-13 and against_doubles < worst + off
    # a spectrum whose reference transition is of species 1: the factor alone
    ref1 = _trans(isos[0])
    for tex in (3.0, 11.0, 47.0, 90.0):
        direct = lr.tau_main(ref1, iso.q_temp, iso.q_val, tex, 12.4, 0.7)
        got = float(mr.mixed_ratio_form(ref1, iso, ref1, mol, tex, 12.4, 14.1, 0.7, is_ref=True))
        assert abs(got - direct) / direct < 1e-13
    # equal columns and one table under two names: the factor is exactly 1
    twin = na.Molecule('twin', mol.q_temp, mol.q_val)
    t2 = twin.transition(*_trans(ks[2]))
    ref = _trans(ks[0])
    tau0 = lr.tau_main(ref, mol.q_temp, mol.q_val, 20.0, 14.0, 0.7)
    assert float(mr.mixed_ratio_form(_trans(t2), twin, ref, mol, 20.0, 14.0, 14.0, 0.7)) == float(br.ratio_form(_trans(ks[2]), ref, tau0, 20.0))


def test_mix_tau_main_equals_the_restatement():
    import nestfit_amd as na
    mol, ks, iso, isos = mr.test_species(na)
    mix = na.LteMix([mol, iso])
    blend = na.LteBlend([ks[0], isos[0], ks[1], isos[2], ks[3]])
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(200):
        tex, sigm = 10 ** rng.uniform(0.4, 1.9), 10 ** rng.uniform(-1.0, 0.2)
        lncols = rng.uniform(12, 15.5, 2)
        got = mix.tau_main(blend, tex, lncols, sigm)
        assert got.shape == (5,)
        for g, t in zip(got, blend):
            m = t.molecule
            want = lr.tau_main(_trans(t), m.q_temp, m.q_val, tex, lncols[0 if m is mol else 1], sigm)
            worst = max(worst, abs(float(g) - want) / want)
    print(f'LteMix.tau_main: worst relative difference {worst:.2e}')
    assert worst < 1e-14
    assert np.array_equal(mix.tau_main(mol.band(ks), 20.0, [14.0, 9.0], 0.5), mol.band(ks).tau_main(20.0, 14.0, 0.5))
    with pytest.raises(ValueError, match='one column density per species'):
        mix.tau_main(blend, 20.0, [14.0], 0.5)


def test_every_value_error():
    import nestfit_amd as na
    mol, ks, iso, isos = mr.test_species(na)
    (m3, t3), (m4, t4) = mr.made_up_species(na, ks[0].nu)
    blend = na.LteBlend(ks + isos)
    assert (blend.n_trans, blend.n_lines, blend.n, blend.nu, blend.molecules) == (7, 9, 9, ks[0].nu, (mol, iso))
    assert na.LteBlend([isos[1], ks[0]]).molecules == (iso, mol) and na.LteBlend(ks[:1]).molecules == (mol,)
    for bad in ([], [ks[0], 'x'], [na.LineTable(1e11, [0.0], [1.0])], 5, [mol.band(ks)]):
        with pytest.raises(ValueError):
            na.LteBlend(bad)
    nine = [mol.transition(4e10 + 1e6 * k, 10.0 + k, 3.0, 1e-6) for k in range(9)]
    assert na.LteBlend(nine[:8]).n_trans == 8
    with pytest.raises(ValueError, match='1..8 transitions'):
        na.LteBlend(nine)
    with pytest.raises(ValueError, match='twice'):
        na.LteBlend([ks[0], isos[0], mol.transition(*_trans(ks[0]))])
    assert na.LteBlend([ks[0], iso.transition(*_trans(ks[0]))]).n_trans == 2     # the same numbers, another species
    many = [(mol, iso, m3)[k].transition(4e10 + 1e6 * k, 10.0 + k, 3.0, 1e-6, voff=np.arange(17.0), tau_wts=np.full(17, 1 / 17)) for k in range(3)]
    with pytest.raises(ValueError, match='at most 50 lines'):
        na.LteBlend(many)
    # the mix
    assert na.LteMix([mol]).N == 4 and na.LteMix([mol, iso, m3, m4]).N == 7
    for bad in ([], [mol, mol], [mol, iso, m3, m4, na.Molecule('fifth', [5.0, 10.0], [1.0, 2.0])], [mol, 'iso'], 7,
                [mol, na.Molecule(mol.name, mol.q_temp, mol.q_val)]):
        with pytest.raises(ValueError):
            na.LteMix(bad)
    # a runner's rows, checked before any device call (there is no device here)
    mix = na.LteMix([mol, iso])
    x = band_axis(ks[0].nu, 64)
    row = lambda t: [x, np.zeros(64), 0.1, t]
    with pytest.raises(ValueError, match="'third', which is no species of the mix"):
        mix.Runner.from_data([row(blend), row(t3)], None)
    with pytest.raises(ValueError, match='no transition in any spectrum.*iso'):
        mix.Runner.from_data([row(mol.band(ks)), row(ks[1])], None)
    with pytest.raises(ValueError, match='LteBlend per spectrum'):
        mix.Runner.from_data([row(na.LineTable(1e11, [0.0], [1.0]))], None)
    with pytest.raises(ValueError, match='baseline_order'):
        mix.Runner.from_data([row(blend)], None, baseline_order=7)
    with pytest.raises(ValueError, match='no species of the mix'):
        mix.Spectrum(x, np.zeros(64), 0.1, t3)
    with pytest.raises(ValueError, match='no species of the mix'):
        mix.tau_main(t3, 20.0, [14.0, 13.0], 0.5)
    # the single-species classes are what they were: two molecules are refused
    with pytest.raises(ValueError, match='one Molecule'):
        mol.band([ks[0], isos[0]])
    with pytest.raises(ValueError, match='one Molecule'):
        na.LteRunner.from_data([row(mol.band(ks)), row(isos[0])], None)
    with pytest.raises(ValueError, match='LteLines'):
        na.LteRunner.from_data([row(blend)], None)
    with pytest.raises(ValueError, match='LteLines or an LteBand'):
        na.LteSpectrum(x, np.zeros(64), 0.1, blend)


def test_immutable_and_compared_by_value():
    import nestfit_amd as na
    mol, ks, iso, isos = mr.test_species(na)
    mol_b, ks_b, iso_b, isos_b = mr.test_species(na)
    a, b = na.LteBlend(ks + isos, name='window'), na.LteBlend(ks_b + isos_b)
    assert a == b and hash(a) == hash(b) and a is not b and len({a, b}) == 1 and a.name == 'window'
    assert a.transitions == tuple(ks + isos) and list(a) == ks + isos and a[4] == isos[0] and len(a) == 7
    assert na.LteBlend(isos + ks) != a and na.LteBlend(ks) != mol.band(ks) and mol.band(ks) != na.LteBlend(ks)
    for key in ('name', '_transitions', 'nu', 'other'):
        with pytest.raises(AttributeError):
            setattr(a, key, 1.0)
    with pytest.raises(AttributeError):
        del a._name
    m1, m2 = na.LteMix([mol, iso]), na.LteMix((mol_b, iso_b))
    assert m1 == m2 and hash(m1) == hash(m2) and na.LteMix([iso, mol]) != m1 and m1.species == (mol, iso) and m1.n_species == 2
    assert (m1.N, m1.NAME, m1.IX_VCEN, m1.IX_SIGM) == (5, 'lte_mix', 0, 3)
    assert m1.PAR_NAMES == ['voff', 'tex', 'lncol', 'sigm', 'lncol2'] and m1.PAR_NAMES_SHORT == ['v', 'Tx', 'lN', 's', 'lN2']
    assert len(m1.TEX_LABELS) == len(m1.TEX_LABELS_WITH_UNITS) == 5 and m1.TEX_LABELS[:4] == na.lte.TEX_LABELS
    assert m1.get_par_names() == m1.PAR_NAMES_SHORT and m1.get_par_names(2) == ['v1', 'v2', 'Tx1', 'Tx2', 'lN1', 'lN2', 's1', 's2', 'lN21', 'lN22']
    assert na.LteMix([mol, iso, *(m for m, _ in mr.made_up_species(na, ks[0].nu))]).PAR_NAMES[4:] == ['lncol2', 'lncol3', 'lncol4']
    assert issubclass(m1.Runner, na.lte._MixRunner) and m1.Runner.MODEL_INFO is m1 and m1.Runner.N_MODEL == 5 and m1.Runner.MODEL == 4
    assert m1.Spectrum.MIX is m1 and m1.Runner is not m2.Runner
    for key in ('N', 'species', 'Runner', 'other'):
        with pytest.raises(AttributeError):
            setattr(m1, key, 1)
    for name in ('LteBlend', 'LteMix'):
        assert name in na.__all__ and getattr(na, name) is getattr(na.lte, name)
    assert na.model_module('lte_mix').IX_VCEN == 0 and na.model_module('lte_mix').IX_SIGM == 3 and na.model_module('lte') is na.lte
    from nestfit_amd import _ffi
    assert 'nfa_specset_create_lte_mix' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'nfa_specset_create_lte_mix')


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void fused6(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0);
}
int fused_size() { return (int)sizeof(FusedPlan); }
}
'''


def test_the_fused_kernels_refuse_a_mix_as_a_banded_set(tmp_path):
    """A mix set always owns a band record, so the engine plans it with banded = true: five parameters per component."""
    src, so = tmp_path / 'plan.cpp', tmp_path / 'libplan.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    assert lib.fused_size() == C.sizeof(FusedPlan)
    why = b'the resident kernel has no form for LTE bands: use nfa_ring_serve'
    batch = b"this runner's points go through the batch kernels: use nfa_ring_serve"
    for ncomp, npar, want in ((1, 5, why), (2, 5, why), (3, 7, why), (4, 6, why), (4, 7, batch), (5, 5, batch)):   # 24 dimensions at most
        for mode in (0, 2):
            s, k, p = shape(n_spec=2, ncomp=ncomp, nhf_max=9, model=4, ndim=npar * ncomp, n_stage=npar, stage_doubles=200 * npar), knobs(), FusedPlan()
            lib.fused6(C.byref(s), C.byref(k), mode, 0, 0, 1, C.byref(p))
            assert p.refusal == want and p.ring_error == want, (ncomp, npar, p.refusal)
            lib.fused6(C.byref(s), C.byref(k), mode, 0, 0, 0, C.byref(p))
            assert p.refusal == (None if want == why else batch)


def test_the_new_entry_point_links_from_c(tmp_path):
    """include/nestfit_amd.h compiles as C99 and a C program that names nfa_specset_create_lte_mix links against the library."""
    from nestfit_amd.build import OUT, build
    build()
    src = tmp_path / 'use_mix.c'
    src.write_text('#include "nestfit_amd.h"\n'
                   'typedef int (*fn_t)(nfa_specset **, int, const int64_t *, const int32_t *, const int32_t *, const double *,\n'
                   '                    const double *, const double *, const double *, const double *, const double *, int,\n'
                   '                    const int32_t *, const int32_t *, const double *, const double *, const double *const *,\n'
                   '                    int64_t, const double *, const double *, const double *);\n'
                   'int main(void) { fn_t f = nfa_specset_create_lte_mix; return f == 0; }\n')
    exe = tmp_path / 'use_mix'
    res = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', f'-I{ROOT / "include"}', str(src), '-o', str(exe),
                          f'-L{OUT.parent}', '-lnestfit_amd', f'-Wl,-rpath,{OUT.parent}', '-Wl,--allow-shlib-undefined'],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ---------------------------------------------------------------------------- the cube driver and the store
def _priors5(na):
    from scipy import stats
    x = np.linspace(0, 1, 200)
    ranges = [(-4, 4), (3.0, 20), (12.0, 14.5), (0.2, 1.5), (11.0, 14.0)]
    return na.PriorTransformer([
        na.Prior(na.Distribution(lo + x * (hi - lo), stats.uniform(lo, hi - lo).pdf(lo + x * (hi - lo))), k)
        for k, (lo, hi) in enumerate(ranges)])


def _stub_backend(fitter, lon, lat, ncomp, nlive, kw):
    """A stand-in for the device: the numpy twin of the sampler on a Gaussian in the unit cube of the fitter's dimensions."""
    from nestfit_amd import sampler

    def loglike(pix, U):
        return -0.5 * np.sum((U - 0.5) ** 2, axis=1) / 0.2 ** 2
    res = sampler.run_nested(loglike, fitter.n_model * ncomp, lon.size, nlive=nlive, batch_target=64, **kw)
    return res, np.full(lon.size, -40.0), 2 * 64


def test_store_round_trip_of_a_mix(tmp_path):
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    from test_lte_bands_cpu import _stack
    mol, ks, iso, isos = mr.test_species(na)
    mix = na.LteMix([mol, iso])
    blend = na.LteBlend(ks + isos, name='J=5-4')
    stack = _stack(na, [blend, isos[1]])                    # a blended cube beside one of a single transition of species 1
    fitter = CubeFitter(stack, _priors5(na), mix.Runner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0, fit_backend=_stub_backend)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs, fitter.species) == (4, 5, {}, (mol, iso))
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        root = store.hdf.attrs
        assert root['model_name'] == 'lte_mix' and int(root['n_params']) == 5 and list(root['par_names']) == mix.PAR_NAMES
        assert list(root['par_names_short']) == mix.PAR_NAMES_SHORT and len(root['tex_labels']) == 5
        assert store.model.IX_VCEN == 0 and store.model.IX_SIGM == 3
        part = store.hdf['/model_partition']
        assert int(part.attrs['n_species']) == 2 and 'temp' not in part
        for k, m in enumerate((mol, iso)):
            g = part[f'species{k}']
            assert g.attrs['name'] == m.name and np.array_equal(np.asarray(g['temp'][...]), m.q_temp) and np.array_equal(np.asarray(g['q'][...]), m.q_val)
        g = store.hdf['/model_lines/spec0']
        assert int(g.attrs['n_trans']) == 7 and g.attrs['name'] == 'J=5-4'
        for j, t in enumerate(ks + isos):
            sub = g[f'trans{j}']
            assert (sub.attrs['nu'], sub.attrs['e_up'], sub.attrs['g_up'], sub.attrs['a_ul'], sub.attrs['name']) == (*_trans(t), t.name)
            assert int(sub.attrs['species']) == (0 if t.molecule is mol else 1)
            assert np.array_equal(np.asarray(sub['voff'][...]), t.voff) and np.array_equal(np.asarray(sub['tau_wts'][...]), t.tau_wts)
        assert int(store.hdf['/model_lines/spec1'].attrs['n_trans']) == 1 and int(store.hdf['/model_lines/spec1/trans0'].attrs['species']) == 1
        back, species = store.read_model_lines(with_species=True)
        assert species == (mol, iso) and store.read_model_species() == species
        assert back == [blend, na.LteBlend([isos[1]])] and all(isinstance(b, na.LteBlend) for b in back) and back[0].name == 'J=5-4'
    with HdfStore(path) as store:                                       # reopened
        assert pp.check_model_lines(store, stack) == [blend, isos[1]]
        # the species swapped: each ladder's numbers under the other molecule
        swapped = na.LteBlend([iso.transition(*_trans(t)) for t in ks] + [mol.transition(*_trans(t)) for t in isos])
        for tables in ([swapped, isos[1]], [blend, mol.transition(*_trans(isos[1]))], [na.LteBlend(isos + ks), isos[1]],
                       [na.LteBlend(ks + isos[:2]), isos[1]], [mol.band(ks), isos[1]], [blend, isos[0]], [blend]):
            other = _stack(na, tables)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.postprocess_run(store, other, predict_backend=lambda *a: None)


def test_a_store_of_one_species_is_written_as_before(tmp_path):
    """The same tree from LteRunner and from the Runner of a mix of that one species, the root's model name and nothing else apart."""
    import nestfit_amd as na
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    from test_lte_bands_cpu import _stack
    from test_lte_cpu import _priors
    mol, ks = top_species(na)
    stack = _stack(na, [mol.band(ks, name='J=5-4'), ks[2]])
    trees = []
    for name, cls in (('plain', na.LteRunner), ('mix', na.LteMix([mol]).Runner)):
        fitter = CubeFitter(stack, _priors(na), cls, lnZ_thresh=11, ncomp_max=1,
                            mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0, fit_backend=_stub_backend)
        assert fitter.n_model == 4
        path = str(tmp_path / name)
        fitter.fit_cube(path, nproc=1)
        with HdfStore(path) as store:
            tree = {}

            def walk(g, at):
                tree[at] = {k: np.asarray(v).tolist() for k, v in dict(g.attrs).items()}
                for key in list(g):
                    item = g[key]
                    if hasattr(item, 'attrs') and not hasattr(item, 'shape'):
                        walk(item, f'{at}/{key}')
                    else:
                        tree[f'{at}/{key}'] = np.asarray(item[...]).tolist()
            walk(store.hdf['/model_lines'], '/model_lines')
            walk(store.hdf['/model_partition'], '/model_partition')
            assert store.read_model_species() == () and store.read_model_lines() == [mol.band(ks), ks[2]]
            trees.append(tree)
    assert trees[0] == trees[1] and any('trans3' in k for k in trees[0])
