"""LTE bands without a GPU (nestfit_amd/lte.py: LteBand): the restatement the device tests compare with, the
host class, the ratio form the device computes tau_main of a band's transitions in, the store round trip, and the launch
plan's refusal of the fused kernels.  The test species is a symmetric top made from closed forms
(tests/band_restatement.py): K = 0..3 of J = 5 - 4 near 40 GHz, 2.5 K^2 km/s apart."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import band_restatement as br
import hf_restatement as hfr
import lte_restatement as lr
from test_launch_plan import FusedPlan, LpKnobs, LpShape, ROOT, knobs, shape
from test_lte_cpu import _priors, _stub_backend, rotor_species

# Hz, Hz, Hz, esu cm, and the lower J.  nu(K) - nu(0) = -2 (J + 1) D_JK K^2: 2.5, 10 and 22.5 km/s towards lower
# frequencies, so K = 0 and 1 blend at sigm > 1.25 km/s and K = 3 stands clear.  E_u = 5.8, 15.2, 43.4, 90.4 K.
A_ROT, B_ROT, D_JK, MU, J_LOW = 200e9, 4.0e9, 33.4e3, 3.9e-18, 4
N_CHAN = 300                       # four rows of 64 channels and one of 44
K0_VOFF, K0_WTS = [-1.4, 0.0, 3.6], [0.25, 0.55, 0.2]      # made up; the satellite at +3.6 km/s lies beyond K = 1's centre


def top_species(na, n_q=32, t_lo=5.0, t_hi=60.0, name='top'):
    """(molecule, [K = 0 with a made-up three-line structure, K = 1, K = 2, K = 3 as one line each])."""
    temps = np.geomspace(t_lo, t_hi, n_q)
    mol = na.Molecule(name, temps, br.top_partition(A_ROT, B_ROT, temps))
    ks = [mol.transition(*br.top_transition(A_ROT, B_ROT, D_JK, MU, J_LOW, K), name=f'K={K}',
                         **(dict(voff=K0_VOFF, tau_wts=K0_WTS) if K == 0 else {})) for K in range(4)]
    return mol, ks


def band_axis(nu0, n=N_CHAN, v_hi=36.0, v_lo=-14.0):
    """Ascending frequencies from v_hi to v_lo km/s about nu0: K = 0..3 at 0..22.5 km/s with room for +-6 km/s of voff."""
    return nu0 * (1.0 - np.linspace(v_hi, v_lo, n) / lr.CKMS)


def _trans(t):
    return t.nu, t.e_up, t.g_up, t.a_ul


def test_the_species_is_what_the_tests_need():
    import nestfit_amd as na
    mol, ks = top_species(na)
    v = [(1.0 - t.nu / ks[0].nu) * lr.CKMS for t in ks]                 # the K components' centres, km/s from K = 0
    assert v[1] == pytest.approx(2.5, abs=0.01) and v[2] == pytest.approx(10.0, abs=0.05) and v[3] == pytest.approx(22.5, abs=0.1)
    assert v[1] < 2 * 10 ** 0.2                                          # K = 0 and 1 blend at the largest sigm drawn
    assert v[3] - v[2] > 6 * 10 ** 0.2                                   # K = 3 stands clear
    assert max(K0_VOFF) > v[1]                                           # velocity rank != transition order
    x = band_axis(ks[0].nu)
    assert x.size % 64 != 0 and np.all(np.diff(x) > 0)
    for t in ks:
        assert x[0] < t.nu * (1 - 6.0 / lr.CKMS) and t.nu * (1 + 6.0 / lr.CKMS) < x[-1]
    e_low = [t.e_up - lr.H * t.nu / lr.KB for t in ks]
    assert e_low == sorted(e_low)                                        # K = 0 is the reference transition


def test_one_transition_bands_restate_the_lte_model_bit_for_bit(nfo):
    import nestfit_amd as na
    from test_lte import N_CHAN as N_LTE, _rows, draw_params
    mol, t10, t21, t32 = rotor_species(na)
    rng = np.random.default_rng(7)
    n = 0
    for ncomp, tables in ((1, (t10,)), (2, (t10, t21, t32)), (3, (t32, t10))):
        rows = _rows(tables, seed=ncomp)
        as_bands = [[x, d, s, mol.band([t])] for x, d, s, t in rows]
        tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]
        for k in range(70):
            theta = draw_params(rng, ncomp, mol, k)
            want_spec, want_lnl = lr.restated(nfo, rows, theta)
            for these in (as_bands, rows):                                # ... and an LteLines as it is
                spec, lnl = br.restated(nfo, these, theta, tbgs)
                assert np.array_equal(spec, want_spec) and lnl == want_lnl and spec.size == len(tables) * N_LTE
            n += 1
    assert n >= 200


def test_band_tau_main_equals_the_restatement():
    import nestfit_amd as na
    mol, ks = top_species(na)
    band = mol.band(ks)
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(200):
        tex, lncol, sigm = 10 ** rng.uniform(0.4, 1.9), rng.uniform(12, 15.5), 10 ** rng.uniform(-1.0, 0.2)
        got = band.tau_main(tex, lncol, sigm)
        assert got.shape == (4,)
        for g, t in zip(got, ks):
            want = lr.tau_main(_trans(t), mol.q_temp, mol.q_val, tex, lncol, sigm)
            worst = max(worst, abs(float(g) - want) / want)
    print(f'LteBand.tau_main: worst relative difference {worst:.2e}')
    assert worst < 1e-14
    grid = band.tau_main(np.array([8.0, 30.0])[:, None], 14.0, np.array([0.3, 0.6, 0.9])[None, :])
    assert grid.shape == (4, 2, 3) and np.array_equal(grid[2], ks[2].tau_main(np.array([8.0, 30.0])[:, None], 14.0, np.array([0.3, 0.6, 0.9])[None, :]))


# The ratio form against the direct formula.  The direct formula is the reference, so it must itself be exact where it is
# asked: its factor exp(-E_u / tex) and every partial product have to stay normal numbers down to a result below 1e-300.
# With a column of 10^13 cm^-2 they do not (exp(-E_u / tex) is denormal before the product falls to 1e-300), so the cold
# end is checked at a column of 10^8; the physical columns are checked over the range the device tests draw.
RATIO_TEX = np.concatenate([np.geomspace(0.128, 90.0, 64), np.geomspace(5.0, 60.0, 32)])


def test_the_ratio_form_agrees_with_the_direct_formula():
    import nestfit_amd as na
    mol, ks = top_species(na)
    ref = _trans(ks[0])
    worst, coldest = 0.0, np.inf
    for lncol, texs in ((8.0, RATIO_TEX), (13.0, RATIO_TEX[RATIO_TEX > 0.14]), (15.5, RATIO_TEX[RATIO_TEX > 2.8])):
        for tex in texs:
            tau0 = lr.tau_main(ref, mol.q_temp, mol.q_val, float(tex), lncol, 0.7)
            for t in ks[1:]:
                direct = lr.tau_main(_trans(t), mol.q_temp, mol.q_val, float(tex), lncol, 0.7)
                assert direct > 2.3e-308                                  # a normal number: the reference is exact here
                got = float(br.ratio_form(_trans(t), ref, tau0, tex))
                worst = max(worst, abs(got - direct) / direct)
                if t is ks[3]:
                    coldest = min(coldest, direct)
    print(f'ratio form: worst relative difference {worst:.2e}; smallest direct K = 3 value {coldest:.2e}')
    assert coldest < 1e-300
    assert worst < 1e-13
    # the reference transition itself: no arithmetic; and where the direct form underflows the ratio form gives 0, not NaN
    tau0 = lr.tau_main(ref, mol.q_temp, mol.q_val, 0.05, 13.0, 0.7)
    assert tau0 > 0 and lr.tau_main(_trans(ks[2]), mol.q_temp, mol.q_val, 0.05, 13.0, 0.7) == 0.0
    with np.errstate(under='ignore'):
        assert float(br.ratio_form(_trans(ks[2]), ref, tau0, 0.05)) == 0.0
        assert np.isnan(br.ratio_form(_trans(ks[2]), ref, np.nan, 10.0))


def test_every_value_error():
    import nestfit_amd as na
    mol, ks = top_species(na)
    assert mol.band(ks).n_lines == 6 and mol.band(ks[:1]).n_trans == 1 and len(mol.band(tuple(ks))) == 4
    for bad in ([], ks + ks, [ks[0], 'x'], [na.LineTable(1e11, [0.0], [1.0])], 5):
        with pytest.raises(ValueError):
            mol.band(bad)
    nine = [mol.transition(4e10 + 1e6 * k, 10.0 + k, 3.0, 1e-6) for k in range(9)]
    assert mol.band(nine[:8]).n_trans == 8
    with pytest.raises(ValueError, match='1..8 transitions'):
        mol.band(nine)
    with pytest.raises(ValueError, match='twice'):
        mol.band([ks[0], ks[1], mol.transition(*_trans(ks[0]))])         # other lines, the same transition
    many = [mol.transition(4e10 + 1e6 * k, 10.0 + k, 3.0, 1e-6, voff=np.arange(17.0), tau_wts=np.full(17, 1 / 17)) for k in range(3)]
    assert mol.band(many[:2]).n_lines == 34
    with pytest.raises(ValueError, match='at most 50 lines'):
        mol.band(many)
    other = na.Molecule('other', mol.q_temp, mol.q_val * 1.01)
    with pytest.raises(ValueError, match='one Molecule'):
        mol.band([ks[0], other.transition(*_trans(ks[1]))])
    with pytest.raises(ValueError, match='Molecule'):
        na.LteBand('top', ks)
    # a runner's rows: bands and transitions of one molecule, checked before any device call
    x = band_axis(ks[0].nu, 64)
    rows = [[x, np.zeros(64), 0.1, mol.band(ks)], [x, np.zeros(64), 0.1, other.transition(*_trans(ks[1]))]]
    with pytest.raises(ValueError, match='one Molecule'):
        na.LteRunner.from_data(rows, None)
    with pytest.raises(ValueError, match='one Molecule'):
        na.lte.check_one_molecule([mol.band(ks), other.band([other.transition(*_trans(ks[1]))])])
    assert na.lte.check_one_molecule([mol.band(ks), ks[1]]) == mol
    with pytest.raises(ValueError, match='LteLines'):
        na.LteRunner.from_data([[x, np.zeros(64), 0.1, na.LineTable(1e11, [0.0], [1.0])]], None)
    with pytest.raises(ValueError, match='baseline_order'):
        na.LteRunner.from_data(rows[:1], None, baseline_order=7)
    from nestfit_amd.cubeio import DataCube
    with pytest.raises(ValueError):
        DataCube(None, 0.1, trans_id=1, lines=mol.band(ks))


def test_immutable_and_compared_by_value():
    import nestfit_amd as na
    mol, ks = top_species(na)
    again, ls = top_species(na)
    a, b = mol.band(ks, name='ladder'), again.band(ls)
    assert a == b and hash(a) == hash(b) and a is not b and len({a, b}) == 1            # the name is a label
    assert a.transitions == tuple(ks) and list(a) == ks and a[1] == ks[1] and a.molecule is mol and a.name == 'ladder'
    assert (a.n_trans, a.n_lines, a.n, a.nu) == (4, 6, 6, ks[0].nu)
    assert mol.band(ks[::-1]) != a and mol.band(ks[::-1]).nu == ks[3].nu                # the caller's order is kept
    assert mol.band(ks[:3]) != a and mol.band(ks[:1]) != ks[0] and ks[0] != mol.band(ks[:1])
    assert isinstance(a, na.LteBand) and na.LteBand is na.lte.LteBand and 'LteBand' in na.__all__
    for key in ('name', '_transitions', 'nu', 'other'):
        with pytest.raises(AttributeError):
            setattr(a, key, 1.0)
    with pytest.raises(AttributeError):
        del a._name
    with pytest.raises(TypeError):
        a.transitions[0] = ks[1]
    from nestfit_amd import _ffi
    assert 'nfa_specset_create_lte_bands' in _ffi.SIGNATURES and hasattr(_ffi.load(), 'nfa_specset_create_lte_bands')


# ---------------------------------------------------------------------------- the cube driver and the store
def _stack(na, tables, n=3, n_chan=64, seed=0):
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    rng = np.random.default_rng(seed)
    cubes = []
    for t in tables:
        x = band_axis(t.nu, n_chan)
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n, 'NAXIS2': n, 'NAXIS3': n_chan,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': t.nu}
        cubes.append(DataCube(SimpleCube(hdr, rng.normal(0, 0.1, (n_chan, n, n))), 0.1, lines=t))
    return CubeStack(cubes)


def test_store_round_trip_of_the_bands(tmp_path):
    import nestfit_amd as na
    from nestfit_amd import postprocess as pp
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    mol, ks = top_species(na)
    band = mol.band(ks, name='J=5-4')
    stack = _stack(na, [band, ks[2]])                      # a banded cube beside one of a single transition
    fitter = CubeFitter(stack, _priors(na), na.LteRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0, fit_backend=_stub_backend)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (4, 4, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'lte' and '/model_partition' in store.hdf
        g = store.hdf['/model_lines/spec0']
        assert int(g.attrs['n_trans']) == 4 and g.attrs['name'] == 'J=5-4' and 'voff' not in g
        for j, t in enumerate(ks):
            sub = g[f'trans{j}']
            assert (sub.attrs['nu'], sub.attrs['e_up'], sub.attrs['g_up'], sub.attrs['a_ul'], sub.attrs['name']) == (*_trans(t), t.name)
            assert np.array_equal(np.asarray(sub['voff'][...]), t.voff) and np.array_equal(np.asarray(sub['tau_wts'][...]), t.tau_wts)
        single = store.hdf['/model_lines/spec1']                        # one transition: written as it always was
        assert 'n_trans' not in single.attrs and single.attrs['nu'] == ks[2].nu and 'trans0' not in single
        back = store.read_model_lines()
        assert back == [band, ks[2]] and isinstance(back[0], na.LteBand) and isinstance(back[1], na.LteLines)
        assert back[0].name == 'J=5-4' and [t.name for t in back[0]] == [t.name for t in ks]
    with HdfStore(path) as store:                                       # reopened
        assert pp.check_model_lines(store, stack) == [band, ks[2]]
        hotter = mol.transition(ks[3].nu, ks[3].e_up * 1.01, ks[3].g_up, ks[3].a_ul)
        for tables in ([mol.band(ks[:3]), ks[2]], [mol.band(ks[:3] + [hotter]), ks[2]], [mol.band(ks[::-1]), ks[2]],
                       [ks[0], ks[2]], [band, mol.band([ks[2]])], [band]):
            other = _stack(na, tables)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.postprocess_run(store, other, predict_backend=lambda *a: None)


# ---------------------------------------------------------------------------- the launch plan
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
void fused5(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, FusedPlan *out) { *out = plan_fused(*s, *k, mode, bl != 0, wt != 0); }
void fused6(const LpShape *s, const LpKnobs *k, int mode, int bl, int wt, int banded, FusedPlan *out) {
    *out = plan_fused(*s, *k, mode, bl != 0, wt != 0, banded != 0);
}
int fused_size() { return (int)sizeof(FusedPlan); }
}
'''


def test_the_fused_kernels_refuse_banded_sets(tmp_path):
    src, so = tmp_path / 'plan.cpp', tmp_path / 'libplan.so'
    src.write_text(SHIM)
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    assert lib.fused_size() == C.sizeof(FusedPlan)
    fields = [f for f, _ in FusedPlan._fields_ if f != 'G'] + ['G.nhf_max', 'G.wave_doubles', 'G.inv_nspec', 'G.inv_nhf', 'G.split']

    def plan(s, mode, bl=0, wt=0, banded=None):
        p, k = FusedPlan(), knobs()
        if banded is None:
            lib.fused5(C.byref(s), C.byref(k), mode, bl, wt, C.byref(p))
        else:
            lib.fused6(C.byref(s), C.byref(k), mode, bl, wt, banded, C.byref(p))
        out = []
        for f in fields:
            v = p
            for part in f.split('.'):
                v = getattr(v, part)
            out.append(v)
        return out
    why = b'the resident kernel has no form for LTE bands: use nfa_ring_serve'
    shapes = [shape(), shape(n_spec=1, ncomp=1, nhf_max=6, model=4, ndim=4, n_stage=4, stage_doubles=800),
              shape(n_spec=3, ncomp=4, lnl_split=2), shape(ncomp=5), shape(nhf_max=40), shape(lnl_split=16),
              shape(n_spec=16, ncomp=4, nhf_max=26, lnl_split=1), shape(ncomp=4, stage_doubles=9000)]
    for s in shapes:
        for mode in (0, 2):
            for bl, wt in ((0, 0), (0, 1), (1, 1)):
                five = plan(s, mode, bl, wt)
                assert plan(s, mode, bl, wt, banded=0) == five            # the five-argument call: banded = false
                six = plan(s, mode, bl, wt, banded=1)
                if five[0] is None or five[0] == b"spectra too short for the point kernel's split":
                    assert six[0] == why and six[1] == why                # what a set is comes before how its launch splits
                else:                                                     # the neighbours' reasons come first
                    assert six[:2] == five[:2]
