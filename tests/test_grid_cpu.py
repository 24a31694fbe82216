"""The excitation-grid model without a GPU (nestfit_amd/excitation.py): `ExcitationGrid.interpolate` and
`GridLines.excitation` against tests/grid_restatement.py, the thermal limit against `LteLines.tau_main`, `covers`, every
ValueError, equality and hashes, the host-side refusals of `_options.check_options(model=5)`, and the plan header's new side,
flags, form and record sizes compiled with the host compiler as tests/test_launch_plan.py does."""
import ctypes as C
import itertools
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import grid_restatement as gr
import lte_restatement as lr
from test_lte_cpu import rotor_species

ROOT = Path(__file__).resolve().parent.parent
ALL_AXES = (gr.AXES_111, gr.AXES_222, gr.AXES_546)


def _coordinates(axes, rng, n=40):
    """Coordinates on the nodes, between them, and below and above every axis."""
    per_axis = []
    for a in axes:
        lo, hi = a[0], a[-1]
        span = max(hi - lo, 1.0)
        per_axis.append(list(a) + [lo - 0.3 * span, hi + 0.4 * span] + list(rng.uniform(lo - 0.2 * span, hi + 0.2 * span, n)))
    pts = [tuple(rng.choice(p) for p in per_axis) for _ in range(6 * n)]
    pts += list(itertools.product(*[[a[0], a[-1], a[0] - 1.0, a[-1] + 1.0] for a in axes]))
    return pts


@pytest.mark.parametrize('axes', ALL_AXES, ids=['1x1x1', '2x2x2', '5x4x6'])
def test_interpolate_and_excitation_equal_the_restatement(axes):
    import nestfit_amd as na
    from nestfit_amd import excitation
    assert excitation.FWHM == gr.FWHM == 2.3548200450309493
    rng = np.random.default_rng(11)
    grid, t10, t21, t32 = gr.rotor_grid(na, axes)
    assert grid.shape == tuple(len(a) for a in axes)
    worst = 0.0
    pts = _coordinates(axes, rng)
    for t in (t10, t21, t32):
        for x in pts:
            for table in (t.tex, t.ltau):
                want = gr.interpolate(axes, table, x)
                got = grid.interpolate(table, *x)
                worst = max(worst, abs(got - want) / abs(want))
        # the whole batch at once: broadcasting
        arr = np.array(pts)
        got = grid.interpolate(t.tex, arr[:, 0], arr[:, 1], arr[:, 2])
        assert got.shape == (len(pts),) and got[3] == grid.interpolate(t.tex, *pts[3])
        # excitation: the third coordinate from lncol and sigm
        for x in pts[:60]:
            sigm = 10 ** rng.uniform(-1.0, 0.3)
            lncol = x[2] + math.log10(gr.FWHM * sigm)
            want_tex, want_ltau = gr.excitation(axes, t.tex, t.ltau, x[0], x[1], lncol, sigm)
            tex, tau = t.excitation(x[0], x[1], lncol, sigm)
            worst = max(worst, abs(tex - want_tex) / want_tex, abs(tau - 10.0 ** want_ltau) / 10.0 ** want_ltau)
    print(f'{grid.shape}: worst relative difference {worst:.2e}')
    assert worst < 1e-14
    # clamped: beyond the grid the edge value holds
    lo = tuple(a[0] for a in axes)
    assert grid.interpolate(t10.tex, lo[0] - 5.0, lo[1] - 2.0, lo[2] - 3.0) == t10.tex[0, 0, 0]
    # (f = 1 there, and v0 + 1 (v1 - v0) is v1 to a rounding, not to the bit)
    assert grid.interpolate(t10.ltau, axes[0][-1] + 50.0, axes[1][-1] + 2.0, axes[2][-1] + 3.0) == pytest.approx(t10.ltau[-1, -1, -1], rel=1e-15)
    # what is not finite, and a sigm that is no ordinary positive number: NaN, as the restatement has it
    with np.errstate(all='ignore'):
        for bad in ((np.nan, 3.0, 13.0, 0.5), (20.0, np.inf, 13.0, 0.5), (20.0, 3.0, -np.inf, 0.5), (20.0, 3.0, 13.0, 0.0),
                    (20.0, 3.0, 13.0, -1.0), (20.0, 3.0, 13.0, np.nan), (20.0, 3.0, 13.0, np.inf)):
            got, want = t10.excitation(*bad), gr.excitation(axes, t10.tex, t10.ltau, *bad)
            assert np.isnan(got[1]) and math.isnan(want[1]), bad
            # tex is the rule in IEEE arithmetic: an infinite coordinate clamps to the edge, a NaN one gives NaN (one node: no effect)
            assert got[0] == want[0] or (math.isnan(got[0]) and math.isnan(want[0])), (bad, got[0], want[0])
            assert math.isnan(want[0]) == any(math.isnan(v) and len(a) > 1 for v, a in
                                              zip((bad[0], bad[1], bad[2] - gr._log10(gr.FWHM * bad[3])), axes)), bad
    out = t21.excitation(np.array([10.0, 30.0])[:, None], 3.0, 13.0, np.array([0.3, 0.6, 0.9])[None, :])
    assert out[0].shape == out[1].shape == (2, 3)


def test_the_spectra_of_the_test_grids_differ_in_tex():
    """The closed-form grids give 1-0 and 3-2 excitation temperatures a factor 1.5 and more apart, everywhere, the clamped
    outside included, and every tex lies above the background."""
    import nestfit_amd as na
    for axes in ALL_AXES:
        _, t10, t21, t32 = gr.rotor_grid(na, axes)
        assert (t10.tex / t32.tex).min() > 1.5 and (t10.tex > t21.tex).all() and (t21.tex > t32.tex).all()
        assert min(t.tex.min() for t in (t10, t21, t32)) > 2.9
        rng = np.random.default_rng(3)
        for _ in range(50):
            theta = np.array([0.0, rng.uniform(5, 70), rng.uniform(4.0, 6.0), rng.uniform(11, 15), 10 ** rng.uniform(-1, 0.2)])
            assert gr.tex_spread((t10, t32), theta) > 1.5 and gr.tex_spread((t10, t21, t32), theta) > 1.5


def test_the_thermal_limit_is_the_lte_model():
    """A grid whose tex table equals tkin (n -> infinity): at its nodes `excitation` is `LteLines.tau_main`."""
    import nestfit_amd as na
    mol, l10, l21, l32 = rotor_species(na)
    _, t10, t21, t32 = gr.rotor_grid(na, thermal=True)
    worst = 0.0
    for g, l in ((t10, l10), (t21, l21), (t32, l32)):
        assert g.nu == l.nu
        for tk, nd, cd in itertools.product(*gr.AXES_546):
            for sigm in (0.2, 1.0 / gr.FWHM, 1.3):
                lncol = cd + math.log10(gr.FWHM * sigm)
                tex, tau = g.excitation(tk, nd, lncol, sigm)
                want = float(l.tau_main(tk, lncol, sigm))
                assert tex == tk
                worst = max(worst, abs(tau - want) / want)
    print(f'thermal limit: worst relative difference of tau_main {worst:.2e}')
    assert worst < 1e-12


def test_covers():
    import nestfit_amd as na
    grid = na.ExcitationGrid(*gr.AXES_546)
    lg = math.log10(gr.FWHM)

    def box(tk=(10, 50), nd=(4.8, 5.4), col=(12.5, 13.5), sg=(0.5, 1.0), ncomp=1):
        lo = np.repeat([-5.0, tk[0], nd[0], col[0], sg[0]], ncomp)
        hi = np.repeat([5.0, tk[1], nd[1], col[1], sg[1]], ncomp)
        return lo, hi
    assert grid.covers(*box()) and grid.covers(*box(ncomp=3))
    assert grid.covers(*box(tk=(9.0, 60.0), nd=(4.7, 5.5)))                                  # touching
    assert not grid.covers(*box(tk=(8.9, 50))) and not grid.covers(*box(tk=(10, 60.1)))
    assert not grid.covers(*box(nd=(4.6, 5.4))) and not grid.covers(*box(nd=(4.8, 5.6)))
    # the sigm-dependent corners: lncd = lncol - log10(FWHM sigm)
    assert grid.covers(*box(col=(11.5 + lg, 14.5 + lg), sg=(1.0, 1.0)))                      # touching both ends
    assert not grid.covers(*box(col=(11.5 + lg, 13.0), sg=(1.0, 1.1)))                       # the wide line falls below
    assert not grid.covers(*box(col=(12.0, 14.5 + lg), sg=(0.9, 1.0)))                       # the narrow one above
    assert not grid.covers(*box(sg=(0.0, 1.0))) and not grid.covers(*box(tk=(np.nan, 50)))
    # an axis of one node has no effect
    one = na.ExcitationGrid([20.0], gr.AXES_546[1], [13.0])
    assert one.covers(*box(tk=(1, 500), col=(5, 25))) and not one.covers(*box(nd=(4.0, 5.0)))
    with pytest.raises(ValueError, match='5 values per component'):
        grid.covers(np.zeros((5, 0)), np.zeros((5, 0)))


def test_every_value_error_equality_and_hashes():
    import nestfit_amd as na
    from nestfit_amd.excitation import GridSpectrum, check_one_grid
    G = na.ExcitationGrid
    for bad, word in (((np.zeros(0), [1.0], [1.0]), '1..64'), ((np.arange(65.0), [1.0], [1.0]), '1..64'),
                      (([1.0, 1.0], [1.0], [1.0]), 'ascending'), (([2.0, 1.0], [1.0], [1.0]), 'ascending'),
                      (([1.0], [1.0, np.nan], [1.0]), 'ascending'), (([1.0], [1.0], [1.0, np.inf]), 'ascending'),
                      (([[1.0, 2.0]], [1.0], [1.0]), 'one-dimensional'), ((['a'], [1.0], [1.0]), 'numbers'),
                      ((np.arange(64.0), np.arange(64.0), np.arange(17.0)), '65536')):
        with pytest.raises(ValueError, match=word):
            G(*bad)
    assert G(np.arange(64.0), np.arange(64.0), np.arange(16.0)).shape == (64, 64, 16)
    grid, t10, t21, _ = gr.rotor_grid(na, gr.AXES_222)
    tex, ltau = np.array(t21.tex), np.array(t21.ltau)
    for kw, word in ((dict(tex=tex[:1]), 'shape'), (dict(ltau=ltau[:, :1]), 'shape'), (dict(tex=-tex), 'populations invert'),
                     (dict(tex=np.where(tex == tex[0, 0, 0], 0.0, tex)), 'populations invert'),
                     (dict(tex=np.where(tex == tex[0, 0, 0], np.nan, tex)), 'populations invert'),
                     (dict(ltau=np.where(ltau == ltau[1, 1, 1], np.inf, ltau)), 'cut the grid'),
                     (dict(tau_wts=[0.5, 0.4], voff=[0.0, 1.0]), 'sum to 1'), (dict(nu=-1.0), 'rest frequency'),
                     (dict(voff=[np.nan]), 'velocity offset')):
        with pytest.raises(ValueError, match=word):
            grid.transition(**{**dict(nu=t21.nu, tex=tex, ltau=ltau), **kw})
    with pytest.raises(ValueError, match='ExcitationGrid'):
        na.GridLines('grid', t21.nu, tex, ltau)
    assert grid.transition(t21.nu, tex, ltau, voff=[0.0, 1.0], tau_wts=[2.0, 6.0], normalise=True).tau_wts.tolist() == [0.25, 0.75]
    # immutable, compared by value, the names labels
    same = na.ExcitationGrid(*gr.AXES_222, name='another name')
    assert same == grid and hash(same) == hash(grid) and grid != na.ExcitationGrid(*gr.AXES_546) and grid != 'grid'
    twin = same.transition(t21.nu, tex, ltau, name='twin')
    assert twin == t21 and hash(twin) == hash(t21) and twin != t10
    assert twin != grid.transition(t21.nu, tex * 1.01, ltau) and twin != grid.transition(t21.nu, tex, ltau + 0.1)
    assert twin != na.LineTable(t21.nu, [0.0], [1.0]) and na.LineTable(t21.nu, [0.0], [1.0]) != twin
    for obj, key in ((grid, 'tkin'), (t21, 'tex'), (t21, 'nu')):
        with pytest.raises(AttributeError, match='immutable'):
            setattr(obj, key, 1.0)
    with pytest.raises(ValueError):
        t21.tex[0, 0, 0] = 1.0
    # the rows of a runner name one grid
    other, o10, *_ = gr.rotor_grid(na, gr.AXES_546)
    assert check_one_grid([t10, t21]) == grid
    with pytest.raises(ValueError, match='share one ExcitationGrid'):
        check_one_grid([t10, o10])
    with pytest.raises(ValueError, match='one GridLines'):
        check_one_grid([t10, na.LineTable(t21.nu, [0.0], [1.0])])
    x = lr.axis(t10.nu, 32, 20.0)
    with pytest.raises(ValueError, match='share one ExcitationGrid'):
        na.GridRunner.from_data([[x, np.zeros(32), 0.1, t10], [x, np.zeros(32), 0.1, o10]], None)
    with pytest.raises(ValueError, match='GridLines'):
        GridSpectrum(x, np.zeros(32), 0.1, na.LineTable(t21.nu, [0.0], [1.0]))
    # the module's metadata
    mod = na.model_module('grid')
    assert mod is na.excitation and (mod.NAME, mod.N, mod.IX_VCEN, mod.IX_SIGM) == ('grid', 5, 0, 4)
    assert mod.PAR_NAMES == ['voff', 'tkin', 'lnden', 'lncol', 'sigm'] and len(mod.get_par_names(2)) == 10
    assert len(mod.TEX_LABELS) == len(mod.TEX_LABELS_WITH_UNITS) == len(mod.PAR_NAMES_SHORT) == 5
    assert sorted(na.MODELS) == ['ammonia', 'diazenylium', 'gaussian']


REFUSED = {'calibration': 0.1, 'correlation': (0.5, 0.25), 'response': (0.25, 0.5, 0.25), 'templates': [np.ones((1, 32))],
           'continuum': 2.0, 'robust': 4.0}
WORDS = {'calibration': 'calibration uncertainty', 'correlation': 'noise correlation', 'response': 'channel response',
         'templates': 'nuisance templates', 'continuum': 'continuum background', 'robust': 'robust likelihood'}


def test_check_options_refuses_the_six_on_the_host():
    from nestfit_amd._options import check_options
    for name, value in REFUSED.items():
        with pytest.raises(ValueError, match='a set of the excitation-grid model takes no ' + WORDS[name]):
            check_options({name: value}, 1, [32], model=5)
        with pytest.raises(ValueError, match='a set of the excitation-grid model takes no ' + WORDS[name]):
            check_options({'baseline_order': 1, 'layered': True, 'noise_uncertainty': 0.1, name: value}, 1, [32], model=5)
        assert getattr(check_options({name: value}, 1, [32], model=3), name) is not None       # the other models take them
        assert getattr(check_options({name: None}, 1, [32], model=5), name) is None            # off is off
    ok = check_options({'baseline_order': 3, 'layered': True, 'noise_uncertainty': 0.2}, 2, [32, 32], masked=True, model=5)
    assert (ok.baseline_order, ok.layered) == (3, True) and ok.noise_uncertainty.tolist() == [0.2, 0.2]


# ---------------------------------------------------------------------------- the plan header
SHIM = r'''
#include "nfa_launch_plan.h"
extern "C" {
unsigned side_flags(int side) { return lnl_side_flags((LnlSide)side); }
int side_form(int side) { return lnl_side_form((LnlSide)side); }
int side_of(int corr, int resp, int tmpl, int cont, int rob, int texs) { return lnl_side_of(corr != 0, resp != 0, tmpl != 0, cont != 0, rob != 0, texs != 0); }
int constants(int i) { const int c[] = {LNL_SIDES, LNL_SIDE_INSTANCES, LNL_SIDE_TEXS, (int)LNL_F_TEXS, NFA_MODEL_GRID, NFA_GRID_PARAMS, NFA_GRID_MAXN, NFA_GRID_MAXCELLS}; return c[i]; }
int drec(int ncomp, int nspec, int texs) { return texs < 0 ? lnl_drec_doubles(ncomp, nspec) : lnl_drec_doubles(ncomp, nspec, texs != 0); }
static LpShape shape(int n_spec, int size, int nhf_max, int ncomp) {
    LpShape s = {};
    s.n_spec = n_spec; s.nhf_max = nhf_max; s.ncomp = ncomp; s.ndim = 5 * ncomp; s.model = NFA_MODEL_GRID; s.wpb = 1;
    for (int q = 0; q < n_spec; ++q) s.size[q] = size;
    s.prog_bytes = 3624; s.line_rec_bytes = 32;
    return s;
}
// {error, form, wide, split, waves, lds, blocks} of the likelihood plan of B items; texs: as the excitation side, else as a
// set with a baseline
void lnl(int n_spec, int size, int nhf_max, int ncomp, long long B, int mode, int write_spec, int layered, int texs, long long *out) {
    const LpShape s = shape(n_spec, size, nhf_max, ncomp);
    LpKnobs k = {}; k.n_cu = 256; k.lnl_queue = 1; k.coalesce = 8;
    LpLaunch L = {}; L.B = B; L.mode = mode; L.group_n = 1; L.group_each = B; L.write_spec = write_spec != 0; L.has_queue = true;
    L.layered = layered != 0; L.baseline = true; L.weighted = true;
    const LnlPlan P = texs ? plan_lnl(s, k, L, false, true) : plan_lnl(s, k, L);
    out[0] = P.error != nullptr; out[1] = P.form; out[2] = P.wide; out[3] = P.G.split; out[4] = P.waves; out[5] = (long long)P.lds; out[6] = P.blocks;
}
// the form of a texs plan whatever the launch says of weights and baseline
int lnl_form_bare(int mode) {
    const LpShape s = shape(2, 1024, 3, 2);
    LpKnobs k = {}; k.n_cu = 256; k.lnl_queue = 1; k.coalesce = 8;
    LpLaunch L = {}; L.B = 4096; L.mode = mode; L.group_n = 1; L.group_each = 4096; L.has_queue = true;
    return plan_lnl(s, k, L, false, true).form;
}
const char *fused(int mode, int texs, int robust) {
    const LpShape s = shape(2, 1024, 3, 2);
    LpKnobs k = {}; k.n_cu = 256;
    return plan_fused(s, k, mode, true, true, false, false, false, false, false, false, false, false, robust != 0, texs != 0).refusal;
}
}
'''
NONE, CORR, RESP, TMPL, CONT, ROBUST, TEXS = range(7)
K_WEIGHTED, K_BASELINE, F_TEXS = 1, 2, 1024
BASELINE_FORM = 4


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('grid_plan')
    src = tmp / 'plan.cpp'
    src.write_text(SHIM)
    so = tmp / 'libplan.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    lib.fused.restype = C.c_char_p
    lib.lnl.argtypes = [C.c_int] * 4 + [C.c_longlong] + [C.c_int] * 4 + [C.c_void_p]
    return lib


def test_the_plan_headers_sixth_side(plan):
    assert [plan.constants(i) for i in range(8)] == [6, 32, TEXS, F_TEXS, 5, 5, 64, 65536]
    assert plan.side_flags(TEXS) == K_WEIGHTED | K_BASELINE | F_TEXS and plan.side_form(TEXS) == BASELINE_FORM
    assert plan.side_flags(CONT) == K_WEIGHTED | K_BASELINE | 256                             # the side it is modelled on
    for bits in itertools.product((0, 1), repeat=5):
        assert plan.side_of(*bits, 1) == TEXS                                                  # first of all
    assert plan.side_of(0, 0, 0, 0, 0, 0) == NONE and plan.side_of(0, 0, 0, 0, 1, 0) == ROBUST
    # the larger record: four leading doubles per (component, spectrum) in place of per component
    for ncomp, nspec in itertools.product((1, 2, 4, 10), (1, 2, 3, 16)):
        assert plan.drec(ncomp, nspec, -1) == plan.drec(ncomp, nspec, 0) == 4 * ncomp + 16 * ncomp * nspec
        assert plan.drec(ncomp, nspec, 1) == 4 * ncomp * nspec + 16 * ncomp * nspec
    # the plan: the baseline form's, slot for slot (the records are in global memory), and that form whatever the launch says
    out_t, out_b = (C.c_longlong * 7)(), (C.c_longlong * 7)()
    for n_spec, size, nhf, ncomp, B, mode, ws, layered in itertools.product((1, 3), (160, 1024), (3, 30), (1, 4), (1, 200, 4096),
                                                                             (0, 2), (0, 1), (0, 1)):
        plan.lnl(n_spec, size, nhf, ncomp, B, mode, ws, layered, 1, out_t)
        plan.lnl(n_spec, size, nhf, ncomp, B, mode, ws, layered, 0, out_b)
        assert list(out_t) == list(out_b) and out_t[0] == 0 and out_t[1] == BASELINE_FORM and out_t[5] <= 160 * 1024
        assert out_t[2] == (nhf > 26)
    assert plan.lnl_form_bare(0) == plan.lnl_form_bare(2) == BASELINE_FORM
    # the fused kernels refuse, and before everything else
    sentence = b'the resident kernel has no form for an excitation per spectrum: use nfa_ring_serve'
    assert plan.fused(0, 1, 0) == plan.fused(2, 1, 0) == plan.fused(2, 1, 1) == sentence
    assert plan.fused(2, 0, 1) == b'the resident kernel has no form for a robust likelihood: use nfa_ring_serve'


DECL_SHIM = r'''
#include "nfa_set_decl.h"
#include <cstdio>
// the plan of a grid declaration of n_spec spectra of 64 channels, one table of n_lines[s] lines each at offsets 0, 1, ...
extern "C" int grid_plan(int n_spec, const int *n_lines, const double *wts, int nt, int nn, int nc, const double *tkin, const double *lnden,
                         const double *lncd, const double *tex, const double *ltau, char *msg, int len, double *out) {
    static double x[64];
    for (int j = 0; j < 64; ++j) x[j] = 1e11 + 1e5 * j;
    const double *xs[MAXSPEC];
    int64_t sizes[MAXSPEC];
    double rest[MAXSPEC], noise[MAXSPEC], voff[MAXSPEC * NFA_MAX_HF_N];
    std::vector<double> data((size_t)64 * n_spec, 0.0);
    int32_t nl[MAXSPEC];
    for (int s = 0; s < n_spec; ++s) { xs[s] = x; sizes[s] = 64; rest[s] = 1e11; noise[s] = 0.1; nl[s] = n_lines[s]; }
    for (int i = 0; i < MAXSPEC * NFA_MAX_HF_N; ++i) voff[i] = (double)(i % NFA_MAX_HF_N);
    int out_handle = 0;
    SetDecl d{DECL_LINES, &out_handle, NFA_MODEL_GRID, n_spec, sizes, xs, 1, data.data(), noise, nullptr, rest, nullptr, nl, voff, wts};
    d.grid = true; d.g_nt = nt; d.g_nn = nn; d.g_nc = nc; d.g_tkin = tkin; d.g_lnden = lnden; d.g_lncd = lncd; d.g_tex = tex; d.g_ltau = ltau;
    SetPlan p; std::string why;
    const int rc = set_plan(d, p, why);
    snprintf(msg, len, "%s", why.c_str());
    out[0] = p.model; out[1] = p.npar; out[2] = p.grid; out[3] = p.kind; out[4] = p.grid_rec.nt; out[5] = p.grid_rec.nn; out[6] = p.grid_rec.nc;
    out[7] = p.grid_rec.tkin[nt > 0 && nt <= 64 ? nt - 1 : 0]; out[8] = p.grid_rec.lncd[0]; out[9] = sizeof(GridRec);
    return rc;
}
extern "C" int layout(int grid_on, int chan_noise, int bl_order, unsigned *out) {
    SetOptions o; o.grid_on = grid_on != 0; o.bl_order = bl_order;
    const SetLayout L = set_layout(o, chan_noise != 0);
    out[0] = L.bufs; out[1] = L.ones; out[2] = L.chan_w; out[3] = set_stages_create(L);
    return 0;
}
'''


def test_the_declaration_of_a_grid_set_and_its_refusals(tmp_path):
    """set_plan (nfa_set_decl.h, nfa_grid_decl.h) on grid declarations, compiled with the host compiler: the plan of a good one,
    and a sentence for each of a count outside 1..64, a product above 65536, an axis that is not finite and strictly ascending,
    a tex that is not finite and positive, an ltau that is not finite and weights that do not sum to 1 -- in that order behind
    the lines creator's own checks.  And what such a set asks of the device from its creation on (nfa_set_state.h)."""
    src = tmp_path / 'decl.cpp'
    src.write_text('#include "nfa_set_state.h"\n' + DECL_SHIM)
    so = tmp_path / 'libdecl.so'
    res = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-O1', '-shared', '-fPIC', f'-I{ROOT / "nestfit_amd" / "csrc"}',
                          str(src), '-o', str(so)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lib = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)

    lib.grid_plan.argtypes = [C.c_int, C.POINTER(C.c_int), dp, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, C.c_char_p, C.c_int, dp]

    def plan(n_lines=(1, 2), wts=(1.0, 0.25, 0.75), tkin=(10.0, 20.0), lnden=(3.0, 4.0, 5.0), lncd=(13.0,), tex=None, ltau=None, n_axes=None):
        n_lines = np.asarray(n_lines, dtype=np.int32)
        wts, tkin, lnden, lncd = (np.ascontiguousarray(a, dtype=np.float64) for a in (wts, tkin, lnden, lncd))
        nt, nn, nc = n_axes or (tkin.size, lnden.size, lncd.size)
        cells = nt * nn * nc * n_lines.size if 0 < nt * nn * nc <= 1 << 20 else n_lines.size
        tex = np.ascontiguousarray(np.full(cells, 8.0) if tex is None else tex, dtype=np.float64)
        ltau = np.ascontiguousarray(np.zeros(cells) if ltau is None else ltau, dtype=np.float64)
        msg, out = C.create_string_buffer(400), np.zeros(10)
        rc = lib.grid_plan(n_lines.size, n_lines.ctypes.data_as(C.POINTER(C.c_int)), wts.ctypes.data_as(dp), nt, nn, nc, tkin.ctypes.data_as(dp),
                           lnden.ctypes.data_as(dp), lncd.ctypes.data_as(dp), tex.ctypes.data_as(dp), ltau.ctypes.data_as(dp), msg, 400,
                           out.ctypes.data_as(dp))
        return rc, msg.value.decode(), out
    rc, msg, out = plan()
    assert (rc, msg) == (0, '') and out.tolist() == [5, 5, 1, 1, 2, 3, 1, 20.0, 13.0, 1568]       # model 5, npar 5, a SET_LINES set
    assert plan(tkin=(10.0,), lnden=(3.0,), lncd=(13.0,))[0] == 0
    assert plan(tkin=np.arange(1.0, 65.0), lnden=np.arange(64.0), lncd=np.arange(16.0))[0] == 0
    twelve = np.arange(12)
    bad = [
        (dict(n_axes=(0, 3, 1)), 'an axis of an excitation grid must have 1..64 nodes (tkin)'),
        (dict(n_axes=(2, 65, 1)), 'an axis of an excitation grid must have 1..64 nodes (lnden)'),
        (dict(n_axes=(2, 3, 0)), 'an axis of an excitation grid must have 1..64 nodes (lncd)'),
        (dict(tkin=np.arange(1.0, 65.0), lnden=np.arange(64.0), lncd=np.arange(17.0)), 'an excitation grid must have at most 65536 nodes (nt * nn * nc)'),
        (dict(tkin=(10.0, 10.0)), 'an axis of an excitation grid must be finite and strictly ascending (tkin)'),
        (dict(lnden=(3.0, np.nan, 5.0)), 'an axis of an excitation grid must be finite and strictly ascending (lnden)'),
        (dict(lncd=(np.inf,)), 'an axis of an excitation grid must be finite and strictly ascending (lncd)'),
        (dict(tex=np.where(twelve == 7, -1.0, 8.0)), 'an excitation temperature of a grid must be finite and positive: cut the grid where the '
                                                     'populations invert or the solver did not converge (spectrum 1, node 1)'),
        (dict(tex=np.where(twelve == 0, np.nan, 8.0)), 'populations invert or the solver did not converge (spectrum 0, node 0)'),
        (dict(ltau=np.where(twelve == 11, np.inf, 0.0)), 'a log10 optical depth of a grid must be finite: cut the grid where it is not (spectrum 1, node 5)'),
        (dict(wts=(1.0, 0.25, 0.7)), 'the weights of a transition must sum to 1 within 1e-6 (spectrum 1)'),
        # doubly wrong: the lines creator's checks come first, then the weights, the counts, the product, the axes, tex, ltau
        (dict(wts=(1.0, -0.25, 0.7), n_axes=(0, 3, 1)), 'a line weight must be finite and not negative (spectrum 1)'),
        (dict(wts=(1.0, 0.25, 0.7), n_axes=(0, 3, 1)), 'the weights of a transition must sum to 1 within 1e-6 (spectrum 1)'),
        (dict(n_axes=(2, 65, 1), tkin=(10.0, 10.0)), '1..64 nodes (lnden)'),
        (dict(tkin=(20.0, 10.0), tex=np.where(twelve == 7, -1.0, 8.0)), 'strictly ascending (tkin)'),
        (dict(tex=np.where(twelve == 7, 0.0, 8.0), ltau=np.where(twelve == 2, np.nan, 0.0)), 'did not converge (spectrum 1, node 1)'),
    ]
    for kw, words in bad:
        rc, msg, _ = plan(**kw)
        assert rc == 1 and msg.endswith(words), (kw, rc, msg)
    # from its creation on such a set has the baseline form's buffers: w == 1 over a scalar noise (no sigmas to form weights
    # from), the zeroed baseline record; a noise per channel forms its weights as ever
    SB_W, SB_WDATA, SB_BL, ST_ONES, ST_BL, ST_FORM_W = 1, 2, 4, 1 << 8, 1 << 14, 1 << 19
    out = (C.c_uint * 4)()
    lib.layout(1, 0, -1, out)
    assert out[0] == SB_W | SB_WDATA | SB_BL and (out[1], out[2]) == (1, 1) and out[3] & ST_ONES and out[3] & ST_BL and not out[3] & ST_FORM_W
    lib.layout(1, 1, 2, out)
    assert out[0] == SB_W | SB_WDATA | SB_BL and (out[1], out[2]) == (0, 1) and out[3] & ST_FORM_W and not out[3] & ST_ONES
    lib.layout(0, 0, -1, out)
    assert out[0] == 0 and out[3] & ST_FORM_W == 0
    lib.layout(0, 1, -1, out)
    assert out[0] == SB_W | SB_WDATA and out[3] & ST_FORM_W                                  # every other set: as before


def test_the_abi_declares_binds_and_exports_the_creator():
    """tests/test_abi.py's pattern for the new symbol: declared in the header, bound in _ffi, and (where the library is built)
    exported."""
    import re
    from nestfit_amd import _ffi
    header = (ROOT / 'include' / 'nestfit_amd.h').read_text()
    m = re.search(r'int nfa_specset_create_grid\(([^;]*)\);', header)
    assert m is not None
    n_args = len([a for a in m.group(1).split(',') if a.strip()])
    res, args = _ffi.SIGNATURES['nfa_specset_create_grid']
    assert res is C.c_int and len(args) == n_args == 20
    for word in ('NFA_MODEL_GRID         5', 'lncol_c - log10(sqrt(8 ln 2) sigm_c)', 'lncd innermost, then lnden, then tkin', 'CLAMPING'):
        assert word in header, word
    if _ffi.LIB_PATH.exists():
        assert hasattr(_ffi.load(), 'nfa_specset_create_grid')


# ---------------------------------------------------------------------------- the cube driver and the store
N_CHAN, NOISE = 64, 0.1
GRID_RANGES = [(-4, 4), (10.0, 50.0), (4.8, 5.4), (12.5, 14.0), (0.2, 1.5)]


def _stack(na, tables, n=3, seed=0):
    from nestfit_amd.cubeio import CubeStack, DataCube, SimpleCube
    rng = np.random.default_rng(seed)
    cubes = []
    for t in tables:
        x = lr.axis(t.nu, N_CHAN, 14.0)
        hdr = {'SIMPLE': True, 'BITPIX': -64, 'NAXIS': 3, 'NAXIS1': n, 'NAXIS2': n, 'NAXIS3': N_CHAN,
               'BUNIT': 'K', 'CTYPE1': 'RA---SIN', 'CTYPE2': 'DEC--SIN', 'CTYPE3': 'FREQ', 'CUNIT3': 'Hz',
               'CRVAL3': float(x[0]), 'CDELT3': float(x[1] - x[0]), 'CRPIX3': 1.0, 'RESTFRQ': t.nu}
        cubes.append(DataCube(SimpleCube(hdr, rng.normal(0, NOISE, (N_CHAN, n, n))), NOISE, lines=t))
    return CubeStack(cubes)


def _priors(na, ranges=GRID_RANGES):
    from scipy import stats
    x = np.linspace(0, 1, 200)
    return na.PriorTransformer([
        na.Prior(na.Distribution(lo + x * (hi - lo), stats.uniform(lo, hi - lo).pdf(lo + x * (hi - lo))), k)
        for k, (lo, hi) in enumerate(ranges)])


def _stub_backend(fitter, lon, lat, ncomp, nlive, kw):
    """A stand-in for the device: the numpy twin of the sampler on a Gaussian in the unit cube (the store's tables do not
    depend on what was fitted)."""
    from nestfit_amd import sampler

    def loglike(pix, U):
        return -0.5 * np.sum((U - 0.5) ** 2, axis=1) / 0.2 ** 2
    res = sampler.run_nested(loglike, 5 * ncomp, lon.size, nlive=nlive, batch_target=64, **kw)
    return res, np.full(lon.size, -40.0), 2 * N_CHAN


@pytest.mark.parametrize('fmt', ['npz', 'hdf5'])
def test_store_round_trip_of_the_grid(tmp_path, monkeypatch, fmt):
    import nestfit_amd as na
    from nestfit_amd import fitter as fit_mod, hdf5, postprocess as pp
    from nestfit_amd.fitter import CubeFitter
    from nestfit_amd.store import HdfStore
    if fmt == 'hdf5' and not hdf5.available():
        pytest.skip('no libhdf5')
    monkeypatch.setenv('NFA_STORE_FORMAT', fmt)
    assert fit_mod._MODEL_ID['grid'] == pp._MODEL_ID['grid'] == 5
    grid, t10, t21, t32 = gr.rotor_grid(na)
    stack = _stack(na, [t10, t32])
    fitter = CubeFitter(stack, _priors(na), na.GridRunner, lnZ_thresh=11, ncomp_max=1,
                        mn_kwargs={'nlive': 20, 'tol': 1.0, 'seed': 3, 'maxiter': 120}, nlive_snr_fact=0, fit_backend=_stub_backend)
    assert (fitter.model_id, fitter.n_model, fitter.runner_kwargs) == (5, 5, {})
    path = str(tmp_path / 'run')
    fitter.fit_cube(path, nproc=1)
    with HdfStore(path) as store:
        assert store.hdf.attrs['model_name'] == 'grid' and store.model is na.excitation
        assert store.hdf.attrs['n_params'] == 5 and list(store.hdf.attrs['par_names']) == ['voff', 'tkin', 'lnden', 'lncol', 'sigm']
        gg = store.hdf['/model_grid']
        assert gg.attrs['name'] == grid.name
        for key in ('tkin', 'lnden', 'lncd'):
            assert np.array_equal(np.asarray(gg[key][...]), getattr(grid, key))
        for k, t in enumerate((t10, t32)):
            g = store.hdf[f'/model_lines/spec{k}']
            assert g.attrs['nu'] == t.nu and g.attrs['name'] == t.name
            assert np.array_equal(np.asarray(g['voff'][...]), t.voff) and np.array_equal(np.asarray(g['tau_wts'][...]), t.tau_wts)
            assert np.array_equal(np.asarray(gg[f'tex{k}'][...]), t.tex) and np.array_equal(np.asarray(gg[f'ltau{k}'][...]), t.ltau)
        back = store.read_model_lines()
        assert back == [t10, t32] and all(isinstance(t, na.GridLines) for t in back)
        assert back[0].grid == grid and back[0].grid.name == grid.name and [t.name for t in back] == ['1-0', '3-2']
        assert len(list(store.iter_pix_groups())) == 9
    with HdfStore(path) as store:                                  # reopened
        assert pp.check_model_lines(store, stack) == [t10, t32]
        # a changed table, another grid, a plain LineTable, another order, a cube less: refused
        warmer = grid.transition(t32.nu, np.array(t32.tex) * 1.01, t32.ltau, name='3-2')
        thicker = grid.transition(t32.nu, t32.tex, np.array(t32.ltau) + 0.01, name='3-2')
        _, o10, _, o32 = gr.rotor_grid(na, gr.AXES_222)
        plain = na.LineTable(t32.nu, t32.voff, t32.tau_wts)
        for tables in ([t10, warmer], [t10, thicker], [o10, o32], [t10, plain], [t32, t10], [t10]):
            other = _stack(na, tables)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.check_model_lines(store, other)
            with pytest.raises(ValueError, match='line tables differ'):
                pp.postprocess_run(store, other, predict_backend=lambda *a: None)
    # two grids in one stack: nothing is written
    with pytest.raises(ValueError, match='share one ExcitationGrid'):
        CubeFitter(_stack(na, [t10, o32]), _priors(na), na.GridRunner, fit_backend=_stub_backend).fit_cube(str(tmp_path / 'two'), nproc=1)
    # the six options the model does not take: refused by the fitter on the host
    with pytest.raises(ValueError, match='a set of the excitation-grid model takes no robust likelihood'):
        CubeFitter(stack, _priors(na), na.GridRunner, runner_kwargs={'robust': 4.0}, fit_backend=_stub_backend)


def test_the_multinest_case_on_the_samplers_twin(nfo):
    """tests/test_grid.py's `run_multinest` case without the device: the sampler's numpy twin (`sampler.run_nested`) over the
    restatement's likelihood for the same rows, priors, nlive, tolerance and seed.  The reference run itself keeps tkin, lnden
    and lncol within 5 posterior standard deviations of the truth, so that the criterion the device run is held to is one the
    model and the data support.  (The twin draws 64 proposals a round where the device draws its 262144: the same algorithm
    and options, not the same random numbers.)

    Measured: 28199 likelihood evaluations; tkin 25.199 +- 0.308 (truth 25), lnden 5.9955 +- 0.0069 (6), lncol 13.3015 +-
    0.0025 (13.3): 0.65, 0.65 and 0.61 standard deviations off."""
    import nestfit_amd as na
    from nestfit_amd import sampler
    import hf_restatement as hfr
    from test_grid import FIT_RANGES, TRUTH_FIT, fit_rows
    rows, grid = fit_rows(na, nfo)
    ut = _priors(na, FIT_RANGES)
    assert grid.covers(*np.array(FIT_RANGES).T)                # the uniform priors' box
    ps = nfo.PriorSet(ut.lower())
    tbgs = [hfr.tbg_of(nfo, x) for x, *_ in rows]

    def loglike(pix, U):
        out = np.empty(U.shape[0])
        for k, row in enumerate(U):
            ps.transform(row, 1)                             # in place, as a runner's loglikelihood leaves it
            out[k] = gr.restated(nfo, rows, row, tbgs)[1]
        return out
    res = sampler.run_nested(loglike, 5, 1, nlive=200, tol=0.5, efr=0.3, seed=5, log_zero=-1e100, free_mask=ut.free_mask(1),
                             ellipsoids=min(100, sampler._NS_ME), batch_target=64)[0]
    mean, std = res.param_constr[0], res.param_constr[1]
    null_lnz = sum(hfr.loglike(d, np.zeros(d.size), noise) for _, d, noise, _ in rows)
    print(f'twin: lnZ - null_lnZ = {res.lnZ - null_lnz:.1f}; mean {mean}, std {std}, truth {TRUTH_FIT}')
    assert not res.truncated and res.lnZ - null_lnz > 11
    for k in (1, 2, 3):
        assert abs(mean[k] - TRUTH_FIT[k]) < 5 * std[k], (k, mean[k], std[k])
    assert std[1] < 2.0 and std[2] < 0.05 and std[3] < 0.02                     # constrained, not the priors' widths
