"""A restatement of the excitation-grid model (include/nestfit_amd.h: nfa_specset_create_grid) with `math` in doubles, for the
tests.  For component c and spectrum s, on the axes tkin, lnden, lncd the spectra share:

    x = (tkin_c, lnden_c, lncol_c - log10(sqrt(8 ln 2) sigm_c))
    per axis a_0 < ... < a_{n-1}:  k = #{ i in 1..n-2 : x >= a_i },  f = clamp((x - a_k) / (a_{k+1} - a_k), 0, 1)
                                   (one node: k = 0, f = 0)
    v(x) = trilinear over the eight corners, each step v0 + f (v1 - v0), lncd innermost, then lnden, then tkin
    tex_{c,s} = tex_s(x)        ltau_{c,s} = ltau_s(x)

and then tests/hf_restatement.hf_predict once per spectrum with (voff_c, tex_{c,s}, ltau_{c,s}, sigm_c) of every component: that
function takes a `tex` per call.  A tkin, lnden or lncol that is not finite, or a sigm that is not an ordinary positive
number, gives a NaN ltau; tex is the rule in IEEE arithmetic whatever the arguments (an infinite coordinate clamps to the edge,
a NaN one gives NaN unless its axis has one node).

The test grids are closed forms over lte_restatement's rigid rotor, no data: the two-level formula

    tex_s = tkin / (1 + (tkin / T0_s) ln(1 + ncrit_s / n)),      T0_s = h nu_s / k,  n = 10^lnden

with the critical densities NCRIT a decade apart (two decades from 1-0 to 3-2), and ltau_s = log10 of
lte_restatement.tau_main at that tex_s with sigm = 1 / sqrt(8 ln 2) (an FWHM of 1 km/s) and lncol = lncd.  The test grids
cover tkin >= 9 K and 10^4.7 <= n <= 10^5.5: there 1-0 is close to thermal and 3-2 well below it, tex_{1-0} / tex_{3-2} >= 1.5
at every node (1.7 at the least), hence -- both interpolants being the same convex combination of their nodes -- everywhere,
the clamped outside included: a kernel that reads one tex per component is wrong by far more than any tolerance.  And every
tex stays above 2.9 K, above the background: every component's term is positive, as in tests/test_lte.py, so that the
per-channel relative tolerances of that test mean what they mean there (no channel is a small difference of large terms)."""
import math

import numpy as np

import hf_restatement as hfr
import lte_restatement as lr

FWHM = math.sqrt(8.0 * math.log(2.0))
NCRIT = (1e4, 1e5, 1e6)                  # of 1-0, 2-1, 3-2 (cm^-3)
# the grids of the tests: (tkin, lnden, lncd), non-uniform
AXES_546 = ([9.0, 12.0, 20.0, 35.0, 60.0], [4.7, 4.9, 5.2, 5.5], [11.5, 12.2, 12.8, 13.3, 13.9, 14.5])
AXES_222 = ([10.0, 40.0], [4.8, 5.4], [12.0, 14.0])
AXES_111 = ([20.0], [5.0], [13.0])


def cell(a, x):
    """(k, f) of coordinate `x` on the axis `a`; a NaN coordinate keeps a NaN fraction."""
    n = len(a)
    if n == 1:
        return 0, 0.0
    k = 0
    for i in range(1, n - 1):
        if x >= a[i]:
            k += 1
    t = (x - a[k]) / (a[k + 1] - a[k])
    return k, (0.0 if t < 0.0 else 1.0 if t > 1.0 else t)


def interpolate(axes, table, x):
    """`table` [nt][nn][nc] (anything indexable so) at x = (tkin, lnden, lncd)."""
    (kt, ft), (kn, fn), (kc, fc) = (cell(a, v) for a, v in zip(axes, x))
    kt1, kn1, kc1 = (k + 1 if len(a) > 1 else k for k, a in zip((kt, kn, kc), axes))

    def along_c(a, b):
        v0, v1 = float(table[a][b][kc]), float(table[a][b][kc1])
        return v0 + fc * (v1 - v0)
    v00, v01, v10, v11 = along_c(kt, kn), along_c(kt, kn1), along_c(kt1, kn), along_c(kt1, kn1)
    v0 = v00 + fn * (v01 - v00)
    v1 = v10 + fn * (v11 - v10)
    return v0 + ft * (v1 - v0)


def _log10(v):
    """log10 as IEEE has it: NaN for a negative number or NaN, -inf for 0, inf for inf."""
    if v != v or v < 0:
        return math.nan
    return -math.inf if v == 0 else math.inf if v == math.inf else math.log10(v)


def excitation(axes, tex_table, ltau_table, tkin, lnden, lncol, sigm):
    """(tex, ltau) of one transition at the physical conditions of one component.  tex is the rule in IEEE arithmetic whatever
    the arguments (an infinite coordinate is clamped to the edge, a NaN one gives NaN unless its axis has one node); ltau is
    NaN where tkin, lnden or lncol is not finite or sigm is not an ordinary positive number."""
    ordinary = all(math.isfinite(v) for v in (tkin, lnden, lncol, sigm)) and sigm > 0
    x = (tkin, lnden, lncol - _log10(FWHM * sigm))
    tex = interpolate(axes, tex_table, x)
    return tex, (interpolate(axes, ltau_table, x) if ordinary else math.nan)


def hf_params(lines, params):
    """Parameter-major (voff, tkin, lnden, lncol, sigm) of every component -> parameter-major (voff, tex, ltau, sigm) for the
    transition `lines`, a nestfit_amd.GridLines (read for its numbers only)."""
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // 5
    axes = [list(map(float, a)) for a in (lines.grid.tkin, lines.grid.lnden, lines.grid.lncd)]
    out = np.empty(4 * ncomp)
    for c in range(ncomp):
        voff, tkin, lnden, lncol, sigm = (float(params[k * ncomp + c]) for k in range(5))
        tex, ltau = excitation(axes, lines.tex, lines.ltau, tkin, lnden, lncol, sigm)
        out[c], out[ncomp + c], out[2 * ncomp + c], out[3 * ncomp + c] = voff, tex, ltau, sigm
    return out


def grid_predict(nfo, xarr, tbg, lines, params):
    """Model spectrum of parameter-major `params` on `xarr` for one transition."""
    return hfr.hf_predict(nfo, xarr, tbg, hfr.table_of(lines), hf_params(lines, params))


def restated(nfo, rows, theta, tbgs=None):
    """(spectra of the rows [xarr, data, noise, GridLines] concatenated, lnL) for one parameter vector."""
    tbgs = tbgs or [hfr.tbg_of(nfo, x) for x, *_ in rows]
    preds = [grid_predict(nfo, x, tbg, tab, theta) for (x, _, _, tab), tbg in zip(rows, tbgs)]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl


# ---------------------------------------------------------------------------- the closed-form grids
def two_level_tex(nu, ncrit, tkin, lnden):
    t0 = lr.H * nu / lr.KB
    return tkin / (1.0 + (tkin / t0) * math.log(1.0 + ncrit / 10.0 ** lnden))


def two_level_tables(trans, q_temp, q_val, ncrit, axes, thermal=False):
    """(tex, ltau), [nt, nn, nc] each, of `trans` = (nu, e_up, g_up, a_ul) over `axes`; thermal: tex = tkin (n -> infinity)."""
    tkin, lnden, lncd = axes
    tex = np.empty((len(tkin), len(lnden), len(lncd)))
    ltau = np.empty_like(tex)
    for i, t in enumerate(tkin):
        for j, d in enumerate(lnden):
            tx = float(t) if thermal else two_level_tex(trans[0], ncrit, float(t), float(d))
            for k, n in enumerate(lncd):
                tex[i, j, k] = tx
                ltau[i, j, k] = math.log10(lr.tau_main(trans, q_temp, q_val, tx, float(n), 1.0 / FWHM))
    return tex, ltau


def rotor_grid(na, axes=AXES_546, thermal=False, wide=False, name='two-level rotor'):
    """(grid, 1-0 with the three-line structure, 2-1 and 3-2 as single lines) of lte_restatement's rigid rotor on `axes`;
    wide: the 3-2 with the made-up structure of 30 lines of tests/test_lte.py (the WIDE kernels)."""
    from test_lte_cpu import B_ROT, MU
    temps = np.geomspace(5.0, 40.0, 32)
    q_val = lr.rotor_partition(B_ROT, temps)
    grid = na.ExcitationGrid(*axes, name=name)
    out = []
    for J, (voff, wts) in enumerate((([-7.1, 0.0, 4.9], [0.2, 0.5, 0.3]), ([0.0], [1.0]), ([0.0], [1.0]))):
        trans = lr.rotor_transition(B_ROT, MU, J)
        tex, ltau = two_level_tables(trans, temps, q_val, NCRIT[J], axes, thermal)
        norm = False
        if wide and J == 2:
            rng = np.random.default_rng(4321)
            voff = np.sort(rng.uniform(-25, 25, 30))
            rng.shuffle(voff)
            wts, norm = rng.uniform(0.01, 0.06, 30), True
        out.append(grid.transition(trans[0], tex, ltau, voff=voff, tau_wts=wts, name=f'{J + 1}-{J}', normalise=norm))
    return (grid, *out)


def tex_spread(tables, theta):
    """The smallest over the components of max / min of the spectra's tex at `theta` (parameter-major)."""
    per = np.stack([hf_params(t, theta) for t in tables])
    ncomp = per.shape[1] // 4
    tex = per[:, ncomp:2 * ncomp]
    return float(np.min(tex.max(axis=0) / tex.min(axis=0)))
