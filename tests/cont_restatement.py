"""A restatement of the model before a CONTINUUM BACKGROUND (include/nestfit_amd.h: nfa_specset_set_continuum)
for the tests.  Behind all components of a spectrum lies a source of brightness temperature Tc >= 0, whose level was taken
off the data; measured against that off-line level a component gives, on the channels where its optical depth is not zero,

    summed:    pred <- pred + (g_c - Tc) a_c                 g_c = T0 (y(T0 / tex_c) - tbg),   a_c = 1 - FastExp(tau_c)
    layered:   pred <- pred + (g_c - Tc - pred) a_c          (component 0 the farthest, tests/layer_restatement.py)
    filled:    ((g_c - Tc [- pred]) f_c) a_c                 in that association

Built from the pinned pieces the sibling restatements use: `nfo.fast_expn`, `nfo.iemtex_interp`, the oracle's `tbg_arr`,
`layer_restatement.line_tau` for the optical depth of a component of a line table, an LTE band, a mix or a filled mix.  For
ammonia and N2H+ the oracle has the whole one-component prediction p_c = g_c a_c; with g_c from `nfo.iemtex_interp` and
`tbg_arr` as in `layer_restatement.oracle_layered`, a_c = p_c / g_c and the component's term is p_c (1 - (Tc [+ pred]) / g_c).

Every function returns the pair (spectrum, S) with S = sum_c (|g_c| + Tc) |a_c| (a_c with the filling factor in it): the
scale the deviations are measured against, because g_c - Tc cancels where J(tex) ~ J(Tcmb) + Tc.

The components of a parameter vector are formed ONCE as `layers` (`*_layers`) or oracle `terms` (`oracle_terms`) and put
before any continuum, summed or layered, by `through` / `through_oracle`: the tests evaluate several (Tc, transfer) on one
set of draws."""
import math

import numpy as np

import band_restatement as br
import hf_restatement as hfr
import layer_restatement as lay
import lte_restatement as lr
import mix_restatement as mr

H, KB = hfr.H, hfr.KB


def through(nfo, xarr, tbg, layers, tc, layered):
    """(spectrum, S) of `layers` = [(tau_c[], tex_c, f_c or None)] in order, the farthest first, before a continuum `tc`."""
    xarr = np.asarray(xarr, dtype=np.float64)
    tc = float(tc)
    pred, S = np.zeros(xarr.size), np.zeros(xarr.size)
    for tarr, tex, ff in layers:
        nz = tarr != 0.0
        T0 = H * xarr[nz] / KB
        g = T0 * (nfo.iemtex_interp(T0 / tex) - tbg[nz])
        a = 1.0 - nfo.fast_expn(tarr[nz])
        d = g - tc
        if layered:
            d = d - pred[nz]
        if ff is None:
            pred[nz] = pred[nz] + d * a
            S[nz] += (np.abs(g) + tc) * np.abs(a)
        else:
            pred[nz] = pred[nz] + (d * ff) * a
            S[nz] += (np.abs(g) + tc) * np.abs(ff * a)
    return pred, S


def hf_layers(nfo, xarr, table, params):
    """The layers of hf_restatement.hf_predict's parameters (voff, tex, ltau, sigm parameter-major) for `table` =
    (nu, voff[], tau_wts[])."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    nu0, tv, tw = table
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // 4
    layers = []
    for c in range(ncomp):
        voff, tex, ltau, sigm = (float(params[k * ncomp + c]) for k in range(4))
        layers.append((lay.line_tau(nfo, xarr, [(nu0, tv, tw, math.pow(10.0, ltau))], voff, sigm), tex, None))
    return layers


def lte_layers(nfo, xarr, lines, params):
    """... of lte_restatement.lte_predict's: one transition, `lines` an LteLines."""
    mol = lines.molecule
    trans = (lines.nu, lines.e_up, lines.g_up, lines.a_ul)
    return hf_layers(nfo, xarr, hfr.table_of(lines), lr.ltau_params(trans, mol.q_temp, mol.q_val, params))


def mix_layers(nfo, xarr, lines, species, params, fill=False):
    """... of mix_restatement.mix_predict's (fill: fill_restatement.fill_predict's): K species, 3 + K (4 + K) parameters."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    species = list(species)
    parts = [(species.index(t.molecule), t.molecule, tr, tv, tw)
             for t, (tr, tv, tw) in zip(lines.transitions if hasattr(lines, 'transitions') else (lines,), br.transitions_of(lines))]
    params = np.asarray(params, dtype=np.float64)
    K = len(species)
    n_par = 3 + K + (1 if fill else 0)
    ncomp = params.size // n_par
    assert params.size == n_par * ncomp
    layers = []
    for c in range(ncomp):
        voff, tex, sigm = float(params[c]), float(params[ncomp + c]), float(params[3 * ncomp + c])
        taus = [(trans[0], tv, tw, br.band_tau_main(trans, mol.q_temp, mol.q_val, tex, mr.lncol_of(params, K, ncomp, c, k), sigm))
                for k, mol, trans, tv, tw in parts]
        ff = 10.0 ** float(params[(3 + K) * ncomp + c]) if fill else None
        layers.append((lay.line_tau(nfo, xarr, taus, voff, sigm), tex, ff))
    return layers


def hf_cont(nfo, xarr, tbg, table, params, tc, layered=False):
    return through(nfo, xarr, tbg, hf_layers(nfo, xarr, table, params), tc, layered)


def mix_cont(nfo, xarr, tbg, lines, species, params, tc, fill=False, layered=False):
    return through(nfo, xarr, tbg, mix_layers(nfo, xarr, lines, species, params, fill), tc, layered)


def oracle_terms(nfo, make_spectrum, predict, n_model, tex_row, xarr, params):
    """Ammonia and N2H+: [(p_c, g_c, tau_c, tex_c)] of the oracle's one-component predictions, as
    layer_restatement.oracle_layered forms them.  make_spectrum(): an oracle spectrum on `xarr`; predict(s, params_c): the
    oracle's predict; tex_row: the row of tex among the n_model parameters of a component (2 ammonia, 1 N2H+).  The
    spectrum's `tbg_arr` comes back as the second value."""
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // n_model
    s = make_spectrum()
    tbg = np.array(s.tbg_arr)
    T0 = H * np.asarray(xarr, dtype=np.float64) / KB
    terms = []
    for c in range(ncomp):
        one = np.ascontiguousarray(params[c::ncomp])
        predict(s, one)
        tex = float(one[tex_row])
        terms.append((np.array(s.get_spec()), T0 * (nfo.iemtex_interp(T0 / tex) - tbg), np.array(s.tarr), tex))
    return terms, tbg


def through_oracle(terms, tc, layered):
    """(spectrum, S) of `oracle_terms`' terms before a continuum `tc`: pred + p_c (1 - (Tc [+ pred]) / g_c)."""
    tc = float(tc)
    n = terms[0][0].size
    pred, S = np.zeros(n), np.zeros(n)
    for p, g, _, _ in terms:
        nz = p != 0.0
        back = tc + pred[nz] if layered else tc
        pred[nz] = pred[nz] + p[nz] * (1.0 - back / g[nz])
        S[nz] += (np.abs(g[nz]) + tc) * np.abs(p[nz] / g[nz])
    return pred, S


def amm_terms(nfo, xarr, trans_id, params):
    return oracle_terms(nfo, lambda: nfo.AmmoniaSpectrum(xarr, np.zeros(len(xarr)), 1.0, trans_id), nfo.amm_predict, 6, 2, xarr, params)


def nnhp_terms(nfo, xarr, trans_id, params):
    return oracle_terms(nfo, lambda: nfo.DiazenyliumSpectrum(xarr, np.zeros(len(xarr)), 1.0, trans_id), nfo.nnhp_predict, 4, 1, xarr, params)


def amm_cont(nfo, xarr, trans_id, params, tc, layered=False):
    return through_oracle(amm_terms(nfo, xarr, trans_id, params)[0], tc, layered)


def nnhp_cont(nfo, xarr, trans_id, params, tc, layered=False):
    return through_oracle(nnhp_terms(nfo, xarr, trans_id, params)[0], tc, layered)


def shifted_background(xarr, tbg, tc):
    """tbg + Tc / T0: the background term with which the restatements WITHOUT a continuum give the same model, T0 (y - tbg -
    Tc / T0) = g - Tc -- the independent route of the CPU test."""
    return np.asarray(tbg) + float(tc) / (H * np.asarray(xarr, dtype=np.float64) / KB)
