"""A restatement of LAYERED radiative transfer (include/nestfit_amd.h: nfa_specset_set_layered) for the tests.
The components of a parameter vector are layers along the line of sight, component 0 the farthest, and each absorbs what
lies behind it: in component order, on the channels where the component's optical depth is not zero,

    pred <- pred + (g_c - pred) a_c        g_c = T0 (y(T0 / tex_c) - tbg),   a_c = 1 - FastExp(tau_c)

(a filled LTE set: pred + ((g_c - pred) 10^lnff_c) a_c) where the summed model adds g_c a_c.

For the line-table, LTE, band, mix and filled models the optical depth of a component is formed by the body of
tests/hf_restatement.py, mix_restatement.py and fill_restatement.py -- the same loop over the lines, from the same pinned
pieces (`nfo.fast_expn`, `nfo.iemtex_interp`, the oracle's background term) -- and only the last line, the one that adds
the component's term, is the recurrence above.  For ammonia and N2H+ the oracle has the whole one-component prediction
p_c = g_c a_c; with g_c from `nfo.iemtex_interp` and `tbg_arr` the same update reads pred + p_c (1 - pred / g_c).

Every function returns the pair (layered spectrum, S) with S = sum_c |g_c a_c| (|f_c g_c a_c| filled), the summed model
of the same parameters term by term in absolute value: the scale the device's deviations are measured against, since a
layered channel can be a small difference of large terms.  `terms`, where given a list, receives one (tau_c, g_c, a_c)
per component, arrays over the channels (a_c with the filling factor in it), for the tests' statements about their draws."""
import math

import numpy as np

import band_restatement as br
import hf_restatement as hfr
import lte_restatement as lr
import mix_restatement as mr

CKMS, H, KB = hfr.CKMS, hfr.H, hfr.KB


def line_tau(nfo, xarr, parts, voff, sigm):
    """tau of one component on `xarr`: `parts` = [(nu_g, voff[], tau_wts[], tau_main)] of every transition of the
    spectrum (hf_restatement.hf_predict's loop over the lines, one transition or several)."""
    tarr = np.zeros(xarr.size)
    for nu_g, tv, tw, tau_main in parts:
        lo, hi = hfr.hf_windows(xarr, (nu_g, tv, tw), voff, sigm)
        for i, v in enumerate(tv):
            if lo[i] < 0:
                continue
            hf_freq = (1.0 - float(v) / CKMS) * nu_g
            hf_width = sigm / CKMS * hf_freq
            hf_nucen = hf_freq - voff / CKMS * hf_freq
            hf_tau = tau_main * float(tw[i])
            hf_idenom = 0.5 / (hf_width * hf_width)
            nu = xarr[lo[i]:hi[i]] - hf_nucen
            tarr[lo[i]:hi[i]] += hf_tau * nfo.fast_expn(nu * nu * hf_idenom)
    return tarr


def through_the_layers(nfo, xarr, tbg, layers, terms=None):
    """(layered, S) of `layers` = [(tau_c[], tex_c, f_c or None)] in order, the farthest first."""
    pred, S = np.zeros(xarr.size), np.zeros(xarr.size)
    for tarr, tex, ff in layers:
        nz = tarr != 0.0
        T0 = H * xarr[nz] / KB
        g = T0 * (nfo.iemtex_interp(T0 / tex) - tbg[nz])
        a = 1.0 - nfo.fast_expn(tarr[nz])
        if ff is None:
            pred[nz] = pred[nz] + (g - pred[nz]) * a
            S[nz] += np.abs(g * a)
        else:
            pred[nz] = pred[nz] + ((g - pred[nz]) * ff) * a
            S[nz] += np.abs((g * ff) * a)
        if terms is not None:
            full_g, full_a = np.zeros(xarr.size), np.zeros(xarr.size)
            full_g[nz], full_a[nz] = g, a if ff is None else ff * a
            terms.append((tarr, full_g, full_a))
    return pred, S


def product_form(terms):
    """sum_c g_c a_c prod_{c' > c} (1 - a_c'): the recurrence written out, from the (tau, g, a) of `terms`."""
    out = np.zeros(terms[0][0].size)
    for c, (_, g, a) in enumerate(terms):
        t = g * a
        for _, _, a2 in terms[c + 1:]:
            t = t * (1.0 - a2)
        out += t
    return out


def hf_layered(nfo, xarr, tbg, table, params, terms=None):
    """hf_restatement.hf_predict layered: `table` = (nu, voff[], tau_wts[]), params voff, tex, ltau, sigm parameter-major."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    nu0, tv, tw = table
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // 4
    layers = []
    for c in range(ncomp):
        voff, tex, ltau, sigm = (float(params[k * ncomp + c]) for k in range(4))
        layers.append((line_tau(nfo, xarr, [(nu0, tv, tw, math.pow(10.0, ltau))], voff, sigm), tex, None))
    return through_the_layers(nfo, xarr, tbg, layers, terms)


def lte_layered(nfo, xarr, tbg, lines, params, terms=None):
    """lte_restatement.lte_predict layered: one transition, `lines` an LteLines."""
    mol = lines.molecule
    trans = (lines.nu, lines.e_up, lines.g_up, lines.a_ul)
    return hf_layered(nfo, xarr, tbg, hfr.table_of(lines), lr.ltau_params(trans, mol.q_temp, mol.q_val, params), terms)


def band_layered(nfo, xarr, tbg, lines, params, terms=None):
    """band_restatement.band_predict layered: `lines` an LteLines or LteBand, params voff, tex, lncol, sigm."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    mol = lines.molecule
    parts = br.transitions_of(lines)
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // 4
    layers = []
    for c in range(ncomp):
        voff, tex, lncol, sigm = (float(params[k * ncomp + c]) for k in range(4))
        taus = [(trans[0], tv, tw, br.band_tau_main(trans, mol.q_temp, mol.q_val, tex, lncol, sigm)) for trans, tv, tw in parts]
        layers.append((line_tau(nfo, xarr, taus, voff, sigm), tex, None))
    return through_the_layers(nfo, xarr, tbg, layers, terms)


def mix_layered(nfo, xarr, tbg, lines, species, params, fill=False, terms=None):
    """mix_restatement.mix_predict (fill: fill_restatement.fill_predict) layered: K species, 3 + K (4 + K) parameters."""
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
        layers.append((line_tau(nfo, xarr, taus, voff, sigm), tex, ff))
    return through_the_layers(nfo, xarr, tbg, layers, terms)


def oracle_layered(nfo, make_spectrum, predict, n_model, tex_row, xarr, params, terms=None):
    """Ammonia and N2H+: the oracle's one-component predictions p_c = g_c a_c put through the layers.  make_spectrum():
    an oracle spectrum on `xarr`; predict(s, params_c): the oracle's predict; tex_row: the row of tex among the n_model
    parameters of a component (2 ammonia, 1 N2H+)."""
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // n_model
    s = make_spectrum()
    tbg = np.array(s.tbg_arr)
    T0 = H * np.asarray(xarr, dtype=np.float64) / KB
    pred, S = np.zeros(T0.size), np.zeros(T0.size)
    for c in range(ncomp):
        one = np.ascontiguousarray(params[c::ncomp])
        predict(s, one)
        p = np.array(s.get_spec())
        g = T0 * (nfo.iemtex_interp(T0 / float(one[tex_row])) - tbg)
        nz = p != 0.0
        pred[nz] = pred[nz] + p[nz] * (1.0 - pred[nz] / g[nz])
        S += np.abs(p)
        if terms is not None:
            a = np.zeros(T0.size)
            a[nz] = p[nz] / g[nz]
            terms.append((np.array(s.tarr), g, a))
    return pred, S


def amm_layered(nfo, xarr, trans_id, params, terms=None):
    return oracle_layered(nfo, lambda: nfo.AmmoniaSpectrum(xarr, np.zeros(len(xarr)), 1.0, trans_id), nfo.amm_predict, 6, 2,
                          xarr, params, terms)


def nnhp_layered(nfo, xarr, trans_id, params, terms=None):
    return oracle_layered(nfo, lambda: nfo.DiazenyliumSpectrum(xarr, np.zeros(len(xarr)), 1.0, trans_id), nfo.nnhp_predict, 4, 1,
                          xarr, params, terms)


def loglike(data, pred, noise):
    return hfr.loglike(data, pred, noise)
