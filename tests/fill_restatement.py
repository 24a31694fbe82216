"""A restatement of filled LTE sets (include/nestfit_amd.h: nfa_specset_create_lte_filled) for the tests: an LTE mix of K
species whose components have a beam filling factor as one more parameter, the last, parameter-major

    voff, tex, lncol_0, sigm, lncol_1, ..., lncol_{K-1}, lnff

This is tests/mix_restatement.mix_predict with a component's term multiplied by 10.0 ** lnff_c before it is added -- the
direct formula

    pred = sum_c 10^lnff_c . T0 (y(T0 / tex_c) - tbg) (1 - FastExp(tau_c))

with tau_c as the mix's restatement forms it.  The test species are mix_restatement's."""
import numpy as np

import band_restatement as br
import hf_restatement as hfr
import mix_restatement as mr
from mix_restatement import CKMS, H, KB, iso_species, made_up_species, test_species  # noqa: F401  (the same species)


def lnff_of(params, n_species, ncomp, c):
    return float(params[(3 + n_species) * ncomp + c])


def fill_predict(nfo, xarr, tbg, lines, species, params):
    """Model spectrum of parameter-major `params` (4 + K per component) on `xarr` for all the transitions of `lines` (an
    LteLines, LteBand or LteBlend of the molecules `species`)."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    species = list(species)
    parts = [(species.index(t.molecule), t.molecule, tr, tv, tw)
             for t, (tr, tv, tw) in zip(lines.transitions if hasattr(lines, 'transitions') else (lines,), br.transitions_of(lines))]
    params = np.asarray(params, dtype=np.float64)
    K = len(species)
    ncomp = params.size // (4 + K)
    assert params.size == (4 + K) * ncomp
    pred = np.zeros(xarr.size)
    for c in range(ncomp):
        voff, tex, sigm = float(params[c]), float(params[ncomp + c]), float(params[3 * ncomp + c])
        tarr = np.zeros(xarr.size)
        for k, mol, trans, tv, tw in parts:
            nu_g = trans[0]
            tau_main = br.band_tau_main(trans, mol.q_temp, mol.q_val, tex, mr.lncol_of(params, K, ncomp, c, k), sigm)
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
        nz = tarr != 0.0
        T0 = H * xarr[nz] / KB
        pred[nz] += 10.0 ** lnff_of(params, K, ncomp, c) * (T0 * (nfo.iemtex_interp(T0 / tex) - tbg[nz]) * (1.0 - nfo.fast_expn(tarr[nz])))
    return pred


def restated(nfo, rows, species, theta, tbgs=None):
    """(spectra of the rows [xarr, data, noise, lines] concatenated, lnL) for one parameter vector."""
    tbgs = tbgs or [hfr.tbg_of(nfo, x) for x, *_ in rows]
    preds = [fill_predict(nfo, x, tbg, tab, species, theta) for (x, _, _, tab), tbg in zip(rows, tbgs)]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl
