"""A restatement of LTE bands (include/nestfit_amd.h: nfa_specset_create_lte_bands) for the tests: a spectrum covers several
transitions g of the species, and line i of transition g has

    hf_freq_i = (1 - v_i / CKMS) nu_g
    tau_i     = tau_main_g(tex, lncol, sigm) w_i

with tau_main_g from tests/lte_restatement.tau_main; everything after that is the loop of tests/hf_restatement.hf_predict
over all the lines of the spectrum, assembled from the same pieces (the oracle's FastExp and 1/(e^x - 1) table, the
window arithmetic of hf_windows).  tau_main passes through log10 and back, as lte_restatement's does, so that a band of
one transition is lte_restatement.restated bit for bit; an optical depth that underflowed to 0 stays 0.

The test species is a symmetric top made here from closed forms -- rotation constants A and B (Hz), a distortion constant
D_JK (Hz), a dipole moment mu (esu cm) and made-up spin weights g_K:

    nu_JK = 2 (J + 1) (B - D_JK K^2)                     J + 1, K -> J, K
    E_u   = h [B J'(J' + 1) + (A - B) K^2] / k           J' = J + 1
    A_ul  = 64 pi^4 nu^3 mu^2 (J'^2 - K^2) / (3 h c^3 J' (2 J' + 1))
    g_u   = (2 J' + 1) g_K
    Q(T)  = sum_J sum_{K <= J} (2 J + 1) g_K exp(-h [B J (J + 1) + (A - B) K^2] / k T)
"""
import math

import numpy as np

import hf_restatement as hfr
import lte_restatement as lr

CKMS, H, KB, CCMS = lr.CKMS, lr.H, lr.KB, lr.CCMS


def spin_weight(K):
    """g_K, made up: 1 for K = 0, 2 for the other K, doubled again where K is a multiple of 3."""
    return 1.0 if K == 0 else 4.0 if K % 3 == 0 else 2.0


def top_transition(A, B, D_JK, mu, J, K):
    """(nu, e_up, g_up, a_ul) of J+1, K -> J, K."""
    Jp = J + 1
    nu = 2.0 * Jp * (B - D_JK * K * K)
    e_up = H * (B * Jp * (Jp + 1) + (A - B) * K * K) / KB
    g_up = (2.0 * Jp + 1.0) * spin_weight(K)
    a_ul = 64.0 * math.pi ** 4 * nu ** 3 * mu ** 2 * (Jp * Jp - K * K) / (3.0 * H * CCMS ** 3 * Jp * (2 * Jp + 1))
    return nu, e_up, g_up, a_ul


def top_partition(A, B, temps, j_max=200):
    """Q at every temperature of `temps`: the direct sum (B > 5 GHz, T < 300 K: converged far below the last bit)."""
    return np.array([sum((2 * J + 1) * spin_weight(K) * math.exp(-H * (B * J * (J + 1) + (A - B) * K * K) / (KB * T))
                         for J in range(j_max) for K in range(J + 1)) for T in temps])


def transitions_of(lines):
    """[(trans, voff[], tau_wts[])] of a nestfit_amd.LteLines or LteBand (read for its numbers only), in its order."""
    parts = lines.transitions if hasattr(lines, 'transitions') else (lines,)
    return [((t.nu, t.e_up, t.g_up, t.a_ul), np.array(t.voff), np.array(t.tau_wts)) for t in parts]


def band_tau_main(trans, q_temp, q_val, tex, lncol, sigm):
    """tau_main of one transition, through log10 and back like lte_restatement.ltau_params (0 and NaN as they are)."""
    tau = lr.tau_main(trans, q_temp, q_val, tex, lncol, sigm)
    return math.pow(10.0, math.log10(tau)) if tau > 0 else tau


def band_predict(nfo, xarr, tbg, lines, params):
    """Model spectrum of parameter-major `params` (voff, tex, lncol, sigm of every component) on `xarr` for all the
    transitions of `lines` (an LteLines or an LteBand)."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    mol = lines.molecule
    parts = transitions_of(lines)
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // 4
    pred = np.zeros(xarr.size)
    for c in range(ncomp):
        voff, tex, lncol, sigm = (float(params[k * ncomp + c]) for k in range(4))
        tarr = np.zeros(xarr.size)
        for trans, tv, tw in parts:
            nu_g = trans[0]
            tau_main = band_tau_main(trans, mol.q_temp, mol.q_val, tex, lncol, sigm)
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
        pred[nz] += T0 * (nfo.iemtex_interp(T0 / tex) - tbg[nz]) * (1.0 - nfo.fast_expn(tarr[nz]))
    return pred


def restated(nfo, rows, theta, tbgs=None):
    """(spectra of the rows [xarr, data, noise, LteLines or LteBand] concatenated, lnL) for one parameter vector."""
    tbgs = tbgs or [hfr.tbg_of(nfo, x) for x, *_ in rows]
    preds = [band_predict(nfo, x, tbg, tab, theta) for (x, _, _, tab), tbg in zip(rows, tbgs)]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl


def ratio_form(trans, ref, tau_ref, tex):
    """tau_main of `trans` from tau_main of the reference transition `ref` of the same spectrum, the device's way
    (lte_band_kernel): tau_ref k exp(-de / tex) expm1(-t0 / tex) / expm1(-t0_ref / tex), numpy doubles."""
    (nu, e, g, a), (nu0, e0, g0, a0) = trans, ref
    t0, t00 = np.float64(H * nu / KB), np.float64(H * nu0 / KB)
    de = (np.float64(e) - t0) - (np.float64(e0) - t00)
    k = (np.float64(g) * a / (np.float64(nu) * nu * nu)) / (np.float64(g0) * a0 / (np.float64(nu0) * nu0 * nu0))
    tex = np.float64(tex)
    q = de / tex
    r = np.float64(np.longdouble(de) - np.longdouble(q) * np.longdouble(tex))      # the division's remainder (the device: one fma)
    return tau_ref * k * (np.exp(-q) * (1.0 - r / tex)) * np.expm1(-t0 / tex) / np.expm1(-t00 / tex)
