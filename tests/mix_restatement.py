"""A restatement of LTE mixes (include/nestfit_amd.h: nfa_specset_create_lte_mix) for the tests: the transitions of a spectrum
belong to K species that share voff, tex and sigm, parameters per component parameter-major

    voff, tex, lncol_0, sigm, lncol_1, ..., lncol_{K-1}

and transition g of species k has tests/lte_restatement.tau_main on ITS OWN species' partition table and column density
-- the direct formula, not the ratio to a reference transition the device forms.  Everything after that is
tests/band_restatement.band_predict's loop over all the lines of the spectrum.

The test species: band_restatement's symmetric top, K = 0..3 of J = 5 - 4, as species 0 (tests/test_lte_bands_cpu.py); an
"isotopologue" from the same closed forms with a rotation constant B smaller by 4.2 km/s / c, K = 0..2, whose ladder so lies
4.2 km/s to the red of the main one (4.2, 6.7 and 14.2 km/s from the main K = 0; the main K = 1 at 2.5 km/s), with its
partition function on another temperature grid of another length; and two made-up species of one single-line transition
each for the sets of four."""
import numpy as np

import band_restatement as br
import hf_restatement as hfr
import lte_restatement as lr
from test_lte_bands_cpu import A_ROT, B_ROT, D_JK, J_LOW, MU, top_species

CKMS, H, KB = lr.CKMS, lr.H, lr.KB
ISO_SHIFT = 4.2                                  # km/s
B_ISO = B_ROT * (1.0 - ISO_SHIFT / CKMS)


def iso_species(na, n_q=21, t_lo=4.0, t_hi=75.0, name='iso'):
    """(molecule, [K = 0, 1, 2 as one line each]) of the isotopologue."""
    temps = np.geomspace(t_lo, t_hi, n_q)
    mol = na.Molecule(name, temps, br.top_partition(A_ROT, B_ISO, temps))
    return mol, [mol.transition(*br.top_transition(A_ROT, B_ISO, D_JK, MU, J_LOW, K), name=f'iso K={K}') for K in range(3)]


def made_up_species(na, nu0):
    """Two further species of one single-line transition each, 17 and 30 km/s to the red of nu0: Q = a T^1.5 on six
    temperatures, and on the two a table needs at least."""
    a_ul = br.top_transition(A_ROT, B_ROT, D_JK, MU, J_LOW, 0)[3]
    t3 = np.geomspace(6.0, 50.0, 6)
    m3 = na.Molecule('third', t3, 0.9 * t3 ** 1.5)
    m4 = na.Molecule('fourth', [8.0, 40.0], [30.0, 30.0 * 5.0 ** 1.5])
    return ((m3, m3.transition(nu0 * (1.0 - 17.0 / CKMS), 12.0, 5.0, 1.5 * a_ul, name='third')),
            (m4, m4.transition(nu0 * (1.0 - 30.0 / CKMS), 25.0, 7.0, 0.7 * a_ul, name='fourth')))


def test_species(na):
    """(top, its K = 0..3, iso, its K = 0..2)."""
    mol, ks = top_species(na)
    iso, isos = iso_species(na)
    return mol, ks, iso, isos


def lncol_of(params, n_species, ncomp, c, k):
    return float(params[(2 if k == 0 else 3 + k) * ncomp + c])


def mix_predict(nfo, xarr, tbg, lines, species, params):
    """Model spectrum of parameter-major `params` (3 + K per component) on `xarr` for all the transitions of `lines` (an
    LteLines, LteBand or LteBlend of the molecules `species`)."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    species = list(species)
    parts = [(species.index(t.molecule), t.molecule, tr, tv, tw)
             for t, (tr, tv, tw) in zip(lines.transitions if hasattr(lines, 'transitions') else (lines,), br.transitions_of(lines))]
    params = np.asarray(params, dtype=np.float64)
    K = len(species)
    ncomp = params.size // (3 + K)
    pred = np.zeros(xarr.size)
    for c in range(ncomp):
        voff, tex, sigm = float(params[c]), float(params[ncomp + c]), float(params[3 * ncomp + c])
        tarr = np.zeros(xarr.size)
        for k, mol, trans, tv, tw in parts:
            nu_g = trans[0]
            tau_main = br.band_tau_main(trans, mol.q_temp, mol.q_val, tex, lncol_of(params, K, ncomp, c, k), sigm)
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


def restated(nfo, rows, species, theta, tbgs=None):
    """(spectra of the rows [xarr, data, noise, lines] concatenated, lnL) for one parameter vector."""
    tbgs = tbgs or [hfr.tbg_of(nfo, x) for x, *_ in rows]
    preds = [mix_predict(nfo, x, tbg, tab, species, theta) for (x, _, _, tab), tbg in zip(rows, tbgs)]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl


def mixed_ratio_form(trans, mol, ref, mol0, tex, lncol, lncol0, sigm, is_ref=False):
    """tau_main of `trans` of species `mol` at column `lncol` the device's way (lte_mix_kernel), numpy doubles: the set-up
    stage's value for the reference transition `ref` AS A TRANSITION OF SPECIES 0 (`mol0`, `lncol0`), the band's ratio
    (none for the reference transition itself), and for another species than 0 the factor
    10^(lncol - lncol0) exp(ln Q_0(tex) - ln Q(tex))."""
    tau_ref = lr.tau_main(ref, mol0.q_temp, mol0.q_val, float(tex), lncol0, sigm)
    out = np.float64(tau_ref) if is_ref else br.ratio_form(trans, ref, tau_ref, tex)
    if mol is not mol0:
        dq = np.float64(lr.ln_partition(mol0.q_temp, mol0.q_val, float(tex))) - np.float64(lr.ln_partition(mol.q_temp, mol.q_val, float(tex)))
        out = out * np.float64(10.0) ** (np.float64(lncol) - np.float64(lncol0)) * np.exp(dq)
    return out


def tau_main_extended(trans, mol, tex, lncol, sigm):
    """lte_restatement.tau_main -- the direct formula -- evaluated in numpy's extended precision (64 mantissa bits on x86) on
    the table as the engine holds it (ln T, ln Q and the slopes in doubles): the reference where the doubles' own
    evaluation is not exact enough to be one.  At tex = 0.165 K, E_u / tex = 550, the double evaluation is 4.9e-14 off."""
    L = np.longdouble
    nu, e_up, g_up, a_ul = (L(v) for v in trans)
    tex = L(tex)
    ln_t, ln_q = np.log(np.asarray(mol.q_temp)), np.log(np.asarray(mol.q_val))
    x = np.log(tex)
    k = 0
    while k < len(ln_t) - 2 and x >= ln_t[k + 1]:
        k += 1
    slope = (ln_q[k + 1] - ln_q[k]) / (ln_t[k + 1] - ln_t[k])
    lq = L(ln_q[k]) + L(slope) * (x - L(ln_t[k]))
    t0 = L(H) * nu / L(KB)
    n_u = L(10.0) ** L(lncol) * g_up * np.exp(-e_up / tex - lq)
    fracterm = L(lr.CCMS) * L(lr.CCMS) * a_ul / (8 * L(np.pi) * (nu * nu))
    widthterm = L(CKMS) / (L(sigm) * nu * np.sqrt(2 * L(np.pi)))
    return n_u * fracterm * np.expm1(t0 / tex) * widthterm
