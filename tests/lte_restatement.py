"""A restatement of the LTE model (include/nestfit_amd.h: nfa_specset_create_lte) with `math` in doubles, for the tests:

    T0_s       = h nu_s / k
    ln Q(T)    linear in ln T between the bracketing entries of the table; outside it the end segment's line continues
    N_u        = 10^lncol g_s exp(-E_s / tex) / Q(tex)
    tau_main_s = N_u c^2 A_s / (8 pi nu_s^2) expm1(T0_s / tex) CKMS / (sigm nu_s sqrt(2 pi))

and then tests/hf_restatement.hf_predict per spectrum with ltau = log10(tau_main_s) of every component.  The test
species is a rigid linear rotor made here from a rotation constant B (Hz) and a dipole moment mu (esu cm), everything
from closed forms:  nu_J = 2B(J+1),  E_u = hB(J+1)(J+2)/k,  g_u = 2J+3,  A = 64 pi^4 nu^3 mu^2 (J+1) / (3 h c^3 (2J+3)),
Q(T) = sum_J (2J+1) exp(-hBJ(J+1)/kT)."""
import math

import numpy as np

import hf_restatement as hfr

# csrc/nh3_data.h
CKMS = hfr.CKMS
H = hfr.H
KB = hfr.KB
CCMS = 29979245800.0


def rotor_transition(B, mu, J):
    """(nu, e_up, g_up, a_ul) of J+1 -> J."""
    nu = 2.0 * B * (J + 1)
    e_up = H * B * (J + 1) * (J + 2) / KB
    g_up = 2.0 * J + 3.0
    a_ul = 64.0 * math.pi ** 4 * nu ** 3 * mu ** 2 * (J + 1) / (3.0 * H * CCMS ** 3 * (2 * J + 3))
    return nu, e_up, g_up, a_ul


def rotor_partition(B, temps):
    """Q at every temperature of `temps`: the direct sum (to J = 400: converged to the last bit below 1000 K for B > 1 GHz)."""
    return np.array([sum((2 * J + 1) * math.exp(-H * B * J * (J + 1) / (KB * T)) for J in range(400)) for T in temps])


def ln_partition(q_temp, q_val, temp):
    """ln Q(temp) of the table: NaN for a temperature that is not an ordinary positive number."""
    if not (temp > 0 and math.isfinite(temp)):
        return math.nan
    ln_t = [math.log(t) for t in q_temp]
    ln_q = [math.log(q) for q in q_val]
    x = math.log(temp)
    k = 0
    while k < len(ln_t) - 2 and x >= ln_t[k + 1]:
        k += 1
    slope = (ln_q[k + 1] - ln_q[k]) / (ln_t[k + 1] - ln_t[k])
    return ln_q[k] + slope * (x - ln_t[k])


def tau_main(trans, q_temp, q_val, tex, lncol, sigm):
    """Peak optical depth of `trans` = (nu, e_up, g_up, a_ul) summed over its lines."""
    nu, e_up, g_up, a_ul = trans
    ln_q = ln_partition(q_temp, q_val, tex)
    if math.isnan(ln_q):
        return math.nan
    t0 = H * nu / KB
    n_u = math.pow(10.0, lncol) * g_up * math.exp(-e_up / tex) / math.exp(ln_q)
    fracterm = CCMS * CCMS * a_ul / (8 * math.pi * (nu * nu))
    widthterm = CKMS / (sigm * nu * math.sqrt(2 * math.pi))
    return n_u * fracterm * math.expm1(t0 / tex) * widthterm


def ltau_params(trans, q_temp, q_val, params):
    """Parameter-major (voff, tex, lncol, sigm) of every component -> (voff, tex, log10 tau_main, sigm) for `trans`."""
    params = np.array(params, dtype=np.float64)
    ncomp = params.size // 4
    for c in range(ncomp):
        tau = tau_main(trans, q_temp, q_val, float(params[ncomp + c]), float(params[2 * ncomp + c]), float(params[3 * ncomp + c]))
        params[2 * ncomp + c] = math.log10(tau) if tau > 0 else math.nan
    return params


def lte_predict(nfo, xarr, tbg, lines, params):
    """Model spectrum of parameter-major `params` on `xarr` for one transition, `lines` a nestfit_amd.LteLines (read
    for its numbers only)."""
    mol = lines.molecule
    trans = (lines.nu, lines.e_up, lines.g_up, lines.a_ul)
    return hfr.hf_predict(nfo, xarr, tbg, hfr.table_of(lines), ltau_params(trans, mol.q_temp, mol.q_val, params))


def restated(nfo, rows, theta):
    """(spectra of the rows [xarr, data, noise, LteLines] concatenated, lnL) for one parameter vector."""
    preds = [lte_predict(nfo, x, hfr.tbg_of(nfo, x), tab, theta) for x, _, _, tab in rows]
    lnl = sum(hfr.loglike(d, p, noise) for (_, d, noise, _), p in zip(rows, preds))
    return np.concatenate(preds), lnl


def axis(nu, n, vhalf):
    return nu * (1.0 - np.linspace(vhalf, -vhalf, n) / CKMS)
