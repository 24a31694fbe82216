"""The likelihood with an uncertain noise level per spectrum, restated in numpy `longdouble` for the tests.

The true noise of spectrum s is t sigma_c with one unknown scale t; tau = 1 / t^2 ~ Gamma(shape a, rate a), a = 1 / (4 f^2)
for the fractional uncertainty f of the level.  With h = chi^2_s / (2 sigma_ref^2) and nu unmasked channels,

    lnL_s = -(a + nu / 2) log1p(h / a),        f = 0:  lnL_s = -h.

chi^2_s comes from the restatements that exist -- a plain weighted sum, tmpl_restatement (baseline and templates),
corr_restatement and resp_restatement (correlated noise, a channel response) -- imported, not edited; model spectra come
from the oracle and the other restatements, never from the device.
"""
import numpy as np

import resp_restatement as rr
import tmpl_restatement as tr

LD = np.longdouble


def shape(f):
    """a = 1 / (4 f^2), longdouble."""
    f = LD(f)
    return 1 / (4 * f * f)


def n_unmasked(noise, n):
    """nu: channels with a finite noise (a scalar noise: all n).  Channels only -- no rank of a baseline comes off."""
    return int(n) if np.ndim(noise) == 0 else int(np.isfinite(np.asarray(noise, dtype=np.float64)).sum())


def term(h, nu, f):
    """lnL_s of h (any shape), longdouble."""
    h = np.asarray(h, dtype=LD)
    if not f > 0:
        return -h
    a = shape(f)
    return -(a + LD(nu) / 2) * np.log1p(np.maximum(h, LD(0)) / a)


def slope(nu, f):
    """c / a = max over h >= 0 of |d lnL_s / d h| (1 for f = 0): what carries a bound on h over to lnL_s."""
    if not f > 0:
        return 1.0
    a = shape(f)
    return float((a + LD(nu) / 2) / a)


def half_chi2(row, preds, order=None, templates=None, rho=None, taps=None):
    """(h[B], M[B]) in longdouble of one spectrum's data row [axis, data, noise, ...] for model rows preds[B, n]: h = chi^2 / (2
    sigma_ref^2) as the set's kind forms it, and the kind's own magnitude M (tests/test_templates.py, test_correlation.py)."""
    preds = np.atleast_2d(np.asarray(preds, dtype=np.float64))
    d, noise = np.asarray(row[1], dtype=np.float64), row[2]
    if rho is not None or taps is not None:
        lnl, M = rr.lnl_rows(d, preds, noise, rr.IDENTITY if taps is None else taps, (0.0, 0.0) if rho is None else rho)
        return -np.asarray(lnl, dtype=LD), np.asarray(M, dtype=LD)
    chi2, ref = tr.chi2_min(d, preds, noise, order, templates)
    return chi2 / (2 * ref * ref), tr.magnitude(d, preds, noise)


def restate(rows, preds, f, order=None, templates=None, rho=None, taps=None):
    """(lnL[B], M[B], sum_s |lnL_s| [B], max_s c_s / a_s) as float64 of model rows preds[B, chan_tot] against the data rows, f one
    value per spectrum.  templates, rho, taps: None or one entry per spectrum."""
    preds = np.atleast_2d(preds)
    B = preds.shape[0]
    want, M, mag = np.zeros(B, dtype=LD), np.zeros(B, dtype=LD), np.zeros(B, dtype=LD)
    worst, at = 1.0, 0
    for k, row in enumerate(rows):
        n = np.size(row[0])
        h, m = half_chi2(row, preds[:, at:at + n], order, None if templates is None else templates[k],
                         None if rho is None else rho[k], None if taps is None else taps[k])
        at += n
        nu = n_unmasked(row[2], n)
        t = term(h, nu, f[k])
        want += t
        mag += np.abs(t)
        M += m
        worst = max(worst, slope(nu, f[k]))
    return want.astype(np.float64), M.astype(np.float64), mag.astype(np.float64), worst
