"""A numpy restatement of the reference's c_hf_predict (nestfit/models/hyperfine.pyx:52-118) for ANY line table, as
c_nnhp_predict calls it (diazenylium.pyx:138-154: voff, tex, ltau, sigm per component, parameter-major).  The oracle has
no custom tables; this is assembled only from pieces the oracle pins -- its FastExp (`nfo.fast_expn`), its 1/(e^x - 1)
table (`nfo.iemtex_interp`), its background term (`tbg_arr` of an oracle spectrum on the same axis) -- and the window
arithmetic of oracle/nf_oracle.c:270-325, operation by operation in IEEE doubles.  Fed the N2H+ tables it equals
`nfo.nnhp_predict` bit for bit (tests/test_hyperfine_cpu.py checks that first)."""
import math

import numpy as np

# csrc/nh3_data.h
CKMS = 299792.458
H = 6.62607015e-27
KB = 1.380649e-16


def tbg_of(nfo, xarr):
    """1 / expm1(h nu / (k T_cmb)) per channel, from the oracle."""
    return nfo.Spectrum(xarr, np.zeros(xarr.size), 1.0, rest_freq=float(xarr[0])).tbg_arr


def hf_windows(xarr, table, voff, sigm):
    """(lo, hi) of every line of `table` = (nu, voff[], tau_wts[]); -1, -1 for a skipped line (nf_oracle.c:270-296)."""
    nu0, tv, _ = table
    n, nu_min, nu_chan = xarr.size, float(xarr[0]), float(xarr[1] - xarr[0])
    lo, hi = np.full(len(tv), -1, dtype=np.int64), np.full(len(tv), -1, dtype=np.int64)
    for i, v in enumerate(tv):
        hf_freq = (1.0 - float(v) / CKMS) * nu0
        hf_width = sigm / CKMS * hf_freq
        hf_offset = voff / CKMS * hf_freq
        hf_nucen = hf_freq - hf_offset
        hf_idenom = 0.5 / (hf_width * hf_width)
        nu_cutoff = math.sqrt(12.5 / hf_idenom)
        a = math.floor((hf_nucen - nu_min - nu_cutoff) / nu_chan)
        b = math.floor((hf_nucen - nu_min + nu_cutoff) / nu_chan)
        if b < 0 or a > n - 1:
            continue
        lo[i], hi[i] = max(a, 0), min(b, n - 1)
    return lo, hi


def hf_predict(nfo, xarr, tbg, table, params):
    """The model spectrum of parameter-major `params` on `xarr` for `table` = (nu, voff[], tau_wts[])."""
    xarr = np.ascontiguousarray(xarr, dtype=np.float64)
    nu0, tv, tw = table
    params = np.asarray(params, dtype=np.float64)
    ncomp = params.size // 4
    pred = np.zeros(xarr.size)
    for c in range(ncomp):
        voff, tex, ltau, sigm = (float(params[k * ncomp + c]) for k in range(4))
        tau_main = math.pow(10.0, ltau)
        tarr = np.zeros(xarr.size)
        lo, hi = hf_windows(xarr, table, voff, sigm)
        for i, v in enumerate(tv):
            if lo[i] < 0:
                continue
            hf_freq = (1.0 - float(v) / CKMS) * nu0
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


def loglike(data, pred, noise):
    """-sum (d - p)^2 / (2 sigma^2) of one spectrum (core.pyx:522-530)."""
    return -float(np.sum((data - pred) ** 2)) / (2.0 * noise * noise)


def table_of(lines):
    """(nu, voff, tau_wts) of a nestfit_amd.LineTable."""
    return lines.nu, np.array(lines.voff), np.array(lines.tau_wts)
