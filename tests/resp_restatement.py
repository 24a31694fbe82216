"""The likelihood of one spectrum seen through a channel response, restated with numpy.

The spectrometer's response h = (h_-T .. h_0 .. h_T), T = 1 or 2, convolves the model before it meets the data:

    p~_j = sum_{k = -T..T} h_k p_{j+k},        p_i := 0 for i < 0 and i >= N,

and chi^2 = (d - p~)^T Q (d - p~), lnL = -chi^2 / (2 sigma_ref^2), with Q the dense inverse of corr_restatement's covariance
(white noise: rho = (0, 0)).  The filter is a plain loop over the taps in extended precision on a zero-padded copy; the
quadratic form is summed in extended precision too.  `p` comes from the other restatements and the oracle, never from the device.
"""
import numpy as np

import corr_restatement as cs

IDENTITY = (0.0, 1.0, 0.0)


def taps5(taps):
    """The taps as five, h_-2 .. h_2: three get zero ends."""
    h = np.asarray(taps, dtype=np.longdouble)
    assert h.ndim == 1 and h.size in (3, 5)
    return np.concatenate([[0], h, [0]]).astype(np.longdouble) if h.size == 3 else h


def filtered(p, taps):
    """p~[..., N] of p[..., N] in longdouble: sum_k h_k p_{j+k}, zero beyond the ends."""
    h = taps5(taps)
    p = np.asarray(p, dtype=np.longdouble)
    n = p.shape[-1]
    wide = np.zeros(p.shape[:-1] + (n + 4,), dtype=np.longdouble)
    wide[..., 2:n + 2] = p
    out = np.zeros(p.shape, dtype=np.longdouble)
    for k in range(-2, 3):
        out += h[k + 2] * wide[..., 2 + k:2 + k + n]
    return out


def filtered_scale(p, taps):
    """sum_k |h_k| |p_{j+k}|: the size of the terms p~_j is a sum of."""
    return filtered(np.abs(np.asarray(p, dtype=np.float64)), np.abs(np.asarray(taps, dtype=np.float64)))


def lnl(d, p, sigma, taps, rho=(0.0, 0.0)):
    """(lnL, M) of one spectrum in longdouble: lnL = -(d - p~)^T Q (d - p~) / 2 with Q = (S R S)^-1 (the sigma_ref^2 of the
    engine's Q cancels), and corr_restatement's magnitude M with p~ for p: (|d|^T |Q| |d| + 2 |d|^T |Q| |p~| + |p~|^T |Q| |p~|) / 2."""
    d = np.asarray(d, dtype=np.longdouble)
    pt = filtered(p, taps)
    Q = np.linalg.inv(cs.covariance(sigma, rho, d.size)).astype(np.longdouble)
    r = d - pt
    ad, ap, A = np.abs(d), np.abs(pt), np.abs(Q)
    return -(r @ Q @ r) / 2, (ad @ A @ ad + 2 * (ad @ A @ ap) + ap @ A @ ap) / 2


def _quad_rows(a, Q, b):
    """a_i^T Q b_i for the rows of a and b [B, N] in longdouble.  Q (float64, a dense inverse) is pentadiagonal but for the
    inversion's rounding: its five bands are summed in extended precision, what the inversion left outside them by BLAS."""
    n = Q.shape[0]
    out = np.zeros(a.shape[0], dtype=np.longdouble)
    rest = Q.copy()
    for k in range(-2, 3):
        band = np.diagonal(Q, k).astype(np.longdouble)
        lo, hi = max(0, -k), min(n, n - k)
        out += np.sum(a[:, lo:hi] * band[None, :] * b[:, lo + k:hi + k], axis=1)
        rest[np.arange(lo, hi), np.arange(lo + k, hi + k)] = 0.0
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return out + np.sum(a64 * (b64 @ rest.T), axis=1)


def lnl_rows(d, preds, sigma, taps, rho=(0.0, 0.0)):
    """`lnl` for model rows preds[B, N] against one spectrum, its Q formed once: (lnL[B], M[B]) in longdouble."""
    d = np.asarray(d, dtype=np.longdouble)
    pt = filtered(np.atleast_2d(preds), taps)
    Q = np.linalg.inv(cs.covariance(sigma, rho, d.size))
    r = d[None, :] - pt
    ad, ap, A = np.broadcast_to(np.abs(d), pt.shape), np.abs(pt), np.abs(Q)
    return -_quad_rows(r, Q, r) / 2, (_quad_rows(ad, A, ad) + 2 * _quad_rows(ad, A, ap) + _quad_rows(ap, A, ap)) / 2


# ---------------------------------------------------------------------------- the width bias (test_response_cpu.py, test_response.py)
# One Gaussian of sigma = 1 channel, centre off the channel grid, Hanning-smoothed, no noise, 128 channels; a grid of
# (peak, sigm) around the truth in steps of 0.02 of it.
BIAS_N, BIAS_CENTRE, BIAS_PEAK, BIAS_SIGM, BIAS_STEP = 128, 63.3, 1.0, 1.0, 0.02
BIAS_PEAKS = BIAS_PEAK * (30 + np.arange(31)) / 50.0                # 0.60 .. 1.20 of the truth, the truth itself exactly
BIAS_SIGMS = BIAS_SIGM * (40 + np.arange(41)) / 50.0                # 0.80 .. 1.60 of the truth
BIAS_TRUE = (20, 10)                                                 # the truth's place on the grid (peak, sigm)
HANNING_RESPONSE = (0.25, 0.5, 0.25)


def gaussian(peak, sigm, n=BIAS_N, centre=BIAS_CENTRE):
    j = np.arange(n, dtype=np.float64)
    return peak * np.exp(-0.5 * ((j - centre) / sigm) ** 2)


def bias_data():
    return np.asarray(filtered(gaussian(BIAS_PEAK, BIAS_SIGM), HANNING_RESPONSE), dtype=np.float64)


def bias_argmin(chi2):
    """(peak index, sigm index) of the smallest entry of chi2[peak, sigm]."""
    return tuple(int(i) for i in np.unravel_index(int(np.argmin(chi2)), chi2.shape))
