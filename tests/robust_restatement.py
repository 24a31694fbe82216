"""The robust likelihood restated: Student-t channel noise with nu degrees of freedom and scale sigma_j per
channel, as the direct sum

    lnL_s = -(nu + 1) / 2 sum_j log1p((d_j - p_j)^2 / (nu sigma_j^2))

over the unmasked channels in numpy `longdouble` -- no g, no difference form, no reference noise.  nu = 0: the Gaussian
-sum (d - p)^2 / (2 sigma^2).  Nothing here is shared with nestfit_amd.
"""
import numpy as np

LD = np.longdouble


def _sigma(noise, n):
    sig = np.broadcast_to(np.asarray(noise, dtype=LD), (n,))
    return sig, np.isfinite(sig)


def lnl_spectrum(d, p, noise, nu):
    """lnL of model rows p[B, n] (or one row [n]) against the data d[n] of ONE spectrum; noise: a scalar or one value per
    channel (inf: masked).  longdouble [B]."""
    d, p = np.asarray(d, dtype=LD), np.atleast_2d(np.asarray(p, dtype=LD))
    sig, live = _sigma(noise, d.size)
    z = np.where(live, (np.where(live, d, 0) - p) / np.where(live, sig, 1), LD(0))
    if nu == 0:
        return -np.sum(z * z, axis=1) / LD(2)
    nu = LD(nu)
    return -(nu + LD(1)) / LD(2) * np.sum(np.log1p(z * z / nu), axis=1)


def magnitude_spectrum(d, p, noise, nu):
    """M of ONE spectrum, the scale the deviations of the device's difference form are measured against:
        (nu + 1) / 2 sum_j [log1p(a d^2) + g (p^2 + 2 |d p|) max(1, 1 / (1 + t))],
    a = 1 / (nu sigma_j^2), g = a / (1 + a d^2), t = p (g p - 2 g d); nu = 0: the Gaussian sum (d^2 + 2 |d p| + p^2) / (2 sigma^2).
    longdouble [B]."""
    d, p = np.asarray(d, dtype=LD), np.atleast_2d(np.asarray(p, dtype=LD))
    sig, live = _sigma(noise, d.size)
    d = np.where(live, d, LD(0))
    inv = np.where(live, LD(1) / np.where(live, sig, 1) ** 2, LD(0))
    if nu == 0:
        return np.sum(inv * (d * d + 2 * np.abs(d * p) + p * p), axis=1) / LD(2)
    nu = LD(nu)
    a = inv / nu
    g = a / (1 + a * d * d)
    t = p * (g * p - 2 * g * d)
    return (nu + 1) / 2 * np.sum(np.log1p(a * d * d) + g * (p * p + 2 * np.abs(d * p)) * np.maximum(LD(1), 1 / (1 + t)), axis=1)


def _nus(nu, n_spec):
    return [nu] * n_spec if np.ndim(nu) == 0 else list(nu)


def restate(rows, preds, nu):
    """(lnL, M) as float64 [B] of model rows preds[B, chan_tot] against the data rows [axis, data, noise, what]; nu: one
    number for all spectra or one per spectrum."""
    preds = np.atleast_2d(preds)
    want, M = np.zeros(preds.shape[0], dtype=LD), np.zeros(preds.shape[0], dtype=LD)
    at = 0
    for (x, d, noise, *_), v in zip(rows, _nus(nu, len(rows))):
        p = preds[:, at:at + x.size]
        at += x.size
        want += lnl_spectrum(d, p, noise, v)
        M += magnitude_spectrum(d, p, noise, v)
    return want.astype(np.float64), M.astype(np.float64)


def spiked_line(seed, n=300, sigma=0.2, peak=1.0, centre=150.0, width=3.0, spikes=((153, 12.0), (155, 9.0))):
    """The science case: (channels, data, clean) of a Gaussian line of `peak` and `width` channels at `centre` in noise of
    `sigma`, with spikes [(channel, height in sigma)] added; `spikes=()` for clean data."""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.float64)
    clean = peak * np.exp(-0.5 * ((j - centre) / width) ** 2)
    data = clean + rng.normal(0, sigma, n)
    for c, h in spikes:
        data[c] += h * sigma
    return j, data, clean


def grid_fit(data, sigma, nu, peaks, centres, width=3.0):
    """(peak, centre) that maximise the restated lnL on the grid, and the lnL grid [peaks, centres] as float64."""
    j = np.arange(data.size, dtype=np.float64)
    lnl = np.empty((len(peaks), len(centres)))
    for k, c in enumerate(centres):
        shape = np.exp(-0.5 * ((j - c) / width) ** 2)
        lnl[:, k] = lnl_spectrum(data, np.outer(peaks, shape), sigma, nu).astype(np.float64)
    a, b = np.unravel_index(int(np.argmax(lnl)), lnl.shape)
    return float(peaks[a]), float(centres[b]), lnl
