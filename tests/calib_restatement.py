"""The gain-marginalised likelihood of one spectrum, restated with numpy in `longdouble`.

The data are d = g p + baseline + noise with a gain g ~ N(1, s^2).  With the weighted products of the baseline-projected
vectors, each over sigma^2,

    a = <p,p>_P / sigma^2        b = <d,p>_P / sigma^2        c = <d,d>_P / sigma^2        lambda = 1 / s^2

the integral over g of exp(-(c - 2 g b + g^2 a) / 2) N(g; 1, s^2) is, unsimplified,

    lnL = -[c + lambda - (b + lambda)^2 / (a + lambda)] / 2 - ln((a + lambda) / lambda) / 2

and for s = 0 the plain -(c - 2 b + a) / 2.  The kernel computes a rearrangement of this about g = 1 (chi^2_1, B - A, log1p);
nothing of that is shared here.  The baseline projection is a weighted least-squares fit of Legendre polynomials
(numpy.polynomial.legendre and numpy.linalg.lstsq, one step of refinement in longdouble), not nestfit_amd's `baseline_fit`.

`pred` comes from the other restatements (hf_restatement, layer_restatement, mix_restatement, the oracle), never from the device.
"""
import numpy as np
from numpy.polynomial import legendre

LD = np.longdouble


def weights_of(noise, size):
    """(w[size], sigma) of a scalar noise (ones, the noise) or of a noise per channel (1 / sigma_c^2, 0 where it is inf, and 1)."""
    if np.ndim(noise) == 0:
        return np.ones(size, dtype=LD), LD(noise)
    noise = np.asarray(noise, dtype=LD)
    w = np.zeros(size, dtype=LD)
    live = np.isfinite(noise)
    w[live] = 1 / noise[live] ** 2
    return w, LD(1)


def project_out(x, w, order):
    """x less its weighted least-squares polynomial of degree <= order over the channels of weight > 0 (0 elsewhere); with n <=
    order such channels the degree is n - 1.  order None: x on those channels."""
    x = np.asarray(x, dtype=LD)
    live = w > 0
    out = np.where(live, x, LD(0))
    if order is None or not live.any():
        return out
    n = x.size
    u = (2.0 * np.arange(n) - (n - 1)) / (n - 1) if n > 1 else np.zeros(n)
    k = min(int(order), int(live.sum()) - 1)
    V = legendre.legvander(u, k)
    sw = np.sqrt(w[live]).astype(np.float64)
    A = V[live] * sw[:, None]
    for _ in range(2):                                    # the fit, then the fit of what it left (the solve itself is float64)
        coef = np.linalg.lstsq(A, (out[live] * sw).astype(np.float64), rcond=None)[0]
        out[live] = out[live] - V[live].astype(LD) @ coef.astype(LD)
    return out


def products(data, pred, noise, baseline_order=None):
    """(a, b, c) above, longdouble."""
    pred = np.asarray(pred, dtype=LD)
    w, sigma = weights_of(noise, pred.size)
    d, p = project_out(data, w, baseline_order), project_out(pred, w, baseline_order)
    s2 = sigma * sigma
    return np.sum(w * p * p) / s2, np.sum(w * d * p) / s2, np.sum(w * d * d) / s2


def marginal_lnl(data, pred, noise, cal, baseline_order=None):
    """lnL of one spectrum with the gain integrated out; cal = s, the fractional 1-sigma calibration uncertainty."""
    a, b, c = products(data, pred, noise, baseline_order)
    if cal == 0:
        return -(c - 2 * b + a) / 2
    lam = 1 / (LD(cal) * LD(cal))
    return -(c + lam - (b + lam) ** 2 / (a + lam)) / 2 - np.log((a + lam) / lam) / 2


def magnitude(data, pred, noise, cal, baseline_order=None):
    """M of tests/test_calibration.py: the size of the terms lnL is a difference of, (C + 2 |B| + A) / (2 sigma^2) + log1p(s^2 A /
    sigma^2) / 2."""
    a, b, c = products(data, pred, noise, baseline_order)
    return (c + 2 * abs(b) + a) / 2 + np.log1p(LD(cal) ** 2 * a) / 2


def gain_posterior(data, pred, noise, cal, baseline_order=None):
    """(mean, standard deviation) of g at the given model: N((b + lambda) / (a + lambda), 1 / (a + lambda)); (1, 0) for s = 0."""
    if cal == 0:
        return LD(1), LD(0)
    a, b, _ = products(data, pred, noise, baseline_order)
    lam = 1 / (LD(cal) * LD(cal))
    return (b + lam) / (a + lam), 1 / np.sqrt(a + lam)
