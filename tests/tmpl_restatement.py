"""Restatement of the likelihood with nuisance templates in numpy `longdouble`, for the tests.

Per spectrum: channel weights w (1 for a scalar noise, (sigma_ref / sigma_c)^2 for a noise per channel, 0 where masked), the
Legendre polynomials P_0..P_K of u = (2 j - (N - 1)) / (N - 1) (K = -1: none) and the templates t_1..t_T; chi2_min = min over
b in span{P, t} of sum w (r - b)^2, r = d - p, and lnL = -sum_s chi2_min,s / (2 sigma_ref,s^2).

It is a weighted least-squares problem solved by QR -- modified Gram-Schmidt on the columns sqrt(w) phi_k in the order P_0..P_K,
t_1..t_T, with the rank rule of DESIGN 4.5: a column whose squared norm after the projections is <= 1e-12 of its squared norm
before them is dropped -- and chi2_min is the squared norm of what is left of sqrt(w) r.  No moments, no Gram matrix, no
Cholesky factor: nothing of the kernel's form.
"""
import numpy as np

LD = np.longdouble
PIVOT = LD(1e-12)


def weights(noise, n):
    """(w[n], sigma_ref) of a spectrum's noise: a scalar, or one value per channel (inf: masked)."""
    if np.ndim(noise) == 0:
        return np.ones(n, dtype=LD), LD(float(noise))
    noise = np.asarray(noise, dtype=np.float64)
    ref = noise[np.isfinite(noise)].min() if np.isfinite(noise).any() else 1.0
    w = np.where(np.isfinite(noise), (LD(ref) / noise.astype(LD)) ** 2, LD(0))
    return w.astype(LD), LD(ref)


def legendre(n, order):
    """P_0..P_order at the n channels by the recurrence, longdouble [order + 1, n] ([0, n] for order None or -1)."""
    order = -1 if order is None else int(order)
    u = (2 * np.arange(n, dtype=LD) - (n - 1)) / LD(n - 1) if n > 1 else np.zeros(n, dtype=LD)
    rows = []
    for k in range(order + 1):
        rows.append(np.ones(n, dtype=LD) if k == 0 else u if k == 1 else ((2 * k - 1) * u * rows[k - 1] - (k - 1) * rows[k - 2]) / LD(k))
    return np.array(rows, dtype=LD).reshape(order + 1, n)


def columns(n, order, templates):
    """The basis functions [K + 1 + T, n]: the polynomials, then the templates each scaled to max |t| = 1."""
    P = legendre(n, order)
    if templates is None or len(templates) == 0:
        return P
    t = np.asarray(templates, dtype=np.float64).reshape(-1, n).astype(LD)
    return np.concatenate([P, t / np.max(np.abs(t), axis=1, keepdims=True)])


def orthonormal(n, w, order, templates):
    """The kept directions as orthonormal rows q[rank, n] of the weighted columns (modified Gram-Schmidt, the rank rule)."""
    sw = np.sqrt(np.asarray(w, dtype=LD))
    q = []
    for phi in columns(n, order, templates):
        v = sw * phi
        before = v @ v
        for e in q:
            v = v - (e @ v) * e
        for e in q:                                           # (a second pass: orthogonal to longdouble's rounding)
            v = v - (e @ v) * e
        d = v @ v
        if d > PIVOT * before:
            q.append(v / np.sqrt(d))
    return np.array(q, dtype=LD).reshape(len(q), n)


def chi2_min(data, pred, noise, order, templates):
    """chi2_min of one spectrum for model rows pred[B, n] (or [n]), and sigma_ref: longdouble."""
    pred = np.atleast_2d(np.asarray(pred, dtype=np.float64)).astype(LD)
    n = pred.shape[1]
    w, ref = weights(noise, n)
    d = np.where(w > 0, np.asarray(data, dtype=np.float64), 0.0).astype(LD)
    r = np.sqrt(w) * (d[None, :] - pred)
    q = orthonormal(n, w, order, templates)
    for e in q:
        r = r - np.outer(r @ e, e)
    return np.sum(r * r, axis=1), ref


def magnitude(data, pred, noise):
    """M of one spectrum: (sum w d^2 + 2 sum w |d| |p| + sum w p^2) / (2 sigma_ref^2), per model row."""
    pred = np.atleast_2d(np.asarray(pred, dtype=np.float64)).astype(LD)
    n = pred.shape[1]
    w, ref = weights(noise, n)
    d = np.abs(np.where(w > 0, np.asarray(data, dtype=np.float64), 0.0).astype(LD))
    p = np.abs(pred)
    return (np.sum(w * d * d) + 2 * (p @ (w * d)) + np.sum(w * p * p, axis=1)) / (2 * ref * ref)


def restate(rows, preds, order, templates):
    """(lnL[B], M[B]) as float64 of model rows preds[B, chan_tot] against the data rows [axis, data, noise, ...]; templates:
    None or one entry (None or [T, n]) per spectrum."""
    preds = np.atleast_2d(preds)
    want, M = np.zeros(preds.shape[0], dtype=LD), np.zeros(preds.shape[0], dtype=LD)
    at = 0
    for k, row in enumerate(rows):
        n = np.size(row[0])
        p = preds[:, at:at + n]
        at += n
        chi2, ref = chi2_min(row[1], p, row[2], order, None if templates is None else templates[k])
        want -= chi2 / (2 * ref * ref)
        M += magnitude(row[1], p, row[2])
    return want.astype(np.float64), M.astype(np.float64)


def gram_condition(n, noise, order, templates):
    """Condition number of the Gram matrix of the kept weighted columns, each normalised to unit length (float64): what the
    kernel's moment form loses against this file's QR.  1 for fewer than two kept directions."""
    w, _ = weights(noise, n)
    sw = np.sqrt(w)
    cols = columns(n, order, templates)
    kept, q = [], []
    for phi in cols:                                          # the same rank rule, remembering which columns stay
        v = sw * phi
        before = v @ v
        for _ in range(2):
            for e in q:
                v = v - (e @ v) * e
        d = v @ v
        if d > PIVOT * before:
            q.append(v / np.sqrt(d))
            kept.append(sw * phi / np.sqrt(before))
    if len(kept) < 2:
        return 1.0
    A = np.array(kept, dtype=np.float64)
    return float(np.linalg.cond(A @ A.T))
