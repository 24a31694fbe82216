"""Weighted posterior moments of model spectra on given spectra: the numpy twin of the arithmetic of
`nfa_runner_predict_moments` (csrc/nfa_moments.h).  The device forms these from spectra that never leave it;
here they are formed from spectra the caller already has -- the route of `postprocess.generate_posterior_profiles` with a
`predict_backend`, and what the tests compare the device against.

Segment g is the rows offsets[g] .. offsets[g + 1] - 1, with weights w_i >= 0.  The moments are taken about the
segment's row of largest weight i* (the first on ties), a row inside the bulk of the posterior as `NestedResult` takes
them for the parameters: with d_i = p_i - p_i*, S0 = sum w_i, S1 = sum w_i d_i and S2 = sum w_i d_i^2,

    mean = p_i* + S1 / S0,    std = sqrt(max(S2 / S0 - (S1 / S0)^2, 0)).

Raw second moments cancel where the posterior is tight: rows that differ by 1e-7 relative leave sum w p^2 / S0 - mean^2
with no correct digit in float64, while d is exact (the difference of two close doubles) and its moments keep theirs.
"""
from collections import namedtuple

import numpy as np

from ._model import signed_peak

PosteriorMoments = namedtuple('PosteriorMoments', 'mean std peak_mean peak_std total_mean total_std')
PosteriorMoments.__doc__ = """mean, std [n_seg, n_chan_tot] (None where the spectra were not asked for); peak_mean, peak_std,
total_mean, total_std [n_seg, n_spec]: the weighted mean and standard deviation, over every segment's rows, of the model
spectra and of the peak and the total of every spectrum."""


def moments_of(spectra, weights, offsets):
    """(mean, std), [n_seg, n_col] each, of the rows of spectra[rows, n_col] with weights[rows] (None: all ones) in the
    segments offsets[n_seg + 1].  A segment without rows or whose weights sum to 0 gives NaN, a segment of one row
    std = 0; rows of weight 0 are left out, whatever they hold.  Computed in the dtype of `spectra` (float64 unless the
    caller hands longdouble)."""
    spectra = np.asarray(spectra)
    if spectra.dtype != np.longdouble:
        spectra = spectra.astype(np.float64, copy=False)
    if spectra.ndim != 2:
        raise ValueError('spectra must be [rows, n_col]')
    dt = spectra.dtype
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets.ndim != 1 or offsets.size < 1 or offsets[0] != 0 or np.any(np.diff(offsets) < 0) or offsets[-1] != spectra.shape[0]:
        raise ValueError('offsets must start at 0, not decrease and end at the number of rows')
    w_all = np.ones(spectra.shape[0], dtype=dt) if weights is None else np.asarray(weights).astype(dt, copy=False)
    if w_all.shape != (spectra.shape[0],) or not np.all(np.isfinite(w_all)) or np.any(w_all < 0):
        raise ValueError('one finite weight >= 0 per row is required')
    n_seg = offsets.size - 1
    mean = np.full((n_seg, spectra.shape[1]), np.nan, dtype=dt)
    std = np.full((n_seg, spectra.shape[1]), np.nan, dtype=dt)
    for g in range(n_seg):
        w = w_all[offsets[g]:offsets[g + 1]]
        s0 = w.sum()
        if w.size == 0 or not s0 > 0:
            continue
        p = spectra[offsets[g]:offsets[g + 1]]
        ref = p[np.argmax(w)]                                # the first on ties
        keep = w > 0
        d = p[keep] - ref
        m1 = (w[keep, None] * d).sum(axis=0) / s0
        m2 = (w[keep, None] * d * d).sum(axis=0) / s0
        mean[g] = ref + m1
        std[g] = np.sqrt(np.maximum(m2 - m1 * m1, 0))
    return mean, std


def row_statistics_of(spectra, spec_offsets, signed=False):
    """(peak, total), [rows, n_spec] each, of spectra[rows, n_chan_tot] whose spectrum k is the channels spec_offsets[k] ..
    spec_offsets[k + 1] - 1: the rule of `CubeRunner.peak_and_integrated`.  peak: the NaN-ignoring maximum, or (signed: a
    set with a continuum) the signed value of largest magnitude (`signed_peak`); total: the NaN-ignoring sum."""
    spectra = np.asarray(spectra)
    top = signed_peak if signed else np.nanmax
    n_spec = len(spec_offsets) - 1
    if spectra.shape[0] == 0:
        return np.empty((0, n_spec)), np.empty((0, n_spec))
    peak = np.stack([top(spectra[:, spec_offsets[k]:spec_offsets[k + 1]], axis=1) for k in range(n_spec)], axis=1)
    total = np.stack([np.nansum(spectra[:, spec_offsets[k]:spec_offsets[k + 1]], axis=1) for k in range(n_spec)], axis=1)
    return peak, total


def posterior_moments_of(spectra, weights, offsets, spec_offsets, signed=False, want_spectra=True):
    """The record `CubeRunner.predict_moments` returns, from given spectra[rows, n_chan_tot]."""
    peak, total = row_statistics_of(spectra, spec_offsets, signed)
    pm, ps = moments_of(peak, weights, offsets)
    tm, ts = moments_of(total, weights, offsets)
    mean, std = moments_of(spectra, weights, offsets) if want_spectra else (None, None)
    return PosteriorMoments(mean, std, pm, ps, tm, ts)
