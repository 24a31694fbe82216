"""The host diagnostics of a runner -- fit_baseline, fit_templates, fit_gain, fit_noise, fit_outliers -- over ROWS, once for
the one-pixel runners and `CubeRunner`: numpy on given arrays, no device.

Every function takes data[B, chan_tot], noise ([B, n_spec], or [B, chan_tot] for a noise per channel, inf: masked), the model
rows spec[B, chan_tot], the set's `offsets` [n_spec + 1] and its `Options` record, and calls the one-spectrum host functions
of `_model` per (spectrum, row).  Model rows that come out of a spectra set with a channel response are the FILTERED model
(DESIGN 4.14), the ones of a spectrum's private one-spectrum set are not: `fit_noise`, the one diagnostic a response enters,
is told which (`filtered`), and filters only rows that are not."""
from collections import namedtuple

import numpy as np

from . import _model as host          # (the one-spectrum functions; `_model` holds the runners that call this module)

# one spectrum of one row: the slice of its channels, their data and model, its noise (a number, or one per channel), the
# channels' relative weights (`channel_weights`: 0 where masked) and the residual data - model (0 where masked)
Piece = namedtuple('Piece', 'k b sl data model noise weight resid')

# what a diagnostic needs of the options, and the ValueError of a runner without it
NEEDS = {
    'baseline': (('baseline_order', 'templates'), 'this runner has no baseline (baseline_order=None)'),
    'templates': (('templates',), 'this runner has no nuisance templates (templates=None)'),
    'gain': (('calibration',), 'this runner has no calibration uncertainty (calibration=None)'),
    'noise': (('noise_uncertainty',), 'this runner has no noise uncertainty (noise_uncertainty=None)'),
    'outliers': (('robust',), 'this runner has no robust likelihood (robust=None)'),
}


def require(which, options):
    """ValueError where the set of `options` has nothing for the diagnostic `which` to fit."""
    names, why = NEEDS[which]
    if all(getattr(options, name) is None for name in names):
        raise ValueError(why)


def pieces(data, noise, spec, offsets):
    """Every (spectrum, row) of the rows as a `Piece`, spectrum by spectrum."""
    data, noise, spec = (np.asarray(a, dtype=np.float64) for a in (data, noise, spec))
    per_channel = noise.shape[1] == spec.shape[1]            # (spectra have two channels and more: never n_spec)
    for k in range(len(offsets) - 1):
        sl = slice(int(offsets[k]), int(offsets[k + 1]))
        for b in range(spec.shape[0]):
            sigma = noise[b, sl] if per_channel else noise[b, k]
            w = host.channel_weights(sigma, sl.stop - sl.start)
            yield Piece(k, b, sl, data[b, sl], spec[b, sl], sigma, w, np.where(w > 0, data[b, sl] - spec[b, sl], 0.0))


def _of(values, k):
    return None if values is None else values[k]


def _nuisance(data, noise, spec, offsets, options):
    """(curves [B, chan_tot], amplitudes: per spectrum [B, T]) of the baseline and the templates on data - spec."""
    tmpl = options.templates
    curves = np.empty(np.shape(spec))
    amps = [np.zeros((len(curves), 0 if _of(tmpl, k) is None else tmpl[k].shape[0])) for k in range(len(offsets) - 1)]
    for p in pieces(data, noise, spec, offsets):
        if tmpl is None:
            curves[p.b, p.sl] = host.baseline_fit(p.resid, p.weight, options.baseline_order)
        else:
            curves[p.b, p.sl], amps[p.k][p.b] = host.nuisance_fit(p.resid, p.weight, options.baseline_order, tmpl[p.k])
    return curves, amps


def fit_baseline(data, noise, spec, offsets, options):
    """Best-fit baselines [B, chan_tot] (`baseline_fit`); with templates the whole nuisance curve, polynomial and templates
    (`nuisance_fit`)."""
    return _nuisance(data, noise, spec, offsets, options)[0]


def fit_templates(data, noise, spec, offsets, options):
    """Best-fit amplitudes of the templates in the caller's scaling: per spectrum [B, T] (`nuisance_fit`)."""
    return _nuisance(data, noise, spec, offsets, options)[1]


def _per_spectrum(rows, n_spec):
    return np.ones((rows, n_spec)), np.zeros((rows, n_spec))


def fit_gain(data, noise, spec, offsets, options):
    """Posterior mean and standard deviation [B, n_spec] each of the spectra's gains (`gain_fit`)."""
    mean, std = _per_spectrum(len(spec), len(offsets) - 1)
    for p in pieces(data, noise, spec, offsets):
        sigma = 1.0 if np.ndim(p.noise) else p.noise          # (channel_weights: 1 / sigma_c^2, or ones)
        mean[p.b, p.k], std[p.b, p.k] = host.gain_fit(p.data, p.model, p.weight, sigma, options.calibration[p.k],
                                                      options.baseline_order)
    return mean, std


def fit_noise(data, noise, spec, offsets, options, *, filtered):
    """Posterior mean and standard deviation [B, n_spec] each of the spectra's noise scales (`half_chi2` as the set forms
    it, `noise_fit`).  filtered: whether `spec` is already the model behind the set's channel response."""
    mean, std = _per_spectrum(len(spec), len(offsets) - 1)
    resp = None if filtered else options.response
    for p in pieces(data, noise, spec, offsets):
        h, nu = host.half_chi2(p.data, p.model, p.noise, options.baseline_order, _of(options.templates, p.k),
                               _of(options.correlation, p.k), _of(resp, p.k))
        mean[p.b, p.k], std[p.b, p.k] = host.noise_fit(h, nu, options.noise_uncertainty[p.k])
    return mean, std


def fit_outliers(data, noise, spec, offsets, options):
    """Every channel's posterior mean precision factor [B, chan_tot] (`robust_outliers`)."""
    out = np.empty(np.shape(spec))
    for p in pieces(data, noise, spec, offsets):
        out[p.b, p.sl] = host.robust_outliers(p.data, p.model, p.noise, options.robust[p.k])
    return out
