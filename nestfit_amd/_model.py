"""Engine-backed pieces shared by the model modules (ammonia, diazenylium, gaussian):
device-resident spectra, the runner handle and the reference's Spectrum / Runner
behaviour (nestfit/core/core.pyx:486-561) on top of the C ABI."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _calls, _diagnostics, _ffi
from ._options import (APPLY_ORDER, MODEL_GAUSSIAN, OPTION_NAMES, TMPL_MAX, Options, check_baseline_order, check_calibration,  # noqa: F401
                       check_continuum, check_correlation, check_layered, check_noise_uncertainty, check_options, check_response,
                       check_robust, check_templates, is_set, model_refusal, normalise, refusal, yule_walker)
from .core import Runner, _as_inplace_vector

MODEL_AMMONIA, MODEL_DIAZENYLIUM, MODEL_HYPERFINE, MODEL_LTE, MODEL_GRID = 0, 1, 3, 4, 5   # (MODEL_GAUSSIAN = 2: _options)
# parameters per component
N_MODEL = {MODEL_AMMONIA: 6, MODEL_DIAZENYLIUM: 4, MODEL_GAUSSIAN: 3, MODEL_HYPERFINE: 4, MODEL_LTE: 4, MODEL_GRID: 5}
TABLED_MODELS = (MODEL_HYPERFINE, MODEL_LTE, MODEL_GRID)   # the models whose spectra bring their line tables (`lines`)

HANNING = (2.0 / 3.0, 1.0 / 6.0)      # (rho_1, rho_2) of white noise smoothed with the Hanning kernel (1/4, 1/2, 1/4)


def ar1(rho):
    """The pair (rho, rho^2) of an AR(1) process: `correlation=ar1(0.5)`."""
    rho = float(rho)
    return (rho, rho * rho)


def corr_bands(rho1, rho2, n):
    """The three bands of R^-1, the inverse (exactly pentadiagonal) of the n x n correlation matrix of the AR(2) process
    with autocorrelations (rho1, rho2), n >= 4: the diagonal [n], the first [n - 1] and the second [n - 2] off-diagonal."""
    phi1, phi2, v = yule_walker(rho1, rho2)
    d0 = np.full(n, 1.0 + phi1 * phi1 + phi2 * phi2)
    d0[[1, n - 2]] = 1.0 + phi1 * phi1
    d0[[0, n - 1]] = 1.0
    d1 = np.full(n - 1, -phi1 * (1.0 - phi2))
    d1[[0, n - 2]] = -phi1
    return d0 / v, d1 / v, np.full(n - 2, -phi2) / v


def corr_lndet(rho1, rho2, n):
    """ln det R of that matrix: (n - 2) ln v + ln(1 - rho1^2)."""
    return (n - 2) * np.log(yule_walker(rho1, rho2)[2]) + np.log(1.0 - rho1 * rho1)


HANNING_RESPONSE = (0.25, 0.5, 0.25)  # the Hanning kernel as a channel response: `response=HANNING_RESPONSE`


def correlation_of_response(taps):
    """The pair (rho_1, rho_2) = (sum_j h_j h_{j+1}, sum_j h_j h_{j+2}) / sum_j h_j^2 that smoothing WHITE noise with the
    taps `h` (3 or 5 of them, one response) produces: `correlation=` beside `response=taps` for a cube whose signal and
    noise were smoothed together.  `correlation_of_response(HANNING_RESPONSE)` is `HANNING`."""
    h = np.asarray(taps, dtype=np.float64)
    if h.ndim != 1 or h.shape[0] not in (3, 5):
        raise ValueError(f'correlation_of_response takes one response of 3 or 5 taps, not {taps!r}')
    c0 = float(np.sum(h * h))
    return (float(np.sum(h[:-1] * h[1:])) / c0, float(np.sum(h[:-2] * h[2:])) / c0)


def smoothed(taps):
    """`{'response': taps, 'correlation': correlation_of_response(taps)}`: a cube smoothed with `taps` after the noise was
    white, to splat into a runner's `from_data` or a `CubeFitter`'s `runner_kwargs`."""
    return {'response': taps, 'correlation': correlation_of_response(taps)}


def ripple(n_chan, period, phase=None):
    """Templates of a standing wave of `period` channels (any real number > 0) on a spectrum of `n_chan` channels, for
    `templates=`: the rows sin(2 pi j / period) and cos(2 pi j / period), float64 [2, n_chan], whose two amplitudes stand for
    an unknown amplitude and phase; with a known `phase` (radians) the one row sin(2 pi j / period + phase), [1, n_chan].
    Several periods: `np.vstack` of several calls (at most 4 rows per spectrum)."""
    n_chan, period = int(n_chan), float(period)
    if n_chan < 1 or not (np.isfinite(period) and period > 0.0):
        raise ValueError(f'ripple: n_chan >= 1 and a finite period > 0 (in channels), not ({n_chan!r}, {period!r})')
    arg = 2.0 * np.pi * np.arange(n_chan, dtype=np.float64) / period
    if phase is None:
        return np.stack([np.sin(arg), np.cos(arg)])
    if not np.isfinite(float(phase)):
        raise ValueError(f'ripple: a finite phase (radians), not {phase!r}')
    return np.sin(arg + float(phase))[None, :]


def nuisance_fit(resid, weight, order, templates):
    """Best-fit nuisance curve of ONE residual spectrum resid[N] under channel weights weight[N] (0: masked) over the span of
    the Legendre polynomials of degree <= `order` (None: none) and the rows of templates[T, N] (None: none): weighted least
    squares with numpy (minimum norm where the span is degenerate).  Returns (curve[N], amplitudes[T] of the templates as
    given)."""
    resid, w = np.asarray(resid, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    n = resid.shape[-1]
    u = (2.0 * np.arange(n) - (n - 1)) / (n - 1) if n > 1 else np.zeros(n)
    cols = [] if order is None else [np.polynomial.legendre.legvander(u, int(order))]
    n_poly = 0 if order is None else int(order) + 1
    T = 0 if templates is None else len(templates)
    if T:
        cols.append(np.asarray(templates, dtype=np.float64).T)
    if not cols:
        return np.zeros(n), np.zeros(0)
    V = np.concatenate(cols, axis=1)
    live = w > 0
    if not live.any():
        return np.zeros(n), np.zeros(T)
    sw = np.sqrt(w[live])
    scale = np.maximum(np.max(np.abs(V), axis=0), 1e-300)    # (the caller's scaling must not enter the rank decision)
    coef = np.linalg.lstsq(V[live] / scale * sw[:, None], resid[live] * sw, rcond=None)[0] / scale
    return V @ coef, coef[n_poly:]


def spec_data_sizes_masked(spec_data):
    """(sizes, masked) of `from_data`'s rows [xarr, data, noise, ...] for `check_correlation`: the channels of every spectrum, and
    whether any channel noise masks a channel (inf).  numpy only."""
    sizes = [int(np.size(row[0])) for row in spec_data]
    masked = any(np.ndim(row[2]) > 0 and not np.all(np.isfinite(np.asarray(row[2], dtype=np.float64))) for row in spec_data)
    return sizes, masked


def _robust_a(noise, n, nu):
    """(a_j, sigma_ref) of one spectrum: a_j = w_j / (nu sigma_ref^2), w_j = (sigma_ref / sigma_j)^2, 0 where masked (inf)."""
    sig = np.broadcast_to(np.asarray(noise, dtype=np.float64), (n,))
    live = np.isfinite(sig)
    ref = float(np.min(sig[live])) if np.any(live) else 1.0
    w = np.where(live, (ref / np.where(live, sig, 1.0)) ** 2, 0.0)
    return w / (nu * (ref * ref)), ref


def robust_lnl(data, pred, noise, nu):
    """The log-likelihood of ONE spectrum under Student-t channel noise with `nu` degrees of freedom, in the form the engine
    takes: with a_j = w_j / (nu sigma_ref^2), g = a / (1 + a d^2) and t = p (g p - 2 g d),
    -(nu + 1) / 2 (sum_j log1p(a_j d_j^2) + sum_j log1p(t_j)).  `noise` is a scalar or one value per channel (inf: masked);
    nu = 0: the Gaussian -chi^2 / (2 sigma^2).  numpy on the host."""
    d, p = np.asarray(data, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    if not nu > 0.0:
        return -half_chi2(d, p, noise)[0]
    a, _ = _robust_a(noise, d.shape[0], float(nu))
    d = np.where(a > 0.0, d, 0.0)
    ad2 = a * d * d
    g = a / (1.0 + ad2)
    gd = g * d
    t = p * (g * p - 2.0 * gd)
    return float(-0.5 * (nu + 1.0) * (np.sum(np.log1p(ad2)) + np.sum(np.log1p(t))))


def robust_outliers(data, pred, noise, nu):
    """The posterior mean of every channel's precision factor under Student-t noise: (nu + 1) / (nu + r_j^2 /
    sigma_j^2), r = data - pred -- about 1 for a good channel, towards 0 for one the fit distrusted; 1 everywhere for nu = 0
    and NaN at a masked channel.  numpy on the host."""
    d, p = np.asarray(data, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    sig = np.broadcast_to(np.asarray(noise, dtype=np.float64), d.shape)
    live = np.isfinite(sig)
    if not nu > 0.0:
        return np.where(live, 1.0, np.nan)
    z = np.where(live, (d - p) / np.where(live, sig, 1.0), 0.0)
    return np.where(live, (nu + 1.0) / (nu + z * z), np.nan)


def robust_prefactor(noise, n, nu):
    """`Spectrum.prefactor` under Student-t channel noise: the sum over the unmasked channels of lgamma((nu + 1) / 2) -
    lgamma(nu / 2) - ln(nu pi sigma_j^2) / 2, the constant that -(nu + 1) / 2 sum log1p(a r^2) leaves out."""
    from math import lgamma, log, pi
    sig = np.broadcast_to(np.asarray(noise, dtype=np.float64), (int(n),))
    sig = sig[np.isfinite(sig)]
    return float(sig.size * (lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * pi)) - np.sum(np.log(sig)))


def signed_peak(spec, axis=-1):
    """The signed value of largest magnitude along `axis`, NaNs ignored (NaN where all are): the peak of a line that may
    absorb (a runner with a continuum background) as `nanmax` is the peak of one that emits."""
    spec = np.asarray(spec, dtype=np.float64)
    bad = np.isnan(spec)
    mag = np.where(bad, -1.0, np.abs(spec))
    ix = np.expand_dims(np.argmax(mag, axis=axis), axis)
    out = np.squeeze(np.take_along_axis(spec, ix, axis=axis), axis)
    return np.where(np.all(bad, axis=axis), np.nan, out)


def noise_shape(f):
    """Shape (= rate) a = 1 / (4 f^2) of the Gamma prior of the noise precision tau = 1 / t^2 for a fractional uncertainty f
    of the noise level: mean 1, std(tau) = 1 / sqrt(a) = 2 f, i.e. std(t) = f to first order."""
    f = np.asarray(f, dtype=np.float64)
    return 1.0 / (4.0 * f * f)


def noise_marginal_lnl(half_chi2, nu, f):
    """The log-likelihood term of a spectrum whose noise level has the fractional uncertainty f:
    -(a + nu / 2) log1p(h / a) for h = chi^2 / (2 sigma^2) >= 0 and nu unmasked channels; -h for f = 0.  numpy, elementwise."""
    h, nu, f = np.broadcast_arrays(np.asarray(half_chi2, dtype=np.float64), np.asarray(nu, dtype=np.float64),
                                   np.asarray(f, dtype=np.float64))
    on = f > 0.0
    a = noise_shape(np.where(on, f, 1.0))
    out = np.where(on, -(a + nu / 2.0) * np.log1p(np.maximum(h, 0.0) / a), -h)
    return out if out.ndim else float(out)


def half_chi2(data, pred, noise, order=None, templates=None, corr=None, resp=None):
    """(h, nu) of ONE spectrum at a model `pred`: h = chi^2 / (2 sigma^2) as a spectra set forms it and nu the unmasked
    channels.  `noise` is a scalar or one value per channel (inf: masked); `order` and `templates` are profiled out
    (`nuisance_fit`), `resp` (five taps) filters the model first and `corr` = (rho_1, rho_2) correlates the noise
    (`corr_bands`).  numpy on the host."""
    d, p = np.asarray(data, dtype=np.float64), np.asarray(pred, dtype=np.float64)
    n = d.shape[0]
    sig = np.broadcast_to(np.asarray(noise, dtype=np.float64), (n,))
    live = np.isfinite(sig)
    if resp is not None:
        p = np.correlate(p, np.asarray(resp, dtype=np.float64), 'same')          # p~_j = sum_k h_k p_{j+k}, 0 beyond the ends
    w = np.where(live, 1.0 / np.where(live, sig, 1.0) ** 2, 0.0)
    r = np.where(live, d - p, 0.0)
    if order is not None or templates is not None:
        r = np.where(live, r - nuisance_fit(r, w, order, templates)[0], 0.0)
    e = r * np.sqrt(w)
    if corr is None or (corr[0] == 0.0 and corr[1] == 0.0):
        chi2 = float(np.sum(e * e))
    else:
        d0, d1, d2 = corr_bands(float(corr[0]), float(corr[1]), n)
        chi2 = float(np.sum(d0 * e * e) + 2.0 * np.sum(d1 * e[:-1] * e[1:]) + 2.0 * np.sum(d2 * e[:-2] * e[2:]))
    return 0.5 * chi2, int(np.count_nonzero(live))


def noise_fit(h, nu, f):
    """Posterior (mean, standard deviation) of the noise scale t of ONE spectrum, true noise = t * stated noise, at a model
    with h = chi^2 / (2 sigma^2) (`half_chi2`) over `nu` unmasked channels: tau = 1 / t^2 given the data is
    Gamma(c, rate r) with c = a + nu / 2 and r = a + h, so E t^k = r^(k/2) Gamma(c - k/2) / Gamma(c).  (1, 0) for f = 0."""
    from math import exp, lgamma, sqrt
    if not f > 0.0:
        return 1.0, 0.0
    a = float(noise_shape(f))
    c, r = a + nu / 2.0, a + max(float(h), 0.0)
    m1 = sqrt(r) * exp(lgamma(c - 0.5) - lgamma(c))
    m2 = r / (c - 1.0) if c > 1.0 else np.inf                 # (c = 1: f = 0.5 and no channel at all)
    return m1, sqrt(max(m2 - m1 * m1, 0.0))


def noise_prefactor(nu, f):
    """What `Spectrum.prefactor` gains with a noise uncertainty f over nu unmasked channels: the theta-independent constant
    lgamma(a + nu / 2) - lgamma(a) - (nu / 2) ln a of the marginal (0 for f = 0), which makes -(a + nu/2) log1p(h / a) +
    prefactor the log of the normalised marginal density as -h + prefactor is at a known noise."""
    from math import lgamma, log
    if f is None or not f > 0.0:
        return 0.0
    a = float(noise_shape(f))
    return lgamma(a + nu / 2.0) - lgamma(a) - (nu / 2.0) * log(a)


def gain_fit(data, pred, weight, sigma, cal, order=None):
    """Posterior (mean, standard deviation) of the gain of ONE spectrum at a given model `pred`: data =
    g pred + baseline + noise, g ~ N(1, cal^2), channel weights `weight` (0: masked), sigma the noise of weight 1; with a
    baseline of degree <= `order`, `baseline_fit`'s projection is taken out of data and model first.  numpy on the host."""
    w = np.asarray(weight, dtype=np.float64)
    d = np.where(w > 0, np.asarray(data, dtype=np.float64), 0.0)
    p = np.asarray(pred, dtype=np.float64)
    if order is not None:
        d = d - baseline_fit(d, w, order)
        p = p - baseline_fit(p, w, order)
    A, B = float(np.sum(w * p * p)), float(np.sum(w * d * p))
    s2, sig2 = float(cal) ** 2, float(sigma) ** 2
    den = sig2 + s2 * A
    return 1.0 + s2 * (B - A) / den, float(cal) * float(sigma) / np.sqrt(den)


def baseline_fit(resid, weight, order):
    """Best-fit baselines of residual spectra resid[..., N] under channel weights weight[..., N] (0: masked, whose residual
    is ignored; the scale of the weights does not matter): the polynomial of degree <= `order` in the channel index that
    minimises sum w (r - b)^2, evaluated at every channel -- the likelihood's baseline, on the host with numpy.
    Legendre basis of u = (2j - (N - 1)) / (N - 1); with n <= order weighted channels the degree is n - 1, with none 0."""
    resid = np.asarray(resid, dtype=np.float64)
    n = resid.shape[-1]
    weight = np.broadcast_to(np.asarray(weight, dtype=np.float64), resid.shape)
    u = (2.0 * np.arange(n) - (n - 1)) / (n - 1) if n > 1 else np.zeros(n)
    flat_r, flat_w = resid.reshape(-1, n), weight.reshape(-1, n)
    out = np.zeros_like(flat_r)
    for i, (r, w) in enumerate(zip(flat_r, flat_w)):
        live = w > 0
        k = min(int(order), int(live.sum()) - 1)
        if k < 0:
            continue
        V = np.polynomial.legendre.legvander(u, k)
        sw = np.sqrt(w[live])
        coef = np.linalg.lstsq(V[live] * sw[:, None], r[live] * sw, rcond=None)[0]
        out[i] = V @ coef
    return out.reshape(resid.shape)


def channel_weights(noise, size):
    """Relative channel weights 1 / sigma_c^2 of one spectrum (a scalar noise: ones; inf: 0)."""
    if np.ndim(noise) == 0:
        return np.ones(size)
    return 1.0 / np.asarray(noise, dtype=np.float64) ** 2


class _SpecSet:
    """Owner of a device-resident set of spectra (one pixel or a cube)."""

    def __init__(self, xarrs, trans_ids, data, noise, model=MODEL_AMMONIA, rest_freqs=None, lines=None, species=None, fill=False):
        """xarrs: list of 1-D axes; data [n_pix, sum(sizes)]; noise [n_pix, n_spec], or [n_pix, sum(sizes)]
        for a noise per channel (nfa_specset_create_channel_noise: inf masks a channel).  lines: the hyperfine
        model's `LineTable` of every spectrum (nfa_specset_create_lines; `trans_ids` and `rest_freqs` are then unused), or
        the LTE model's `LteLines` of every spectrum, all of one `Molecule` (nfa_specset_create_lte); where a spectrum covers
        several transitions, its `LteBand` (nfa_specset_create_lte_bands).  species: the ordered `Molecule`s of an LTE mix,
        whose `lines` may be `LteBlend`s as well and of any of them (nfa_specset_create_lte_mix); 3 + len(species) parameters
        per component.  fill: such a set with a beam filling factor per component as one more parameter, the last
        (nfa_specset_create_lte_filled)."""
        self.model = int(model)
        if (self.model in TABLED_MODELS) != (lines is not None):
            raise ValueError('the hyperfine model (3), the LTE model (4) and the excitation-grid model (5), and no other, take '
                             '`lines`: one LineTable (LteLines, GridLines) per spectrum')
        molecule = None
        self.grid = None
        if self.model == MODEL_GRID:
            from .excitation import check_one_grid
            if species is not None or fill:
                raise ValueError('`species` and `fill` belong to the LTE model (4)')
            lines = list(lines)
            if len(lines) != len(xarrs):
                raise ValueError('`lines` must hold one GridLines per spectrum')
            self.grid = check_one_grid(lines)
            trans_ids = [-1] * len(lines)
        elif lines is not None:
            from .hyperfine import LineTable
            from .lte import LteBand, LteBlend, check_mix_lines, check_one_molecule, transitions_of
            lines = list(lines)
            if species is not None:
                if self.model != MODEL_LTE:
                    raise ValueError('`species` belong to the LTE model (4)')
                if len(lines) != len(xarrs):
                    raise ValueError('`lines` must hold one LineTable per spectrum')
                lines = check_mix_lines(species, lines)
                species = tuple(species)
            elif len(lines) != len(xarrs) or not all(isinstance(t, (LineTable, LteBand)) for t in lines):
                raise ValueError('`lines` must hold one LineTable per spectrum')
            elif self.model == MODEL_LTE:
                molecule = check_one_molecule(lines)
            elif any(isinstance(t, LteBand) for t in lines):
                raise ValueError('an LteBand belongs to the LTE model (4)')
            trans_ids = [-1] * len(lines)
        elif species is not None:
            raise ValueError('`species` come with `lines`')
        if fill and species is None:
            raise ValueError('a filling factor (`fill`) belongs to an LTE mix: `species` and `lines`')
        self.fill = bool(fill)
        self.molecule = molecule
        self.species = species
        self.n_model = N_MODEL[self.model] if species is None else 3 + len(species) + (1 if fill else 0)
        self.lines = lines
        lib = _ffi.engine()
        self.n_spec = len(xarrs)
        self.sizes = np.array([x.size for x in xarrs], dtype=np.int64)
        self.trans_ids = np.asarray(trans_ids, dtype=np.int32)
        self.xarrs = [np.ascontiguousarray(x, dtype=np.float64) for x in xarrs]
        data = np.ascontiguousarray(data, dtype=np.float64)
        noise = np.ascontiguousarray(noise, dtype=np.float64)
        self.n_pix = int(data.shape[0])
        self.chan_tot = int(self.sizes.sum())
        assert data.shape == (self.n_pix, self.chan_tot)
        # (spectra have two channels and more: the two shapes never coincide)
        self.per_channel = noise.shape == (self.n_pix, self.chan_tot)
        assert self.per_channel or noise.shape == (self.n_pix, self.n_spec)
        # channels that enter the likelihood, per pixel
        self.n_chan = (np.isfinite(noise).sum(axis=1) if self.per_channel
                       else np.full(self.n_pix, self.chan_tot)).astype(np.int64)
        xp = (_ffi._dp * self.n_spec)(*[_ffi.dptr(x) for x in self.xarrs])
        h = C.c_void_p()
        self.rest_freqs = (None if rest_freqs is None
                           else np.ascontiguousarray(rest_freqs, dtype=np.float64))
        sizes_p = self.sizes.ctypes.data_as(_ffi._lp)
        if self.grid is not None:                   # the excitation-grid model: the lines creator's arguments and the grid
            g = self.grid
            self.rest_freqs = np.array([t.nu for t in lines], dtype=np.float64)
            n_lines = np.array([t.n for t in lines], dtype=np.int32)
            voff = np.ascontiguousarray(np.concatenate([t.voff for t in lines]), dtype=np.float64)
            tau_wts = np.ascontiguousarray(np.concatenate([t.tau_wts for t in lines]), dtype=np.float64)
            tex = np.ascontiguousarray(np.stack([t.tex for t in lines]), dtype=np.float64)
            ltau = np.ascontiguousarray(np.stack([t.ltau for t in lines]), dtype=np.float64)
            axes = [np.ascontiguousarray(a) for a in (g.tkin, g.lnden, g.lncd)]
            rc = lib.nfa_specset_create_grid(
                C.byref(h), self.n_spec, sizes_p, n_lines.ctypes.data_as(_ffi._ip), _ffi.dptr(self.rest_freqs), _ffi.dptr(voff),
                _ffi.dptr(tau_wts), axes[0].size, _ffi.dptr(axes[0]), axes[1].size, _ffi.dptr(axes[1]), axes[2].size,
                _ffi.dptr(axes[2]), _ffi.dptr(tex), _ffi.dptr(ltau), xp, self.n_pix, _ffi.dptr(data),
                None if self.per_channel else _ffi.dptr(noise), _ffi.dptr(noise) if self.per_channel else None)
        elif lines is not None:                     # the caller's tables: exactly one of the two noise arguments
            self.rest_freqs = np.array([t.nu for t in lines], dtype=np.float64)
            banded = species is not None or any(isinstance(t, LteBand) for t in lines)
            n_trans = np.array([len(transitions_of(t)) for t in lines], dtype=np.int32)
            if banded:                              # one entry per transition, the spectra one after the other
                lines = [t for band in lines for t in transitions_of(band)]
            n_lines = np.array([t.n for t in lines], dtype=np.int32)
            freqs = np.array([t.nu for t in lines], dtype=np.float64)
            voff = np.ascontiguousarray(np.concatenate([t.voff for t in lines]), dtype=np.float64)
            tau_wts = np.ascontiguousarray(np.concatenate([t.tau_wts for t in lines]), dtype=np.float64)
            head = (C.byref(h), self.n_spec, sizes_p, *((n_trans.ctypes.data_as(_ffi._ip),) if banded else ()),
                    n_lines.ctypes.data_as(_ffi._ip), _ffi.dptr(freqs), _ffi.dptr(voff), _ffi.dptr(tau_wts))
            tail = (xp, self.n_pix, _ffi.dptr(data),
                    None if self.per_channel else _ffi.dptr(noise), _ffi.dptr(noise) if self.per_channel else None)
            if species is not None:
                e_up, g_up, a_ul = (np.array([getattr(t, k) for t in lines], dtype=np.float64)
                                    for k in ('e_up', 'g_up', 'a_ul'))
                of = np.array([species.index(t.molecule) for t in lines], dtype=np.int32)
                n_q = np.array([m.n for m in species], dtype=np.int32)
                q_temp = np.ascontiguousarray(np.concatenate([m.q_temp for m in species]))
                q_val = np.ascontiguousarray(np.concatenate([m.q_val for m in species]))
                create = lib.nfa_specset_create_lte_filled if fill else lib.nfa_specset_create_lte_mix
                rc = create(*head, _ffi.dptr(e_up), _ffi.dptr(g_up), _ffi.dptr(a_ul), len(species), of.ctypes.data_as(_ffi._ip),
                            n_q.ctypes.data_as(_ffi._ip), _ffi.dptr(q_temp), _ffi.dptr(q_val), *tail)
            elif molecule is not None:
                e_up, g_up, a_ul = (np.array([getattr(t, k) for t in lines], dtype=np.float64)
                                    for k in ('e_up', 'g_up', 'a_ul'))
                q_temp, q_val = np.ascontiguousarray(molecule.q_temp), np.ascontiguousarray(molecule.q_val)
                create = lib.nfa_specset_create_lte_bands if banded else lib.nfa_specset_create_lte
                rc = create(*head, _ffi.dptr(e_up), _ffi.dptr(g_up), _ffi.dptr(a_ul), molecule.n,
                            _ffi.dptr(q_temp), _ffi.dptr(q_val), *tail)
            else:
                rc = lib.nfa_specset_create_lines(*head, *tail)
        else:
            create = lib.nfa_specset_create_channel_noise if self.per_channel else lib.nfa_specset_create_model
            rc = create(C.byref(h), self.model, self.n_spec, sizes_p, self.trans_ids.ctypes.data_as(_ffi._ip),
                        None if self.rest_freqs is None else _ffi.dptr(self.rest_freqs), xp, self.n_pix,
                        _ffi.dptr(data), _ffi.dptr(noise))
        _ffi.check(rc)
        self.handle = h
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.options = Options()                             # what the set has: ss.robust, ss.templates, ... read it
        self.masked = bool(self.per_channel and not np.all(np.isfinite(noise)))

    def __getattr__(self, name):
        """`ss.robust`, `ss.templates`, ...: the set's normalised options by their names, read from the one record."""
        if name in OPTION_NAMES:
            return getattr(self.options, name)
        raise AttributeError(name)

    def _set(self, name, value, args=None, **about):
        """The body of every setter: the option's value check (`_options.normalise`; `about`: the model and the pixels, where
        a setter lets it ask), the rules table against what the set has where the value switches the option on
        (`_options.refusal`), the engine's nfa_specset_set_* with `args(value)` (by default the array, or NULL for none),
        then the record."""
        value = normalise(name, value, self.n_spec, self.sizes, **about)
        if is_set(value):
            why = model_refusal(name, self.model) or refusal(name, self.options.has(self.masked))
            if why is not None:
                raise ValueError(why)
        call = getattr(_ffi.load(), 'nfa_specset_set_' + name.replace('_order', ''))
        _ffi.check(call(self.handle, *(args(value) if args else (None if value is None else _ffi.dptr(value),))))
        setattr(self.options, name, value)

    def set_robust(self, nu):
        """The degrees of freedom of the spectra's Student-t channel noise (`check_robust`'s argument), or none (None,
        zeros): nfa_specset_set_robust.  null_lnZ() follows."""
        self._set('robust', nu)

    def get_robust(self):
        """The degrees of freedom as the engine holds them (nfa_specset_robust): None, or float64 [n_spec]."""
        out = np.zeros(self.n_spec)
        return out if _ffi.load().nfa_specset_robust(self.handle, _ffi.dptr(out)) else None

    def set_continuum(self, tc):
        """The continuum brightness temperature behind the components, per (pixel, spectrum) (`check_continuum`'s argument:
        a number, [n_spec] or [n_pix, n_spec]), or none (None, zeros): nfa_specset_set_continuum.  null_lnZ() does not
        change: the null model has no absorber."""
        self._set('continuum', tc, model=self.model, n_pix=self.n_pix)

    def get_continuum(self):
        """The continuum as the engine holds it (nfa_specset_continuum): None, or float64 [n_pix, n_spec]."""
        out = np.zeros((self.n_pix, self.n_spec))
        return out if _ffi.load().nfa_specset_continuum(self.handle, _ffi.dptr(out)) else None

    def _packed_templates(self, tmpl):
        """The two arguments of nfa_specset_set_templates: the templates as [TMPL_MAX, chan_tot] and every spectrum's count."""
        if tmpl is None:
            return None, None
        vals = np.zeros((TMPL_MAX, self.chan_tot))
        counts = np.zeros(self.n_spec, dtype=np.int32)
        for k, a in enumerate(tmpl):
            if a is not None:
                counts[k] = a.shape[0]
                vals[:a.shape[0], self.offsets[k]:self.offsets[k + 1]] = a
        return _ffi.dptr(vals), counts.ctypes.data_as(_ffi._ip)

    def set_templates(self, tmpl):
        """Nuisance templates per spectrum, profiled out of the likelihood with the baseline (`check_templates`'s argument),
        or none (None): nfa_specset_set_templates.  null_lnZ() then is the model of baseline and templates alone."""
        self._set('templates', tmpl, self._packed_templates)

    def get_templates(self):
        """The templates as the engine holds them (nfa_specset_templates): None, or a list of n_spec entries, None or
        float64 [T, N_s], in the caller's scaling."""
        vals = np.zeros((TMPL_MAX, self.chan_tot))
        counts = np.zeros(self.n_spec, dtype=np.int32)
        if not _ffi.load().nfa_specset_templates(self.handle, _ffi.dptr(vals), counts.ctypes.data_as(_ffi._ip)):
            return None
        return [vals[:counts[k], self.offsets[k]:self.offsets[k + 1]].copy() if counts[k] else None for k in range(self.n_spec)]

    def set_response(self, resp):
        """The channel response of the spectra (`check_response`'s argument), or none (None, the identity):
        nfa_specset_set_response.  null_lnZ() does not change."""
        self._set('response', resp)

    def set_correlation(self, corr):
        """The autocorrelations (rho_1, rho_2) of the channel noise along the spectral axis (`check_correlation`'s argument),
        or none (None, zeros): nfa_specset_set_correlation.  null_lnZ() follows."""
        self._set('correlation', corr)

    def set_noise_uncertainty(self, f):
        """The fractional uncertainty of every spectrum's noise level, integrated out of the likelihood
        (`check_noise_uncertainty`'s argument), or none (None, zeros): nfa_specset_set_noise_uncertainty.  null_lnZ()
        follows."""
        self._set('noise_uncertainty', f)

    def set_calibration(self, cal):
        """A calibration uncertainty per spectrum, integrated out of the likelihood (`check_calibration`'s argument), or
        none (None, zeros): nfa_specset_set_calibration.  null_lnZ() does not change."""
        self._set('calibration', cal)

    def set_layered(self, on):
        """Layered transfer (True) or the summed model (False): nfa_specset_set_layered.  Layered, component 0 is the
        farthest from the observer and each component absorbs those behind it."""
        self._set('layered', on, lambda v: (int(v),))

    def set_baseline(self, order):
        """A polynomial baseline of degree <= `order` per (pixel, spectrum) profiled out of the likelihood, or none
        (None / -1): nfa_specset_set_baseline.  null_lnZ() then is the baseline-only model's."""
        self._set('baseline_order', order, lambda v: (-1 if v is None else v,))

    def null_lnZ(self):
        out = np.empty((self.n_pix, self.n_spec))
        _ffi.check(_ffi.load().nfa_specset_null_lnz(self.handle, _ffi.dptr(out)))
        return out

    def tbg(self):
        out = np.empty(self.chan_tot)
        _ffi.check(_ffi.load().nfa_specset_tbg(self.handle, _ffi.dptr(out)))
        return out

    def __del__(self):
        if getattr(self, 'handle', None) is not None:
            try:
                _ffi.load().nfa_specset_destroy(self.handle)
            except Exception:
                pass
            self.handle = None


class _RunnerHandle:
    def __init__(self, specset, utrans, ncomp, cold=False, lte=False):
        lib = _ffi.engine()
        self.specset = specset
        self.utrans = utrans
        ph = utrans._device_handle() if utrans is not None else None
        h = C.c_void_p()
        _ffi.check(lib.nfa_runner_create(C.byref(h), specset.handle, ph, int(ncomp), int(bool(cold)),
                                         int(bool(lte))))
        self.handle = h

    def set_exp_mode(self, mode):
        """Pin the numerical mode of this runner ('table' / 'fast' or 0 / 2); None or -1
        = follow the process default (`nestfit_amd.set_exp_mode`) again."""
        mode = -1 if mode is None else {'table': 0, 'fast': 2}.get(mode, mode)
        _ffi.check(_ffi.load().nfa_runner_set_exp_mode(self.handle, int(mode)))

    def get_exp_mode(self):
        return _ffi.load().nfa_runner_get_exp_mode(self.handle)

    def __del__(self):
        if getattr(self, 'handle', None) is not None:
            try:
                _ffi.load().nfa_runner_destroy(self.handle)
            except Exception:
                pass
            self.handle = None


def _pix_ptr(pix, B):
    if pix is None:
        return None, None
    pix = np.ascontiguousarray(pix, dtype=np.int32)
    assert pix.shape == (B,)
    return pix, pix.ctypes.data_as(_ffi._ip)



class EngineSpectrumMixin:
    """Spectrum whose model values are computed by the engine: one private spectra set of
    one pixel, runner handles cached per (ncomp, cold, lte)."""
    MODEL = MODEL_AMMONIA

    def _attach(self, trans_id, rest_freq=None, lines=None, species=None, fill=False):
        self._ss = _SpecSet([self.xarr], [trans_id], self.data.reshape(1, -1),
                            np.reshape(self.noise, (1, -1)), model=self.MODEL,
                            rest_freqs=None if rest_freq is None else [rest_freq],
                            lines=None if lines is None else [lines], species=species, fill=fill)
        self.null_lnZ = float(self._ss.null_lnZ()[0, 0])
        self._runners = {}

    def _runner(self, ncomp, cold=False, lte=False):
        key = (int(ncomp), bool(cold), bool(lte))
        if key not in self._runners:
            self._runners[key] = _RunnerHandle(self._ss, None, *key)
        return self._runners[key]

    def _predict(self, params, n_model, cold=False, lte=False):
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.ndim != 1 or params.shape[0] == 0 or params.shape[0] % n_model != 0:
            raise ValueError(f'Invalid parameter vector length: {params.shape}')
        run = self._runner(params.shape[0] // n_model, cold, lte)
        spec = np.empty((1, self.size))
        lnl = np.empty(1)
        _ffi.check(_ffi.load().nfa_runner_predict_batch(run.handle, None, _ffi.dptr(params), 1,
                                                        _ffi.dptr(spec), _ffi.dptr(lnl)))
        self._pred = spec[0]
        self._lnL = float(lnl[0])

    # reference: core.pyx:532-545
    @property
    def sum_spec(self):
        return np.nansum(self._pred)

    @property
    def max_spec(self):
        return np.nanmax(self._pred)

    @property
    def loglikelihood(self):
        return self.null_lnZ if self._lnL is None else self._lnL

    def get_spec(self):
        return np.array(self._pred)


# ---- the runner surface: what a one-pixel runner (`EngineRunner`) and a `CubeRunner` show of their set's options ------------
# Per option: `value`, the words of the read-only property; `sets`, the words of `set_<name>`; `null_lnZ`, what the setter does
# with the runner's null_lnZ -- 'read' it from the set, 'refresh' it (a one-pixel runner: `_refresh_null_lnZ`; a CubeRunner
# reads) or None: leave it; `prefactor`: a one-pixel runner hands every spectrum's value on to the `Spectrum`'s own setter,
# which keeps its `prefactor`.  A one-pixel runner's spectra each own a private one-spectrum set, which follows none of this:
# what that means stands with each setter.
RunnerOption = namedtuple('RunnerOption', 'value sets null_lnZ prefactor')
_OWN_LNL = ("a spectrum's own `loglikelihood` is the plain one; the runner's `loglikelihood`, `loglikelihood_batch` and "
            "`predict_batch` ")
SURFACE = {
    'robust': RunnerOption(
        "None, or the float64 array [n_spec] of the degrees of freedom of the spectra's Student-t channel noise.",
        "Sets (a number, or one per spectrum) or removes (None, zeros) the robust likelihood of the runner's spectra (DESIGN "
        "4.18); null_lnZ follows, and a one-pixel runner's spectra's `prefactor`.  Those spectra's private one-spectrum sets "
        "stay Gaussian: " + _OWN_LNL + "are the robust ones.", 'refresh', True),
    'continuum': RunnerOption(
        "None, or the float64 array of the continuum brightness temperatures behind the spectra (K): [n_spec] of a one-pixel "
        "runner, [n_pix, n_spec] of a CubeRunner.",
        "Sets (a number or one value per spectrum; a CubeRunner: or [n_pix, n_spec]; in K) or removes (None, zeros) the continuum "
        "background of the runner's spectra.  null_lnZ is read again and does not change: the null model has no absorber.  A "
        "one-pixel runner's spectra's private one-spectrum sets have no continuum: `predict` fills them from the runner's own "
        "set (`_predict_layered`).", 'refresh', False),
    'noise_uncertainty': RunnerOption(
        "None, or the float64 array of the fractional uncertainties of the spectra's noise levels.",
        "Sets (a number, or one per spectrum) or removes (None, zeros) the uncertainty of the noise levels of the runner's "
        "spectra; null_lnZ follows, and a one-pixel runner's spectra's `prefactor`.  Those spectra's private one-spectrum sets "
        "keep the noise exact: " + _OWN_LNL + "are the marginal ones.", 'refresh', True),
    'templates': RunnerOption(
        "None, or the list of the spectra's nuisance templates: per spectrum None or a float64 array [T, N_s].",
        "Sets (a list with an array [T, N_s] or None per spectrum) or removes (None) the nuisance templates of the runner's "
        "spectra; null_lnZ follows.  A one-pixel runner's spectra's private one-spectrum sets have none: " + _OWN_LNL
        + "profile the templates out.", 'refresh', False),
    'response': RunnerOption(
        "None, or the float64 array [n_spec, 5] of the spectra's channel responses (h_-2 .. h_2).",
        "Sets (3 or 5 taps, or such a row per spectrum) or removes (None, the identity) the channel response of the runner's "
        "spectra; null_lnZ is untouched.  A one-pixel runner's spectra's private one-spectrum sets stay unfiltered: "
        "`predict(params)` leaves the unsmoothed model in the spectra; the runner's `loglikelihood`, `loglikelihood_batch` and "
        "`predict_batch` are the filtered ones.", None, False),
    'correlation': RunnerOption(
        "None, or the float64 array [n_spec, 2] of the spectra's noise autocorrelations (rho_1, rho_2).",
        "Sets (a pair, or one per spectrum) or removes (None, zeros) the noise correlation of the runner's spectra; null_lnZ "
        "follows, and a one-pixel runner's spectra's `prefactor`.  Those spectra's private one-spectrum sets stay white: a "
        "spectrum's own `loglikelihood` and `null_lnZ` (and what `predict` leaves there) are white-noise values and must not be "
        "combined with its correlated `prefactor`; the runner's `loglikelihood`, `loglikelihood_batch` and `predict_batch` are "
        "the correlated ones.", 'read', True),
    'calibration': RunnerOption(
        "None, or the float64 array of the spectra's fractional calibration uncertainties.",
        "Sets (a number, or one per spectrum) or removes (None, zeros) the calibration uncertainty of the runner's spectra; "
        "null_lnZ is untouched.", None, False),
}
# the options a runner hands to its set through its own setters, which keep null_lnZ (read right after set_baseline) and the
# spectra's prefactors in step; `layered` goes to the set itself
RUNNER_SETS = ('baseline_order', *SURFACE)


def _option_property(name):
    def get(self):
        value = getattr(self._ss, name)
        if value is None:
            return None
        if name == 'templates':
            return [None if a is None else a.copy() for a in value]
        return (value[0] if name == 'continuum' and self.ONE_PIXEL else value).copy()
    return property(get, doc=SURFACE[name].value)


def _option_setter(name):
    def set_option(self, value):
        if name == 'continuum' and self.ONE_PIXEL:           # (one value per spectrum at the most, in and out)
            value = check_continuum(value, self.n_spec, None, self.MODEL)
        getattr(self._ss, 'set_' + name)(value)
        self._after_set(name)
    set_option.__name__, set_option.__qualname__, set_option.__doc__ = 'set_' + name, 'RunnerSurface.set_' + name, SURFACE[name].sets
    return set_option


class RunnerSurface:
    """The part of a runner that is its spectra set's (`self._ss`) and its handle's (`self._run`): for every option of
    SURFACE the read-only property of its name, a copy of the set's normalised value, and `set_<name>`, the set's setter and
    then the class's `_after_set(name)`; `set_baseline`, whose value is the mirrored attribute `baseline_order`."""
    ONE_PIXEL = False                                        # a cube's continuum is [n_pix, n_spec], one pixel's [n_spec]

    def set_baseline(self, order):
        """Sets (0..3) or removes (None) the baseline of the runner's spectra; null_lnZ follows."""
        self._ss.set_baseline(order)
        self.baseline_order = self._ss.baseline_order
        self._read_null_lnZ()

    def _after_set(self, name):
        if SURFACE[name].null_lnZ is not None:
            self._read_null_lnZ()

    def set_exp_mode(self, mode):
        """Numerical mode of this runner alone (None: the process default again): runners of different
        modes can then be used side by side, also from different threads."""
        self._run.set_exp_mode(mode)


for _name in SURFACE:
    setattr(RunnerSurface, _name, _option_property(_name))
    setattr(RunnerSurface, 'set_' + _name, _option_setter(_name))


def apply_options(options, ss, runner=None):
    """Hands the options of the record `options` that are on to the new spectra set `ss`, in APPLY_ORDER: through the set's
    setters, or, with an EngineRunner `runner`, the RUNNER_SETS among them through the runner's."""
    for name in APPLY_ORDER:
        value = getattr(options, name)
        if is_set(value):
            owner = runner if runner is not None and name in RUNNER_SETS else ss
            getattr(owner, 'set_' + name.replace('_order', ''))(value)


def _noise_row(spectra):
    """The noise of one pixel's spectra as a set takes it: [1, n_spec], or, with a noise per channel in any spectrum, for all of
    them: [1, chan_tot]."""
    if any(np.ndim(s.noise) for s in spectra):
        return np.concatenate([np.broadcast_to(s.noise, (s.size,)) for s in spectra]).reshape(1, -1)
    return np.array([[s.noise for s in spectra]])


class EngineRunner(RunnerSurface, Runner):
    """Runner attributes and methods common to the three models (reference:
    ammonia.pyx:369-447, diazenylium.pyx:161-231, gaussian.pyx:57-112)."""
    MODEL = MODEL_AMMONIA
    N_MODEL = 6
    ONE_PIXEL = True

    def _setup(self, spectra, utrans, ncomp, cold=False, lte=False, rest_freqs=None, options=None):
        """options: the mapping of the keywords that the runner's constructor took as `**options` -- the likelihood options
        of its spectra set (see `_options` for each) and nothing else: any other key is the constructor's TypeError."""
        assert ncomp > 0
        options = check_options(options or {}, len(spectra), [s.size for s in spectra],
                                any(np.ndim(s.noise) and not np.all(np.isfinite(s.noise)) for s in spectra), self.MODEL,
                                caller=type(self).__init__.__qualname__)
        self.n_model = self.N_MODEL
        self.utrans = utrans
        self.ncomp = int(ncomp)
        self.n_spec = len(spectra)
        self.n_params = self.n_model * self.ncomp
        self.ndim = self.n_params  # no nuisance parameters
        self.null_lnZ = 0.0
        self.n_chan_tot = 0
        for spec in spectra:
            self.null_lnZ += spec.null_lnZ
            self.n_chan_tot += spec.n_chan
        self.run_lnZ = np.nan
        data = np.concatenate([s.data for s in spectra]).reshape(1, -1)
        self._ss = _SpecSet([s.xarr for s in spectra], [s.trans_id for s in spectra], data, _noise_row(spectra),
                            model=self.MODEL, rest_freqs=rest_freqs,
                            lines=[s.lines for s in spectra] if self.MODEL in TABLED_MODELS else None,
                            species=getattr(self, 'SPECIES', None), fill=getattr(self, 'FILL', False))
        self._run = _RunnerHandle(self._ss, utrans, self.ncomp, cold, lte)
        self.layered, self.baseline_order = options.layered, options.baseline_order
        apply_options(options, self._ss, self)

    def _read_null_lnZ(self):
        self.null_lnZ = float(self._ss.null_lnZ().sum())

    def _after_set(self, name):
        """What a setter of SURFACE leaves behind: null_lnZ by the option's rule, and the spectra's prefactors."""
        rule = SURFACE[name]
        if rule.null_lnZ == 'read':
            self._read_null_lnZ()
        elif rule.null_lnZ == 'refresh':
            self._refresh_null_lnZ()
        if rule.prefactor:
            value = getattr(self._ss, name)
            for k, s in enumerate(self._model_spectra()):
                getattr(s, 'set_' + name)(None if value is None else value[k])

    def _refresh_null_lnZ(self):
        """null_lnZ after a setter that can remove what it depended on: the runner's own set's wherever that set's likelihood is
        not the plain one at p = 0 (a baseline, templates, a correlation, a noise uncertainty), else the spectra's own values
        (the reference's spectrum-alone sum)."""
        ss = self._ss
        if (self.baseline_order is not None or ss.templates is not None or ss.correlation is not None
                or ss.noise_uncertainty is not None or ss.robust is not None):
            self._read_null_lnZ()
        else:
            self.null_lnZ = float(sum(s.null_lnZ for s in self._model_spectra()))

    def _predict_through_set(self):
        """Whether `predict` takes the model from the runner's own spectra set: the spectra's one-spectrum sets are summed and
        stand before the cosmic background alone."""
        return self.layered or self._ss.continuum is not None

    def _predict_layered(self, params):
        """`predict` of a layered runner, and of one with a continuum background: the spectra's own one-spectrum sets are summed
        ones before the cosmic background alone, so the model comes from the runner's set (`predict_batch`) and goes into every
        spectrum, with the spectrum's lnL formed on the host."""
        spec, _ = self.predict_batch(params.reshape(1, -1))
        off = self._ss.offsets
        for k, s in enumerate(self._model_spectra()):
            s._pred = spec[0, off[k]:off[k + 1]].copy()
            w = channel_weights(s.noise, s.size)
            resid = np.where(w > 0, s.data - s._pred, 0.0)
            scale = 1.0 if np.ndim(s.noise) else float(s.noise) ** 2           # (channel_weights: 1 / sigma_c^2, or ones)
            s._lnL = float(-np.sum(w * resid * resid) / (2.0 * scale))

    def _model_spectra(self):
        return list(self.spectra)

    def _diagnose(self, which, params, batch=False, **how):
        """`_diagnostics.fit_<which>` on the one row of this pixel: the spectra's data and noise and the model they hold after
        `predict(params)`, which this calls (batch: `predict_batch`'s row, and the spectra stay as they are)."""
        _diagnostics.require(which, self._ss.options)
        spectra = self._model_spectra()
        if batch:
            spec = self.predict_batch(np.asarray(params, dtype=np.float64).reshape(1, -1))[0]
        else:
            self.predict(params)
            spec = np.concatenate([s.get_spec() for s in spectra])[None]
        return getattr(_diagnostics, 'fit_' + which)(np.concatenate([s.data for s in spectra])[None], _noise_row(spectra), spec,
                                                     self._ss.offsets, self._ss.options, **how)

    def fit_baseline(self, params):
        """Best-fit baseline of every spectrum for physical `params` (after `predict`, which this calls): one array of
        n_chan_tot values, the spectra concatenated.  numpy on the host (`baseline_fit`): for residual plots, not the hot
        path.  A runner with nuisance templates returns the whole nuisance curve, polynomial and templates
        (`nuisance_fit`).  ValueError without a baseline and without templates."""
        return self._diagnose('baseline', params)[0]

    def fit_templates(self, params):
        """Best-fit amplitudes of every spectrum's templates, in the caller's scaling, for physical `params` (after `predict`,
        which this calls): a list of n_spec arrays [T] (empty for a spectrum without templates).  numpy on the host
        (`nuisance_fit`).  ValueError without templates."""
        return [a[0] for a in self._diagnose('templates', params)]

    def fit_gain(self, params):
        """Posterior mean and standard deviation of every spectrum's gain at physical `params` (after `predict`, which
        this calls): two arrays of n_spec values, 1 and 0 for a spectrum whose uncertainty is 0.  numpy on the host
        (`gain_fit`, with `fit_baseline`'s projection where there is a baseline).  ValueError without a calibration."""
        mean, std = self._diagnose('gain', params)
        return mean[0], std[0]

    def fit_noise(self, params):
        """Posterior mean and standard deviation of every spectrum's noise scale t (true noise = t * stated noise) at
        physical `params`: two arrays of n_spec values, 1 and 0 for a spectrum whose uncertainty is 0.  numpy on the host
        (`half_chi2`, `noise_fit`, after `predict`, which this calls) with the spectra's chi^2 as the runner's set forms
        them, whatever it profiles out, filters or correlates: where `predict` goes through the runner's set, the spectra
        hold the filtered model already.  ValueError without a noise uncertainty."""
        mean, std = self._diagnose('noise', params, filtered=self._predict_through_set())
        return mean[0], std[0]

    def fit_outliers(self, params):
        """Per spectrum, every channel's posterior mean precision factor (nu + 1) / (nu + r_j^2 / sigma_j^2) at physical
        `params`: a list of n_spec arrays, about 1 for a good channel and towards 0 for one the fit distrusted (1 everywhere
        in a spectrum with nu = 0, NaN at a masked channel).  numpy on the host (`robust_outliers`) over `predict_batch`'s
        spectra.  ValueError without a robust likelihood."""
        out = self._diagnose('outliers', params, batch=True)
        off = self._ss.offsets
        return [out[0, off[k]:off[k + 1]] for k in range(self.n_spec)]

    def loglikelihood(self, utheta):
        """lnL of one unit-cube point; `utheta` is overwritten with the physical
        parameters exactly like the reference (core.pyx:558-561)."""
        utheta = _as_inplace_vector(utheta)
        if utheta.shape[0] != self.ndim:
            raise _calls.shape_error(self, utheta.shape[0])
        return float(self.loglikelihood_batch(utheta.reshape(1, -1))[0])

    def loglikelihood_batch(self, U, out=None):
        """lnL[B] for unit-cube rows U[B, ndim] (overwritten with parameters).  `out`: where lnL goes; with `U`
        and `out` from `nestfit_amd.pinned_empty` the kernels work on the caller's arrays directly (no copies)."""
        U = _calls.unit_rows(self, U)
        lnL = _calls.out_array(out, (U.shape[0],), 'of one value per row')
        _ffi.check(_ffi.load().nfa_runner_loglike_batch(self._run.handle, None, _ffi.dptr(U),
                                                        _ffi.dptr(lnL), U.shape[0]))
        return lnL

    def _check_params(self, params):
        params = np.ascontiguousarray(params, dtype=np.float64)
        if params.shape[0] != self.ndim:
            raise _calls.shape_error(self, params.shape[0])
        return params

    def predict_batch(self, theta, want_spectra=True):
        """spectra[B, n_chan_tot] and lnL[B] for parameter rows theta[B, ndim]."""
        theta = _calls.parameter_rows(self, theta)
        B = theta.shape[0]
        spec = np.empty((B, self._ss.chan_tot)) if want_spectra else None
        lnl = np.empty(B)
        _ffi.check(_ffi.load().nfa_runner_predict_batch(
            self._run.handle, None, _ffi.dptr(theta), B,
            _ffi.dptr(spec) if want_spectra else None, _ffi.dptr(lnl)))
        return spec, lnl

    def row_statistics(self, theta):
        """(peak, total), [B, n_spec] each, of the model spectra of parameter rows theta[B, ndim], formed on the device
        (`CubeRunner.row_statistics`)."""
        return _calls._row_statistics(self._run.handle, None, _calls.parameter_rows(self, theta), self.n_spec)

    def predict_moments(self, theta, weights=None):
        """Weighted moments of the model spectra over the parameter rows theta[B, ndim] with weights[B] >= 0 (None: all
        ones), one segment: a `PosteriorMoments` record of one row per field (`CubeRunner.predict_moments`)."""
        theta = _calls.parameter_rows(self, theta)
        offsets = np.array([0, theta.shape[0]], dtype=np.int64)
        return _calls._predict_moments(self._run.handle, None, offsets, theta, weights, None, True, self._ss.chan_tot, self.n_spec)

    def normal_equations(self, theta, step, lower=None, upper=None, chunk_rows=None, want_curvature=True):
        """The normal equations of a least-squares fit at the parameter rows theta[B, ndim]: a `NormalEquations` record
        of chi2, grad = J^T W r and curv = J^T W J (`CubeRunner.normal_equations`)."""
        return _calls._normal_equations(self._run.handle, None, _calls.parameter_rows(self, theta), step, lower, upper, chunk_rows,
                                        want_curvature)

    def chi_squared(self, theta):
        """chi2[B] of the parameter rows theta[B, ndim] (`CubeRunner.chi_squared`)."""
        return _calls._normal_equations(self._run.handle, None, _calls.parameter_rows(self, theta), None, None, None, None, False,
                                        want_grad=False).chi2

    def sample_posterior(self, **kw):
        """The posterior of the runner's pixel at its component count by ensemble MCMC on the device: an `EnsembleResult` of
        one row (`nestfit_amd.ensemble.sample_pixels`' keywords; `par_bins`, `covariance`, `moments`: the marginal
        histograms, parameter covariances and model moments of the chain)."""
        return _calls._sample_posterior(self, None, **kw)


def par_names(short, ncomp=None):
    if ncomp is not None:
        return [f'{label}{n}' for label in short for n in range(1, ncomp + 1)]
    return short
