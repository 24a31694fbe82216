"""Pixel sharding of a cube over GPUs (one process per GPU) and the device-
resident multi-pixel runner.

The reference fits map pixels independently and stripes them over processes with
``(lon_ix[i::nproc], lat_ix[i::nproc])`` (nestfit/main.py:565-571); each process
writes its own chunk file and nothing is exchanged while sampling
(nestfit/main.py:423-474, docs/store_spec.rst:12-32).  Here rank r owns the same
stripe, uploads its pixels once and evaluates batches of (pixel, unit-cube row)
items.  The only collective is the end-of-run gather of fixed-size per-pixel
records (`nestfit_amd.comm`: RCCL over xGMI through the engine's C ABI).
"""
import ctypes as C

import numpy as np

from . import _ffi
from ._model import _RunnerHandle, _SpecSet, apply_options, baseline_fit, check_options, gain_fit, half_chi2, noise_fit, nuisance_fit, robust_outliers, signed_peak
from .core import _as_inplace_matrix


def get_multiproc_indices(shape, nproc):
    """Same striping as the reference (nestfit/main.py:565-571)."""
    lon_ix, lat_ix = np.indices(shape)
    return [(lon_ix[i::nproc, ...].flatten(), lat_ix[i::nproc, ...].flatten()) for i in range(nproc)]


def shard_pixels(shape, rank, world):
    """(lon, lat) index arrays of the pixels owned by `rank` (i_lon % world == rank)."""
    if min(shape) < 1 or not (0 <= rank < world):
        raise ValueError('invalid shard request')
    return get_multiproc_indices(shape, world)[rank]


class CubeRunner:
    """AmmoniaRunner semantics for many pixels that share their frequency axes.

    Parameters
    ----------
    xarrs : list of 1-D frequency axes (Hz, ascending), one per transition
    trans_ids : list of int
    data : array [n_pix, sum(len(x) for x in xarrs)], K, spectra concatenated per pixel
    noise : array [n_pix, n_spec], K; or [n_pix, sum(len(x) for x in xarrs)], a noise per channel
        (inf masks a channel, whose data are then ignored: see `core.Spectrum`)
    utrans : PriorTransformer
    baseline_order : None, or 0..3: a polynomial baseline of that degree per (pixel, spectrum), profiled out of the
        likelihood in closed form; null_lnZ is then the baseline-only model's
    layered : layered radiative transfer: component 0 is the farthest from the observer and every component
        absorbs those behind it; False (default): the components are summed.  Not for the Gaussian model (ValueError).
    calibration : None, or the fractional 1-sigma uncertainty of the spectra's intensity scales (a number, or one per
        spectrum, each in [0, 1]; shared by all pixels), integrated out of the likelihood per (pixel, spectrum) in closed
        form; null_lnZ is unchanged
    correlation : None, or the first two autocorrelations (rho_1, rho_2) of the channel noise along the spectral axis (a pair
        such as `HANNING` or `ar1(rho)`, or an array [n_spec, 2]; shared by all pixels) for cubes that were smoothed, regridded
        or oversampled; not with masked channels, a baseline or a calibration; null_lnZ follows
    response : None, or the channel response of the spectrometer (3 or 5 taps such as `HANNING_RESPONSE`, or an array
        [n_spec, 3 | 5]; shared by all pixels) with which the model is convolved before it meets the data; not
        with masked channels, a baseline or a calibration; null_lnZ is unchanged
    templates : None, or a list with one entry per spectrum, each None or an array [T, N_s] of 1..4 fixed shapes on the
        spectrum's channels (`ripple(n_chan, period)`: a standing wave of known period; shared by all pixels) whose amplitudes
        are profiled out of the likelihood per (pixel, spectrum) together with the baseline; not with a
        calibration, a correlation or a response; null_lnZ is then the model of baseline and templates alone
    robust : None, or the degrees of freedom of Student-t channel noise (a number, or one per spectrum, each 0 -- Gaussian -- or
        in [1, 1e6]; shared by all pixels): spikes and unflagged bad channels cost the logarithm of their residual (DESIGN
        4.18); with none of the other likelihood options; null_lnZ is the same expression at p = 0
    noise_uncertainty : None, or the fractional 1-sigma uncertainty of the spectra's noise levels (a number, or one per
        spectrum, each in [0, 0.5]; shared by all pixels), integrated out of the likelihood per (pixel, spectrum) in closed
        form; with everything but a calibration; null_lnZ is the same function of the parts at p = 0
    continuum : None, or the brightness temperature Tc >= 0 (K) of a continuum source behind all components: a number, one
        value per spectrum or an array [n_pix, n_spec], from the continuum map that was subtracted from the data -- data, not
        a parameter; the line goes negative wherever J(tex) < J(Tcmb) + Tc; not with the Gaussian model, a
        calibration, a correlation, a response or templates; null_lnZ is unchanged
    """

    def __init__(self, xarrs, trans_ids, data, noise, utrans, ncomp=1, cold=False, lte=False,
                 model=0, rest_freqs=None, *, lines=None, species=None, fill=False, **options):
        """model: 0 ammonia (default), 1 diazenylium, 2 gaussian (then `rest_freqs` = [Hz]), 3 hyperfine (then `lines` =
        one `LineTable` per spectrum; `trans_ids` is not used), 4 LTE (then `lines` = one `LteLines`, or one `LteBand` of several
        transitions, per spectrum, all of one `Molecule`; or, an LTE mix, `lines` = an `LteLines`, `LteBand` or `LteBlend` per
        spectrum of the ordered `Molecule`s `species` -- without `species`, lines of several molecules take them in the order of
        their first appearance).  An LTE mix has 3 + len(species) parameters per component; fill: and a beam filling factor
        as one more, the last (`LteMix(species, fill=True)`; one species included).  options: the likelihood options above."""
        assert ncomp > 0
        sizes = [np.size(x) for x in xarrs]
        masked = np.shape(noise)[-1] == sum(sizes) and not np.all(np.isfinite(noise))
        options = check_options(options, len(xarrs), sizes, masked, model, int(np.shape(data)[0]),      # before any device call
                                caller='CubeRunner.__init__')
        if species is None and int(model) == 4 and lines is not None:
            from .lte import LteBand, LteBlend, LteLines, lines_species
            lines = list(lines)
            if all(isinstance(t, (LteLines, LteBand, LteBlend)) for t in lines):
                found = lines_species(lines)
                if len(found) > 1 or fill or any(isinstance(t, LteBlend) for t in lines):
                    species = found
        self._ss = _SpecSet(xarrs, trans_ids, data, noise, model=model, rest_freqs=rest_freqs, lines=lines, species=species,
                            fill=fill)
        self._run = _RunnerHandle(self._ss, utrans, ncomp, cold, lte)
        self.layered, self.baseline_order = options.layered, options.baseline_order
        apply_options(options, self._ss)
        self._data, self._noise = data, noise                # (fit_baseline, fit_gain, fit_noise)
        self.utrans = utrans
        self.ncomp = int(ncomp)
        self.n_model = self._ss.n_model                      # (an LTE mix: from the species of its lines, not from N_MODEL)
        self.n_params = self.ndim = self.n_model * self.ncomp
        self.n_pix = self._ss.n_pix
        self.n_spec = self._ss.n_spec
        self.n_chan_tot = self._ss.chan_tot
        self.n_chan = self._ss.n_chan                        # per pixel: the channels that enter the likelihood
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)      # per pixel

    def set_exp_mode(self, mode):
        """Numerical mode of this runner alone (None: the process default again)."""
        self._run.set_exp_mode(mode)

    def loglikelihood_batch(self, pix, U, out=None):
        """lnL[B] of unit-cube rows U[B, ndim] against pixels pix[B]; U is overwritten
        with the physical parameters (like Runner.loglikelihood, core.pyx:558-561).  `out`: where lnL goes;
        arrays from `nestfit_amd.pinned_empty` are used by the kernels in place (no copies)."""
        U = _as_inplace_matrix(U)
        if U.shape[1] != self.ndim:
            raise ValueError(f'Invalid shape for ncomp={self.ncomp}: {U.shape[1]}')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        if pix.shape != (U.shape[0],):
            raise ValueError('one pixel index per row is required')
        lnL = np.empty(U.shape[0]) if out is None else out
        if lnL.shape != (U.shape[0],) or lnL.dtype != np.float64 or not lnL.flags.c_contiguous:
            raise ValueError('out must be a contiguous float64 array of one value per row')
        _ffi.check(_ffi.load().nfa_runner_loglike_batch(self._run.handle, pix.ctypes.data_as(_ffi._ip),
                                                        _ffi.dptr(U), _ffi.dptr(lnL), U.shape[0]))
        return lnL


    def predict_batch(self, pix, theta, want_spectra=True, out=None):
        """Model spectra [B, n_chan_tot] and lnL[B] of physical parameter rows theta[B, ndim]
        against pixels pix[B]: `runner.predict` for many pixels at once (the spectra-out mode of
        the post-processing, nestfit/main.py:1106-1113, 1186).  `out`: where the spectra go; an array from
        `nestfit_amd.pinned_empty` is written by the kernel itself (no staging copy of B x n_chan_tot doubles)."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.ndim:
            raise ValueError(f'Invalid shape for ncomp={self.ncomp}: {theta.shape}')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        if pix.shape != (theta.shape[0],):
            raise ValueError('one pixel index per row is required')
        B = theta.shape[0]
        spec = (np.empty((B, self.n_chan_tot)) if out is None else out) if want_spectra else None
        if spec is not None and (spec.shape != (B, self.n_chan_tot) or spec.dtype != np.float64 or not spec.flags.c_contiguous):
            raise ValueError('out must be a contiguous float64 array [B, n_chan_tot]')
        lnl = np.empty(B)
        _ffi.check(_ffi.load().nfa_runner_predict_batch(
            self._run.handle, pix.ctypes.data_as(_ffi._ip), _ffi.dptr(theta), B,
            _ffi.dptr(spec) if want_spectra else None, _ffi.dptr(lnl)))
        return spec, lnl

    def fit_baseline(self, pix, theta):
        """Best-fit baselines [B, n_chan_tot] of physical parameter rows theta[B, ndim] against pixels pix[B]: the
        polynomials the likelihood profiles out, fitted with numpy to data - predict_batch (for residual plots, not the
        hot path).  A runner with nuisance templates returns the whole nuisance curve, polynomial and templates.  ValueError
        without a baseline and without templates."""
        if self._ss.templates is not None:
            return self._fit_nuisance(pix, theta)[0]
        if self.baseline_order is None:
            raise ValueError('this runner has no baseline (baseline_order=None)')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        spec, _ = self.predict_batch(pix, theta)
        data = np.asarray(self._data, dtype=np.float64)[pix]
        noise = np.asarray(self._noise, dtype=np.float64)[pix]
        off = self._ss.offsets
        out = np.empty_like(spec)
        for k in range(self.n_spec):
            sl = slice(off[k], off[k + 1])
            w = 1.0 / noise[:, sl] ** 2 if self._ss.per_channel else np.ones_like(spec[:, sl])
            resid = np.where(w > 0, data[:, sl] - spec[:, sl], 0.0)
            out[:, sl] = baseline_fit(resid, w, self.baseline_order)
        return out

    def _fit_nuisance(self, pix, theta):
        """(curves [B, n_chan_tot], amplitudes: per spectrum [B, T]) of `nuisance_fit` on data - predict_batch."""
        tmpl = self._ss.templates
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        spec, _ = self.predict_batch(pix, theta)
        data = np.asarray(self._data, dtype=np.float64)[pix]
        noise = np.asarray(self._noise, dtype=np.float64)[pix]
        off = self._ss.offsets
        out = np.empty_like(spec)
        amps = [np.zeros((len(pix), 0 if t is None else t.shape[0])) for t in tmpl]
        for k in range(self.n_spec):
            sl = slice(off[k], off[k + 1])
            for b in range(len(pix)):
                w = 1.0 / noise[b, sl] ** 2 if self._ss.per_channel else np.ones(off[k + 1] - off[k])
                resid = np.where(w > 0, data[b, sl] - spec[b, sl], 0.0)
                out[b, sl], amps[k][b] = nuisance_fit(resid, w, self.baseline_order, tmpl[k])
        return out, amps

    def fit_templates(self, pix, theta):
        """Best-fit amplitudes of the templates, in the caller's scaling, of physical parameter rows theta[B, ndim] against
        pixels pix[B]: a list of n_spec arrays [B, T].  numpy on `predict_batch`'s spectra.  ValueError without templates."""
        if self._ss.templates is None:
            raise ValueError('this runner has no nuisance templates (templates=None)')
        return self._fit_nuisance(pix, theta)[1]

    @property
    def templates(self):
        """None, or the list of the spectra's nuisance templates: per spectrum None or a float64 array [T, N_s]."""
        tmpl = self._ss.templates
        return None if tmpl is None else [None if a is None else a.copy() for a in tmpl]

    def set_templates(self, tmpl):
        """Sets (a list with an array [T, N_s] or None per spectrum) or removes (None) the nuisance templates; null_lnZ
        follows."""
        self._ss.set_templates(tmpl)
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)

    def set_baseline(self, order):
        """Sets (0..3) or removes (None) the baseline; null_lnZ follows."""
        self._ss.set_baseline(order)
        self.baseline_order = self._ss.baseline_order
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)

    @property
    def response(self):
        """None, or the float64 array [n_spec, 5] of the spectra's channel responses (h_-2 .. h_2)."""
        resp = self._ss.response
        return None if resp is None else resp.copy()

    def set_response(self, resp):
        """Sets (3 or 5 taps, or such a row per spectrum) or removes (None, the identity) the channel response; null_lnZ is
        untouched."""
        self._ss.set_response(resp)

    @property
    def correlation(self):
        """None, or the float64 array [n_spec, 2] of the spectra's noise autocorrelations (rho_1, rho_2)."""
        corr = self._ss.correlation
        return None if corr is None else corr.copy()

    def set_correlation(self, corr):
        """Sets (a pair, or one per spectrum) or removes (None, zeros) the noise correlation; null_lnZ follows."""
        self._ss.set_correlation(corr)
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)

    @property
    def calibration(self):
        """None, or the float64 array of the spectra's fractional calibration uncertainties."""
        cal = self._ss.calibration
        return None if cal is None else cal.copy()

    def fit_gain(self, pix, theta):
        """Posterior mean and standard deviation [B, n_spec] each of the spectra's gains at physical parameter rows
        theta[B, ndim] against pixels pix[B] (1 and 0 where a spectrum's uncertainty is 0): numpy on `predict_batch`'s
        spectra, with `fit_baseline`'s projection where there is a baseline.  ValueError without a calibration."""
        cal = self.calibration
        if cal is None:
            raise ValueError('this runner has no calibration uncertainty (calibration=None)')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        spec, _ = self.predict_batch(pix, theta)
        data = np.asarray(self._data, dtype=np.float64)[pix]
        noise = np.asarray(self._noise, dtype=np.float64)[pix]
        off = self._ss.offsets
        mean, std = np.ones((len(pix), self.n_spec)), np.zeros((len(pix), self.n_spec))
        for k in range(self.n_spec):
            sl = slice(off[k], off[k + 1])
            for b in range(len(pix)):
                w = 1.0 / noise[b, sl] ** 2 if self._ss.per_channel else np.ones(off[k + 1] - off[k])
                sigma = 1.0 if self._ss.per_channel else noise[b, k]
                mean[b, k], std[b, k] = gain_fit(data[b, sl], spec[b, sl], w, sigma, cal[k], self.baseline_order)
        return mean, std

    @property
    def robust(self):
        """None, or the float64 array [n_spec] of the degrees of freedom of the spectra's Student-t channel noise."""
        nu = self._ss.robust
        return None if nu is None else nu.copy()

    def set_robust(self, nu):
        """Sets (a number, or one per spectrum) or removes (None, zeros) the robust likelihood; null_lnZ
        follows."""
        self._ss.set_robust(nu)
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)

    def fit_outliers(self, pix, theta):
        """Every channel's posterior mean precision factor (nu + 1) / (nu + r_j^2 / sigma_j^2), [B, chan_tot], at physical
        parameter rows theta[B, ndim] against pixels pix[B]: about 1 for a good channel, towards 0 for one the fit distrusted
        (1 in a spectrum with nu = 0, NaN at a masked channel).  numpy on `predict_batch`'s spectra (`robust_outliers`).
        ValueError without a robust likelihood."""
        nu = self.robust
        if nu is None:
            raise ValueError('this runner has no robust likelihood (robust=None)')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        spec, _ = self.predict_batch(pix, theta)
        data = np.asarray(self._data, dtype=np.float64)[pix]
        noise = np.asarray(self._noise, dtype=np.float64)[pix]
        off = self._ss.offsets
        out = np.empty_like(spec)
        for k in range(self.n_spec):
            sl = slice(off[k], off[k + 1])
            out[:, sl] = robust_outliers(data[:, sl], spec[:, sl], noise[:, sl] if self._ss.per_channel else noise[:, k:k + 1], nu[k])
        return out

    @property
    def continuum(self):
        """None, or the float64 array [n_pix, n_spec] of the continuum brightness temperatures behind the spectra (K)."""
        tc = self._ss.continuum
        return None if tc is None else tc.copy()

    def set_continuum(self, tc):
        """Sets (a number, one value per spectrum or [n_pix, n_spec], in K) or removes (None, zeros) the continuum background;
        null_lnZ is read again and does not change: the null model has no absorber."""
        self._ss.set_continuum(tc)
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)

    @property
    def noise_uncertainty(self):
        """None, or the float64 array of the fractional uncertainties of the spectra's noise levels."""
        f = self._ss.noise_uncertainty
        return None if f is None else f.copy()

    def set_noise_uncertainty(self, f):
        """Sets (a number, or one per spectrum) or removes (None, zeros) the uncertainty of the spectra's noise levels;
        null_lnZ follows."""
        self._ss.set_noise_uncertainty(f)
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)

    def fit_noise(self, pix, theta):
        """Posterior mean and standard deviation [B, n_spec] each of the spectra's noise scales t (true noise = t * stated
        noise) at physical parameter rows theta[B, ndim] against pixels pix[B] (1 and 0 where a spectrum's uncertainty is
        0): numpy on `predict_batch`'s spectra (`half_chi2`, `noise_fit`).  ValueError without a noise uncertainty."""
        f = self.noise_uncertainty
        if f is None:
            raise ValueError('this runner has no noise uncertainty (noise_uncertainty=None)')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        spec, _ = self.predict_batch(pix, theta)
        data = np.asarray(self._data, dtype=np.float64)[pix]
        noise = np.asarray(self._noise, dtype=np.float64)[pix]
        off = self._ss.offsets
        tmpl, corr, resp = self._ss.templates, self._ss.correlation, self._ss.response
        mean, std = np.ones((len(pix), self.n_spec)), np.zeros((len(pix), self.n_spec))
        for k in range(self.n_spec):
            sl = slice(off[k], off[k + 1])
            for b in range(len(pix)):
                h, nu = half_chi2(data[b, sl], spec[b, sl], noise[b, sl] if self._ss.per_channel else noise[b, k],
                                  self.baseline_order, None if tmpl is None else tmpl[k], None if corr is None else corr[k],
                                  None if resp is None else resp[k])
                mean[b, k], std[b, k] = noise_fit(h, nu, f[k])
        return mean, std

    def peak_and_integrated(self, pix, theta):
        """max_spec and sum_spec of every spectrum for parameter rows (core.pyx:532-539 as
        `deblend_hf_intensity` uses them, main.py:1110-1113): two arrays [B, n_spec].  A runner with a continuum background
        returns the signed value of largest magnitude (`signed_peak`) in place of the maximum: the line may absorb."""
        if getattr(self, '_scratch_spec', None) is None or self._scratch_spec.shape[0] < theta.shape[0]:
            self._scratch_spec = _ffi.pinned_empty((max(theta.shape[0], 1), self.n_chan_tot))
        spec, _ = self.predict_batch(pix, theta, out=self._scratch_spec[:theta.shape[0]])
        off = self._ss.offsets
        top = np.nanmax if self._ss.continuum is None else signed_peak
        peak = np.stack([top(spec[:, off[k]:off[k + 1]], axis=1) for k in range(self.n_spec)], axis=1)
        tot = np.stack([np.nansum(spec[:, off[k]:off[k + 1]], axis=1) for k in range(self.n_spec)], axis=1)
        return peak, tot

    def row_statistics(self, pix, theta):
        """(peak, total), [B, n_spec] each, of the model spectra of parameter rows theta[B, ndim] against pixels pix[B]:
        the numbers of `peak_and_integrated`, formed on the device (csrc/nfa_moments.h: row_stats_kernel) -- the spectra do
        not cross the bus.  peak is the same to the bit; total is the sum of the same channels in another order."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.ndim:
            raise ValueError(f'Invalid shape for ncomp={self.ncomp}: {theta.shape}')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        if pix.shape != (theta.shape[0],):
            raise ValueError('one pixel index per row is required')
        return _row_statistics(self._run.handle, pix, theta, self.n_spec)

    def predict_moments(self, pix, offsets, theta, weights=None, chunk_rows=None, want_spectra=True):
        """Weighted moments of the model spectra over segments of parameter rows: segment g is the rows
        offsets[g] .. offsets[g + 1] - 1 of theta[rows, ndim] (physical parameters, as for `predict_batch`), all of pixel
        pix[g], with weights[rows] >= 0 (None: all ones) -- a pixel's weighted posterior sample, say.  Returns a
        `PosteriorMoments` record: mean, std [n_seg, n_chan_tot] (None without `want_spectra`) and peak_mean, peak_std,
        total_mean, total_std [n_seg, n_spec], the moments of `row_statistics`' two numbers.  NaN for a segment without rows
        or whose weights sum to 0.  The rows are predicted `chunk_rows` at a time (None: 4096; a multiple of 64) and
        reduced on the device; `nestfit_amd.moments` is the same arithmetic in numpy on given spectra."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.ndim:
            raise ValueError(f'Invalid shape for ncomp={self.ncomp}: {theta.shape}')
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or offsets.size < 1:
            raise ValueError('offsets must hold n_seg + 1 row numbers')
        if offsets[-1] != theta.shape[0]:
            raise ValueError('the last offset must be the number of rows of theta')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        if pix.shape != (offsets.size - 1,):
            raise ValueError('one pixel index per segment is required')
        return _predict_moments(self._run.handle, pix, offsets, theta, weights, chunk_rows, want_spectra,
                                self.n_chan_tot, self.n_spec)

    def normal_equations(self, pix, theta, step, lower=None, upper=None, chunk_rows=None, want_curvature=True):
        """The normal equations of a least-squares fit at the points (pix[B], theta[B, ndim]): a
        `NormalEquations` record of chi2[B] = sum W r^2, grad[B, ndim] = J^T W r (minus half the gradient of chi^2) and
        curv[B, ndim, ndim] = J^T W J (None without `want_curvature`), with r = data - model, W the channels' inverse
        variances and J the central difference of `predict_batch`'s spectra over theta_k +- step[k], the probes clipped
        into [lower[k], upper[k]] where those are given (a parameter whose probes coincide is fixed: a zero row and column).
        The probe rows are predicted `chunk_rows` at a time (None: 4096; a multiple of 64 and at least 1 + 2 ndim) and
        reduced on the device; `nestfit_amd.lsq.normal_equations_from_spectra` is the same arithmetic in numpy."""
        pix, theta = self._lsq_points(pix, theta)
        return _normal_equations(self._run.handle, pix, theta, step, lower, upper, chunk_rows, want_curvature)

    def chi_squared(self, pix, theta):
        """chi2[B] = sum W (data - model)^2 of the points (pix[B], theta[B, ndim]): `normal_equations`' chi2, the same
        bits, from one predicted row per point."""
        pix, theta = self._lsq_points(pix, theta)
        return _normal_equations(self._run.handle, pix, theta, None, None, None, None, False, want_grad=False).chi2

    def _lsq_points(self, pix, theta):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != self.ndim:
            raise ValueError(f'Invalid shape for ncomp={self.ncomp}: {theta.shape}')
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        if pix.shape != (theta.shape[0],):
            raise ValueError('one pixel index per row is required')
        return pix, theta


def _row_statistics(handle, pix, theta, n_spec):
    """nfa_runner_row_statistics on checked arrays (pix: int32[B] or None)."""
    B = theta.shape[0]
    peak, total = np.empty((B, n_spec)), np.empty((B, n_spec))
    _ffi.check(_ffi.load().nfa_runner_row_statistics(handle, None if pix is None else pix.ctypes.data_as(_ffi._ip),
                                                     _ffi.dptr(theta), B, _ffi.dptr(peak), _ffi.dptr(total)))
    return peak, total


def _normal_equations(handle, pix, theta, step, lower, upper, chunk_rows, want_curvature, want_grad=True):
    """nfa_runner_normal_equations on checked points (pix: int32[B] or None; theta: float64[B, ndim]) -> `NormalEquations`."""
    from .lsq import NormalEquations
    B, ndim = theta.shape

    def vector(a, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (ndim,):
            raise ValueError(f'{name} must hold one value per parameter')
        return a
    step, lower, upper = vector(step, 'step'), vector(lower, 'lower'), vector(upper, 'upper')
    chi2 = np.empty(B)
    grad = np.empty((B, ndim)) if want_grad else None
    curv = np.empty((B, ndim, ndim)) if want_curvature else None
    opt = lambda a: None if a is None else _ffi.dptr(a)
    _ffi.check(_ffi.load().nfa_runner_normal_equations(
        handle, None if pix is None else pix.ctypes.data_as(_ffi._ip), _ffi.dptr(theta), B, opt(step), opt(lower), opt(upper),
        0 if chunk_rows is None else int(chunk_rows), _ffi.dptr(chi2), opt(grad), opt(curv)))
    return NormalEquations(chi2, grad, curv)


def _predict_moments(handle, pix, offsets, theta, weights, chunk_rows, want_spectra, n_chan_tot, n_spec):
    """nfa_runner_predict_moments on checked arrays (pix: int32[n_seg] or None) -> `PosteriorMoments`."""
    from .moments import PosteriorMoments
    n_seg = offsets.size - 1
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (theta.shape[0],):
            raise ValueError('one weight per row is required')
    mean = np.empty((n_seg, n_chan_tot)) if want_spectra else None
    std = np.empty((n_seg, n_chan_tot)) if want_spectra else None
    smean, sstd = np.empty((n_seg, n_spec, 2)), np.empty((n_seg, n_spec, 2))
    opt = lambda a: None if a is None else _ffi.dptr(a)
    _ffi.check(_ffi.load().nfa_runner_predict_moments(
        handle, n_seg, None if pix is None else pix.ctypes.data_as(_ffi._ip), offsets.ctypes.data_as(_ffi._lp),
        _ffi.dptr(theta), opt(weights), 0 if chunk_rows is None else int(chunk_rows), opt(mean), opt(std),
        _ffi.dptr(smean), _ffi.dptr(sstd)))
    return PosteriorMoments(mean, std, smean[:, :, 0].copy(), sstd[:, :, 0].copy(), smean[:, :, 1].copy(), sstd[:, :, 1].copy())
