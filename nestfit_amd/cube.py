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
import numpy as np

from . import _calls, _diagnostics, _ffi
from ._model import RunnerSurface, _RunnerHandle, _SpecSet, apply_options, check_options, signed_peak


def get_multiproc_indices(shape, nproc):
    """Same striping as the reference (nestfit/main.py:565-571)."""
    lon_ix, lat_ix = np.indices(shape)
    return [(lon_ix[i::nproc, ...].flatten(), lat_ix[i::nproc, ...].flatten()) for i in range(nproc)]


def shard_pixels(shape, rank, world):
    """(lon, lat) index arrays of the pixels owned by `rank` (i_lon % world == rank)."""
    if min(shape) < 1 or not (0 <= rank < world):
        raise ValueError('invalid shard request')
    return get_multiproc_indices(shape, world)[rank]


class CubeRunner(RunnerSurface):
    """AmmoniaRunner semantics for many pixels that share their frequency axes.  The likelihood options below are read-only
    properties of their names and have setters (`set_robust`, ..., `set_baseline`: `_model.SURFACE`).

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
        as one more, the last (`LteMix(species, fill=True)`; one species included).  5 excitation grid (then `lines` = one
        `GridLines` per spectrum, all on one `ExcitationGrid`; five parameters per component).  options: the likelihood options
        above."""
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
        self._read_null_lnZ()

    def _read_null_lnZ(self):
        self.null_lnZ = self._ss.null_lnZ().sum(axis=1)      # per pixel

    def loglikelihood_batch(self, pix, U, out=None):
        """lnL[B] of unit-cube rows U[B, ndim] against pixels pix[B]; U is overwritten
        with the physical parameters (like Runner.loglikelihood, core.pyx:558-561).  `out`: where lnL goes;
        arrays from `nestfit_amd.pinned_empty` are used by the kernels in place (no copies)."""
        U = _calls.unit_rows(self, U)
        pix = _calls.pixel_indices(pix, U.shape[0])
        lnL = _calls.out_array(out, (U.shape[0],), 'of one value per row')
        _ffi.check(_ffi.load().nfa_runner_loglike_batch(self._run.handle, pix.ctypes.data_as(_ffi._ip),
                                                        _ffi.dptr(U), _ffi.dptr(lnL), U.shape[0]))
        return lnL

    def predict_batch(self, pix, theta, want_spectra=True, out=None):
        """Model spectra [B, n_chan_tot] and lnL[B] of physical parameter rows theta[B, ndim]
        against pixels pix[B]: `runner.predict` for many pixels at once (the spectra-out mode of
        the post-processing, nestfit/main.py:1106-1113, 1186).  `out`: where the spectra go; an array from
        `nestfit_amd.pinned_empty` is written by the kernel itself (no staging copy of B x n_chan_tot doubles)."""
        theta = _calls.parameter_rows(self, theta)
        B = theta.shape[0]
        pix = _calls.pixel_indices(pix, B)
        spec = _calls.out_array(out, (B, self.n_chan_tot), '[B, n_chan_tot]') if want_spectra else None
        lnl = np.empty(B)
        _ffi.check(_ffi.load().nfa_runner_predict_batch(
            self._run.handle, pix.ctypes.data_as(_ffi._ip), _ffi.dptr(theta), B,
            _ffi.dptr(spec) if want_spectra else None, _ffi.dptr(lnl)))
        return spec, lnl

    def _diagnose(self, which, pix, theta, **how):
        """`_diagnostics.fit_<which>` on the rows of the points (pix[B], theta[B, ndim]): the pixels' data and noise and
        `predict_batch`'s spectra -- behind a channel response the filtered model."""
        _diagnostics.require(which, self._ss.options)
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        spec, _ = self.predict_batch(pix, theta)
        return getattr(_diagnostics, 'fit_' + which)(np.asarray(self._data, dtype=np.float64)[pix],
                                                     np.asarray(self._noise, dtype=np.float64)[pix], spec, self._ss.offsets,
                                                     self._ss.options, **how)

    def fit_baseline(self, pix, theta):
        """Best-fit baselines [B, n_chan_tot] of physical parameter rows theta[B, ndim] against pixels pix[B]: the
        polynomials the likelihood profiles out, fitted with numpy to data - predict_batch (for residual plots, not the
        hot path).  A runner with nuisance templates returns the whole nuisance curve, polynomial and templates.  ValueError
        without a baseline and without templates."""
        return self._diagnose('baseline', pix, theta)

    def fit_templates(self, pix, theta):
        """Best-fit amplitudes of the templates, in the caller's scaling, of physical parameter rows theta[B, ndim] against
        pixels pix[B]: a list of n_spec arrays [B, T].  numpy on `predict_batch`'s spectra.  ValueError without templates."""
        return self._diagnose('templates', pix, theta)

    def fit_gain(self, pix, theta):
        """Posterior mean and standard deviation [B, n_spec] each of the spectra's gains at physical parameter rows
        theta[B, ndim] against pixels pix[B] (1 and 0 where a spectrum's uncertainty is 0): numpy on `predict_batch`'s
        spectra, with `fit_baseline`'s projection where there is a baseline.  ValueError without a calibration."""
        return self._diagnose('gain', pix, theta)

    def fit_noise(self, pix, theta):
        """Posterior mean and standard deviation [B, n_spec] each of the spectra's noise scales t (true noise = t * stated
        noise) at physical parameter rows theta[B, ndim] against pixels pix[B] (1 and 0 where a spectrum's uncertainty is
        0): numpy on `predict_batch`'s spectra (`half_chi2`, `noise_fit`).  ValueError without a noise uncertainty."""
        return self._diagnose('noise', pix, theta, filtered=True)

    def fit_outliers(self, pix, theta):
        """Every channel's posterior mean precision factor (nu + 1) / (nu + r_j^2 / sigma_j^2), [B, chan_tot], at physical
        parameter rows theta[B, ndim] against pixels pix[B]: about 1 for a good channel, towards 0 for one the fit distrusted
        (1 in a spectrum with nu = 0, NaN at a masked channel).  numpy on `predict_batch`'s spectra (`robust_outliers`).
        ValueError without a robust likelihood."""
        return self._diagnose('outliers', pix, theta)

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
        theta = _calls.parameter_rows(self, theta)
        return _calls._row_statistics(self._run.handle, _calls.pixel_indices(pix, theta.shape[0]), theta, self.n_spec)

    def predict_moments(self, pix, offsets, theta, weights=None, chunk_rows=None, want_spectra=True):
        """Weighted moments of the model spectra over segments of parameter rows: segment g is the rows
        offsets[g] .. offsets[g + 1] - 1 of theta[rows, ndim] (physical parameters, as for `predict_batch`), all of pixel
        pix[g], with weights[rows] >= 0 (None: all ones) -- a pixel's weighted posterior sample, say.  Returns a
        `PosteriorMoments` record: mean, std [n_seg, n_chan_tot] (None without `want_spectra`) and peak_mean, peak_std,
        total_mean, total_std [n_seg, n_spec], the moments of `row_statistics`' two numbers.  NaN for a segment without rows
        or whose weights sum to 0.  The rows are predicted `chunk_rows` at a time (None: 4096; a multiple of 64) and
        reduced on the device; `nestfit_amd.moments` is the same arithmetic in numpy on given spectra."""
        theta = _calls.parameter_rows(self, theta)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or offsets.size < 1:
            raise ValueError('offsets must hold n_seg + 1 row numbers')
        if offsets[-1] != theta.shape[0]:
            raise ValueError('the last offset must be the number of rows of theta')
        pix = _calls.pixel_indices(pix, offsets.size - 1, per='segment')
        return _calls._predict_moments(self._run.handle, pix, offsets, theta, weights, chunk_rows, want_spectra,
                                       self.n_chan_tot, self.n_spec)

    def normal_equations(self, pix, theta, step, lower=None, upper=None, chunk_rows=None, want_curvature=True):
        """The normal equations of a least-squares fit at the points (pix[B], theta[B, ndim]): a
        `NormalEquations` record of chi2[B] = sum W r^2, grad[B, ndim] = J^T W r (minus half the gradient of chi^2) and
        curv[B, ndim, ndim] = J^T W J (None without `want_curvature`), with r = data - model, W the channels' inverse
        variances and J the central difference of `predict_batch`'s spectra over theta_k +- step[k], the probes clipped
        into [lower[k], upper[k]] where those are given (a parameter whose probes coincide is fixed: a zero row and column).
        The probe rows are predicted `chunk_rows` at a time (None: 4096; a multiple of 64 and at least 1 + 2 ndim) and
        reduced on the device; `nestfit_amd.lsq.normal_equations_from_spectra` is the same arithmetic in numpy."""
        theta = _calls.parameter_rows(self, theta)
        return _calls._normal_equations(self._run.handle, _calls.pixel_indices(pix, theta.shape[0]), theta, step, lower, upper,
                                        chunk_rows, want_curvature)

    def chi_squared(self, pix, theta):
        """chi2[B] = sum W (data - model)^2 of the points (pix[B], theta[B, ndim]): `normal_equations`' chi2, the same
        bits, from one predicted row per point."""
        theta = _calls.parameter_rows(self, theta)
        return _calls._normal_equations(self._run.handle, _calls.pixel_indices(pix, theta.shape[0]), theta, None, None, None, None,
                                        False, want_grad=False).chi2

    def sample_posterior(self, pix, **kw):
        """The posteriors of the pixels pix[P] at the runner's component count by ensemble MCMC on the device: an
        `EnsembleResult` of one row per pixel (`nestfit_amd.ensemble.sample_pixels`' keywords; `par_bins`,
        `covariance`, `moments`: the marginal histograms, parameter covariances and model moments of the chain)."""
        return _calls._sample_posterior(self, np.ascontiguousarray(pix, dtype=np.int32), **kw)

