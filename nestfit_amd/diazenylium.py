"""Host-side mirror of ``nestfit.models.diazenylium`` (reference:
nestfit/models/diazenylium.pyx:108-264): N2H+ J = 1-0, 2-1, 3-2 with 15 / 40 / 45
hyperfine lines on the same device kernels as ammonia (c_hf_predict,
nestfit/models/hyperfine.pyx:52-118).  Parameters per component: voff, tex, ltau, sigm.
"""
import numpy as np

from ._model import MODEL_DIAZENYLIUM, EngineRunner, EngineSpectrumMixin, check_baseline_order, check_calibration, check_continuum, check_robust, check_correlation, check_noise_uncertainty, check_layered, check_response, check_templates, spec_data_sizes_masked, par_names
from .core import HyperfineSpectrum

N_LEVELS = 3
N_PARAMS = 4


class DiazenyliumSpectrum(EngineSpectrumMixin, HyperfineSpectrum):
    """N2H+ spectrum (reference: diazenylium.pyx:108-136).

    Parameters
    ----------
    xarr : array, Hz, ascending
    data : array, K
    noise : number, K
    trans_id : 1 -> (1-0), 2 -> (2-1), 3 -> (3-2)
    """
    MODEL = MODEL_DIAZENYLIUM

    def __init__(self, xarr, data, noise, trans_id=1):
        assert trans_id in range(1, N_LEVELS + 1)
        # the reference passes rest_freq=self.trans.nu before trans is assigned: 0 (diazenylium.pyx:129-131)
        HyperfineSpectrum.__init__(self, xarr, data, noise, rest_freq=0.0, trans_id=trans_id)
        self._attach(trans_id)

    @property
    def tbg_arr(self):
        return self._ss.tbg()


def nnhp_predict(s, params):
    """Model spectrum of `s` for parameter-major `params` (reference:
    diazenylium.pyx:138-158); result in ``s.get_spec()`` / ``s.loglikelihood``."""
    s._predict(params, N_PARAMS)


class DiazenyliumRunner(EngineRunner):
    """Prior transform + model + log-likelihood (reference: diazenylium.pyx:161-231)."""
    MODEL = MODEL_DIAZENYLIUM
    N_MODEL = N_PARAMS

    def __init__(self, spectra, utrans, ncomp=1, baseline_order=None, layered=False, calibration=None, correlation=None, response=None, templates=None,
                 noise_uncertainty=None, continuum=None, robust=None):
        assert ncomp > 0
        baseline_order = check_baseline_order(baseline_order)
        layered = check_layered(layered)
        self.spectra = list(spectra)
        self._setup(self.spectra, utrans, ncomp, baseline_order=baseline_order, layered=layered,
                    calibration=calibration, correlation=correlation, response=response, templates=templates,
                    noise_uncertainty=noise_uncertainty, continuum=continuum, robust=robust)

    @classmethod
    def from_data(cls, spec_data, utrans, **kwargs):
        check_baseline_order(kwargs.get('baseline_order'))            # before any device call
        check_layered(kwargs.get('layered', False))
        check_calibration(kwargs.get('calibration'), len(spec_data))
        check_noise_uncertainty(kwargs.get('noise_uncertainty'), len(spec_data), kwargs.get('calibration'))
        check_robust(kwargs.get('robust'), len(spec_data), kwargs.get('baseline_order'), kwargs.get('calibration'), kwargs.get('correlation'),
                     kwargs.get('response'), kwargs.get('templates'), kwargs.get('noise_uncertainty'), kwargs.get('continuum'))
        check_continuum(kwargs.get('continuum'), len(spec_data), None, cls.MODEL, kwargs.get('calibration'), kwargs.get('correlation'),
                        kwargs.get('response'), kwargs.get('templates'))
        check_correlation(kwargs.get('correlation'), len(spec_data), *spec_data_sizes_masked(spec_data),
                          baseline_order=kwargs.get('baseline_order'), calibration=kwargs.get('calibration'))
        check_response(kwargs.get('response'), len(spec_data), *spec_data_sizes_masked(spec_data),
                       baseline_order=kwargs.get('baseline_order'), calibration=kwargs.get('calibration'))
        check_templates(kwargs.get('templates'), len(spec_data), spec_data_sizes_masked(spec_data)[0], kwargs.get('calibration'),
                        kwargs.get('correlation'), kwargs.get('response'))
        spectra = np.array([DiazenyliumSpectrum(*args) for args in spec_data])
        return cls(spectra, utrans, **kwargs)

    def get_spectra(self):
        return np.array(self.spectra)

    def predict(self, params):
        params = self._check_params(params)
        if self._predict_through_set():
            return self._predict_layered(params)
        for s in self.spectra:
            nnhp_predict(s, params)


# Aliases and metadata at module scope (reference: diazenylium.pyx:234-264)
N = N_PARAMS
IX_VCEN = 0
IX_SIGM = 3
NAME = 'diazenylium'
model_predict = nnhp_predict
ModelSpectrum = DiazenyliumSpectrum
ModelRunner = DiazenyliumRunner

PAR_NAMES = ['voff', 'tex', 'ltau', 'sigm']
PAR_NAMES_SHORT = ['v', 'Tx', 'lt', 's']

TEX_LABELS = [
    r'$v_\mathrm{lsr}$',
    r'$T_\mathrm{ex}$',
    r'$\log(\tau_0)$',
    r'$\sigma_\mathrm{v}$',
]

TEX_LABELS_WITH_UNITS = [
    r'$v_\mathrm{lsr} \ [\mathrm{km\, s^{-1}}]$',
    r'$T_\mathrm{ex} \ [\mathrm{K}]$',
    r'$\log(\tau_0)$',
    r'$\sigma_\mathrm{v} \ [\mathrm{km\, s^{-1}}]$',
]


def get_par_names(ncomp=None):
    return par_names(PAR_NAMES_SHORT, ncomp)
