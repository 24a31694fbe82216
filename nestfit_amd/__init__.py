"""nestfit_amd -- MI355X-native NH3 hyperfine log-likelihood engine.

Drop-in for the hot path of autocorr/nestfit (``AmmoniaRunner.loglikelihood`` /
prior transform / ``amm_predict``); see DESIGN.md and INTEGRATION.md.
"""
from . import _ffi
from ._ffi import EngineError, device_count, get_exp_mode, pinned_empty, set_device, set_exp_mode
from .core import (ConstantPrior, CenSepPrior, Distribution, DuplicatePrior, OrderedPrior, Prior,
                   PriorTransformer, ResolvedCenSepPrior, ResolvedPlacementPrior, SpacedPrior)
from .ammonia import AmmoniaRunner, AmmoniaSpectrum, amm_predict
from .diazenylium import DiazenyliumRunner, DiazenyliumSpectrum, nnhp_predict
from .gaussian import GaussianRunner, gauss_predict
from ._model import HANNING, HANNING_RESPONSE, ar1, check_robust, correlation_of_response, ripple, robust_lnl, smoothed
from . import ammonia, diazenylium, ensemble, excitation, gaussian, hyperfine, lsq, lte
from .excitation import ExcitationGrid, GridLines, GridRunner, GridSpectrum, grid_predict
from .hyperfine import HyperfineRunner, LineTable
from .lte import LteBand, LteBlend, LteLines, LteMix, LteRunner, LteSpectrum, Molecule, lte_predict

# registry like nestfit/models/__init__.py:3-7
MODELS = {m.NAME: m for m in (ammonia, diazenylium, gaussian)}


def model_module(name):
    """The model module of a store's `model_name`: one of MODELS (the reference's three), `hyperfine`, the model of
    caller-supplied line tables, `lte`, one species in LTE across several transitions, or `LteMix` for 'lte_mix', several
    species in LTE (the class: the parameter slots every mix shares, `IX_VCEN` and `IX_SIGM`; names and the number of
    parameters belong to a mix of given species, which a store's root attributes describe), or `excitation` for 'grid', non-LTE
    excitation from a caller's grid; None for an unknown name."""
    return {hyperfine.NAME: hyperfine, lte.NAME: lte, LteMix.NAME: LteMix, excitation.NAME: excitation}.get(name) or MODELS.get(name)


from .prior_constructors import get_irdc_priors, get_synth_priors

__all__ = [
    'EngineError', 'device_count', 'set_device', 'set_exp_mode', 'get_exp_mode', 'pinned_empty',
    'Distribution', 'Prior', 'ConstantPrior', 'DuplicatePrior', 'OrderedPrior', 'SpacedPrior',
    'CenSepPrior', 'ResolvedCenSepPrior', 'ResolvedPlacementPrior', 'PriorTransformer',
    'AmmoniaSpectrum', 'AmmoniaRunner', 'amm_predict', 'get_irdc_priors', 'get_synth_priors',
    'DiazenyliumSpectrum', 'DiazenyliumRunner', 'nnhp_predict', 'GaussianRunner', 'gauss_predict',
    'MODELS', 'hyperfine', 'LineTable', 'HyperfineRunner', 'model_module', 'lsq', 'ensemble',
    'lte', 'Molecule', 'LteLines', 'LteBand', 'LteSpectrum', 'LteRunner', 'lte_predict', 'LteBlend', 'LteMix',
    'excitation', 'ExcitationGrid', 'GridLines', 'GridSpectrum', 'GridRunner', 'grid_predict',
]
